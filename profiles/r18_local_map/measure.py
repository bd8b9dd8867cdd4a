"""What the egocentric local map (navsim_local_map, NavGymEnv(observe_local_map=G)) costs.  Writes
profiles/r18_local_map/summary.txt (NAVSIM_OUT overrides the directory).

    python profiles/r18_local_map/measure.py throughput             # (2) env-steps/s through NavGymEnv.step(), map on / off
    python profiles/r18_local_map/measure.py --ten-steps off|g32|g64
                                                                    # reset() + ten steps on the c3-shaped world (`g32`, `g64`: a
                                                                    # 32 x 32 resp. 64 x 64 map of 4 channels), nothing else: run
                                                                    # it under rocprofv3 --kernel-trace --stats --output-format csv
    python profiles/r18_local_map/measure.py --kernels STATS off|g32|g64
                                                                    # (1) the kernels of such a run (its kernel_stats.csv) appended
                                                                    # to the summary: local_map_kernel beside the step kernel, the
                                                                    # bytes it writes and the write rate that implies

(2): two environments of the same world alternate in one process, in windows of NAVSIM_WINDOW steps, NAVSIM_REPS windows each, a
host clock around a window that ends in a device synchronise; both are driven by the same recorded random actions, so the step's
own work is the same.
"""
import collections, csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r18_local_map"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
SIZES = dict(g32=32, g64=64)
CHANNELS = 4
HBM_ACHIEVABLE = 6.3e12          # bytes/s a streaming kernel reaches on the MI355X (a float4 copy: 6.29 TB/s measured, 8 TB/s nominal)

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    names, avg_us = collections.Counter(), {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or "?"
            names[name] += int(row["Calls"]) if "Calls" in row else 1
            if "AverageNs" in row:
                avg_us[name] = float(row["AverageNs"]) / 1e3
    variant = sys.argv[3] if len(sys.argv) > 3 else "off"
    with open(SUMMARY, "a") as f:
        f.write("\n(1) kernels of reset() + ten steps of `%s` on the c3-shaped world, %d arenas x 20 pedestrians (rocprofv3 --kernel-trace "
                "--stats): launches, average us, name\n" % (variant, E))
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            if "local_map" in k or "navsim_step" in k or n >= 10:
                f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        ours = [k for k in avg_us if "local_map" in k]
        step = [k for k in avg_us if "navsim_step" in k and names[k] >= 10]
        f.write("  launches of kernels with 'local_map' in their name: %d\n" % sum(names[k] for k in ours))
        if ours and step and variant in SIZES:
            G = SIZES[variant]
            written = E * CHANNELS * G * G * 4
            t = avg_us[ours[0]]
            rate = written / (t * 1e-6)
            f.write("  local_map_kernel %.2f us = x %.3f of the step kernel's %.2f us\n" % (t, t / avg_us[step[0]], avg_us[step[0]]))
            f.write("  it writes %d x %d x %d x %d x 4 B = %.1f MB: %.2f TB/s, %.2f of the %.1f TB/s a streaming kernel reaches "
                    "(the least time the writes could take: %.1f us)\n"
                    % (E, CHANNELS, G, G, written / 1e6, rate / 1e12, rate / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12,
                       written / HBM_ACHIEVABLE * 1e6))
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "5"))
C3 = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234)


def actions(n):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((64, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    which = sys.argv[2] if len(sys.argv) > 2 else "off"
    kw = dict(C3)
    if which != "off":
        kw.update(observe_local_map=SIZES[which])
    env = nav_gym_env.make("NavGym-v0", **kw)
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []


def on_off(label, kw, G):
    envs = {"off": nav_gym_env.make("NavGym-v0", **kw), "on": nav_gym_env.make("NavGym-v0", **dict(kw, observe_local_map=G))}
    acts = actions(kw["num_envs"])
    for env in envs.values():
        env.reset()

    def run(name, n, k0):
        for t in range(n):
            envs[name].step(acts[(k0 + t) % 64])

    for name in envs:
        run(name, 30, 0)
    torch.cuda.synchronize()
    times = {name: [] for name in envs}
    k0 = 30
    for r in range(reps):
        for name in envs:                                    # alternating: the two share whatever else the machine does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, window, k0)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / window)
        k0 += window
    base = np.median(times["off"])
    lines.append("%s, %d arenas, %d windows of %d steps per variant, alternating (us per step; M env-steps/s from the median)"
                 % (label, kw["num_envs"], reps, window))
    for name in envs:
        t = np.array(times[name]) * 1e6
        lines.append("  %-4s median %8.1f us  min %8.1f  max %8.1f   %6.2f M env-steps/s   x %.3f of off   (+%.1f us)"
                     % (name, np.median(t), t.min(), t.max(), kw["num_envs"] / np.median(t), np.median(t) / (base * 1e6),
                        np.median(t) - base * 1e6))
    m = envs["on"].local_map()
    lines.append("  `on`, last step: the map is %s, %.1f %% of its wall cells are 0, %.1f %% of its cells are covered by a pedestrian"
                 % (tuple(m.shape), 100.0 * float((m[:, 0] == 0).float().mean()), 100.0 * float((m[:, 1] == 0).float().mean())))
    print("\n".join(lines[-4:]), flush=True)
    for env in envs.values():
        env.close()


what = sys.argv[1] if len(sys.argv) > 1 else "all"
if what in ("all", "throughput"):
    on_off("(2a) NavGymEnv.step() on the c3-shaped world, observe_local_map=32 (4 channels, 0.1 m cells)", C3, 32)
    on_off("(2b) the same, observe_local_map=64", C3, 64)
text = "\n".join(lines) + "\n"
with open(SUMMARY, "a") as f:
    f.write(text + "\n")
