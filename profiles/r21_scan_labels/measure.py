"""What the scan ground truth (navsim_scan_labels, NavGymEnv(scan_labels=True)) costs.  Writes
profiles/r21_scan_labels/summary.txt (NAVSIM_OUT overrides the directory).

    python profiles/r21_scan_labels/measure.py throughput           # (2) env-steps/s through NavGymEnv.step(), labels on / off
    python profiles/r21_scan_labels/measure.py --ten-steps c3|c2 on|off
                                                                    # reset() + ten steps on the c3-shaped world (4096 arenas x 20
                                                                    # pedestrians x 1081 beams) or the c2-shaped one (no
                                                                    # pedestrians), nothing else: run it under rocprofv3
                                                                    # --kernel-trace --stats --output-format csv
    python profiles/r21_scan_labels/measure.py --kernels STATS c3|c2 on|off
                                                                    # (1) the kernels of such a run (its kernel_stats.csv) appended
                                                                    # to the summary: scan_labels_kernel beside the step kernel

(2): two environments of the same world alternate in one process, in windows of NAVSIM_WINDOW steps, NAVSIM_REPS windows each, a
host clock around a window that ends in a device synchronise; both are driven by the same recorded random actions, so the step's
own work is the same.
"""
import collections, csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r21_scan_labels"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    names, avg_us = collections.Counter(), {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or "?"
            names[name] += int(row["Calls"]) if "Calls" in row else 1
            if "AverageNs" in row:
                avg_us[name] = float(row["AverageNs"]) / 1e3
    world, variant = sys.argv[3], sys.argv[4]
    with open(SUMMARY, "a") as f:
        f.write("\n(1) kernels of reset() + ten steps on the %s-shaped world, %d arenas, scan_labels %s (rocprofv3 --kernel-trace --stats): "
                "launches, average us, name\n" % (world, E, variant))
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            if "scan_labels" in k or "navsim_step" in k or n >= 10:
                f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        ours = [k for k in avg_us if "scan_labels" in k]
        step = [k for k in avg_us if "navsim_step" in k and names[k] >= 10]
        f.write("  launches of kernels with 'scan_labels' in their name: %d\n" % sum(names[k] for k in ours))
        if ours and step:
            t = avg_us[ours[0]]
            f.write("  scan_labels_kernel %.2f us = x %.3f of the step kernel's %.2f us in the same trace\n" % (t, t / avg_us[step[0]], avg_us[step[0]]))
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "5"))
WORLDS = dict(c3=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def actions(n):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((64, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[sys.argv[2]], scan_labels=sys.argv[3] == "on"))
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []


def on_off(label, kw):
    envs = {"off": nav_gym_env.make("NavGym-v0", **kw), "on": nav_gym_env.make("NavGym-v0", **dict(kw, scan_labels=True))}
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
    lab = envs["on"].scan_labels()["label"]
    share = [100.0 * float((lab == k).float().mean()) for k in range(4)]
    lines.append("  `on`, last step: beams without a return %.1f %%, on walls %.1f %%, on pedestrian bodies %.1f %%, on legs %.1f %%" % tuple(share))
    print("\n".join(lines[-4:]), flush=True)
    for env in envs.values():
        env.close()


what = sys.argv[1] if len(sys.argv) > 1 else "all"
if what in ("all", "throughput"):
    on_off("(2a) NavGymEnv.step() on the c3-shaped world (20 pedestrians), scan_labels on against off", WORLDS["c3"])
    on_off("(2b) the same on the c2-shaped world (no pedestrians)", WORLDS["c2"])
text = "\n".join(lines) + "\n"
with open(SUMMARY, "a") as f:
    f.write(text + "\n")
