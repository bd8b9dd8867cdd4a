"""What info['humans'] costs through NavGymEnv.step() on the c3-shaped world (4096 arenas, 1081 beams, 500 x 500 maps, 20
social-force pedestrians, same-step auto-reset): two environments of the same world alternate in one process,

    off     observe_humans=None
    on      observe_humans=10, three lines of sight per pedestrian: one launch behind the step (navsim_ped_observe)

in windows of NAVSIM_WINDOW steps, NAVSIM_REPS windows each, a host clock around a window that ends in a device synchronise.
Writes profiles/r15_ped_observe/summary.txt (NAVSIM_OUT overrides the directory): per variant the median, minimum and maximum
window, and the ratio to `off`.

    python profiles/_diag/ped_observe_steps.py                    # the two variants
    python profiles/_diag/ped_observe_steps.py --ten-steps [on]   # reset() + ten steps of `off` (or `on`), nothing else: run it
                                                                  # under rocprofv3 --kernel-trace --stats to see that `off`
                                                                  # launches nothing new, and what the kernel of `on` takes
    python profiles/_diag/ped_observe_steps.py --kernels CSV off|on   # the kernels of such a run (its kernel_stats.csv), counted,
                                                                  # appended to the summary; `on`: the kernel beside the step's
"""
import collections, csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r15_ped_observe"))
os.makedirs(OUT, exist_ok=True)

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    names, avg_us = collections.Counter(), {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or "?"
            names[name] += int(row["Calls"]) if "Calls" in row else 1
            if "AverageNs" in row:
                avg_us[name] = float(row["AverageNs"]) / 1e3
    variant = sys.argv[3] if len(sys.argv) > 3 else "off"
    with open(os.path.join(OUT, "summary.txt"), "a") as f:
        f.write("\nkernels of reset() + ten steps of `%s` (rocprofv3 --kernel-trace --stats): launches, average us, name\n" % variant)
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        f.write("  launches of kernels with 'ped_observe' in their name: %d\n" % sum(n for k, n in names.items() if "ped_observe" in k))
        obs = [k for k in avg_us if "ped_observe" in k]
        step = [k for k in avg_us if "navsim_step" in k and names[k] >= 10]
        if obs and step:
            f.write("  ped_observe_kernel %.2f us next to the step kernel's %.2f us: x %.3f of the step it follows\n"
                    % (avg_us[obs[0]], avg_us[step[0]], avg_us[obs[0]] / avg_us[step[0]]))
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "7"))
kw = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234)
ON = dict(observe_humans=10, observe_params=dict(rays=3))
g = torch.Generator(device="cuda:0"); g.manual_seed(78)
acts = torch.rand((64, E, 2), generator=g, device="cuda:0", dtype=torch.float64)
acts[..., 0] *= 0.5; acts[..., 1] = acts[..., 1] * 1.28 - 0.64

if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    env = nav_gym_env.make("NavGym-v0", **dict(kw, **(ON if sys.argv[2:3] == ["on"] else {})))
    env.reset()
    for t in range(10):
        env.step(acts[t])
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

envs = {"off": nav_gym_env.make("NavGym-v0", **kw), "on": nav_gym_env.make("NavGym-v0", **dict(kw, **ON))}
for env in envs.values():
    env.reset()


def run(name, n, k0):
    env = envs[name]
    for t in range(n):
        env.step(acts[(k0 + t) % 64])


for name in envs:                                            # warm-up: every variant
    run(name, 30, 0)
torch.cuda.synchronize()
times = {name: [] for name in envs}
k0 = 30
for r in range(reps):
    for name in envs:                                        # alternating: the two share whatever else the machine does
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(name, window, k0)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / window)
    k0 += window
h = envs["on"].observed_humans()
lines = ["NavGymEnv.step() on the c3-shaped world, %d arenas x 20 pedestrians, %d windows of %d steps per variant, variants alternating in one process"
         % (E, reps, window),
         "(host clock around a window that ends in a device synchronise; us per step, M env-steps/s from the median)"]
base = np.median(times["off"])
for name in envs:
    t = np.array(times[name]) * 1e6
    lines.append("  %-4s median %7.1f us  min %7.1f  max %7.1f   %6.2f M env-steps/s   x %.3f of off   (+%.1f us)"
                 % (name, np.median(t), t.min(), t.max(), E / np.median(t), np.median(t) / (base * 1e6), np.median(t) - base * 1e6))
lines.append("  `on` after the run: %.2f pedestrians seen per arena, %.2f rows used of 10, %d arenas see more than 10"
             % (h["count"].double().mean().item(), (h["index"] >= 0).sum(dim=1).double().mean().item(), int((h["count"] > 10).sum().item())))
text = "\n".join(lines) + "\n"
print(text)
with open(os.path.join(OUT, "summary.txt"), "w") as f:
    f.write(text)
for env in envs.values():
    env.close()
