"""What the local planner (navsim_dwa, NavGymEnv(local_planner='dwa')) costs and how it drives.  Writes
profiles/r17_dwa/summary.txt (NAVSIM_OUT overrides the directory).

    python profiles/r17_dwa/measure.py throughput              # (2) env-steps/s through NavGymEnv.step(), planner on / off
    python profiles/r17_dwa/measure.py behaviour               # (3) 150 steps on 64 outdoor arenas: planner, zero, random actions
    python profiles/r17_dwa/measure.py --ten-steps off|on|max  # reset() + ten steps on the c3-shaped world (`on`: the defaults, 5 x 9
                                                               # candidates over 8 steps; `max`: 16 x 32 over 32), nothing else: run
                                                               # it under rocprofv3 --kernel-trace --stats --output-format csv
    python profiles/r17_dwa/measure.py --kernels STATS off|on|max
                                                               # (1) the kernels of such a run (its kernel_stats.csv) appended to
                                                               # the summary: dwa_kernel beside the step kernel

(2): two environments of the same world alternate in one process, in windows of NAVSIM_WINDOW steps, NAVSIM_REPS windows each, a
host clock around a window that ends in a device synchronise; both are driven by the same recorded random actions, so the step's
own work is the same.  (3): every arena's FIRST episode under same-step auto-reset: success, crash, or neither within 150 steps.
"""
import collections, csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r17_dwa"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")

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
        f.write("\n(1) kernels of reset() + ten steps of `%s` on the c3-shaped world, 4096 arenas x 20 pedestrians (rocprofv3 --kernel-trace "
                "--stats): launches, average us, name\n" % variant)
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            if "dwa_" in k or "navsim_step" in k or n >= 10:
                f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        dwa = [k for k in avg_us if "dwa_" in k]
        step = [k for k in avg_us if "navsim_step" in k and names[k] >= 10]
        f.write("  launches of kernels with 'dwa_' in their name: %d\n" % sum(names[k] for k in dwa))
        if dwa and step:
            f.write("  dwa_kernel %.2f us = x %.3f of the step kernel's %.2f us\n" % (avg_us[dwa[0]], avg_us[dwa[0]] / avg_us[step[0]], avg_us[step[0]]))
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "5"))
C3 = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234)
MAX = dict(n_v=16, n_w=32, horizon=32)


def actions(n):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((64, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    which = sys.argv[2] if len(sys.argv) > 2 else "off"
    kw = dict(C3)
    if which != "off":
        kw.update(local_planner="dwa", local_planner_params=MAX if which == "max" else None)
    env = nav_gym_env.make("NavGym-v0", **kw)
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []


def on_off(label, kw, params=None):
    envs = {"off": nav_gym_env.make("NavGym-v0", **kw),
            "on": nav_gym_env.make("NavGym-v0", **dict(kw, local_planner="dwa", local_planner_params=params))}
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
    st = envs["on"].planner_action()["status"]
    lines.append("  `on`, last step: %.1f %% of the arenas blocked" % (100.0 * float((st == 2).float().mean())))
    print("\n".join(lines[-4:]), flush=True)
    for env in envs.values():
        env.close()


def behaviour(label, driver, steps=150, **kw):
    """Every arena's first episode: how it ended within `steps` steps."""
    n = 64
    base = dict(num_envs=n, n_beams=512, map_size=400, indoor_ratio=0.0, min_goal_dist=3.0, max_goal_dist=8.0, device="cuda:0", seed=4321)
    base.update(kw)
    if driver == "planner":
        base.update(local_planner="dwa")
    env = nav_gym_env.make("NavGym-v0", **base)
    env.reset()
    rng = torch.Generator(device="cuda:0"); rng.manual_seed(5)
    first = torch.zeros(n, dtype=torch.int32, device="cuda:0")      # 0 running, 1 success, 2 crash
    blocked = 0
    for t in range(steps):
        if driver == "planner":
            plan = env.planner_action()
            act = plan["action"]
            blocked += int((plan["status"] == 2).sum())
        elif driver == "zero":
            act = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
        else:
            act = torch.rand((n, 2), generator=rng, device="cuda:0", dtype=torch.float64)
            act[:, 0] *= 0.5; act[:, 1] = act[:, 1] * 1.28 - 0.64
        _, _, done, info = env.step(act)
        code = torch.where(info["is_success"] > 0, 1, torch.where(info["is_crash"] > 0, 2, 0)).to(torch.int32)
        first = torch.where((first == 0) & done, code, first)
    f = first.cpu().numpy()
    lines.append("  %-46s %-8s success %2d  crash %2d  neither %2d  of %d%s"
                 % (label, driver, int((f == 1).sum()), int((f == 2).sum()), int((f == 0).sum()), n,
                    "   (planner blocked in %.1f %% of the arena-steps)" % (100.0 * blocked / (n * steps)) if driver == "planner" else ""))
    print(lines[-1], flush=True)
    env.close()


what = sys.argv[1] if len(sys.argv) > 1 else "all"
if what in ("all", "throughput"):
    on_off("(2a) NavGymEnv.step() on the c3-shaped world, the defaults (5 x 9 candidates, 8 steps)", C3)
    on_off("(2b) the same, 16 x 32 candidates over 32 steps", C3, MAX)
if what in ("all", "behaviour"):
    lines.append("(3) the first episode of 64 outdoor arenas (400 x 400 cells, goals 3 .. 8 m away), 150 steps, same-step auto-reset")
    for label, kw in (("no pedestrians", dict(pedestrian_model="none", num_humans=0)),
                      ("no pedestrians, goal_path=True", dict(pedestrian_model="none", num_humans=0, goal_path=True)),
                      ("8 social-force pedestrians", dict(pedestrian_model="sfm", num_humans=8)),
                      ("8 social-force pedestrians, goal_path=True", dict(pedestrian_model="sfm", num_humans=8, goal_path=True))):
        for driver in ("planner", "zero", "random"):
            if driver != "planner" and "goal_path" in kw:
                continue                                     # (the goal path changes nothing for a driver that does not read it)
            behaviour(label, driver, **kw)
text = "\n".join(lines) + "\n"
with open(SUMMARY, "a") as f:
    f.write(text + "\n")
