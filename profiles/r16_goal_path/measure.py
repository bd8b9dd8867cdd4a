"""What the goal path (navsim_goal_path, NavGymEnv(goal_path=True)) costs.  Writes profiles/r16_goal_path/summary.txt (NAVSIM_OUT
overrides the directory).

    python profiles/r16_goal_path/measure.py                       # (2) rebuild-all calls and their sweeps, (3) env-steps/s on / off
    python profiles/r16_goal_path/measure.py --ten-steps off|on    # reset() + ten steps on the c3-shaped world (`on`: + ten calls
                                                                   # that find every key current), nothing else: run it under
                                                                   # rocprofv3 --kernel-trace --stats
    python profiles/r16_goal_path/measure.py --kernels STATS off|on [TRACE]
                                                                   # (1) the kernels of such a run (its kernel_stats.csv) appended to
                                                                   # the summary; `on` with its kernel_trace.csv: the two kernels
                                                                   # dispatch by dispatch -- the reset's call, the ten steps' calls,
                                                                   # the ten calls that rebuild nothing -- beside the step's

(2): device events around ONE call with rebuild = every arena, median of 5, and the sweeps each arena's relaxation took
(navsim_debug_goal_path_sweeps).  (3): two environments of the same world alternate in one process, in windows of NAVSIM_WINDOW
steps, NAVSIM_REPS windows each, a host clock around a window that ends in a device synchronise.
"""
import collections, csv, ctypes as C, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r16_goal_path"))
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
        f.write("\n(1) kernels of reset() + ten steps of `%s` on the c3-shaped world, 4096 arenas (rocprofv3 --kernel-trace --stats): "
                "launches, average us, name\n" % variant)
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            if "goal_" in k or "navsim_step" in k or n >= 10:
                f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        f.write("  launches of kernels with 'goal_' in their name: %d\n" % sum(n for k, n in names.items() if "goal_" in k))
        step = [k for k in avg_us if "navsim_step" in k and names[k] >= 10]
        if len(sys.argv) > 4 and step:                      # the trace: one row per dispatch, in order
            us = {"goal_field": [], "goal_query": []}
            with open(sys.argv[4]) as g:
                rows = sorted(csv.DictReader(g), key=lambda r: int(r["Start_Timestamp"]))
            for row in rows:
                for k in us:
                    if k in row["Kernel_Name"]:
                        us[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
            med = lambda v: sorted(v)[len(v) // 2]
            f.write("  dispatch by dispatch (kernel trace; us): the reset()'s call rebuilds all 4096 fields, each step's call the fields of "
                    "the arenas that restarted in it (about 20), the last ten calls none\n")
            for k, v in us.items():
                if len(v) == 21:
                    f.write("    %-18s reset() %9.2f | ten steps: median %8.2f min %8.2f max %8.2f | rebuilds nothing: median %6.2f min %6.2f max %6.2f\n"
                            % (k + "_kernel", v[0], med(v[1:11]), min(v[1:11]), max(v[1:11]), med(v[11:]), min(v[11:]), max(v[11:])))
                else:
                    f.write("    %-18s %d dispatches: %s\n" % (k + "_kernel", len(v), " ".join("%.2f" % x for x in v)))
            if all(len(v) == 21 for v in us.values()):
                none = med(us["goal_field"][11:]) + med(us["goal_query"][11:])
                some = med(us["goal_field"][1:11]) + med(us["goal_query"][1:11])
                f.write("    a call that rebuilds nothing: %.2f us of kernel time = x %.3f of the step kernel's %.2f us; a step's call: %.2f us = x %.3f\n"
                        % (none, none / avg_us[step[0]], avg_us[step[0]], some, some / avg_us[step[0]]))
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "5"))
C3 = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234)
C2 = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234)
REF = dict(num_envs=E, map_size="reference", randomize_maps=True, pedestrian_model="sfm", device="cuda:0", seed=1234)


def actions(n):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((64, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    env = nav_gym_env.make("NavGym-v0", **dict(C3, goal_path=(sys.argv[2:3] == ["on"])))
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    if env.goal_path_on:
        for t in range(10):                                  # nothing changed since the last step's call: every key is current
            env.sim.goal_path()
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []


def rebuild_all(label, n, **kw):
    """One call that rebuilds every field, timed by device events; the sweeps per arena; then a call that rebuilds nothing."""
    env = nav_gym_env.make("NavGym-v0", **dict(kw, num_envs=n, goal_path=True))
    env.reset()
    sim = env.sim
    sweeps = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    sim.lib.navsim_debug_goal_path_sweeps(C.c_void_p(sweeps.data_ptr()))
    every = torch.ones(n, dtype=torch.uint8, device="cuda:0")
    one = torch.zeros(n, dtype=torch.uint8, device="cuda:0"); one[int(sweeps.numel()) // 2] = 1
    ms_all, ms_none, ms_one = [], [], []
    for rep in range(5):
        for which, store in ((every, ms_all), (None, ms_none), (one, ms_one)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); sim.goal_path(rebuild=which); b.record()
            torch.cuda.synchronize()
            store.append(a.elapsed_time(b))
    sim.lib.navsim_debug_goal_path_sweeps(None)
    s = sweeps.cpu().numpy()
    h = sim.goal_path_host()
    d = env.goal_field().cpu().numpy().view(np.uint16)
    reach = (d != 0xFFFF).reshape(n, -1).sum(axis=1)
    lines.append("  %-28s %5d arenas, %3d x %3d nav cells: rebuild-all call %8.3f ms (min %.3f) = %7.1f us per arena; sweeps min %d "
                 "median %d max %d; reachable cells median %d; a call that rebuilds ONE field %.1f us, none %.1f us (events around both launches); "
                 "status OK %.0f %% off-field %.0f %%"
                 % (label, n, d.shape[1], d.shape[2], np.median(ms_all), min(ms_all), np.median(ms_all) * 1e3 / n, s.min(), np.median(s),
                    s.max(), np.median(reach), np.median(ms_one) * 1e3, np.median(ms_none) * 1e3, 100.0 * (h["status"] & 1).mean(), 100.0 * (h["status"] == 4).mean()))
    print(lines[-1], flush=True)
    env.close()


def on_off(label, kw):
    envs = {"off": nav_gym_env.make("NavGym-v0", **kw), "on": nav_gym_env.make("NavGym-v0", **dict(kw, goal_path=True))}
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
    r0 = envs["on"].sim.goal_path_rebuilds()
    for r in range(reps):
        for name in envs:                                    # alternating: the two share whatever else the machine does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, window, k0)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / window)
        k0 += window
    per_step = (envs["on"].sim.goal_path_rebuilds() - r0) / float(reps * window)
    base = np.median(times["off"])
    lines.append("%s, %d arenas, %d windows of %d steps per variant, alternating (us per step; M env-steps/s from the median)"
                 % (label, kw["num_envs"], reps, window))
    for name in envs:
        t = np.array(times[name]) * 1e6
        lines.append("  %-4s median %8.1f us  min %8.1f  max %8.1f   %6.2f M env-steps/s   x %.3f of off   (+%.1f us)"
                     % (name, np.median(t), t.min(), t.max(), kw["num_envs"] / np.median(t), np.median(t) / (base * 1e6),
                        np.median(t) - base * 1e6))
    lines.append("  `on`: %.1f fields rebuilt per step" % per_step)
    print("\n".join(lines[-4:]), flush=True)
    for env in envs.values():
        env.close()


what = sys.argv[1] if len(sys.argv) > 1 else "all"
if what in ("all", "rebuild"):
    lines.append("(2) rebuild-all calls (device events, median of 5) and sweeps per arena")
    rebuild_all("500 x 500 outdoor maps", 1024, n_beams=64, map_size=500, indoor_ratio=0.0, pedestrian_model="none", device="cuda:0", seed=1234)
    rebuild_all("1000 x 1000 reference worlds", 512, n_beams=64, map_size="reference", pedestrian_model="none", device="cuda:0", seed=1234)
if what in ("all", "c2"):
    on_off("(3a) NavGymEnv.step() on the c2-shaped world", C2)
if what in ("all", "reference"):
    on_off("(3b) NavGymEnv.step() on map_size='reference', randomize_maps=True", REF)
text = "\n".join(lines) + "\n"
with open(SUMMARY, "a") as f:
    f.write(text + "\n")
