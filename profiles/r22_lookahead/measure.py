"""What the action lookahead (navsim_lookahead, NavGymEnv(lookahead=K)) costs.  Appends to profiles/r22_lookahead/summary.txt
(NAVSIM_OUT overrides the directory).

    python profiles/r22_lookahead/measure.py --calls c3|c2          # reset() + ten steps, then ten lookahead() calls for each of
                                                                    # K = 9 / 64 at the default cap and at range_max, nothing else:
                                                                    # run it under rocprofv3 --kernel-trace --output-format csv
    python profiles/r22_lookahead/measure.py --kernels TRACE c3|c2  # (1) the kernels of such a run (its kernel_trace.csv): the
                                                                    # lookahead kernel's four groups of ten beside the step kernel
    python profiles/r22_lookahead/measure.py pair                   # (2) NavGymEnv: lookahead() + step() against step() alone, the
                                                                    # same environment (the lookahead only reads), alternating windows
    python profiles/r22_lookahead/measure.py --off c2               # reset() + ten steps with the feature off (for the off trace)
"""
import csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r22_lookahead"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
COMBOS = ((9, "default"), (9, "range_max"), (64, "default"), (64, "range_max"))

if len(sys.argv) > 3 and sys.argv[1] == "--kernels":
    look, step, other = [], [], set()
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            if "lookahead" in name:
                look.append((int(row["Start_Timestamp"]), us, name))
            elif "navsim_step" in name:
                step.append(us)
    look.sort()
    step_us = sorted(step)[len(step) // 2]
    with open(SUMMARY, "a") as f:
        f.write("\n(1) %s-shaped world, %d arenas x 1081 beams: kernel times from rocprofv3 --kernel-trace; the step kernel's median over "
                "%d launches is %.2f us\n" % (sys.argv[3], E, len(step), step_us))
        if sys.argv[3].endswith("off"):
            f.write("  launches of kernels with 'lookahead' in their name: %d\n" % len(look))
        for i, (K, R) in enumerate(COMBOS):
            grp = sorted(us for _, us, _ in look[10 * i:10 * i + 10])
            if grp:
                med = grp[len(grp) // 2]
                f.write("  K = %2d, R = %-9s  median %8.2f us  min %8.2f  max %8.2f   x %.3f of the step kernel   (%.2f us per candidate)\n"
                        % (K, R, med, grp[0], grp[-1], med / step_us, med / K))
        if look:
            f.write("  kernel: %s\n" % look[0][2].replace("(anonymous namespace)::", "")[:150])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

WORLDS = dict(c3=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def actions(n, k=64):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((k, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 2 and sys.argv[1] in ("--calls", "--off"):
    on = sys.argv[1] == "--calls"
    env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[sys.argv[2]], **(dict(lookahead=9) if on else {})))
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    if on:
        sim = env.sim
        for K, R in COMBOS:
            sim.enable_lookahead(K, None if R == "default" else dict(range=sim.cfg.range_max))
            cand = acts[:K].permute(1, 0, 2).contiguous()
            for _ in range(10):
                sim.lookahead(cand)
            torch.cuda.synchronize()
        from nav_gym_amd import sim as simmod
        dmax = float(sim.t["scan_discomfort"].max().item())
        with open(SUMMARY, "a") as f:
            f.write("\n%s: default cap %.2f m (largest discomfort threshold %.3f m), range_max %.1f m\n"
                    % (sys.argv[2], simmod.lookahead_defaults(sim.cfg, dmax)["range"], dmax, sim.cfg.range_max))
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "5"))
lines = []
for world in ("c3", "c2"):
    for K in (9, 64):
        env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], lookahead=K))
        env.reset()
        acts = actions(E)
        cand = acts[:K].permute(1, 0, 2).contiguous()

        def run(look, n, k0):
            for t in range(n):
                if look:
                    env.lookahead(cand)
                env.step(acts[(k0 + t) % 64])

        run(True, 30, 0)
        torch.cuda.synchronize()
        times = {False: [], True: []}
        k0 = 30
        for r in range(reps):
            for look in (False, True):                       # alternating: the two share whatever else the machine does
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(look, window, k0)
                torch.cuda.synchronize()
                times[look].append((time.perf_counter() - t0) / window * 1e6)
                k0 += window
        off, on = np.median(times[False]), np.median(times[True])
        lines.append("(2) NavGymEnv on the %s-shaped world, %d arenas, K = %d at the default cap, %d windows of %d steps each way, alternating: "
                     "step() alone median %.1f us (min %.1f, max %.1f); lookahead() + step() %.1f us (min %.1f, max %.1f): + %.1f us, x %.3f"
                     % (world, E, K, reps, window, off, min(times[False]), max(times[False]), on, min(times[True]), max(times[True]),
                        on - off, on / off))
        print(lines[-1], flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
