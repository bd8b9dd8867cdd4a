"""What the action-sequence rollout (navsim_rollout, NavGymEnv(rollout=K)) costs.  Appends to profiles/r23_rollout/summary.txt
(NAVSIM_OUT overrides the directory).

    python profiles/r23_rollout/measure.py --calls c3|c2          # reset() + ten steps, then for (K, H) = (16, 8) and (64, 16) at the
                                                                  # default cap: ten rollout() calls and ten lookahead() calls of the
                                                                  # same K, nothing else: run it under rocprofv3 --kernel-trace
                                                                  # --output-format csv
    python profiles/r23_rollout/measure.py --kernels TRACE c3|c2  # (1) the kernels of such a run (its kernel_trace.csv): the rollout
                                                                  # kernel beside the step kernel and beside H lookahead launches
    python profiles/r23_rollout/measure.py pair                   # (2) NavGymEnv: rollout() + step() against step() alone, the same
                                                                  # environment (the rollout only reads), alternating windows
    python profiles/r23_rollout/measure.py --off c2               # reset() + ten steps with the feature off (for the off trace)
"""
import csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r23_rollout"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
COMBOS = ((16, 8), (64, 16))
CALLS = 10

if len(sys.argv) > 3 and sys.argv[1] == "--kernels":
    roll, look, step = [], [], []
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            item = (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, name)
            if "rollout" in name:
                roll.append(item)
            elif "lookahead" in name:
                look.append(item)
            elif "navsim_step" in name:
                step.append(item[1])
    roll.sort(); look.sort()
    step_us = sorted(step)[len(step) // 2]
    with open(SUMMARY, "a") as f:
        f.write("\n(1) %s-shaped world, %d arenas x 1081 beams: kernel times from rocprofv3 --kernel-trace; the step kernel's median over "
                "%d launches is %.2f us\n" % (sys.argv[3], E, len(step), step_us))
        if sys.argv[3].endswith("off"):
            f.write("  launches of kernels with 'rollout' in their name: %d\n" % len(roll))
        for i, (K, H) in enumerate(COMBOS):
            grp = sorted(us for _, us, _ in roll[CALLS * i:CALLS * i + CALLS])
            lk = sorted(us for _, us, _ in look[CALLS * i:CALLS * i + CALLS])
            if grp:
                med = grp[len(grp) // 2]
                f.write("  K = %2d, H = %2d  median %10.2f us  min %10.2f  max %10.2f   x %.1f of the step kernel   %.2f us per sequence-step "
                        "of one arena (x E: %.3f ns per sequence-step of the batch)\n"
                        % (K, H, med, grp[0], grp[-1], med / step_us, med / (K * H), med / (K * H) / E * 1e3))
                if lk:
                    lmed = lk[len(lk) // 2]
                    f.write("                   navsim_lookahead at K = %d: median %.2f us a launch, x H = %.2f us for H launches: the rollout is "
                            "x %.3f of that\n" % (K, lmed, lmed * H, med / (lmed * H)))
        if roll:
            f.write("  kernel: %s\n" % roll[0][2].replace("(anonymous namespace)::", "")[:150])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

WORLDS = dict(c3=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def sequences(n, K, H):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((n, K, H, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 2 and sys.argv[1] in ("--calls", "--off"):
    on = sys.argv[1] == "--calls"
    env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[sys.argv[2]], **(dict(rollout=16) if on else {})))
    env.reset()
    acts = sequences(E, 1, 10)[:, 0]
    for t in range(10):
        env.step(acts[:, t].contiguous())
    if on:
        sim = env.sim
        lengths = []
        for K, H in COMBOS:
            sim.enable_rollout(K, H)
            sim.enable_lookahead(K)
            seq = sequences(E, K, H)
            for _ in range(CALLS):
                out = sim.rollout(seq)
            torch.cuda.synchronize()
            lengths.append((K, H, float(out["length"].double().mean().item()), float((out["exact_steps"] == H).double().mean().item())))
            cand = seq[:, :, 0].contiguous()
            for _ in range(CALLS):
                sim.lookahead(cand)
            torch.cuda.synchronize()
        from nav_gym_amd import sim as simmod
        dmax = float(sim.t["scan_discomfort"].max().item())
        with open(SUMMARY, "a") as f:
            f.write("\n%s: default cap %.2f m (largest discomfort threshold %.3f m); random sequences (v in 0 .. 0.5, w in -0.64 .. 0.64): %s\n"
                    % (sys.argv[2], simmod.rollout_defaults(sim.cfg, dmax)["range"], dmax,
                       "; ".join("K = %d, H = %d: mean length %.2f steps, exact over the horizon %.1f %%" % (K, H, L, 100 * X)
                                 for K, H, L, X in lengths)))
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []
for world in ("c3", "c2"):
    for (K, H), window, reps in zip(COMBOS, (40, 8), (3, 3)):
        env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], rollout=K, rollout_params=dict(horizon=H)))
        env.reset()
        acts = sequences(E, 1, 64)[:, 0]
        seq = sequences(E, K, H)

        def run(roll, n, k0):
            for t in range(n):
                if roll:
                    env.rollout(seq)
                env.step(acts[:, (k0 + t) % 64].contiguous())

        run(True, 5, 0)
        torch.cuda.synchronize()
        times = {False: [], True: []}
        k0 = 5
        for r in range(reps):
            for roll in (False, True):                       # alternating: the two share whatever else the machine does
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(roll, window, k0)
                torch.cuda.synchronize()
                times[roll].append((time.perf_counter() - t0) / window * 1e6)
                k0 += window
        off, on = np.median(times[False]), np.median(times[True])
        lines.append("(2) NavGymEnv on the %s-shaped world, %d arenas, K = %d, H = %d at the default cap, %d windows of %d steps each way, "
                     "alternating: step() alone median %.1f us (min %.1f, max %.1f); rollout() + step() %.1f us (min %.1f, max %.1f): + %.1f us, "
                     "x %.1f" % (world, E, K, H, reps, window, off, min(times[False]), max(times[False]), on, min(times[True]),
                                 max(times[True]), on - off, on / off))
        print(lines[-1], flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
