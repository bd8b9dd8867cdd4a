"""What the lookahead observations (navsim_lookahead_obs, NavGymEnv(lookahead_obs=K)) cost.  Appends to
profiles/r26_lookahead_obs/summary.txt (NAVSIM_OUT overrides the directory).

    python profiles/r26_lookahead_obs/measure.py --calls c3|c2          # reset() + ten steps, then ten calls each of navsim_lookahead
                                                                        # at R = range_max and of navsim_lookahead_obs with rows
                                                                        # 'full' and 'scan', for K = 9 and 64, nothing else: run it
                                                                        # under rocprofv3 --kernel-trace --output-format csv
    python profiles/r26_lookahead_obs/measure.py --kernels TRACE c3|c2  # (1) the kernels of such a run (its kernel_trace.csv): the
                                                                        # six groups of ten beside the step kernel, the bytes written
    python profiles/r26_lookahead_obs/measure.py pair                   # (2) NavGymEnv: lookahead_obs() + step() against step() alone,
                                                                        # the same environment, alternating windows
    python profiles/r26_lookahead_obs/measure.py --off c2               # reset() + ten steps with the feature off (for the off trace)
"""
import csv, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r26_lookahead_obs"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
B = 1081
GROUPS = tuple((K, what) for K in (9, 64) for what in ("lookahead", "full", "scan"))     # the order --calls launches them in
HBM_PEAK = 8.0e12                                                                          # bytes / s (MI355X, HBM3E)


def bytes_written(K, S, rows):
    """What one arena's workgroup stores: the nine shared arrays (54 B a candidate + the status byte), scan, tail, goals,
    truncated and, with rows 'full', the row.  (A crashing candidate's scan slots are stored twice; not counted.)"""
    per = 54 + 4 * B + 28 + 16 + 1 + (4 * (S * B + 7) if rows == "full" else 0)
    return K * per + 1


if len(sys.argv) > 3 and sys.argv[1] == "--kernels":
    groups, step = {"lookahead_obs": [], "lookahead": []}, []
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            if "lookahead_obs_kernel" in name:
                groups["lookahead_obs"].append((int(row["Start_Timestamp"]), us, name))
            elif "lookahead_kernel" in name:
                groups["lookahead"].append((int(row["Start_Timestamp"]), us, name))
            elif "navsim_step" in name:
                step.append(us)
    for v in groups.values():
        v.sort()
    step_us = sorted(step)[len(step) // 2]
    meta = {}
    if os.path.exists(os.path.join(OUT, "calls_%s.json" % sys.argv[3])):
        meta = json.load(open(os.path.join(OUT, "calls_%s.json" % sys.argv[3])))
    S = int(meta.get("S", 1))
    with open(SUMMARY, "a") as f:
        f.write("\n(1) %s-shaped world, %d arenas x %d beams, stack of %d: kernel times from rocprofv3 --kernel-trace; the step kernel's "
                "median over %d launches is %.2f us\n" % (sys.argv[3], E, B, S, len(step), step_us))
        if sys.argv[3].endswith("off"):
            f.write("  launches of kernels with 'lookahead_obs' in their name: %d\n" % len(groups["lookahead_obs"]))
        med = {}
        for K in (9, 64):
            for i, what in enumerate(("lookahead", "full", "scan")):
                src = groups["lookahead"] if what == "lookahead" else groups["lookahead_obs"]
                at = 10 * (0 if K == 9 else 1) if what == "lookahead" else 10 * ((0 if K == 9 else 2) + (i - 1))
                grp = sorted(us for _, us, _ in src[at:at + 10])
                if not grp:
                    continue
                m = med[(K, what)] = grp[len(grp) // 2]
                line = "  K = %2d, %-26s median %8.2f us  min %8.2f  max %8.2f   x %.3f of the step kernel" % (
                    K, "navsim_lookahead(range_max)" if what == "lookahead" else "lookahead_obs rows=%s" % what, m, grp[0], grp[-1], m / step_us)
                if what != "lookahead":
                    nbytes = E * bytes_written(K, S, what)
                    line += "   x %.3f of that lookahead launch   %.1f MB written, %.1f GB/s (%.1f %% of the HBM peak)" % (
                        m / med[(K, "lookahead")], nbytes / 1e6, nbytes / m / 1e3, 100.0 * nbytes / (m * 1e-6) / HBM_PEAK)
                f.write(line + "\n")
        for v in groups.values():
            if v:
                f.write("  kernel: %s\n" % v[0][2].replace("(anonymous namespace)::", "")[:150])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

WORLDS = dict(c3=dict(num_envs=E, n_beams=B, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=B, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def actions(n, k=64):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((k, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 2 and sys.argv[1] in ("--calls", "--off"):
    on = sys.argv[1] == "--calls"
    env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[sys.argv[2]], **(dict(lookahead_obs=9) if on else {})))
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    if on:
        sim = env.sim
        for K in (9, 64):
            cand = acts[:K].permute(1, 0, 2).contiguous()
            sim.enable_lookahead(K, dict(range=sim.cfg.range_max))
            for _ in range(10):
                sim.lookahead(cand)
            torch.cuda.synchronize()
            for rows in ("full", "scan"):
                sim.enable_lookahead_obs(K, dict(rows=rows))
                for _ in range(10):
                    sim.lookahead_obs(cand)
                torch.cuda.synchronize()
        out = sim.lookahead_obs_host()
        std = sim.t["scan_noise_std"]
        with open(os.path.join(OUT, "calls_%s.json" % sys.argv[2]), "w") as f:
            json.dump(dict(S=int(sim.cfg.n_scan_stack)), f)
        with open(SUMMARY, "a") as f:
            f.write("\n%s: range_max %.1f m, stack of %d, add_scan_noise %d, noise std in [%.4f, %.4f] m; of the %d x 64 candidates of the last "
                    "call %d crash (%d arenas run the re-scan), %d are done\n"
                    % (sys.argv[2], sim.cfg.range_max, sim.cfg.n_scan_stack, sim.cfg.add_scan_noise, float(std.min()), float(std.max()), E,
                       int((out["is_crash"] != 0).sum()), int((out["is_crash"] != 0).any(axis=1).sum()), int(out["done"].sum())))
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

window, reps = int(os.environ.get("NAVSIM_WINDOW", "100")), int(os.environ.get("NAVSIM_REPS", "5"))
lines = []
for world in ("c3", "c2"):
    for K, rows in ((9, "full"), (9, "scan"), (64, "full")):
        env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], lookahead_obs=K, lookahead_obs_params=dict(rows=rows)))
        env.reset()
        acts = actions(E)
        cand = acts[:K].permute(1, 0, 2).contiguous()

        def run(look, n, k0):
            for t in range(n):
                if look:
                    env.lookahead_obs(cand)
                env.step(acts[(k0 + t) % 64])

        run(True, 20, 0)
        torch.cuda.synchronize()
        times = {False: [], True: []}
        k0 = 20
        for r in range(reps):
            for look in (False, True):                       # alternating: the two share whatever else the machine does
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(look, window, k0)
                torch.cuda.synchronize()
                times[look].append((time.perf_counter() - t0) / window * 1e6)
                k0 += window
        off, on = np.median(times[False]), np.median(times[True])
        lines.append("(2) NavGymEnv on the %s-shaped world, %d arenas, K = %d, rows='%s', %d windows of %d steps each way, alternating: "
                     "step() alone median %.1f us (min %.1f, max %.1f); lookahead_obs() + step() %.1f us (min %.1f, max %.1f): + %.1f us, x %.3f"
                     % (world, E, K, rows, reps, window, off, min(times[False]), max(times[False]), on, min(times[True]), max(times[True]),
                        on - off, on / off))
        print(lines[-1], flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
