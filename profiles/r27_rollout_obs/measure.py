"""What the rollout observations (navsim_rollout_obs, NavGymEnv(rollout_obs=K)) cost.  Appends to
profiles/r27_rollout_obs/summary.txt (NAVSIM_OUT overrides the directory).

    python profiles/r27_rollout_obs/measure.py --calls c3|c2          # reset() + ten steps, then for (K, H) = (16, 8) and (64, 16):
                                                                      # navsim_rollout at R = range_max, H launches of
                                                                      # navsim_lookahead_obs with rows='scan' at the same K, and
                                                                      # navsim_rollout_obs with rows 'last' and 'all', nothing else:
                                                                      # run it under rocprofv3 --kernel-trace --output-format csv
    python profiles/r27_rollout_obs/measure.py --kernels TRACE c3|c2  # (1) the kernels of such a run (its kernel_trace.csv) beside
                                                                      # the step kernel, the bytes written
    python profiles/r27_rollout_obs/measure.py pair                   # (2) NavGymEnv: rollout_obs() + step() against step() alone,
                                                                      # the same environment, alternating windows
    python profiles/r27_rollout_obs/measure.py --off c2               # reset() + ten steps with the feature off (for the off trace)
    python profiles/r27_rollout_obs/measure.py events c3|c2 TAG       # device-event times of the four rollout_obs shapes on the
                                                                      # library that is loaded (NAVSIM_LIB: a build with other bounds)
"""
import csv, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r27_rollout_obs"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
B = 1081
SHAPES = ((16, 8), (64, 16))
REPS = {(16, 8): 10, (64, 16): 5}
HBM_PEAK = 8.0e12                                                                          # bytes / s (MI355X, HBM3E)


def bytes_written(K, H, S, rows):
    """What an arena's K workgroups store at full length: the ten shared arrays (32 B a sequence-step, 41 B a sequence, the status
    byte), obs_last once per step (the in-place shift) and goals_last, and with rows 'all' every row and its goals once more."""
    D = S * B + 7
    per_seq = 41 + 32 * H + 4 * S * B * H + 28 + 16 + ((4 * D + 16) * H if rows == "all" else 0)
    return K * per_seq + 1


def groups_of():
    """The launches of --calls in their order: (kernel name part, K, H, what, launches per repetition, repetitions)"""
    out = []
    for K, H in SHAPES:
        n = REPS[(K, H)]
        out += [("rollout_kernel", K, H, "navsim_rollout(range_max)", 1, n), ("lookahead_obs_kernel", K, H, "H x lookahead_obs rows=scan", H, n),
                ("rollout_obs_kernel", K, H, "rollout_obs rows=last", 1, n), ("rollout_obs_kernel", K, H, "rollout_obs rows=all", 1, n)]
    return out


if len(sys.argv) > 3 and sys.argv[1] == "--kernels":
    found = {"rollout_obs_kernel": [], "rollout_kernel": [], "lookahead_obs_kernel": []}
    step = []
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            for part in found:                                  # ("rollout_kernel" is no part of "rollout_obs_kernel")
                if part in name:
                    found[part].append((int(row["Start_Timestamp"]), us, name))
                    break
            else:
                if "navsim_step" in name:
                    step.append(us)
    for v in found.values():
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
            f.write("  launches of kernels with 'rollout_obs' in their name: %d\n" % len(found["rollout_obs_kernel"]))
        else:
            at = {k: 0 for k in found}
            med = {}
            for part, K, H, what, per, n in groups_of():
                rows = found[part][at[part]:at[part] + per * n]
                at[part] += per * n
                if len(rows) < per * n:
                    f.write("  K = %2d, H = %2d, %s: %d of %d launches in the trace\n" % (K, H, what, len(rows), per * n))
                    continue
                grp = sorted(sum(us for _, us, _ in rows[i * per:(i + 1) * per]) for i in range(n))      # a repetition: `per` launches
                m = med[(K, H, what)] = grp[len(grp) // 2]
                line = "  K = %2d, H = %2d, %-28s median %10.2f us  min %10.2f  max %10.2f   %7.2f us a sequence-step   x %.1f of the step kernel" % (
                    K, H, what, m, grp[0], grp[-1], m / (K * H), m / step_us)
                if part == "rollout_obs_kernel":
                    nbytes = E * bytes_written(K, H, S, what.split("=")[1])
                    line += "   x %.3f of navsim_rollout(range_max), x %.3f of the H lookahead_obs launches   %.1f MB written at full length, %.1f GB/s (%.2f %% of the HBM peak)" % (
                        m / med[(K, H, "navsim_rollout(range_max)")], m / med[(K, H, "H x lookahead_obs rows=scan")], nbytes / 1e6, nbytes / m / 1e3,
                        100.0 * nbytes / (m * 1e-6) / HBM_PEAK)
                f.write(line + "\n")
            for v in found.values():
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


def sequences(acts, K, H):
    """[E,K,H,2]: sequence k repeats candidate k's action, turning the other way every fourth step"""
    seq = acts[:K].permute(1, 0, 2)[:, :, None, :].repeat(1, 1, H, 1)
    seq[:, :, 3::4, 1] *= -1.0
    return seq.contiguous()


def release(sim, name):
    sim.products.pop(name, None)
    torch.cuda.empty_cache()


if len(sys.argv) > 2 and sys.argv[1] in ("--calls", "--off"):
    on = sys.argv[1] == "--calls"
    env = nav_gym_env.make("NavGym-v0", **WORLDS[sys.argv[2]])
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    if on:
        sim = env.sim
        last = {}
        for K, H in SHAPES:
            n = REPS[(K, H)]
            seq = sequences(acts, K, H)
            sim.enable_rollout(K, H, dict(range=sim.cfg.range_max))
            for _ in range(n):
                sim.rollout(seq)
            torch.cuda.synchronize()
            release(sim, "rollout")
            sim.enable_lookahead_obs(K, dict(rows="scan"))
            cands = [seq[:, :, h].contiguous() for h in range(H)]
            for _ in range(n):
                for h in range(H):
                    sim.lookahead_obs(cands[h])
            torch.cuda.synchronize()
            release(sim, "lookahead_obs")
            del cands
            for rows in ("last", "all"):
                sim.enable_rollout_obs(K, H, dict(rows=rows))
                for _ in range(n):
                    out = sim.rollout_obs(seq)
                torch.cuda.synchronize()
                last[(K, H)] = dict(length=out["length"].float().mean().item(), crash=int(((out["outcome"] & 2) != 0).sum().item()),
                                    ended=int((out["length"] < H).sum().item()))
                release(sim, "rollout_obs")
        std = sim.t["scan_noise_std"]
        with open(os.path.join(OUT, "calls_%s.json" % sys.argv[2]), "w") as f:
            json.dump(dict(S=int(sim.cfg.n_scan_stack)), f)
        with open(SUMMARY, "a") as f:
            f.write("\n%s: range_max %.1f m, stack of %d, add_scan_noise %d, noise std in [%.4f, %.4f] m; %s\n"
                    % (sys.argv[2], sim.cfg.range_max, sim.cfg.n_scan_stack, sim.cfg.add_scan_noise, float(std.min()), float(std.max()),
                       "; ".join("(K, H) = (%d, %d): mean length %.2f, %d of %d sequences are shorter than H, %d end in a crash (the re-scan; a crash at the last step leaves the length at H)"
                                 % (K, H, v["length"], v["ended"], E * K, v["crash"]) for (K, H), v in last.items())))
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

if len(sys.argv) > 3 and sys.argv[1] == "events":
    env = nav_gym_env.make("NavGym-v0", **WORLDS[sys.argv[2]])
    env.reset()
    acts = actions(E)
    for t in range(10):
        env.step(acts[t])
    sim = env.sim
    parts = []
    for K, H in SHAPES:
        seq = sequences(acts, K, H)
        for rows in ("last", "all"):
            sim.enable_rollout_obs(K, H, dict(rows=rows))
            sim.rollout_obs(seq)
            torch.cuda.synchronize()
            ms = []
            for _ in range(REPS[(K, H)]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); sim.rollout_obs(seq); e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            parts.append("(%d, %d) %s %.2f ms (min %.2f, max %.2f)" % (K, H, rows, float(np.median(ms)), min(ms), max(ms)))
            release(sim, "rollout_obs")
    line = "(0b) %s on the %s-shaped world, one rollout_obs() launch between two device events, median: %s" % (sys.argv[3], sys.argv[2], "; ".join(parts))
    print(line, flush=True)
    with open(SUMMARY, "a") as f:
        f.write(line + "\n")
    env.close()
    sys.exit(0)

window, reps = int(os.environ.get("NAVSIM_WINDOW", "20")), int(os.environ.get("NAVSIM_REPS", "3"))
lines = []
for world in ("c3", "c2"):
    for K, H, rows in ((16, 8, "last"), (16, 8, "all"), (64, 16, "last")):
        env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], rollout_obs=K, rollout_obs_params=dict(horizon=H, rows=rows)))
        env.reset()
        acts = actions(E)
        seq = sequences(acts, K, H)

        def run(look, n, k0):
            for t in range(n):
                if look:
                    env.rollout_obs(seq)
                env.step(acts[(k0 + t) % 64])

        run(True, 5, 0)
        torch.cuda.synchronize()
        times = {False: [], True: []}
        k0 = 5
        for r in range(reps):
            for look in (False, True):                       # alternating: the two share whatever else the machine does
                n = window * (10 if not look else 1)         # (step() alone is some hundred times shorter: ten times the steps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(look, n, k0)
                torch.cuda.synchronize()
                times[look].append((time.perf_counter() - t0) / n * 1e6)
                k0 += n
        off, on = np.median(times[False]), np.median(times[True])
        lines.append("(2) NavGymEnv on the %s-shaped world, %d arenas, (K, H) = (%d, %d), rows='%s', %d windows each way (%d steps with, %d without), "
                     "alternating: step() alone median %.1f us (min %.1f, max %.1f); rollout_obs() + step() %.2f ms (min %.2f, max %.2f): x %.1f"
                     % (world, E, K, H, rows, reps, window, 10 * window, off, min(times[False]), max(times[False]), on / 1e3, min(times[True]) / 1e3,
                        max(times[True]) / 1e3, on / off))
        print(lines[-1], flush=True)
        env.close()
        del env, seq
        torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
