"""What the MPPI local planner (navsim_mppi, NavGymEnv(local_planner='mppi')) costs.  Appends to profiles/r24_mppi/summary.txt
(NAVSIM_OUT overrides the directory).

    python profiles/r24_mppi/measure.py --calls c3|c2          # reset() + ten steps with goal_path on, then at the defaults and at
                                                               # (K, H) = (64, 16): ten mppi() calls, nothing else: run it under
                                                               # rocprofv3 --kernel-trace --output-format csv
    python profiles/r24_mppi/measure.py --kernels TRACE c3|c2  # (1) the kernels of such a run (its kernel_trace.csv): sample, rollout
                                                               # and update beside the step kernel
    python profiles/r24_mppi/measure.py pair                   # (2) NavGymEnv: step() with the planner on against off, two
                                                               # environments over the same world, alternating windows
    python profiles/r24_mppi/measure.py --off c2               # reset() + ten steps with the feature off (for the off trace)
    python profiles/r24_mppi/measure.py --bench FILE           # (3) the lines of an alternating bench.py run (NEW / PARENT + JSON)
"""
import csv, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r24_mppi"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
CALLS = 10


def combos():
    from nav_gym_amd import lib, sim
    d = sim.mppi_defaults(lib.default_config(n_envs=1))
    return ((d["n_samples"], d["horizon"]), (64, 16))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


if len(sys.argv) > 2 and sys.argv[1] == "--bench":
    runs, tag = {"NEW": [], "PARENT": []}, None
    for line in open(sys.argv[2]):
        line = line.strip()
        if line in runs:
            tag = line
        elif line.startswith("{") and tag:
            runs[tag].append(json.loads(line)["value"] / 1e6)
    new, par = runs["NEW"], runs["PARENT"]
    spread = max(par) - min(par)
    diff = median(new) - median(par)
    with open(SUMMARY, "a") as f:
        f.write("\n(3) feature off: bench.py --gpus 1 --steps 200 --warmup 20 on this library (NEW) and on the parent commit's (PARENT), "
                "alternating, M env-steps/s (raw lines: bench_ab.txt):\n  NEW    %s   median %.2f\n  PARENT %s   median %.2f   spread %.2f\n"
                "  median difference %+.2f M (%+.2f %%): %s the parent's own run-to-run spread.\n"
                % ("  ".join("%.2f" % v for v in new), median(new), "  ".join("%.2f" % v for v in par), median(par), spread, diff,
                   100 * diff / median(par), "inside" if abs(diff) <= spread else "OUTSIDE"))
    sys.exit(0)

if len(sys.argv) > 3 and sys.argv[1] == "--kernels":
    kinds = {"mppi_sample": [], "rollout_kernel": [], "mppi_update": []}
    step, names = [], {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            item = (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
            for k in kinds:
                if k in name:
                    kinds[k].append(item)
                    names[k] = name
            if "navsim_step" in name:
                step.append(item[1])
    for v in kinds.values():
        v.sort()
    step_us = median(step)
    with open(SUMMARY, "a") as f:
        f.write("\n(1) %s-shaped world, %d arenas x 1081 beams: kernel times from rocprofv3 --kernel-trace; the step kernel's median over "
                "%d launches is %.2f us\n" % (sys.argv[3], E, len(step), step_us))
        if sys.argv[3].endswith("off"):
            f.write("  launches of kernels with 'mppi' in their name: %d; with 'rollout': %d\n"
                    % (len(kinds["mppi_sample"]) + len(kinds["mppi_update"]), len(kinds["rollout_kernel"])))
        else:
            for i, (K, H) in enumerate(combos()):
                med = {k: median([us for _, us in v[CALLS * i:CALLS * i + CALLS]]) for k, v in kinds.items() if v}
                total = sum(med.values())
                f.write("  K = %2d, H = %2d  sample %8.2f us (%.2f %%)  rollout %10.2f us (%.2f %%)  update %8.2f us (%.2f %%)  the call's kernels "
                        "%10.2f us = x %.1f of the step kernel\n"
                        % (K, H, med["mppi_sample"], 100 * med["mppi_sample"] / total, med["rollout_kernel"], 100 * med["rollout_kernel"] / total,
                           med["mppi_update"], 100 * med["mppi_update"] / total, total, total / step_us))
            for k, name in names.items():
                f.write("  kernel: %s\n" % name.replace("(anonymous namespace)::", "")[:150])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

WORLDS = dict(c3=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def actions(n, T):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((n, T, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 2 and sys.argv[1] in ("--calls", "--off"):
    on = sys.argv[1] == "--calls"
    env = nav_gym_env.make("NavGym-v0", **dict(WORLDS[sys.argv[2]], **(dict(goal_path=True) if on else {})))
    env.reset()
    acts = actions(E, 10)
    for t in range(10):
        env.step(acts[:, t].contiguous())
    if on:
        sim, notes = env.sim, []
        for K, H in combos():
            sim.enable_mppi(dict(n_samples=K, horizon=H), robot_type=env.robot_type)
            for _ in range(CALLS):
                out = sim.mppi(field=True)
            torch.cuda.synchronize()
            roll = sim.products["mppi"].extra["roll"]
            notes.append("K = %d, H = %d: mean length %.2f steps, mean ess %.1f, status 2 in %d arenas" %
                         (K, H, float(roll["length"].double().mean().item()), float(out["ess"].mean().item()), int((out["status"] == 2).sum().item())))
        with open(SUMMARY, "a") as f:
            f.write("\n%s: ten mppi() calls from one state (the plan is kept: rule 2), goal field on: %s\n" % (sys.argv[2], "; ".join(notes)))
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

lines = []
for world in ("c3", "c2"):
    for (K, H), window, reps in zip(combos(), (10, 8), (3, 3)):
        envs = {False: nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], goal_path=True)),
                True: nav_gym_env.make("NavGym-v0", **dict(WORLDS[world], goal_path=True, local_planner="mppi",
                                                           local_planner_params=dict(n_samples=K, horizon=H)))}
        acts = actions(E, 64)
        for env in envs.values():
            env.reset()

        def run(on, n, k0):
            for t in range(n):
                envs[on].step(acts[:, (k0 + t) % 64].contiguous())

        run(True, 3, 0); run(False, 3, 0)
        torch.cuda.synchronize()
        times = {False: [], True: []}
        k0 = 3
        for r in range(reps):
            for on in (False, True):                         # alternating: the two share whatever else the machine does
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(on, window, k0)
                torch.cuda.synchronize()
                times[on].append((time.perf_counter() - t0) / window * 1e6)
            k0 += window
        off, on_ = np.median(times[False]), np.median(times[True])
        lines.append("(2) NavGymEnv on the %s-shaped world, %d arenas, goal_path on, K = %d, H = %d, %d windows of %d steps each way, alternating: "
                     "step() with the planner off median %.1f us (min %.1f, max %.1f); on %.1f us (min %.1f, max %.1f): + %.1f us, x %.1f"
                     % (world, E, K, H, reps, window, off, min(times[False]), max(times[False]), on_, min(times[True]), max(times[True]),
                        on_ - off, on_ / off))
        print(lines[-1], flush=True)
        for env in envs.values():
            env.close()
        del envs
        torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
