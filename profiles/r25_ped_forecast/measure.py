"""What the pedestrian forecast (navsim_ped_forecast, NavGymEnv(ped_forecast=H)) costs, and how far the constant-velocity model
lies from the true one.  Appends to profiles/r25_ped_forecast/summary.txt (NAVSIM_OUT overrides the directory; NAVSIM_TAG names
the library in the lines, e.g. the one-wavefront build).

    python profiles/r25_ped_forecast/measure.py --calls           # c3-shaped world: reset() + ten steps, then for model = true,
                                                                  # const_vel and H = 8, 16, 32 ten ped_forecast() calls, nothing
                                                                  # else: run it under rocprofv3 --kernel-trace --output-format csv
    python profiles/r25_ped_forecast/measure.py --kernels TRACE   # (1) the kernels of such a run (its kernel_trace.csv) beside the
                                                                  # step kernel
    python profiles/r25_ped_forecast/measure.py pair              # (2) NavGymEnv: step() with the forecast on against off, two
                                                                  # environments over the same world, alternating windows
    python profiles/r25_ped_forecast/measure.py fact              # (3) 64 outdoor arenas, 8 social-force pedestrians, 150 steps:
                                                                  # the displacement of const_vel from true at h = H - 1
    python profiles/r25_ped_forecast/measure.py --bench FILE      # (4) the lines of an alternating bench.py run (NEW / PARENT + JSON)
"""
import csv, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r25_ped_forecast"))
os.makedirs(OUT, exist_ok=True)
SUMMARY = os.path.join(OUT, "summary.txt")
TAG = os.environ.get("NAVSIM_TAG", "one wavefront per arena (the default build)")
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
CALLS = 10
COMBOS = [(m, H) for m in ("true", "const_vel") for H in (8, 16, 32)]


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
        f.write("\n(4) feature off: bench.py --gpus 1 --steps 200 --warmup 20 on this library (NEW) and on the parent commit's (PARENT), "
                "alternating, M env-steps/s (raw lines: bench_ab.txt):\n  NEW    %s   median %.2f\n  PARENT %s   median %.2f   spread %.2f\n"
                "  median difference %+.2f M (%+.2f %%): %s the parent's own run-to-run spread.\n"
                % ("  ".join("%.2f" % v for v in new), median(new), "  ".join("%.2f" % v for v in par), median(par), spread, diff,
                   100 * diff / median(par), "inside" if abs(diff) <= spread else "OUTSIDE"))
    sys.exit(0)

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    fore, step, name_ = [], [], ""
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            item = (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
            if "ped_forecast_kernel" in name:
                fore.append(item); name_ = name
            if "navsim_step" in name:
                step.append(item[1])
    fore.sort()
    step_us = median(step)
    with open(SUMMARY, "a") as f:
        f.write("\n(1) %s; c3-shaped world, %d arenas x 20 pedestrians, robot = hold: kernel times from rocprofv3 --kernel-trace, median of "
                "%d launches each; the step kernel's median over %d launches in the same trace is %.2f us\n" % (TAG, E, CALLS, len(step), step_us))
        for i, (m, H) in enumerate(COMBOS):
            us = median([u for _, u in fore[CALLS * i:CALLS * i + CALLS]])
            f.write("  model = %-9s H = %2d  %9.2f us  = %6.2f us a forecast step  = x %.2f of the step kernel\n" % (m, H, us, us / H, us / step_us))
        f.write("  kernel: %s\n" % name_.replace("(anonymous namespace)::", "")[:150])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

C3 = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234)


def actions(n, T):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((n, T, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


if len(sys.argv) > 1 and sys.argv[1] == "--calls":
    env = nav_gym_env.make("NavGym-v0", **C3)
    env.reset()
    acts = actions(E, 10)
    for t in range(10):
        env.step(acts[:, t].contiguous())
    sim, notes = env.sim, []
    for m, H in COMBOS:
        sim.enable_ped_forecast(H, dict(robot="hold", model=m))
        for _ in range(CALLS):
            out = sim.ped_forecast()
        torch.cuda.synchronize()
        notes.append("%s H = %d: mean exact_steps %.2f" % (m, H, float(out["exact_steps"].double().mean().item())))
    with open(SUMMARY, "a") as f:
        f.write("\n%s: ten ped_forecast() calls from one state per setting: %s\n" % (TAG, "; ".join(notes)))
    env.close()
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "fact":
    H = 16
    env = nav_gym_env.make("NavGym-v0", num_envs=64, n_beams=256, map_size=400, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=8,
                           device="cuda:0", seed=7)
    env.reset()
    sim = env.sim
    products = {m: sim._ped_forecast_product(H, 0, i) for i, m in enumerate(("true", "const_vel"))}      # robot = hold
    acts = actions(64, 150)
    err = torch.zeros(H, dtype=torch.float64, device="cuda:0")
    count = 0
    for t in range(150):
        env.step(acts[:, t].contiguous())
        rows = {}
        for m, p in products.items():
            sim.products["ped_forecast"] = p
            rows[m] = sim.ped_forecast()["pose"][..., :2]
        live = (torch.arange(sim.cfg.max_peds, device="cuda:0")[None, :] < sim.t["n_peds"][:, None])[:, None, :]      # [E,1,N]
        d = (rows["true"] - rows["const_vel"]).norm(dim=3)                                                       # [E,H,N]
        err += (d * live).sum(dim=(0, 2))
        count += int(live.sum().item())
    err = (err / count).cpu().numpy()
    line = ("(3) 64 outdoor arenas (400 x 400 cells), 8 social-force pedestrians each, 150 steps of random actions, robot = hold: mean "
            "displacement of const_vel from true over %d pedestrian-steps at h = 7 (1.6 s ahead): %.3f m; at h = 15 (3.2 s): %.3f m; at "
            "h = 0: %.4f m" % (count, err[7], err[15], err[0]))
    print(line, flush=True)
    with open(SUMMARY, "a") as f:
        f.write("\n" + line + "\n")
    env.close()
    sys.exit(0)

lines = []
for H, model in ((16, "true"), (16, "const_vel")):
    envs = {False: nav_gym_env.make("NavGym-v0", **C3),
            True: nav_gym_env.make("NavGym-v0", **dict(C3, ped_forecast=H, ped_forecast_params=dict(model=model)))}
    acts = actions(E, 64)
    for env in envs.values():
        env.reset()

    def run(on, n, k0):
        for t in range(n):
            envs[on].step(acts[:, (k0 + t) % 64].contiguous())

    run(True, 3, 0); run(False, 3, 0)
    torch.cuda.synchronize()
    times, window, reps, k0 = {False: [], True: []}, 10, 3, 3
    for r in range(reps):
        for on in (False, True):                         # alternating: the two share whatever else the machine does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(on, window, k0)
            torch.cuda.synchronize()
            times[on].append((time.perf_counter() - t0) / window * 1e6)
        k0 += window
    off, on_ = np.median(times[False]), np.median(times[True])
    lines.append("(2) %s; NavGymEnv on the c3-shaped world, %d arenas, ped_forecast = %d, model = %s, robot = hold, %d windows of %d steps "
                 "each way, alternating: step() with the forecast off median %.1f us (min %.1f, max %.1f); on %.1f us (min %.1f, max "
                 "%.1f): + %.1f us, x %.2f" % (TAG, E, H, model, reps, window, off, min(times[False]), max(times[False]), on_,
                                             min(times[True]), max(times[True]), on_ - off, on_ / off))
    print(lines[-1], flush=True)
    for env in envs.values():
        env.close()
    del envs
    torch.cuda.empty_cache()
with open(SUMMARY, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
