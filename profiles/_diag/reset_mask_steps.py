"""env.reset(mask) with 1/16 of the arenas masked: the env's default reset path (staged worlds, navsim_reset_install) against
pregen_pipeline=0 (navsim_restart + navsim_reset_obs + navsim_regen in chunks), the two envs alternating in one process.
A host clock around the call, which ends in a device synchronise; the median of NAVSIM_CALLS calls after warm-up, NAVSIM_BETWEEN
steps between calls so that the passes restage.  Also the steady env-steps/s of both envs between resets.
NAVSIM_WORLD = c5 (512 arenas, Husky, 1081 beams, 500 x 500 outdoor maps, 20 pedestrians) | refdef (the reference's own
configuration, 1024 arenas); NAVSIM_ENVS overrides the arena count."""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
import numpy as np
import torch, nav_gym_env

world = os.environ.get("NAVSIM_WORLD", "c5")
calls, between = int(os.environ.get("NAVSIM_CALLS", "24")), int(os.environ.get("NAVSIM_BETWEEN", "12"))
if world == "c5":
    E = int(os.environ.get("NAVSIM_ENVS", "512"))
    kw = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, randomize_maps=True, pedestrian_model="sfm", num_humans=20,
              robot_type="husky", plan_paths=False, device="cuda:0", seed=1234)
    lin_hi, rot_hi = 1.0, 2.0
else:
    E = int(os.environ.get("NAVSIM_ENVS", "1024"))
    kw = dict(num_envs=E, map_size="reference", randomize_maps=True, device="cuda:0", seed=1234)
    lin_hi, rot_hi = 0.5, 0.64
envs = {"staged": nav_gym_env.make("NavGym-v0", **kw), "pregen_pipeline=0": nav_gym_env.make("NavGym-v0", pregen_pipeline=0, **kw)}
for env in envs.values():
    env.reset()
assert envs["staged"].pregen_pipeline > 0 and envs["pregen_pipeline=0"].pregen_pipeline == 0
g = torch.Generator(device="cuda:0"); g.manual_seed(78)
acts = torch.rand((64, E, 2), generator=g, device="cuda:0", dtype=torch.float64)
acts[..., 0] *= lin_hi; acts[..., 1] = (acts[..., 1] * 2.0 - 1.0) * rot_hi
rng = np.random.default_rng(5)
warm = 4
reset_s = {k: [] for k in envs}
step_s = {k: [] for k in envs}
late = []
k_act = 0
for c in range(warm + calls):
    mask = np.zeros(E, bool); mask[rng.choice(E, E // 16, replace=False)] = True
    for name, env in envs.items():                       # the two envs alternately: the same steps, the same masks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(between):
            env.step(acts[(k_act + t) % 64])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        env.reset(mask)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if c >= warm:
            step_s[name].append((t1 - t0) / between); reset_s[name].append(t2 - t1)
            if name == "staged":
                late.append(int(env.sim.rs_late.sum().item()))
    k_act += between
print("world %s, %d arenas, reset(mask) of %d arenas, %d calls after %d warm-up calls, %d steps between calls"
      % (world, E, E // 16, calls, warm, between))
for name, env in envs.items():
    r, s = np.array(reset_s[name]) * 1e6, np.array(step_s[name])
    print("  %-18s reset(mask): median %8.1f us (min %8.1f, max %8.1f); steps between resets: %.2f M env-steps/s (median step %.1f us); counters %s"
          % (name, np.median(r), r.min(), r.max(), E / np.median(s) / 1e6, np.median(s) * 1e6, env.counters()))
print("  staged: arenas per call whose world was not staged (regenerated on the spot): median %d, max %d of %d"
      % (int(np.median(late)), max(late), E // 16))
for env in envs.values():
    env.close()
