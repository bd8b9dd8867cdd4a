"""What the Python around the four launches behind the step costs the host per step: NavGymEnv's run of observed pedestrians,
goal path, local planner and local map, through NavSim's four call methods, with the library's entry points replaced by
functions that return at once.  No GPU: the buffers lie in host memory, nothing is launched.  What is left is exactly the code
the record and the run list rewrote -- the native calls are the same in both trees, their cost is not in this figure.

    python profiles/r19_step_products/host_overhead.py TREE LABEL     # TREE: the root of a checkout (its package is used)

One process measures one tree; parent and this tree are run alternately.  4096 arenas (the figure does not depend on it: nothing
is computed), same-step auto-reset, the buffer parity flipped before every run as a step does.  A window is NAVSIM_WINDOW (20000)
runs; prints the median, fastest and slowest of NAVSIM_REPS (15) windows in us per run.
"""
import os, sys, time

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, "nav-gym_amd")]
import numpy as np
import torch, nav_gym_amd
from nav_gym_amd import abi, registry, sim as simmod

assert os.path.abspath(nav_gym_amd.__file__).startswith(ROOT), nav_gym_amd.__file__
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
window, reps = int(os.environ.get("NAVSIM_WINDOW", "20000")), int(os.environ.get("NAVSIM_REPS", "15"))
env = registry.make("NavGym-v0", num_envs=E, n_beams=64, map_size=100, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=6, seed=1,
                    plan_paths=False, observe_humans=6, goal_path=True, local_planner="dwa", observe_local_map=32,
                    local_map_params=dict(visible_only=True))


class Library(object):                                    # the entry points the four products call: nothing happens
    navsim_ped_observe = navsim_goal_path = navsim_dwa = navsim_local_map = staticmethod(lambda *a: 0)
    navsim_goal_field_bytes = staticmethod(lambda cfg: 1)


simmod._stream = lambda: None
s = simmod.NavSim.__new__(simmod.NavSim)                  # the state the enable_* calls and the four call methods read, no more
s.lib, s.cfg, s.st, s.device, s.cur, s.products = Library, env.cfg.copy(), abi.NavsimState(), torch.device("cpu"), 0, {}
s.out_buf = [{"done": torch.zeros(E, dtype=torch.uint8)} for _ in range(2)]
s.enable_ped_observe(dict(max_obs=6)); s.enable_goal_path(); s.enable_dwa(); s.enable_local_map(32)
env.sim, env._bool = s, torch.bool
if hasattr(env, "_run_products"):
    run = env._run_products
else:                                                     # the parent: the four calls as its step() writes them out
    def run():
        env._observe(); env._goal_path(); env._plan(); env._local_map()
times = []
for r in range(reps + 1):
    t0 = time.perf_counter()
    for _ in range(window):
        s.cur ^= 1
        run()
    times.append((time.perf_counter() - t0) / window * 1e6)
times = times[1:]                                         # (the first window warms up)
print("%-6s us per run of the four products: median %6.3f  min %6.3f  max %6.3f   (%d windows of %d runs)"
      % (sys.argv[2], np.median(times), min(times), max(times), reps, window), flush=True)
