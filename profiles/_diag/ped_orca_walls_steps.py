"""c3-shaped world (4096 arenas, 20 pedestrians, 1081 beams, 500 x 500 maps): the time of one navsim_ped_orca call and of one
navsim_ped_orca_walls call (max_rects 8, time_horizon_obst 2 and 5) on the state the world has after 30 steps, by device events
around 200 back-to-back calls, seven rounds, the variants alternating inside every round.  NAVSIM_PARENT_LIB=<path of a
libnavsim_hip.so built from the parent commit> adds that library's navsim_ped_orca to the rounds (same process, same state,
same ABI): the K = 0 instantiation must not have moved.  Prints median (min .. max) microseconds per call.
(profiles/_diag/ped_orca_steps.py is the end-to-end rate through NavGymEnv.step().)"""
import ctypes as C
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
import numpy as np
import torch, nav_gym_env
from nav_gym_amd import abi, sim as simmod

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
N = int(os.environ.get("NAVSIM_PEDS", "20"))
CALLS, ROUNDS, WARM = int(os.environ.get("NAVSIM_CALLS", "200")), 7, 30
DEV = "cuda:0"

env = nav_gym_env.make("NavGym-v0", num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, device=DEV, seed=1234,
                       pedestrian_model="orca", num_humans=N, plan_paths=False)
env.reset()
g = torch.Generator(device=DEV); g.manual_seed(78)
acts = torch.rand((WARM, E, 2), generator=g, device=DEV, dtype=torch.float64)
acts[..., 0] *= 0.5; acts[..., 1] = acts[..., 1] * 1.28 - 0.64
for t in range(WARM):
    env.step(acts[t])
sim = env.sim
dropped = torch.zeros((E, N), dtype=torch.int32, device=DEV)
params = {tho: simmod.ped_orca_params(sim.cfg, dict(time_horizon_obst=tho), env.robot_type) for tho in (2.0, 5.0)}
variants = {"navsim_ped_orca": lambda: sim.ped_orca(params[5.0]),
            "navsim_ped_orca_walls K 8, horizon 2": lambda: sim.ped_orca_walls(params[2.0], 8, dropped),
            "navsim_ped_orca_walls K 8, horizon 5": lambda: sim.ped_orca_walls(params[5.0], 8, dropped)}
parent = os.environ.get("NAVSIM_PARENT_LIB")
if parent:
    P = C.CDLL(parent)
    assert P.navsim_abi_version() == abi.ABI_VERSION
    P.navsim_ped_orca.argtypes = [C.POINTER(abi.NavsimConfig), C.POINTER(abi.NavsimState), C.POINTER(abi.NavsimPedOrcaParams),
                                  C.c_void_p, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def parent_call():
        rc = P.navsim_ped_orca(C.byref(sim.cfg), C.byref(sim.st), C.byref(params[5.0]), sim.t["ped_cmd"].data_ptr(), stream)
        assert rc == 0, rc
    variants = dict({"navsim_ped_orca, parent commit": parent_call}, **variants)
    # same answer from both libraries on this state
    sim.ped_orca(params[5.0]); a = sim.t["ped_cmd"].clone()
    parent_call(); torch.cuda.synchronize()
    assert torch.equal(a, sim.t["ped_cmd"]), "the parent's navsim_ped_orca answers differently"

times = {k: [] for k in variants}
for k, f in variants.items():                                       # every shape warmed
    for _ in range(20):
        f()
torch.cuda.synchronize()
for r in range(ROUNDS):
    for k, f in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            f()
        b.record()
        torch.cuda.synchronize()
        times[k].append(a.elapsed_time(b) / CALLS * 1e3)
live = int(sim.t["n_peds"].sum().item())
print("%d arenas, %d live pedestrians; %d calls per round, %d rounds; microseconds per call: median (min .. max)"
      % (E, live, CALLS, ROUNDS))
for k, v in times.items():
    print("%-40s %8.1f (%.1f .. %.1f)" % (k, float(np.median(v)), min(v), max(v)), flush=True)
print("dropped > 0 at horizon 5: %.1f %% of the live pedestrians" % (100.0 * float((dropped > 0).sum().item()) / max(live, 1)))
env.close()
