"""TEST INFRASTRUCTURE (GPU): navsim_lookahead through the C ABI into sentinel-filled outputs, a simulator's state saved and put
back, and the small worlds of tests/test_gpu_lookahead.py."""
import ctypes as C

import numpy as np

from gpu_support import device_world, host_arrays, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.LOOKAHEAD_OUT)
STEP_KEYS = ("reward", "done", "is_success", "is_crash", "distance")       # what navsim_step returns too
MAPS = ("field", "field_overflow", "rect_table", "rect_index", "costmap")  # read-only in a step: not saved


def call(gpu, cfg, st, actions, R, ped_cmd=None, skip=None):
    """navsim_lookahead into sentinel-filled outputs -> NumPy arrays.  actions: [E,K,2] float64."""
    torch, E = gpu.torch, cfg.n_envs
    actions = np.ascontiguousarray(actions, np.float64)
    K = actions.shape[1]
    out = {}
    for k, (dtype, tail) in abi.LOOKAHEAD_OUT.items():
        shape = (E,) + tuple(K if s == "K" else s for s in tail)
        out[k] = torch.full(shape, 77, dtype=getattr(torch, dtype), device=gpu.dev)
    o = abi.NavsimLookaheadOut(**{k: v.data_ptr() for k, v in out.items()})
    p = abi.NavsimLookaheadParams(n_actions=K, range=float(R))
    t_act = to_device(gpu, actions)
    t_cmd = None if ped_cmd is None else to_device(gpu, np.ascontiguousarray(ped_cmd, np.float64))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_lookahead(C.byref(cfg), C.byref(st), C.byref(p), t_act.data_ptr(),
                                         None if t_cmd is None else t_cmd.data_ptr(), None if t_skip is None else t_skip.data_ptr(),
                                         C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def save_state(g):
    return {k: v.clone() for k, v in g.t.items() if k not in MAPS}


def load_state(g, saved):
    for k, v in saved.items():
        g.t[k].copy_(v)


def room(E, H, W, ring, block):
    """Walled rooms [E,H,W] with one block (x0, x1, y0, y1 in cells) in every arena."""
    occ = np.zeros((E, H, W), np.uint8)
    occ[:, :ring] = 1; occ[:, -ring:] = 1; occ[:, :, :ring] = 1; occ[:, :, -ring:] = 1
    x0, x1, y0, y1 = block
    occ[:, y0:y1, x0:x1] = 1
    return occ


def place(g, cfg, e, x, y, th=0.0, goal=None):
    """Robot of arena e at (x, y, th) in metres, standing (prev_pose the same); goal: (dx, dy) from there."""
    t = g.t
    pose = to_device(g, np.array([x, y, th]))
    t["robot_pose"][e] = pose
    t["prev_pose"][e] = pose
    if goal is not None:
        t["robot_goal"][e] = to_device(g, np.array([x + goal[0], y + goal[1]]))


def sim_world(gpu, cfg, occ, n_peds, **kw):
    """A NavSim over make_world's arrays with the Keti thresholds, first observation taken -> g (NavSim copies cfg: read g.cfg)."""
    arrays = device_world(gpu, cfg, occ, n_peds, **dict(dict(min_goal_dist=1.5, max_goal_dist=4.0, robot_clearance=0.9), **kw))
    g = gpu.sim.NavSim(cfg, arrays)
    g.host0 = host_arrays(arrays, occ)                 # the oracle's copy of the world as it was made (fresh_oracle)
    g.reset_obs()
    g.torch, g.dev = gpu.torch, gpu.dev                # (to_device(g, ...) then works like to_device(gpu, ...))
    return g
