"""TEST INFRASTRUCTURE (GPU): navsim_dwa through the C ABI into sentinel-filled outputs and the comparison of its outputs with
those of tests/dwa_spec.py -- for tests/test_gpu_dwa.py and the geometries of tests/test_gpu_map_geometry.py."""
import ctypes as C

import numpy as np

import dwa_spec as spec
import gpu_support
from gpu_support import eq, same_bits, to_device
from nav_gym_amd import abi

KEYS = spec.KEYS
BITS = ("twist", "action", "scores", "clearance")            # compared as raw bits; best, status and first_hit by value


def c_params(gpu, cfg, params):
    return gpu.sim.dwa_params(cfg, params)


def call(gpu, cfg, st, params, subgoal=None, skip=None, want_rc=0, n_out=None, with_scores=True, n_cand=None):
    """navsim_dwa into sentinel-filled outputs (n_out rows; None: cfg.n_envs) -> NumPy arrays."""
    p = c_params(gpu, cfg, params) if isinstance(params, dict) else params
    torch, E = gpu.torch, cfg.n_envs if n_out is None else n_out
    Cn = p.n_v * p.n_w if n_cand is None else n_cand
    out = dict(twist=torch.full((E, 2), 777.0, dtype=torch.float64, device=gpu.dev),
               action=torch.full((E, 2), 777.0, dtype=torch.float64, device=gpu.dev),
               clearance=torch.full((E,), 777.0, dtype=torch.float32, device=gpu.dev),
               best=torch.full((E,), 7777, dtype=torch.int32, device=gpu.dev),
               status=torch.full((E,), 77, dtype=torch.uint8, device=gpu.dev),
               scores=torch.full((E, Cn), 777.0, dtype=torch.float64, device=gpu.dev),
               first_hit=torch.full((E, Cn), 7777, dtype=torch.int32, device=gpu.dev))
    o = abi.NavsimDwaOut(**{k: (v.data_ptr() if with_scores or k not in ("scores", "first_hit") else None) for k, v in out.items()})
    t_sub = None if subgoal is None else to_device(gpu, np.asarray(subgoal, np.float32))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_dwa(C.byref(cfg), C.byref(st), C.byref(p), None if subgoal is None else t_sub.data_ptr(),
                                   None if skip is None else t_skip.data_ptr(), C.byref(o), None)
    assert rc == want_rc, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def untouched(dev, keys=KEYS):
    for k in keys:
        assert (dev[k] == (7777 if k in ("best", "first_hit") else (77 if k == "status" else 777.0))).all(), k


def same(dev, want, what, keys=KEYS):
    for k in keys:
        a, b = dev[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        (same_bits if k in BITS else eq)(a, b, "%s: %s" % (what, k))


STATE = dict(robot_pose=np.float64, robot_goal=np.float64, prev_action=np.float64)
PED_STATE = dict(n_peds=np.int32, ped_pose=np.float64, ped_vel=np.float64)


def device_state(gpu, cfg, occ, w, overflow=False, map_slot=None, peds=True):
    return gpu_support.device_state(gpu, cfg, occ, w, dict(STATE, **PED_STATE) if peds else STATE, overflow, map_slot)
