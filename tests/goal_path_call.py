"""TEST INFRASTRUCTURE (GPU): navsim_goal_path through the C ABI into sentinel-filled outputs and a navsim_goal_field of the
test's own, the comparison of its outputs with the specification's, and the adapter of tests/goal_path_spec.py -- for
tests/test_gpu_goal_path.py and the geometries of tests/test_gpu_map_geometry.py."""
import ctypes as C

import numpy as np

import goal_path_spec as spec
import gpu_support
from gpu_support import eq, same_bits, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.GOAL_PATH_OUT)
INF = spec.INF
H3 = 3 * 0.05                        # the least hard_clearance: three map cells (0.15000000000000002, as the entry computes it)


def c_params(**kw):
    p = dict(spec.DEFAULT, **kw)
    return abi.NavsimGoalPathParams(hard_clearance=p["hard_clearance"], clearance=p["clearance"], lookahead=p["lookahead"],
                                    band_cost=p["band_cost"])


class GoalField:
    """A navsim_goal_field of its own: dist filled with a sentinel, the keys -1, the counter 0."""

    def __init__(self, gpu, cfg):
        torch = gpu.torch
        Hc, Wc = spec.grid_shape(cfg)
        self.dist = torch.full((cfg.n_envs, Hc, Wc), 0x7777, dtype=torch.int16, device=gpu.dev)
        self.key = torch.full((cfg.n_envs, 3), -1, dtype=torch.int64, device=gpu.dev)
        self.rebuilds = torch.zeros(1, dtype=torch.int64, device=gpu.dev)
        self.c = abi.NavsimGoalField(dist=self.dist.data_ptr(), key=self.key.data_ptr(), rebuilds=self.rebuilds.data_ptr())

    def host(self):
        return self.dist.cpu().numpy().view(np.uint16)

    def count(self):
        return int(self.rebuilds.item())


def call(gpu, cfg, st, params, field=None, rebuild=None, skip=None, want_rc=0, n_out=None):
    """navsim_goal_path into sentinel-filled outputs (n_out rows; None: cfg.n_envs) -> NumPy arrays (+ 'dist', and the field
    object as 'field')."""
    p = c_params(**params) if isinstance(params, dict) else params
    torch, E = gpu.torch, cfg.n_envs if n_out is None else n_out
    field = field or GoalField(gpu, cfg)
    out = dict(distance=torch.full((E,), 777.0, dtype=torch.float32, device=gpu.dev),
               subgoal=torch.full((E, 2), 777.0, dtype=torch.float32, device=gpu.dev),
               status=torch.full((E,), 77, dtype=torch.uint8, device=gpu.dev))
    o = abi.NavsimGoalPathOut(**{k: v.data_ptr() for k, v in out.items()})
    t_rebuild = None if rebuild is None else to_device(gpu, np.asarray(rebuild, np.uint8))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_goal_path(C.byref(cfg), C.byref(st), C.byref(p), None if rebuild is None else t_rebuild.data_ptr(),
                                         None if skip is None else t_skip.data_ptr(), C.byref(field.c), C.byref(o), None)
    assert rc == want_rc, rc
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(dist=field.host(), field=field)
    return res


def same(dev, want, what, arenas=None):
    """status, dist, distance and subgoal (raw bits) of `arenas` (None: all)."""
    sel = slice(None) if arenas is None else np.asarray(arenas)
    for k in ("status", "dist", "distance", "subgoal"):
        a, b = dev[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        (same_bits if k in ("distance", "subgoal") else eq)(a[sel], b[sel], "%s: %s" % (what, k))


STATE = dict(robot_pose=np.float64, robot_goal=np.float64, episode=np.int64)


def device_state(gpu, cfg, occ, w, overflow=False, map_slot=None):
    return gpu_support.device_state(gpu, cfg, occ, w, STATE, overflow, map_slot)


def answer(cfg, fields, w, params, **kw):
    return spec.goal_path(cfg, fields, w["robot_pose"], w["robot_goal"], params, **kw)
