"""TEST INFRASTRUCTURE (GPU): navsim_ped_forecast through the C ABI into sentinel-filled outputs, and the step itself as its
reference: the saved state put back, H navsim_step calls with the forecast's actions, the pedestrians and the robot behind every
step stacked.  The state's save and restore are tests/lookahead_call.py's."""
import ctypes as C

import numpy as np

import lookahead_call as lc
from gpu_support import to_device
from nav_gym_amd import abi

KEYS = tuple(abi.FORECAST_OUT)


def call(gpu, cfg, st, H, robot=abi.FORECAST_ACTIONS, model=abi.FORECAST_TRUE, actions=None, ped_cmd=None, skip=None):
    """navsim_ped_forecast into sentinel-filled outputs -> NumPy arrays.  actions: [E,H,2] float64 (or None)."""
    torch, E = gpu.torch, cfg.n_envs
    out = {}
    for k, (dtype, tail) in abi.FORECAST_OUT.items():
        shape = (E,) + tuple({"H": H, "N": cfg.max_peds}.get(s, s) for s in tail)
        out[k] = torch.full(shape, 77, dtype=getattr(torch, dtype), device=gpu.dev)
    o = abi.NavsimPedForecastOut(**{k: v.data_ptr() for k, v in out.items()})
    p = abi.NavsimPedForecastParams(horizon=H, robot=robot, model=model)
    t_act = None if actions is None else to_device(gpu, np.ascontiguousarray(actions, np.float64))
    assert t_act is None or tuple(t_act.shape) == (E, H, 2)
    t_cmd = None if ped_cmd is None else to_device(gpu, np.ascontiguousarray(ped_cmd, np.float64))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = gpu.lib.load().navsim_ped_forecast(C.byref(cfg), C.byref(st), C.byref(p), ptr(t_act), ptr(t_cmd), ptr(t_skip), C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def steps_of(gpu, g, saved, actions, ped_cmd=None):
    """The saved state put back, then H navsim_step calls with actions[:, h] -> what the state holds behind each step, stacked
    [E,H,...]: ped_pose, ped_vel, robot_pose, done, and -- where the state has them -- ped_due, ped_waypoints, ped_n_waypoints,
    ped_wp_head.  The saved state is put back at the end."""
    names = ("ped_pose", "ped_vel", "robot_pose") + tuple(k for k in ("ped_due", "ped_waypoints", "ped_n_waypoints", "ped_wp_head")
                                                          if k in g.t)
    seq = {k: [] for k in names + ("done",)}
    lc.load_state(g, saved)
    if ped_cmd is not None:
        g.set_ped_cmd(ped_cmd)
    for h in range(actions.shape[1]):
        _, o = g.step(to_device(gpu, actions[:, h]))
        seq["done"].append(o["done"].cpu().numpy().copy())
        for k in names:
            seq[k].append(g.t[k].cpu().numpy().copy())
    lc.load_state(g, saved)
    return {k: np.stack(v, axis=1) for k, v in seq.items()}


def first_done(step):
    """[E]: index of the arena's first done step, H where it has none."""
    done = step["done"] != 0
    return np.where(done.any(axis=1), done.argmax(axis=1), done.shape[1]).astype(np.int64)


__all__ = ["call", "steps_of", "first_done", "KEYS"]
