"""TEST INFRASTRUCTURE (GPU): navsim_mppi through the C ABI.  The workspace persists between calls, so the caller makes it once
(make_ws: sentinel-filled but for plan_key, which starts at -1 as the header asks) and may copy it (copy_ws); the outputs of every
call are sentinel-filled.  The state's save and restore and the small worlds are tests/lookahead_call.py's."""
import ctypes as C

import numpy as np

from gpu_support import to_device
from nav_gym_amd import abi

SENTINEL = 77
ROLL_KEYS = tuple(abi.ROLLOUT_OUT)
OUT_KEYS = tuple(abi.MPPI_OUT)


def _shape(E, tail, K, H):
    return (E,) + tuple({"K": K, "H": H}.get(s, s) for s in tail)


def make_ws(gpu, E, K, H):
    """{'plan', 'plan_key', 'actions', 'cost', 'roll': {navsim_rollout's ten}} of device tensors"""
    torch = gpu.torch
    ws = {k: torch.full(_shape(E, tail, K, H), SENTINEL, dtype=getattr(torch, d), device=gpu.dev) for k, (d, tail) in abi.MPPI_WS.items()}
    ws["plan_key"][:, 0] = -1
    ws["roll"] = {k: torch.full(_shape(E, tail, K, H), SENTINEL, dtype=getattr(torch, d), device=gpu.dev)
                  for k, (d, tail) in abi.ROLLOUT_OUT.items()}
    return ws


def copy_ws(ws):
    out = {k: v.clone() for k, v in ws.items() if k != "roll"}
    out["roll"] = {k: v.clone() for k, v in ws["roll"].items()}
    return out


def ws_numpy(ws):
    out = {k: v.cpu().numpy() for k, v in ws.items() if k != "roll"}
    out["roll"] = {k: v.cpu().numpy() for k, v in ws["roll"].items()}
    return out


def ws_struct(ws):
    return abi.NavsimMppiWs(roll=abi.NavsimRolloutOut(**{k: v.data_ptr() for k, v in ws["roll"].items()}),
                            **{k: v.data_ptr() for k, v in ws.items() if k != "roll"})


def params_struct(p, R, gamma=1.0):
    """abi.NavsimMppiParams of a tests/mppi_spec.py parameter dict"""
    s = abi.NavsimMppiParams(n_samples=int(p["n_samples"]), horizon=int(p["horizon"]), iterations=int(p["iterations"]),
                             stop_sample=int(p["stop_sample"]), select=int(p["select"]), range=float(R), gamma=float(gamma),
                             beta=float(p["beta"]), alpha=float(p["alpha"]), lam=float(p["lam"]), w_goal=float(p["w_goal"]),
                             w_crash=float(p["w_crash"]), off_field_cost=float(p["off_field_cost"]))
    for k in ("sigma", "lo", "hi", "init_action"):
        getattr(s, k)[:] = [float(p[k][0]), float(p[k][1])]
    return s


def raw(gpu, cfg, st, p, ws, out, field=None, gp=None, ped_cmd=None, skip=None):
    """The bare call with whatever pointers the caller gives (structs or None) -> the return code"""
    return gpu.lib.load().navsim_mppi(C.byref(cfg) if cfg is not None else None, C.byref(st) if st is not None else None,
                                      C.byref(p) if p is not None else None, C.byref(field) if field is not None else None,
                                      C.byref(gp) if gp is not None else None, ped_cmd, skip,
                                      C.byref(ws) if ws is not None else None, C.byref(out) if out is not None else None, None)


def call(gpu, cfg, st, p, R, ws, gamma=1.0, field=None, gp=None, ped_cmd=None, skip=None):
    """navsim_mppi on the workspace `ws` into sentinel-filled outputs -> NumPy arrays of `out`.  p: a tests/mppi_spec.py parameter
    dict; field: the uint16 device tensor [E,Hc,Wc] (gp: abi.NavsimGoalPathParams) or None."""
    torch, E = gpu.torch, cfg.n_envs
    out = {k: torch.full(_shape(E, tail, 0, 0), SENTINEL, dtype=getattr(torch, d), device=gpu.dev) for k, (d, tail) in abi.MPPI_OUT.items()}
    o = abi.NavsimMppiOut(**{k: v.data_ptr() for k, v in out.items()})
    t_cmd = None if ped_cmd is None else to_device(gpu, np.ascontiguousarray(ped_cmd, np.float64))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    f = None if field is None else abi.NavsimGoalField(dist=field.data_ptr(), key=None, rebuilds=None)
    rc = raw(gpu, cfg, st, params_struct(p, R, gamma), ws_struct(ws), o, field=f, gp=gp,
             ped_cmd=None if t_cmd is None else t_cmd.data_ptr(), skip=None if t_skip is None else t_skip.data_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}
