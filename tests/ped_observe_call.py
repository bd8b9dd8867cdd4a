"""TEST INFRASTRUCTURE (GPU): navsim_ped_observe through the C ABI into sentinel-filled outputs, the comparison of its outputs
with the specification's, and the adapter of tests/ped_observe_spec.py -- for tests/test_gpu_ped_observe.py and the geometries
of tests/test_gpu_map_geometry.py."""
import ctypes as C

import numpy as np

import gpu_support
import ped_observe_spec as spec
from gpu_support import eq, same_bits, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.PED_OBSERVATION)
STATE = dict(robot_pose=np.float64, n_peds=np.int32, ped_pose=np.float64, ped_vel=np.float64)


def c_params(**kw):
    p = dict(spec.DEFAULT, **kw)
    return abi.NavsimPedObserveParams(ped_radius=p["ped_radius"], sensor_range=p["sensor_range"], max_obs=p["max_obs"],
                                      rays=p["rays"], occlusion=p["occlusion"], fov=p["fov"])


def call(gpu, cfg, st, params, skip=None, visible=True):
    """navsim_ped_observe into sentinel-filled outputs -> NumPy arrays."""
    p = c_params(**params) if isinstance(params, dict) else params
    torch, E, N, K = gpu.torch, cfg.n_envs, cfg.max_peds, p.max_obs
    out = dict(state=torch.full((E, K, 5), 777.0, dtype=torch.float32, device=gpu.dev),
               index=torch.full((E, K), 777, dtype=torch.int32, device=gpu.dev),
               count=torch.full((E,), 777, dtype=torch.int32, device=gpu.dev),
               visible=torch.full((E, N), 77, dtype=torch.uint8, device=gpu.dev))
    o = abi.NavsimPedObservation()
    for k, v in out.items():
        setattr(o, k, v.data_ptr() if (visible or k != "visible") else None)
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_ped_observe(C.byref(cfg), C.byref(st), C.byref(p), None if skip is None else t_skip.data_ptr(),
                                           C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(dev, want, what):
    for k in ("count", "visible", "index", "state"):               # (the small arrays first: their mismatch says more)
        assert dev[k].dtype == want[k].dtype and dev[k].shape == want[k].shape, (what, k, dev[k].dtype, dev[k].shape)
        (same_bits if k == "state" else eq)(dev[k], want[k], "%s: %s" % (what, k))


def device_state(gpu, cfg, occ, w, overflow=False, map_slot=None):
    return gpu_support.device_state(gpu, cfg, occ, w, STATE, overflow, map_slot)


def answer(cfg, fields, w, params, **kw):
    return spec.observe(cfg, fields, w["robot_pose"], w["n_peds"], w["ped_pose"], w["ped_vel"], params, **kw)
