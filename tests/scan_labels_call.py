"""TEST INFRASTRUCTURE (GPU): navsim_scan_labels through the C ABI into sentinel-filled outputs, the comparison of its outputs
with the specification's (tests/scan_labels_spec.py), and raw device states of that module's worlds -- for
tests/test_gpu_scan_labels.py."""
import ctypes as C

import numpy as np

import gpu_support
from gpu_support import eq, same_bits, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.SCAN_LABELS_OUT)
STATE = dict(robot_pose=np.float64, n_peds=np.int32, ped_pose=np.float64, ped_dist=np.float64, ped_has_legs=np.uint8)
STATE_NO_PEDS = dict(robot_pose=np.float64)


def call(gpu, cfg, st, skip=None, hits=True):
    """navsim_scan_labels into sentinel-filled outputs -> NumPy arrays."""
    torch, E, N, B = gpu.torch, cfg.n_envs, cfg.max_peds, cfg.n_beams
    out = dict(range=torch.full((E, B), 777.0, dtype=torch.float32, device=gpu.dev),
               label=torch.full((E, B), 77, dtype=torch.uint8, device=gpu.dev),
               index=torch.full((E, B), 77, dtype=torch.int8, device=gpu.dev),
               hits=torch.full((E, N), 777, dtype=torch.int32, device=gpu.dev))
    o = abi.NavsimScanLabelsOut()
    for k, v in out.items():
        setattr(o, k, v.data_ptr() if (hits or k != "hits") else None)
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_scan_labels(C.byref(cfg), C.byref(st), None if skip is None else t_skip.data_ptr(), C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(dev, want, what, keys=KEYS):
    for k in ("hits", "label", "index", "range"):                 # (the small arrays first: their mismatch says more)
        if k not in keys or k not in dev:
            continue
        assert dev[k].dtype == want[k].dtype and dev[k].shape == want[k].shape, (what, k, dev[k].dtype, dev[k].shape)
        (same_bits if k == "range" else eq)(dev[k], want[k], "%s: %s" % (what, k))


def device_state(gpu, cfg, occ, w, overflow=False, map_slot=None, rects=False):
    """navsim_state of the world `w` (host arrays) over the field of occ [M,H,W]; rects: with the record table of the packed
    field (the kernel's rect_table path).  -> (st, keepalive)"""
    st, keep = gpu_support.device_state(gpu, cfg, occ, w, STATE_NO_PEDS if cfg.ped_model == abi.PED_NONE else STATE, overflow, map_slot)
    if rects:
        occ_t = to_device(gpu, occ)
        keep["rect_table"] = gpu.sim.build_rects(occ_t, keep["field"], cfg.field_format, keep.get("field_overflow"))
        st.rect_table = keep["rect_table"].data_ptr()
    return st, keep
