"""CPU: action lookahead (include/navsim.h navsim_lookahead) -- the entry's place in the C ABI, its argument refusals (all of them
come back before the device is touched), the keyword on NavGymEnv and the default cap.  The device against navsim_step itself is
tests/test_gpu_lookahead.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["reward", "done", "is_success", "is_crash", "discomfort", "distance", "margin", "pose", "status"]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7                  # an entry more, no new version
    assert C.sizeof(abi.NavsimConfig) == L.navsim_sizeof_config() and C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert re.search(r"\bint navsim_lookahead\(", header)
    assert "navsim_lookahead" in abi.EXPORTS and hasattr(L, "navsim_lookahead")
    assert re.search(r"#define NAVSIM_LOOKAHEAD_MAX\s+64\b", header) and abi.LOOKAHEAD_MAX == 64
    assert struct_fields(header, "navsim_lookahead_params") == ["n_actions", "range"] == [n for n, _ in abi.NavsimLookaheadParams._fields_]
    assert C.sizeof(abi.NavsimLookaheadParams) == 16 and abi.NavsimLookaheadParams.range.offset == 8
    assert struct_fields(header, "navsim_lookahead_out") == FIELDS == [n for n, _ in abi.NavsimLookaheadOut._fields_] == list(abi.LOOKAHEAD_OUT)
    assert C.sizeof(abi.NavsimLookaheadOut) == 9 * C.sizeof(C.c_void_p)
    # the element types the header states, against the table the Python layer allocates from
    body = re.search(r"typedef struct navsim_lookahead_out \{(.*?)\} navsim_lookahead_out;", header, re.S).group(1)
    ctype = {"float64": "double", "float32": "float", "uint8": "uint8_t"}
    for name, (dtype, _) in abi.LOOKAHEAD_OUT.items():
        assert re.search(r"\b%s\*\s+%s;" % (ctype[dtype], name), body), name


def test_output_layout_and_default_range():
    from nav_gym_amd import lib, sim
    lay = sim.blob_layout(abi.LOOKAHEAD_OUT, 5, {"K": 9})
    assert [(k, shape) for k, _, _, _, shape in lay[:-1]] == [(k, (5, 9, 3) if k == "pose" else (5,) if k == "status" else (5, 9)) for k in FIELDS]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))
    cfg = lib.default_config(n_envs=1)
    # the smallest multiple of 0.25 m that lies 0.1 m above the largest discomfort threshold, never above the lidar's range
    for dmax, want in ((0.0, 0.25), (0.15, 0.25), (0.151, 0.5), (0.9, 1.0), (0.91, 1.25), (1.4, 1.5)):
        assert sim.lookahead_defaults(cfg, dmax) == dict(range=want), dmax
    cfg.range_max = 1.1
    assert sim.lookahead_defaults(cfg, 0.91) == dict(range=1.1)
    assert sim.LOOKAHEAD_KEYS == ("range",) and sim.lookahead_range_min(0.5) == 0.6


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, max_peds=4, ped_model=abi.PED_SFM, map_h=16, map_w=16, n_beams=8)
    robot = ("robot_pose", "robot_goal", "prev_action", "prev_pose", "steps", "field", "scan_threshold", "scan_discomfort")
    peds = ("n_peds", "ped_pose", "ped_vel", "ped_prev_yaw", "ped_dist", "ped_has_legs")
    sfm = ("ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head")

    def state(skip=(), **more):
        st = abi.NavsimState()
        for k in robot + peds + sfm:
            setattr(st, k, None if k in skip else ptr)
        for k, v in more.items():
            setattr(st, k, v)
        return st

    def outputs(skip=()):
        o = abi.NavsimLookaheadOut()
        for k in abi.LOOKAHEAD_OUT:
            setattr(o, k, None if k in skip else ptr)
        return o

    def params(K=3, R=1.0):
        return abi.NavsimLookaheadParams(n_actions=K, range=R)

    ref_ = lambda x: None if x is None else C.byref(x)

    def call(c=cfg, s=None, p=None, a=ptr, cmd=None, o=None):
        s = state() if s is None else s
        p = params() if p is None else p
        o = outputs() if o is None else o
        return L.navsim_lookahead(ref_(c), ref_(None if s == "null" else s), ref_(None if p == "null" else p), a, cmd, None,
                                  ref_(None if o == "null" else o), None)

    def changed(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert call(c=changed(n_envs=0)) == abi.OK                                    # (the arguments below are otherwise acceptable)
    assert call(c=None) == call(s="null") == call(p="null") == call(o="null") == call(a=None) == abi.E_ARG
    for k in FIELDS:
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    for K in (0, -1, 65):
        assert call(p=params(K=K)) == abi.E_ARG, K
    for R in (0.0, -1.0, float("nan"), float("inf"), cfg.range_max * 1.0001):
        assert call(p=params(R=R)) == abi.E_ARG, R
    for k in robot + peds + sfm:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
    assert call(c=changed(max_waypoints=0)) == abi.E_ARG
    assert call(c=changed(ped_model=abi.PED_EXTERNAL)) == abi.E_ARG              # no commands: neither the argument nor the state's
    for k, bad in (("n_envs", -1), ("n_beams", 0), ("max_peds", 0), ("max_peds", 65), ("map_h", 0), ("map_w", 0), ("march_rule", 3),
                   ("march_rule", -1), ("resolution", 0.0), ("time_step", 0.0), ("time_step", float("nan")), ("action_kind", 2),
                   ("ped_model", 3)):
        assert call(c=changed(**{k: bad})) == abi.E_ARG, (k, bad)
    assert call(c=changed(action_kind=abi.ACTION_WHEELS, wheel_radius=0.0)) == abi.E_ARG
    assert call(c=changed(shared_field=1), s=state(map_slot=ptr)) == abi.E_ARG
    assert call(c=changed(field_format=2)) == abi.E_UNSUPPORTED
    assert call(c=changed(field_format=abi.FIELD_F32), s=state(rect_table=ptr)) == abi.E_UNSUPPORTED     # records need the packed field
    assert call(c=changed(field_format=abi.FIELD_U16T, map_h=1032), s=state(rect_table=ptr)) == abi.E_UNSUPPORTED
    assert call(c=changed(angle_min=-3.2, angle_last=3.2)) == abi.E_UNSUPPORTED   # wider than 2 pi with pedestrians to merge
    assert call(c=changed(n_beams=13700)) == abi.E_UNSUPPORTED                    # 12 B per beam: beyond a compute unit's 160 KB of LDS
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted
    assert call(c=changed(n_envs=0, n_beams=13000)) == abi.OK
    assert call(c=changed(n_envs=0, max_peds=64), p=params(K=64, R=cfg.range_max)) == abi.OK
    assert call(c=changed(n_envs=0), p=params(K=1)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, max_peds=0), s=state(skip=peds + sfm)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, angle_min=-3.2, angle_last=3.2)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm), cmd=ptr) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm, ped_cmd=ptr)) == abi.OK


# ---- the keyword on NavGymEnv -------------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead=9, lookahead_params=dict(range=1.5))
    assert env.lookahead_k == 9 and env.lookahead_params == dict(range=1.5) and env._products == []
    with pytest.raises(RuntimeError):
        env.lookahead(np.zeros((9, 2)))                    # before reset()
    for bad in (0, -1, 65, True, 2.0, "9"):
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, lookahead=bad)
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_params=dict(range=1.5))        # params without lookahead=
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, lookahead=4, lookahead_params=dict(reach=1.5))
    for model, more in (("orca", {}), ("policy", dict(policy_weights="weights.pth"))):
        with pytest.raises(ValueError, match="lookahead is not available"):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead=4, pedestrian_model=model, **more)
        assert nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, pedestrian_model=model, **more).lookahead_k is None
    ext = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead=4, pedestrian_model="external")
    with pytest.raises(ValueError, match="human_actions"):
        ext.lookahead(np.zeros((4, 2)))
    for model in ("sfm", "none"):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, lookahead=64, pedestrian_model=model).lookahead_k == 64
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.lookahead_k is None
    with pytest.raises(RuntimeError):
        plain.lookahead(np.zeros((1, 2)))
    assert "lookahead" not in registry.spec("NavGym-v0")["kwargs"]
