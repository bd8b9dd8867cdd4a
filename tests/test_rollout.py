"""CPU: action-sequence rollout (include/navsim.h navsim_rollout) -- the entry's place in the C ABI, its argument refusals (all of
them come back before the device is touched), the keywords on NavGymEnv, the defaults and the [K,H,2] broadcast.  The device
against navsim_step itself is tests/test_gpu_rollout.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["reward", "pose", "ret", "length", "outcome", "discomfort_steps", "min_margin", "distance", "exact_steps", "status"]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7                  # an entry more, no new version
    assert C.sizeof(abi.NavsimConfig) == L.navsim_sizeof_config() and C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert re.search(r"\bint navsim_rollout\(", header)
    assert "navsim_rollout" in abi.EXPORTS and hasattr(L, "navsim_rollout")
    assert re.search(r"#define NAVSIM_ROLLOUT_MAX_K\s+256\b", header) and abi.ROLLOUT_MAX_K == 256
    assert re.search(r"#define NAVSIM_ROLLOUT_MAX_H\s+32\b", header) and abi.ROLLOUT_MAX_H == 32
    names = ["n_seq", "horizon", "range", "gamma"]
    assert struct_fields(header, "navsim_rollout_params") == names == [n for n, _ in abi.NavsimRolloutParams._fields_]
    P = abi.NavsimRolloutParams
    assert C.sizeof(P) == 24 and (P.n_seq.offset, P.horizon.offset, P.range.offset, P.gamma.offset) == (0, 4, 8, 16)
    assert struct_fields(header, "navsim_rollout_out") == FIELDS == [n for n, _ in abi.NavsimRolloutOut._fields_] == list(abi.ROLLOUT_OUT)
    assert C.sizeof(abi.NavsimRolloutOut) == 10 * C.sizeof(C.c_void_p)
    # the element types the header states, against the table the Python layer allocates from
    body = re.search(r"typedef struct navsim_rollout_out \{(.*?)\} navsim_rollout_out;", header, re.S).group(1)
    ctype = {"float64": "double", "float32": "float", "uint8": "uint8_t", "int32": "int32_t"}
    for name, (dtype, _) in abi.ROLLOUT_OUT.items():
        assert re.search(r"\b%s\*\s+%s;" % (ctype[dtype], name), body), name
    # the outcome's bits are the episode statistics'
    assert (abi.OUTCOME_SUCCESS, abi.OUTCOME_CRASH, abi.OUTCOME_TIME_LIMIT) == (1, 2, 4)
    # the header states the predicate of rule 8 and what is out of scope
    text = re.search(r"action-sequence rollout.*?int navsim_rollout\(", header, re.S).group(0)
    for phrase in ("ped_n_waypoints[e,i] - 1", "< 0.5", "exact_steps", "Out of scope", "PROPERTY"):
        assert phrase in text, phrase


def test_output_layout_defaults_and_range_bounds():
    from nav_gym_amd import lib, sim
    lay = sim.blob_layout(abi.ROLLOUT_OUT, 5, {"K": 9, "H": 6})
    shape = {"reward": (5, 9, 6), "pose": (5, 9, 6, 3), "status": (5,)}
    assert [(k, s) for k, _, _, _, s in lay[:-1]] == [(k, shape.get(k, (5, 9))) for k in FIELDS]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))
    cfg = lib.default_config(n_envs=1)
    # range: the lookahead's default and lower bound
    for dmax in (0.0, 0.15, 0.151, 0.9, 0.91, 1.4):
        assert sim.rollout_defaults(cfg, dmax) == dict(range=sim.lookahead_defaults(cfg, dmax)["range"], gamma=1.0), dmax
        assert sim.rollout_defaults(cfg, dmax)["range"] >= sim.lookahead_range_min(dmax)
    assert sim.rollout_defaults(cfg, 0.91)["range"] == 1.25
    cfg.range_max = 1.1
    assert sim.rollout_defaults(cfg, 0.91) == dict(range=1.1, gamma=1.0)
    assert sim.ROLLOUT_KEYS == ("range", "gamma")


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
        o = abi.NavsimRolloutOut()
        for k in abi.ROLLOUT_OUT:
            setattr(o, k, None if k in skip else ptr)
        return o

    def params(K=3, H=4, R=1.0, gamma=1.0):
        return abi.NavsimRolloutParams(n_seq=K, horizon=H, range=R, gamma=gamma)

    ref_ = lambda x: None if x is None else C.byref(x)

    def call(c=cfg, s=None, p=None, a=ptr, cmd=None, o=None):
        s = state() if s is None else s
        p = params() if p is None else p
        o = outputs() if o is None else o
        return L.navsim_rollout(ref_(c), ref_(None if s == "null" else s), ref_(None if p == "null" else p), a, cmd, None,
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
    for K in (0, -1, 257):
        assert call(p=params(K=K)) == abi.E_ARG, K
    for H in (0, -1, 33):
        assert call(p=params(H=H)) == abi.E_ARG, H
    for R in (0.0, -1.0, float("nan"), float("inf"), cfg.range_max * 1.0001):
        assert call(p=params(R=R)) == abi.E_ARG, R
    for gamma in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(p=params(gamma=gamma)) == abi.E_ARG, gamma
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
    assert call(c=changed(n_envs=2 ** 23 + 1), p=params(K=256)) == abi.E_UNSUPPORTED      # more than 2^31 - 1 workgroups
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted
    assert call(c=changed(n_envs=0, n_beams=13000)) == abi.OK
    assert call(c=changed(n_envs=0, max_peds=64), p=params(K=256, H=32, R=cfg.range_max, gamma=0.0)) == abi.OK
    assert call(c=changed(n_envs=0), p=params(K=1, H=1)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, max_peds=0), s=state(skip=peds + sfm)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, angle_min=-3.2, angle_last=3.2)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm), cmd=ptr) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm, ped_cmd=ptr)) == abi.OK


# ---- the keywords on NavGymEnv ------------------------------------------------------------------------------------------------
def test_env_keywords():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, rollout=9, rollout_params=dict(horizon=6, range=1.5, gamma=0.9))
    assert (env.rollout_k, env.rollout_h) == (9, 6) and env.rollout_params == dict(horizon=6, range=1.5, gamma=0.9)
    assert env._products == []                                # nothing runs behind the step
    assert nav_gym_env.make("NavGym-v0", num_envs=3, rollout=4).rollout_h == 8      # the default horizon
    with pytest.raises(RuntimeError):
        env.rollout(np.zeros((9, 6, 2)))                      # before reset()
    for bad in (0, -1, 257, True, 2.0, "9"):
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, rollout=bad)
    for bad in (0, -1, 33, True, 2.0, "8"):
        with pytest.raises(ValueError, match="horizon"):
            nav_gym_env.make("NavGym-v0", num_envs=3, rollout=4, rollout_params=dict(horizon=bad))
    for bad in (-0.1, 1.1, float("nan"), "1", True):
        with pytest.raises(ValueError, match="gamma"):
            nav_gym_env.make("NavGym-v0", num_envs=3, rollout=4, rollout_params=dict(gamma=bad))
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, rollout_params=dict(horizon=4))           # params without rollout=
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, rollout=4, rollout_params=dict(steps=4))  # an unknown key
    for model, more in (("orca", {}), ("policy", dict(policy_weights="weights.pth"))):
        with pytest.raises(ValueError, match="rollout is not available"):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, rollout=4, pedestrian_model=model, **more)
        assert nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, pedestrian_model=model, **more).rollout_k is None
    ext = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, rollout=4, pedestrian_model="external")
    with pytest.raises(ValueError, match="human_actions"):
        ext.rollout(np.zeros((4, 8, 2)))
    for model in ("sfm", "none"):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, rollout=256, pedestrian_model=model).rollout_k == 256
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.rollout_k is None and plain.rollout_h is None and plain.rollout_params is None
    with pytest.raises(RuntimeError):
        plain.rollout(np.zeros((1, 8, 2)))
    assert "rollout" not in registry.spec("NavGym-v0")["kwargs"]


def test_actions_broadcast():
    """An array-like [K,H,2] is taken by every arena; [E,K,H,2] passes; any other shape is refused."""
    from nav_gym_amd.env import NavGymEnv
    seq = np.arange(4 * 3 * 2, dtype=np.float32).reshape(4, 3, 2)
    t = NavGymEnv._rollout_actions(seq, 5, 4, 3)
    assert tuple(t.shape) == (5, 4, 3, 2) and str(t.dtype) == "torch.float64" and t.is_contiguous()
    assert all(np.array_equal(t[e].numpy(), seq.astype(np.float64)) for e in range(5))
    t[0, 0, 0, 0] = 99.0                                       # a writable copy of its own
    assert seq[0, 0, 0] == 0.0 and t[1, 0, 0, 0] == 0.0
    full = np.random.default_rng(0).uniform(-1, 1, (5, 4, 3, 2))
    assert np.array_equal(NavGymEnv._rollout_actions(full.tolist(), 5, 4, 3).numpy(), full)
    for bad in (np.zeros((4, 3)), np.zeros((3, 4, 2)), np.zeros((5, 4, 3, 3)), np.zeros((4, 4, 3, 2))):
        with pytest.raises(ValueError, match="shape"):
            NavGymEnv._rollout_actions(bad, 5, 4, 3)
