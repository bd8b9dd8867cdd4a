"""CPU: rollout observations (include/navsim.h navsim_rollout_obs) -- the entry's place in the C ABI, its argument refusals (all of
them come back before the device is touched) and the keyword on NavGymEnv.  The device against navsim_step itself is
tests/test_gpu_rollout_obs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ["reward", "pose", "ret", "length", "outcome", "discomfort_steps", "min_margin", "distance", "exact_steps", "status"]
FIELDS = SHARED + ["obs_last", "goals_last", "obs_all", "goals_all"]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7                  # an entry more, no new version
    assert C.sizeof(abi.NavsimConfig) == L.navsim_sizeof_config() and C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert re.search(r"\bint navsim_rollout_obs\(", header)
    assert header.index("int navsim_ped_forecast(") < header.index("int navsim_rollout_obs(")
    assert "navsim_rollout_obs" in abi.EXPORTS and hasattr(L, "navsim_rollout_obs")
    names = ["n_seq", "horizon", "noise", "gamma"]
    assert struct_fields(header, "navsim_rollout_obs_params") == names == [n for n, _ in abi.NavsimRolloutObsParams._fields_]
    P = abi.NavsimRolloutObsParams
    assert C.sizeof(P) == 24 and (P.n_seq.offset, P.horizon.offset, P.noise.offset, P.gamma.offset) == (0, 4, 8, 16)
    assert struct_fields(header, "navsim_rollout_obs_out") == FIELDS == [n for n, _ in abi.NavsimRolloutObsOut._fields_] \
        == list(abi.ROLLOUT_OBS_OUT)
    assert list(abi.ROLLOUT_OBS_OUT)[:10] == list(abi.ROLLOUT_OUT) == SHARED       # the rollout's ten arrays lead, unchanged
    assert all(abi.ROLLOUT_OBS_OUT[k] == abi.ROLLOUT_OUT[k] for k in SHARED)
    assert C.sizeof(abi.NavsimRolloutObsOut) == 14 * C.sizeof(C.c_void_p)
    for i, name in enumerate(FIELDS):
        assert getattr(abi.NavsimRolloutObsOut, name).offset == i * C.sizeof(C.c_void_p), name
    body = re.search(r"typedef struct navsim_rollout_obs_out \{(.*?)\} navsim_rollout_obs_out;", header, re.S).group(1)
    ctype = {"float64": "double", "float32": "float", "uint8": "uint8_t", "int32": "int32_t"}
    for name, (dtype, _) in abi.ROLLOUT_OBS_OUT.items():
        assert re.search(r"\b%s\*\s+%s;" % (ctype[dtype], name), body), name
    # the existing structs and entries are as they were
    assert C.sizeof(abi.NavsimRolloutOut) == 10 * C.sizeof(C.c_void_p) and C.sizeof(abi.NavsimRolloutParams) == 24
    assert C.sizeof(abi.NavsimLookaheadObsOut) == 14 * C.sizeof(C.c_void_p) and C.sizeof(abi.NavsimLookaheadObsParams) == 8


def test_output_layout_and_parameters():
    from nav_gym_amd import sim
    sym = {"K": 5, "H": 6, "D": 3 * 67 + 7}
    shapes = dict(reward=(4, 5, 6), pose=(4, 5, 6, 3), status=(4,), obs_last=(4, 5, 208), goals_last=(4, 5, 4),
                  obs_all=(4, 5, 6, 208), goals_all=(4, 5, 6, 4))
    lay = sim.blob_layout(abi.ROLLOUT_OBS_OUT, 4, sym)
    assert [(k, shape) for k, _, _, _, shape in lay[:-1]] == [(k, shapes.get(k, (4, 5))) for k in FIELDS]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))
    small = sim.blob_layout(abi.ROLLOUT_OBS_OUT, 4, sym, omit=("obs_all", "goals_all"))
    assert [k for k, _, _, _, _ in small[:-1]] == FIELDS[:-2]
    assert lay[-1][3] - small[-1][3] >= 4 * 5 * 6 * 208 * 4                      # rows='all' costs E*K*H*(S*B+7)*4 bytes per set
    assert sim.ROLLOUT_OBS_KEYS == ("gamma", "noise", "rows")
    assert sim.rollout_obs_defaults() == dict(gamma=1.0, noise="step", rows="last")
    assert sim.rollout_obs_choice(dict(gamma=1.0, noise="step", rows="last")) == (1.0, abi.LOOKOBS_NOISE_STEP, "last")
    assert sim.rollout_obs_choice(dict(gamma=0, noise="off", rows="all")) == (0.0, abi.LOOKOBS_NOISE_OFF, "all")
    for bad in (dict(gamma=1.0, noise="on", rows="last"), dict(gamma=1.0, noise=1, rows="last"), dict(gamma=1.0, noise="step", rows="full"),
                dict(gamma=1.0, noise="step", rows=None), dict(gamma=1.5, noise="step", rows="last"),
                dict(gamma=-0.1, noise="step", rows="last"), dict(gamma=float("nan"), noise="step", rows="last"),
                dict(gamma="1", noise="step", rows="last"), dict(gamma=True, noise="step", rows="last")):
        with pytest.raises(ValueError):
            sim.rollout_obs_choice(bad)


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, max_peds=4, ped_model=abi.PED_SFM, map_h=16, map_w=16, n_beams=8, n_scan_stack=3, add_scan_noise=1)
    robot = ("robot_pose", "robot_goal", "prev_action", "prev_pose", "steps", "field", "scan_threshold", "scan_discomfort")
    peds = ("n_peds", "ped_pose", "ped_vel", "ped_prev_yaw", "ped_dist", "ped_has_legs")
    sfm = ("ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head")
    rows = ("n_hist",)
    noise = ("scan_noise_std", "episode")

    def state(skip=(), **more):
        st = abi.NavsimState()
        for k in robot + peds + sfm + rows + noise:
            setattr(st, k, None if k in skip else ptr)
        for k, v in more.items():
            setattr(st, k, v)
        return st

    def outputs(skip=()):
        o = abi.NavsimRolloutObsOut()
        for k in abi.ROLLOUT_OBS_OUT:
            setattr(o, k, None if k in skip else ptr)
        return o

    def params(K=3, H=4, noise=abi.LOOKOBS_NOISE_STEP, gamma=1.0):
        return abi.NavsimRolloutObsParams(n_seq=K, horizon=H, noise=noise, gamma=gamma)

    ref_ = lambda x: None if x is None else C.byref(x)

    def call(c=cfg, s=None, p=None, a=ptr, cmd=None, prev=ptr, o=None):
        s = state() if s is None else s
        p = params() if p is None else p
        o = outputs() if o is None else o
        return L.navsim_rollout_obs(ref_(c), ref_(None if s == "null" else s), ref_(None if p == "null" else p), a, cmd, prev, None,
                                    ref_(None if o == "null" else o), None)

    def changed(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert call(c=changed(n_envs=0)) == abi.OK                                    # (the arguments below are otherwise acceptable)
    assert call(c=None) == call(s="null") == call(p="null") == call(o="null") == call(a=None) == abi.E_ARG
    # the rollout's ten arrays and the last row are mandatory; the rows of all steps come both or neither
    for k in SHARED + ["obs_last", "goals_last"]:
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    assert call(o=outputs(skip=("obs_all",))) == abi.E_ARG and call(o=outputs(skip=("goals_all",))) == abi.E_ARG
    assert call(c=changed(n_envs=0), o=outputs(skip=("obs_all", "goals_all"))) == abi.OK
    for K in (0, -1, abi.ROLLOUT_MAX_K + 1):
        assert call(p=params(K=K)) == abi.E_ARG, K
    for H in (0, -1, abi.ROLLOUT_MAX_H + 1):
        assert call(p=params(H=H)) == abi.E_ARG, H
    for gamma in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(p=params(gamma=gamma)) == abi.E_ARG, gamma
    for bad in (2, -1, 7):
        assert call(p=params(noise=bad)) == abi.E_ARG, bad
    # a stack needs the previous observation and the history length, whatever rows are asked for; a stack of one needs neither
    assert call(prev=None) == abi.E_ARG and call(s=state(skip=("n_hist",))) == abi.E_ARG
    assert call(prev=None, o=outputs(skip=("obs_all", "goals_all"))) == abi.E_ARG
    assert call(c=changed(n_envs=0, n_scan_stack=1), prev=None, s=state(skip=("n_hist",))) == abi.OK
    assert call(c=changed(n_scan_stack=0)) == abi.E_ARG
    # each step's draw needs its inputs -- only when it is asked for and the configuration has noise
    for k in noise:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
        assert call(c=changed(n_envs=0), s=state(skip=(k,)), p=params(noise=abi.LOOKOBS_NOISE_OFF)) == abi.OK, k
        assert call(c=changed(n_envs=0, add_scan_noise=0), s=state(skip=(k,))) == abi.OK, k
    # what navsim_rollout refuses, for its reasons
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
    assert call(c=changed(n_envs=0, max_peds=64), p=params(K=abi.ROLLOUT_MAX_K, H=abi.ROLLOUT_MAX_H, gamma=0.0)) == abi.OK
    assert call(c=changed(n_envs=0), p=params(K=1, H=1, noise=abi.LOOKOBS_NOISE_OFF)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, max_peds=0), s=state(skip=peds + sfm)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, angle_min=-3.2, angle_last=3.2)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm), cmd=ptr) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm, ped_cmd=ptr)) == abi.OK


# ---- the keyword on NavGymEnv -------------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    make = lambda **kw: nav_gym_env.make("NavGym-v0", **dict(dict(num_envs=3), **kw))
    env = make(num_humans=5, rollout_obs=9, rollout_obs_params=dict(horizon=5, gamma=0.9, noise="off", rows="all"))
    assert (env.rollout_obs_k, env.rollout_obs_h) == (9, 5) and env._products == []
    assert env.rollout_obs_params == dict(horizon=5, gamma=0.9, noise="off", rows="all")
    assert env.rollout_k is None and env.lookahead_obs_k is None                 # independent of rollout= and lookahead_obs=
    with pytest.raises(RuntimeError):
        env.rollout_obs(np.zeros((9, 5, 2)))               # before reset()
    assert make(rollout_obs=4).rollout_obs_h == 8                                # the default horizon
    for bad in (0, -1, abi.ROLLOUT_MAX_K + 1, True, 2.0, "9"):
        with pytest.raises(ValueError):
            make(rollout_obs=bad)
    with pytest.raises(ValueError):
        make(rollout_obs_params=dict(noise="off"))                               # params without rollout_obs=
    with pytest.raises(ValueError):
        make(rollout_obs=4, rollout_obs_params=dict(range=1.5))                  # an unknown key: there is no range
    for bad in (dict(horizon=0), dict(horizon=abi.ROLLOUT_MAX_H + 1), dict(horizon=2.0), dict(horizon=True), dict(gamma=-0.1),
                dict(gamma=1.5), dict(gamma="1"), dict(gamma=float("nan")), dict(noise="on"), dict(noise=True), dict(rows="full"),
                dict(rows="All"), dict(rows=None)):
        with pytest.raises(ValueError):
            make(rollout_obs=4, rollout_obs_params=bad)
    for ok in (dict(noise="step"), dict(rows="last"), dict(horizon=1), dict(horizon=abi.ROLLOUT_MAX_H, gamma=0, noise="off", rows="all"), {}):
        assert make(rollout_obs=4, rollout_obs_params=ok).rollout_obs_k == 4
    for model, more in (("orca", {}), ("policy", dict(policy_weights="weights.pth"))):
        with pytest.raises(ValueError, match="rollout_obs is not available"):
            make(num_humans=5, rollout_obs=4, pedestrian_model=model, **more)
        assert make(num_humans=5, pedestrian_model=model, **more).rollout_obs_k is None
    ext = make(num_humans=5, rollout_obs=4, pedestrian_model="external")
    with pytest.raises(ValueError, match="human_actions"):
        ext.rollout_obs(np.zeros((4, 8, 2)))
    for model in ("sfm", "none"):
        assert make(rollout_obs=abi.ROLLOUT_MAX_K, pedestrian_model=model).rollout_obs_k == abi.ROLLOUT_MAX_K
    three = make(rollout=5, rollout_params=dict(horizon=3), lookahead_obs=7, rollout_obs=6, rollout_obs_params=dict(horizon=4))
    assert (three.rollout_k, three.rollout_h, three.lookahead_obs_k, three.rollout_obs_k, three.rollout_obs_h) == (5, 3, 7, 6, 4)
    plain = make()
    assert plain.rollout_obs_k is None and plain.rollout_obs_h is None and plain.rollout_obs_params is None       # off by default
    assert plain._products == []
    with pytest.raises(RuntimeError):
        plain.rollout_obs(np.zeros((1, 8, 2)))
    kwargs = registry.spec("NavGym-v0")["kwargs"]
    assert "rollout_obs" not in kwargs and "rollout_obs_params" not in kwargs


def test_action_broadcasting():
    """[K,H,2] array-likes are taken by every arena; anything else but [E,K,H,2] is refused (rollout()'s rule, shared)."""
    from nav_gym_amd.env import NavGymEnv
    seq = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    a = NavGymEnv._rollout_actions(seq.tolist(), 5, 3, 4)
    assert tuple(a.shape) == (5, 3, 4, 2) and a.dtype.is_floating_point and a.element_size() == 8 and a.is_contiguous()
    assert all(np.array_equal(a[e].numpy(), seq) for e in range(5))
    full = np.random.default_rng(0).uniform(-1, 1, (5, 3, 4, 2))
    assert np.array_equal(NavGymEnv._rollout_actions(full, 5, 3, 4).numpy(), full)
    for bad in (np.zeros((3, 4)), np.zeros((4, 3, 2)), np.zeros((5, 3, 4, 3)), np.zeros((2, 3, 4, 2))):
        with pytest.raises(ValueError):
            NavGymEnv._rollout_actions(bad, 5, 3, 4)
