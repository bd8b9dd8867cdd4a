"""CPU: lookahead observations (include/navsim.h navsim_lookahead_obs) -- the entry's place in the C ABI, its argument refusals (all
of them come back before the device is touched), the keyword on NavGymEnv, and rules 6 - 8 (row pose behind a crash, tail, the
shared re-scan, the row assembled from the previous observation; tests/lookahead_obs_spec.py) against the reference's recorded
crash and success traces.  The device against navsim_step itself is tests/test_gpu_lookahead_obs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lookahead_obs_spec as spec
from helpers import load_trace, struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ["reward", "done", "is_success", "is_crash", "discomfort", "distance", "margin", "pose", "status"]
FIELDS = SHARED + ["scan", "tail", "goals", "truncated", "obs"]
NEW_MANDATORY = ("scan", "tail", "goals", "truncated")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7                  # an entry more, no new version
    assert C.sizeof(abi.NavsimConfig) == L.navsim_sizeof_config() and C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert re.search(r"\bint navsim_lookahead_obs\(", header)
    assert "navsim_lookahead_obs" in abi.EXPORTS and hasattr(L, "navsim_lookahead_obs")
    assert re.search(r"#define NAVSIM_LOOKOBS_NOISE_OFF\s+0\b", header) and abi.LOOKOBS_NOISE_OFF == 0
    assert re.search(r"#define NAVSIM_LOOKOBS_NOISE_STEP\s+1\b", header) and abi.LOOKOBS_NOISE_STEP == 1
    assert struct_fields(header, "navsim_lookahead_obs_params") == ["n_actions", "noise"] == [n for n, _ in abi.NavsimLookaheadObsParams._fields_]
    assert C.sizeof(abi.NavsimLookaheadObsParams) == 8 and abi.NavsimLookaheadObsParams.noise.offset == 4
    assert struct_fields(header, "navsim_lookahead_obs_out") == FIELDS == [n for n, _ in abi.NavsimLookaheadObsOut._fields_] \
        == list(abi.LOOKAHEAD_OBS_OUT)
    assert list(abi.LOOKAHEAD_OBS_OUT)[:9] == list(abi.LOOKAHEAD_OUT) == SHARED   # the lookahead's nine arrays lead, unchanged
    assert all(abi.LOOKAHEAD_OBS_OUT[k] == abi.LOOKAHEAD_OUT[k] for k in SHARED)
    assert C.sizeof(abi.NavsimLookaheadObsOut) == 14 * C.sizeof(C.c_void_p)
    body = re.search(r"typedef struct navsim_lookahead_obs_out \{(.*?)\} navsim_lookahead_obs_out;", header, re.S).group(1)
    ctype = {"float64": "double", "float32": "float", "uint8": "uint8_t"}
    for name, (dtype, _) in abi.LOOKAHEAD_OBS_OUT.items():
        assert re.search(r"\b%s\*\s+%s;" % (ctype[dtype], name), body), name


def test_output_layout_and_parameters():
    from nav_gym_amd import sim
    sym = {"K": 9, "B": 67, "D": 3 * 67 + 7}
    shapes = dict(scan=(5, 9, 67), tail=(5, 9, 7), goals=(5, 9, 4), truncated=(5, 9), obs=(5, 9, 208), pose=(5, 9, 3), status=(5,))
    lay = sim.blob_layout(abi.LOOKAHEAD_OBS_OUT, 5, sym)
    assert [(k, shape) for k, _, _, _, shape in lay[:-1]] == [(k, shapes.get(k, (5, 9))) for k in FIELDS]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))
    small = sim.blob_layout(abi.LOOKAHEAD_OBS_OUT, 5, sym, omit=("obs",))
    assert [k for k, _, _, _, _ in small[:-1]] == FIELDS[:-1]
    assert lay[-1][3] - small[-1][3] >= 5 * 9 * 208 * 4                          # rows='full' costs E*K*(S*B+7)*4 bytes per set
    assert sim.LOOKAHEAD_OBS_KEYS == ("noise", "rows") and sim.LOOKAHEAD_KEYS == ("range",)
    assert sim.lookahead_obs_defaults() == dict(noise="step", rows="full")
    assert sim.lookahead_obs_choice(dict(noise="step", rows="full")) == (abi.LOOKOBS_NOISE_STEP, "full")
    assert sim.lookahead_obs_choice(dict(noise="off", rows="scan")) == (abi.LOOKOBS_NOISE_OFF, "scan")
    for bad in (dict(noise="on", rows="full"), dict(noise=1, rows="full"), dict(noise="step", rows="all"), dict(noise="step", rows=None)):
        with pytest.raises(ValueError):
            sim.lookahead_obs_choice(bad)


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
        o = abi.NavsimLookaheadObsOut()
        for k in abi.LOOKAHEAD_OBS_OUT:
            setattr(o, k, None if k in skip else ptr)
        return o

    def params(K=3, noise=abi.LOOKOBS_NOISE_STEP):
        return abi.NavsimLookaheadObsParams(n_actions=K, noise=noise)

    ref_ = lambda x: None if x is None else C.byref(x)

    def call(c=cfg, s=None, p=None, a=ptr, cmd=None, prev=ptr, o=None):
        s = state() if s is None else s
        p = params() if p is None else p
        o = outputs() if o is None else o
        return L.navsim_lookahead_obs(ref_(c), ref_(None if s == "null" else s), ref_(None if p == "null" else p), a, cmd, prev, None,
                                      ref_(None if o == "null" else o), None)

    def changed(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert call(c=changed(n_envs=0)) == abi.OK                                    # (the arguments below are otherwise acceptable)
    assert call(c=None) == call(s="null") == call(p="null") == call(o="null") == call(a=None) == abi.E_ARG
    for k in SHARED + list(NEW_MANDATORY):
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    assert call(c=changed(n_envs=0), o=outputs(skip=("obs",)), prev=None) == abi.OK       # the full row is optional
    for K in (0, -1, 65):
        assert call(p=params(K=K)) == abi.E_ARG, K
    for bad in (2, -1, 7):
        assert call(p=params(noise=bad)) == abi.E_ARG, bad
    # the full row of a stack needs the previous observation and the history length; a stack of one needs neither
    assert call(prev=None) == abi.E_ARG and call(s=state(skip=("n_hist",))) == abi.E_ARG
    assert call(c=changed(n_envs=0), prev=None, s=state(skip=("n_hist",)), o=outputs(skip=("obs",))) == abi.OK
    assert call(c=changed(n_envs=0, n_scan_stack=1), prev=None, s=state(skip=("n_hist",))) == abi.OK
    assert call(c=changed(n_scan_stack=0)) == abi.E_ARG
    # the step's draw needs its inputs -- only when it is asked for and the configuration has noise
    for k in noise:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
        assert call(c=changed(n_envs=0), s=state(skip=(k,)), p=params(noise=abi.LOOKOBS_NOISE_OFF)) == abi.OK, k
        assert call(c=changed(n_envs=0, add_scan_noise=0), s=state(skip=(k,))) == abi.OK, k
    # what navsim_lookahead refuses, for its reasons
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
    assert call(c=changed(n_envs=0, max_peds=64), p=params(K=64)) == abi.OK
    assert call(c=changed(n_envs=0), p=params(K=1, noise=abi.LOOKOBS_NOISE_OFF)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, max_peds=0), s=state(skip=peds + sfm)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_NONE, angle_min=-3.2, angle_last=3.2)) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm), cmd=ptr) == abi.OK
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), s=state(skip=sfm, ped_cmd=ptr)) == abi.OK


# ---- the keyword on NavGymEnv -------------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead_obs=9, lookahead_obs_params=dict(noise="off", rows="scan"))
    assert env.lookahead_obs_k == 9 and env.lookahead_obs_params == dict(noise="off", rows="scan") and env._products == []
    assert env.lookahead_k is None                                               # independent of lookahead=
    with pytest.raises(RuntimeError):
        env.lookahead_obs(np.zeros((9, 2)))                # before reset()
    for bad in (0, -1, 65, True, 2.0, "9"):
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs=bad)
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs_params=dict(noise="off"))  # params without lookahead_obs=
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs=4, lookahead_obs_params=dict(range=1.5))
    for bad in (dict(noise="on"), dict(noise=True), dict(rows="all"), dict(rows="Full")):
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs=4, lookahead_obs_params=bad)
    for ok in (dict(noise="step"), dict(rows="full"), dict(noise="off", rows="scan"), {}):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs=4, lookahead_obs_params=ok).lookahead_obs_k == 4
    for model, more in (("orca", {}), ("policy", dict(policy_weights="weights.pth"))):
        with pytest.raises(ValueError, match="lookahead_obs is not available"):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead_obs=4, pedestrian_model=model, **more)
        assert nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, pedestrian_model=model, **more).lookahead_obs_k is None
    ext = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, lookahead_obs=4, pedestrian_model="external")
    with pytest.raises(ValueError, match="human_actions"):
        ext.lookahead_obs(np.zeros((4, 2)))
    for model in ("sfm", "none"):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, lookahead_obs=64, pedestrian_model=model).lookahead_obs_k == 64
    both = nav_gym_env.make("NavGym-v0", num_envs=3, lookahead=5, lookahead_obs=7)
    assert (both.lookahead_k, both.lookahead_obs_k) == (5, 7)
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.lookahead_obs_k is None and plain.lookahead_obs_params is None  # off by default
    with pytest.raises(RuntimeError):
        plain.lookahead_obs(np.zeros((1, 2)))
    kwargs = registry.spec("NavGym-v0")["kwargs"]
    assert "lookahead_obs" not in kwargs and "lookahead_obs_params" not in kwargs


# ---- rules 6 - 8 against the reference's recorded traces -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crash_S3", "success_S2"])
def test_row_assembly_against_recorded_traces(name):
    """Every step of a recorded episode as one arena with three candidates: (0) the action the reference took, with the newest scan
    slot the trace recorded; (1) a candidate that does not crash, with a scan of its own; (2) a candidate that crashes, from a
    pose of its own.  The assembled row of (0) must be the recorded row -- behind a crash through the revert and the shared re-scan
    -- (1) keeps its scan and pose, and (2) carries the re-scan and prev_pose."""
    tr = load_trace(name)
    S, B = int(tr["S"]), int(tr["B"])
    T = len(tr["actions"])
    obs_prev = tr["first_obs"].astype(np.float32)
    n_hist = spec.first_n_hist(S)
    pose0 = tr["init_robot_pose"]
    prev_pose = np.array([pose0[0], pose0[1], spec.wrap_pi(pose0[2])])           # what a reset leaves (the step's phase 6)
    prev_action = np.zeros(2)
    seen = dict(crash=0, success=0, plain=0, filled=0)
    for t in range(T):
        crashed = bool(tr["is_crash"][t])
        recorded = np.concatenate([tr["obs_scan"][t], tr["obs_tail"][t].astype(np.float32)])
        newest = tr["obs_scan"][t][(S - 1) * B:]
        other = np.full(B, 1.25, np.float32)                                     # candidate 1's scan
        away = prev_pose + np.array([0.3, -0.2, 0.5])                            # where a crashing candidate would have stood
        # candidate 0: behind a crash the trace's newest slot IS the re-scan and its scan A is lost: any scan will do
        scans = np.stack([other * 2 if crashed else newest, other, other * 3])
        crash = np.array([crashed, False, True])
        rescan = newest if crashed else np.full(B, 0.5, np.float32)
        poses = spec.row_pose(crash, prev_pose, np.stack([away if crashed else tr["traj_robot_pose"][t], away, away]))
        tail = spec.tails(prev_pose, poses, prev_action)
        row = spec.rows(obs_prev, n_hist, spec.crash_copy(scans, crash, rescan), tail, S)
        assert row.dtype == np.float32 and row.shape == (3, S * B + 7)
        assert np.array_equal(row[0], recorded), "step %d: %d elements differ" % (t, (row[0] != recorded).sum())
        assert np.array_equal(row[1, (S - 1) * B:S * B], other) and np.array_equal(row[1, S * B + 2:S * B + 4], away[:2].astype(np.float32))
        assert np.array_equal(row[2, (S - 1) * B:S * B], rescan) and np.array_equal(row[2, S * B:], spec.tails(prev_pose, prev_pose[None], prev_action)[0])
        g = spec.goals(poses, tr["robot_goal"])
        assert np.array_equal(g[:, :2], row[:, S * B + 2:S * B + 4]) and np.array_equal(g[0, 2:], tr["robot_goal"].astype(np.float32))
        for j in range(S - 1):                                                   # history slots are shared by the candidates
            assert np.array_equal(row[1, j * B:(j + 1) * B], other if S - 1 - j > n_hist else obs_prev[(j + 1) * B:(j + 2) * B])
        seen["crash"] += crashed; seen["success"] += bool(tr["is_success"][t]); seen["plain"] += not tr["done"][t]
        seen["filled"] += n_hist < S - 1
        # the state the next step starts from (env.py:725-727)
        obs_prev, n_hist = recorded, spec.next_n_hist(n_hist, S)
        prev_pose = np.array([poses[0, 0], poses[0, 1], spec.wrap_pi(poses[0, 2])])
        prev_action = tr["actions"][t]
    assert seen["plain"] >= 3 and seen["crash" if name.startswith("crash") else "success"] >= 1, seen
    assert seen["filled"] >= (1 if S > 2 else 0), seen
