"""CPU: episode statistics (include/navsim.h navsim_episode_stats_update / _clear) -- the entries' place in the C ABI, their
argument refusals, the keyword on NavGymEnv, and hand-made cases of the specification (tests/episode_stats_spec.py).  The
device against that specification is tests/test_gpu_episode_stats.py."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import episode_stats_spec as spec
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()         # the layouts the step's kernarg views rest on
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    for name in ("navsim_episode_stats_update", "navsim_episode_stats_clear"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in abi.EXPORTS and hasattr(L, name), name
    # the struct's field list, written out again: twelve device pointers in the header's order
    body = re.search(r"typedef struct navsim_episode_stats \{(.*?)\} navsim_episode_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == ["ret", "length", "path_length", "min_clearance", "discomfort_steps", "ep_return", "ep_length",
                      "ep_path_length", "ep_min_clearance", "ep_discomfort_steps", "ep_outcome", "totals"]
    assert [n for n, _ in abi.NavsimEpisodeStats._fields_] == fields
    assert C.sizeof(abi.NavsimEpisodeStats) == 12 * C.sizeof(C.c_void_p)
    assert abi.EPISODE_TOTALS == spec.TOTALS
    assert (abi.EPISODE_SUCCESS, abi.EPISODE_CRASH, abi.EPISODE_TIME_LIMIT) == (spec.SUCCESS, spec.CRASH, spec.TIME_LIMIT)
    assert [k for k, _ in spec.ACCUMULATORS] == list(abi.EPISODE_ACCUMULATORS)
    assert [k for k, _ in spec.PUBLISHED] == list(abi.EPISODE_PUBLISHED)


def _filled(cls, ptr, skip=()):
    s = cls()
    for name, _ in cls._fields_:
        setattr(s, name, None if name in skip else ptr)
    return s


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, n_beams=8, n_scan_stack=1, auto_reset=abi.AUTORESET_NONE)
    st = abi.NavsimState()
    st.scan_threshold = st.scan_discomfort = ptr
    io_fields = ("obs", "reward", "done", "is_success", "is_crash")
    io = abi.NavsimStepIO()
    for k in io_fields:
        setattr(io, k, ptr)
    good = _filled(abi.NavsimEpisodeStats, ptr)
    up = lambda c=cfg, s_=st, i=io, e=good: L.navsim_episode_stats_update(
        None if c is None else C.byref(c), None if s_ is None else C.byref(s_), None if i is None else C.byref(i),
        None if e is None else C.byref(e), None)
    assert up(c=None) == up(s_=None) == up(i=None) == up(e=None) == abi.E_ARG
    for name, _ in abi.NavsimEpisodeStats._fields_:
        if name != "totals":                                                     # (totals may be NULL)
            assert up(e=_filled(abi.NavsimEpisodeStats, ptr, skip=(name,))) == abi.E_ARG, name
            assert L.navsim_episode_stats_clear(C.byref(cfg), C.byref(_filled(abi.NavsimEpisodeStats, ptr, skip=(name,))),
                                                None, None) == abi.E_ARG, name
    for k in io_fields:
        io2 = abi.NavsimStepIO()
        for j in io_fields:
            setattr(io2, j, None if j == k else ptr)
        assert up(i=io2) == abi.E_ARG, k
    for k in ("scan_threshold", "scan_discomfort"):
        st2 = abi.NavsimState()
        st2.scan_threshold = st2.scan_discomfort = ptr
        setattr(st2, k, None)
        assert up(s_=st2) == abi.E_ARG, k
    same = cfg.copy(); same.auto_reset = abi.AUTORESET_SAME_STEP
    assert up(c=same) == abi.E_ARG                                               # same-step without io.final_obs
    nxt = cfg.copy(); nxt.auto_reset = abi.AUTORESET_NEXT_STEP
    assert up(c=nxt) == abi.E_ARG                                                # next-step without io.reset_mask
    for k, bad in (("n_envs", -1), ("n_beams", 0), ("n_scan_stack", 0)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        assert up(c=c2) == abi.E_ARG, k
    wide = cfg.copy(); wide.n_beams = 8193                 # the two threshold tables no longer fit 64 KB of LDS
    assert up(c=wide) == abi.E_UNSUPPORTED
    wide.n_beams = 8192; wide.n_envs = 0                   # (the widest row that does; nothing to launch)
    assert up(c=wide) == abi.OK
    assert L.navsim_episode_stats_clear(None, C.byref(good), None, None) == abi.E_ARG
    assert L.navsim_episode_stats_clear(C.byref(cfg), None, None, None) == abi.E_ARG
    # nothing to do is not an error, and launches nothing
    empty = cfg.copy(); empty.n_envs = 0
    assert up(c=empty) == abi.OK and L.navsim_episode_stats_clear(C.byref(empty), C.byref(good), None, None) == abi.OK


# ---- the keyword on NavGymEnv -----------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, episode_stats=True)
    assert env.episode_stats is True
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.episode_stats is True and twin.num_envs == 3
    assert nav_gym_env.make("NavGym-v0", num_envs=3, episode_stats=True, autoreset_mode="next_step").episode_stats
    assert nav_gym_env.make("NavGym-v0", num_envs=3, episode_stats=True, auto_reset=False, final_observation=False).episode_stats
    with pytest.raises(ValueError):                       # the terminal step of a same-step restart is read from its terminal row
        nav_gym_env.make("NavGym-v0", num_envs=3, episode_stats=True, final_observation=False)
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.episode_stats is False
    with pytest.raises(RuntimeError):
        plain.episode_totals()
    assert env.episode_totals() == {k: 0 for k in abi.EPISODE_TOTALS}            # before the first reset(): nothing finished
    assert "episode_stats" not in registry.spec("NavGym-v0")["kwargs"]


# ---- hand-made cases of the specification -----------------------------------------------------------------------------------
B, S = 4, 2
THR = np.full(B, 0.5, np.float32)
DTHR = np.full(B, 0.8, np.float32)


def _row(scan, old_scan=None, prev_xy=(0.0, 0.0), xy=(0.0, 0.0)):
    old = np.full(B, 3.0, np.float32) if old_scan is None else np.asarray(old_scan, np.float32)
    return np.concatenate([old, np.asarray(scan, np.float32), np.asarray(list(prev_xy) + list(xy) + [0, 0, 0], np.float32)])


def _one(auto_reset=spec.AUTORESET_NONE):
    return spec.EpisodeStats(1, B, S, auto_reset, THR, DTHR)


def test_spec_crash_row_suppresses_discomfort():
    s = _one()
    s.update([_row([3, 3, 0.7, 3])], [1.0], [0], [0], [0])                       # inside the discomfort zone only
    assert s.discomfort_steps[0] == 1
    s.update([_row([3, 0.4, 0.7, 3])], [1.0], [0], [0], [0])                     # a beam inside the crash zone as well
    assert s.discomfort_steps[0] == 1 and s.length[0] == 2
    assert s.min_clearance[0] == np.float64(np.float32(0.4)) - np.float64(np.float32(0.5))


def test_spec_outcomes():
    s = _one()
    assert s.update([_row([3, 3, 3, 3])], [2.0], [1], [1.0], [1.0]) == [0]
    assert s.ep_outcome[0] == 3 and s.ep_length[0] == 1 and s.ep_return[0] == 2.0
    assert s.update([_row([3, 3, 3, 3])], [0.5], [1], [0.0], [0.0], truncated=[1]) == [0]
    assert s.ep_outcome[0] == 4
    assert s.update([_row([3, 3, 3, 3])], [0.5], [1], [0.0], [0.0], truncated=None) == [0]
    assert s.ep_outcome[0] == 0                                                  # done without a flag: no bit
    assert s.totals_dict() == dict(episodes=3, successes=1, crashes=1, time_limits=1, steps=3)
    assert (s.ret[0], s.length[0], s.path_length[0], s.min_clearance[0], s.discomfort_steps[0]) == (0, 0, 0, np.inf, 0)


def test_spec_older_stack_slot_is_ignored():
    s = _one()
    s.update([_row([3, 3, 3, 2], old_scan=[0.1, 0.1, 0.1, 0.1])], [0.0], [0], [0], [0])
    assert s.discomfort_steps[0] == 0
    assert s.min_clearance[0] == 2.0 - np.float64(np.float32(0.5))


def test_spec_path_return_and_modes():
    s = _one()
    s.update([_row([3, 3, 3, 3], prev_xy=(1.0, 1.0), xy=(4.0, 5.0))], [0.25], [0], [0], [0])
    s.update([_row([3, 3, 3, 3], prev_xy=(4.0, 5.0), xy=(4.0, 5.5))], [0.5], [0], [0], [0])
    assert s.path_length[0] == 5.5 and s.ret[0] == 0.75 and s.length[0] == 2
    # same-step: the terminal row of a finished arena is final_obs, the row in obs belongs to the next episode
    s = _one(spec.AUTORESET_SAME_STEP)
    s.update([_row([0.1, 3, 3, 3])], [1.0], [1], [0], [1.0], final_obs=[_row([3, 3, 3, 1], prev_xy=(0, 0), xy=(3, 4))])
    assert s.ep_min_clearance[0] == 0.5 and s.ep_path_length[0] == 5.0 and s.ep_outcome[0] == 2
    # next-step: the step that resets an arena is no step of an episode
    s = _one(spec.AUTORESET_NEXT_STEP)
    s.update([_row([3, 3, 3, 3])], [1.0], [0], [0], [0], reset_mask=[0])
    s.update([_row([0.1, 3, 3, 3])], [7.0], [1], [1.0], [0], reset_mask=[1])
    assert (s.length[0], s.ret[0], s.min_clearance[0]) == (1, 1.0, 2.5) and s.totals_dict()["episodes"] == 0
    # clear(mask)
    s = spec.EpisodeStats(2, B, S, spec.AUTORESET_NONE, THR, DTHR)
    s.update([_row([3, 3, 3, 3])] * 2, [1.0, 1.0], [0, 0], [0, 0], [0, 0])
    s.clear([0, 1])
    assert list(s.length) == [1, 0] and list(s.min_clearance) == [2.5, np.inf]
