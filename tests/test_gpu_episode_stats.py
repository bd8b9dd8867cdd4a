"""GPU: episode statistics (include/navsim.h navsim_episode_stats_update / _clear; NavGymEnv(episode_stats=True)) against the
NumPy specification of tests/episode_stats_spec.py, bit for bit: the kernel on synthetic buffers, rollouts through the gym
surface under the three reset protocols, one world on its three step paths, the rows' lifetime, the state_dict round trip and
the single-environment form."""
import collections
import ctypes as C

import numpy as np
import pytest

import episode_stats_spec as spec
from gpu_support import gpu, same_bits, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

KEYS = (("r", "ep_return"), ("l", "ep_length"), ("path_length", "ep_path_length"), ("min_clearance", "ep_min_clearance"),
        ("discomfort_steps", "ep_discomfort_steps"), ("outcome", "ep_outcome"))


# ---- a. the kernel on synthetic buffers ---------------------------------------------------------------------------------------
E_A, B_A, S_A = 5, 65, 2            # two workgroups of four arenas, the second partial; lane 0 takes a second beam; two slots
KINDS = ((0, 1, 2, 1, 2), (1, 2, 0, 0, 1), (2, 0, 1, 2, 0))       # per call and arena: 0 clear, 1 discomfort, 2 crash + discomfort
DONE = ((4,), (1, 2), (3,))                                        # arenas that finish in calls 1, 2, 3


def _synthetic_calls(with_truncated):
    rng = np.random.default_rng(11)
    D = S_A * B_A + abi.OBS_TAIL
    thr = rng.uniform(0.2, 0.4, B_A).astype(np.float32)
    dthr = (thr + np.float32(0.3)).astype(np.float32)

    def rows(c):
        r = np.empty((E_A, D), np.float32)
        r[:, :B_A] = rng.uniform(1.0, 5.0, (E_A, B_A))
        r[:, 3] = 0.01; r[:, B_A - 1] = 0.005                      # the OLDER slot holds smaller values than the newest ever does
        r[:, B_A:2 * B_A] = rng.uniform(1.0, 5.0, (E_A, B_A))
        r[:, 2 * B_A:] = rng.uniform(-3.0, 3.0, (E_A, abi.OBS_TAIL))
        for e in range(E_A):                                       # the row's minimum sits at beam 64: lane 0's second beam
            kind = KINDS[c][e]
            r[e, B_A + 64] = thr[64] + np.float32((0.45, 0.1, -0.05)[kind])
            if kind == 2:
                r[e, B_A + 7] = dthr[7] - np.float32(0.01)         # inside the discomfort zone as well
        return r

    calls, prev_done = [], np.zeros(E_A, np.uint8)
    for c in range(3):
        done = np.zeros(E_A, np.uint8); done[list(DONE[c])] = 1
        succ, crash, trunc = np.zeros(E_A, np.float32), np.zeros(E_A, np.float32), np.zeros(E_A, np.uint8)
        if c == 0:
            crash[4] = 1
        if c == 1:
            succ[1] = 1; succ[2] = 1; crash[2] = 1                 # arena 2: both flags, outcome 3
        if c == 2:
            trunc[3] = 1                                           # (read only when the array is given)
        calls.append(dict(obs=rows(c), final_obs=rows(c), reward=rng.normal(size=E_A), done=done, is_success=succ, is_crash=crash,
                          truncated=trunc if with_truncated else None, reset_mask=prev_done.copy()))
        prev_done = done
    return thr, dthr, calls


@pytest.mark.parametrize("with_truncated", [False, True])
@pytest.mark.parametrize("mode", [abi.AUTORESET_NONE, abi.AUTORESET_SAME_STEP, abi.AUTORESET_NEXT_STEP])
def test_kernel_equals_the_spec_on_synthetic_buffers(gpu, mode, with_truncated):
    """Three consecutive updates: every accumulator, every published row and every total equals the specification's bit for
    bit after each call.  An arena that finishes in call 2 accumulates afresh in call 3 (next-step: it is in call 3's reset
    mask instead and stays untouched, and arena 4, finished in call 1, is the one that starts afresh)."""
    torch, L = gpu.torch, gpu.lib.load()
    thr, dthr, calls = _synthetic_calls(with_truncated)
    cfg = gpu.lib.default_config(n_envs=E_A, n_beams=B_A, n_scan_stack=S_A, auto_reset=mode)
    ref = spec.EpisodeStats(E_A, B_A, S_A, mode, thr, dthr)
    dev = {k: torch.full((E_A,), 77, dtype=getattr(torch, np.dtype(d).name), device=gpu.dev) for k, d in spec.ACCUMULATORS}
    dev.update({k: torch.zeros(E_A, dtype=getattr(torch, np.dtype(d).name), device=gpu.dev) for k, d in spec.PUBLISHED})
    dev["totals"] = torch.zeros(len(spec.TOTALS), dtype=torch.int64, device=gpu.dev)
    stats = abi.NavsimEpisodeStats()
    for k, v in dev.items():
        setattr(stats, k, v.data_ptr())
    st = abi.NavsimState()
    t_thr, t_dthr = to_device(gpu, thr), to_device(gpu, dthr)
    st.scan_threshold, st.scan_discomfort = t_thr.data_ptr(), t_dthr.data_ptr()
    assert L.navsim_episode_stats_clear(C.byref(cfg), C.byref(stats), None, None) == 0       # 77 -> (0, 0, 0, +inf, 0)

    def compare(what):
        torch.cuda.synchronize()
        for k, _ in spec.ACCUMULATORS + spec.PUBLISHED:
            same_bits(dev[k].cpu().numpy(), getattr(ref, k), "%s: %s" % (what, k))
        assert dev["totals"].cpu().numpy().tolist() == ref.totals.tolist(), what

    compare("after clear")
    for c, call in enumerate(calls):
        args = dict(call)
        if mode != abi.AUTORESET_SAME_STEP:
            args["final_obs"] = None
        if mode != abi.AUTORESET_NEXT_STEP:
            args["reset_mask"] = None
        keep = {k: to_device(gpu, v) for k, v in args.items() if v is not None}
        io = abi.NavsimStepIO()
        for k, v in keep.items():
            setattr(io, k, v.data_ptr())
        assert L.navsim_episode_stats_update(C.byref(cfg), C.byref(st), C.byref(io), C.byref(stats), None) == 0
        finished = ref.update(**args)
        assert finished == list(DONE[c])
        compare("call %d" % (c + 1))
    want = dict(episodes=4, successes=2, crashes=2, time_limits=int(with_truncated), steps=ref.totals_dict()["steps"])
    assert ref.totals_dict() == want
    if mode == abi.AUTORESET_NEXT_STEP:
        assert ref.length.tolist() == [3, 0, 0, 0, 1]              # arenas 1, 2: reset by call 3, untouched; arena 4 afresh
    else:
        assert ref.length.tolist() == [3, 1, 1, 0, 2]
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    t_mask = to_device(gpu, mask)
    assert L.navsim_episode_stats_clear(C.byref(cfg), C.byref(stats), t_mask.data_ptr(), None) == 0
    ref.clear(mask)
    compare("after clear(mask)")


# ---- b - f. through NavGymEnv ------------------------------------------------------------------------------------------------
def _env(**kw):
    import nav_gym_amd
    from nav_gym_amd import registry
    # 5 m arenas: two small boxes each, so that a robot has room to drive before it meets a wall
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([2, 2], "int"), obstacle_width=([0.3, 0.5], "float"))
    base = dict(num_envs=6, map_size=100, n_beams=64, seed=SEED, plan_paths=False, min_goal_dist=2.0, max_goal_dist=4.0,
                indoor_ratio=0.0, num_humans=2, max_episode_steps=12, episode_stats=True, env_param_range=ranges)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


SEED = 3            # chosen on the device so that the rollouts below hold crash and time-limit episodes under every protocol


def _drive(E):
    """Half the arenas drive straight ahead at full speed, half stand still."""
    a = np.zeros((E, 2))
    a[: E // 2, 0] = 0.5
    return a


def _np(x):
    return x.detach().cpu().numpy()


def _rollout(env, K, reset_done=False, check_spec=True, first_reset=True):
    """K steps; the specification is fed what step() itself returned.  Returns the finished episodes in order, as
    (step, arena, {key: value}), after comparing each with the specification's row bit for bit."""
    import torch
    cfg = env.cfg
    if first_reset:
        env.reset()
    ref = spec.EpisodeStats(env.num_envs, cfg.n_beams, cfg.n_scan_stack, cfg.auto_reset, _np(env.scan_threshold),
                            _np(env.scan_discomfort_threshold))
    act = _drive(env.num_envs)
    episodes = []
    for t in range(K):
        o, rew, done, info = env.step(act)
        d = _np(done)
        assert "episode" in info and info["_episode"] is done
        ep = {name: _np(info["episode"][name]) for name, _ in KEYS}
        fin = _np(info["final_observation"]["observation"]) if "final_observation" in info else None
        finished = ref.update(_np(o["observation"]), _np(rew), d, _np(info["is_success"]), _np(info["is_crash"]),
                              truncated=_np(info["TimeLimit.truncated"]) if "TimeLimit.truncated" in info else None,
                              final_obs=fin, reset_mask=_np(info["reset_mask"]) if "reset_mask" in info else None)
        assert finished == np.flatnonzero(d).tolist()
        for e in finished:
            row = {name: ep[name][e] for name, _ in KEYS}
            if check_spec:
                for name, k in KEYS:
                    same_bits(row[name], getattr(ref, k)[e], "step %d arena %d %s" % (t, e, name))
            episodes.append((t, e, row))
        if reset_done and d.any():
            env.reset(mask=done)
            ref.clear(d)
    torch.cuda.synchronize()
    if check_spec:
        for k, _ in spec.ACCUMULATORS:
            same_bits(_np(env.sim.ep_acc[k]), getattr(ref, k), "accumulator %s" % k)
    return episodes, ref


@pytest.mark.parametrize("protocol", ["same_step", "next_step", "reset_mask"])
def test_rollouts_equal_the_spec(gpu, protocol):
    """40 steps of six arenas with a time limit of 12: info['episode'] of every finished episode and episode_totals() equal
    the specification fed with step()'s own return values, under same-step and next-step auto-reset and under
    auto_reset=False with reset(mask=done)."""
    kw = dict(auto_reset=False) if protocol == "reset_mask" else dict(autoreset_mode=protocol)
    env = _env(**kw)
    episodes, ref = _rollout(env, 40, reset_done=protocol == "reset_mask")
    outcomes = [int(row["outcome"]) for _, _, row in episodes]
    print(protocol, "episodes", len(episodes), "outcomes", sorted(collections.Counter(outcomes).items()),
          "lengths", sorted(collections.Counter(int(row["l"]) for _, _, row in episodes).items()))
    totals = env.episode_totals()
    assert totals == ref.totals_dict()
    assert totals["episodes"] == len(episodes) and totals["steps"] == sum(int(row["l"]) for _, _, row in episodes)
    assert any(o & spec.CRASH for o in outcomes), "the rollout holds no crash episode"
    assert any(o & spec.TIME_LIMIT for o in outcomes), "the rollout holds no time-limit episode"
    assert all(int(row["l"]) <= 12 for _, _, row in episodes)
    assert env.episode_totals() == {k: 0 for k in spec.TOTALS}                 # reset=True: counted since the last call
    env.close()


def test_one_world_on_three_step_paths(gpu):
    """randomize_maps: navsim_regen behind every step, the pipelined reset path (the default) and the graph replay run the
    same rollout -- and publish the same finished episodes, each equal to the specification."""
    kw = dict(num_envs=12, map_size=200, min_goal_dist=2.0, max_goal_dist=6.0, num_humans=3, randomize_maps=True,
              max_episode_steps=9)
    envs = [_env(pregen_pipeline=0, use_graphs=False, **kw), _env(use_graphs=False, **kw), _env(use_graphs=True, **kw)]
    assert [e.pregen_pipeline > 0 for e in envs] == [False, True, False]
    runs = [_rollout(e, 30)[0] for e in envs]
    assert [e._step_path for e in envs] == ["plain", "pipelined", "graphed"]
    assert len(runs[0]) >= 12
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for (t0, e0, r0), (t1, e1, r1) in zip(runs[0], other):
            assert (t0, e0) == (t1, e1)
            for name, _ in KEYS:
                same_bits(r0[name], r1[name], "step %d arena %d %s" % (t0, e0, name))
    totals = [e.episode_totals() for e in envs]
    assert totals[0] == totals[1] == totals[2] and totals[0]["episodes"] == len(runs[0])
    for e in envs:
        e.close()


def test_rows_stay_intact_through_the_next_step(gpu):
    """The documented pair lifetime: what step t returned in info['episode'] is unchanged after step t + 1."""
    import torch
    env = _env(max_episode_steps=2)                                 # somebody finishes in every other step
    env.reset()
    act, checked = _drive(6), 0
    prev = None
    for t in range(9):
        _, _, done, info = env.step(act)
        if prev is not None:
            views, copies, was_done = prev
            for name, _ in KEYS:
                assert torch.equal(views[name][was_done], copies[name][was_done]), (t, name)
            checked += int(was_done.sum())
        prev = (info["episode"], {k: v.clone() for k, v in info["episode"].items()}, done.clone())
    assert checked >= 12
    env.close()


def test_state_dict_round_trip(gpu):
    """7 steps, snapshot, 10 more steps; load; the same 10 steps again publish the same rows and totals.  A snapshot without
    the statistics loads with cleared ones; one with them loads into an environment without the feature."""
    env = _env()
    _rollout(env, 7)
    sd = env.state_dict()
    assert all("episode." + k in sd for k, _ in spec.ACCUMULATORS) and "episode.totals" in sd
    first, _ = _rollout(env, 10, check_spec=False, first_reset=False)
    totals_first = env.episode_totals(reset=False)
    env.load_state_dict(sd)
    for k, _ in spec.ACCUMULATORS:
        same_bits(_np(env.sim.ep_acc[k]), sd["episode." + k].numpy(), k)
    second, _ = _rollout(env, 10, check_spec=False, first_reset=False)
    assert len(first) == len(second) > 0
    for (t0, e0, r0), (t1, e1, r1) in zip(first, second):
        assert (t0, e0) == (t1, e1)
        for name, _ in KEYS:
            same_bits(r0[name], r1[name], "step %d arena %d %s" % (t0, e0, name))
    assert env.episode_totals(reset=False) == totals_first
    bare = {k: v for k, v in sd.items() if not k.startswith("episode.")}
    env.load_state_dict(bare)
    assert env.episode_totals() == {k: 0 for k in spec.TOTALS}
    assert _np(env.sim.ep_acc["length"]).tolist() == [0] * 6 and np.isinf(_np(env.sim.ep_acc["min_clearance"])).all()
    plain = _env(episode_stats=False)
    plain.reset()
    plain.load_state_dict(sd)                                       # the statistics are ignored
    _, _, _, info = plain.step(_drive(6))
    assert "episode" not in info and "_episode" not in info
    env.close(); plain.close()


def test_single_environment(gpu):
    """num_envs == 1: info['episode'] appears only in the step that ends the episode, as Python scalars."""
    env = _env(num_envs=1, max_episode_steps=5)
    assert not env.auto_reset
    for episode in range(2):
        env.reset()
        for t in range(5):
            _, rew, done, info = env.step(np.zeros(2))
            assert ("episode" in info) == done and "_episode" not in info
            if done:
                break
        assert done
        ep = info["episode"]
        assert set(ep) == {name for name, _ in KEYS}
        assert ep["l"] == t + 1 and type(ep["l"]) is int and type(ep["r"]) is float and type(ep["outcome"]) is int
        assert type(ep["path_length"]) is float and type(ep["min_clearance"]) is float and type(ep["discomfort_steps"]) is int
        if info["TimeLimit.truncated"]:
            assert t == 4 and ep["outcome"] == spec.TIME_LIMIT and ep["path_length"] == 0.0
    assert env.episode_totals()["episodes"] == 2
    env.close()
