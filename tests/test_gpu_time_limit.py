"""GPU: the time limit inside the fused step (include/navsim.h navsim_config.max_episode_steps, navsim_step_io.truncated,
ABI 7) -- nothing changes below the limit, the flags, the device against the CPU oracle (which has no limit: the tests apply
the restart the oracle would do at `done` themselves), worlds that draw new maps, and the gym surface (NavGymEnv)."""
import ctypes as C

import numpy as np
import pytest

import ref
from nav_gym_amd import abi
from gpu_support import (gpu, action_rows, env_rollout, eq, fresh_oracle, fresh_sim, limit_config, limit_world, nav_env,  # noqa: F401
                         random_actions, state_equal, to_numpy)

pytestmark = pytest.mark.gpu

E, SIZE, N = 48, 240, 8


def _restart_state(r, mask):
    """navsim_restart_cpu alone: the state-only restart the step does at the end of an episode (NEXT_STEP's restart_next,
    and the state part of the same-step restart)."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    L = ref.lib()
    L.navsim_restart_cpu.argtypes = [C.POINTER(abi.NavsimConfig), C.POINTER(abi.NavsimState), C.c_void_p]
    assert L.navsim_restart_cpu(C.byref(r.cfg), C.byref(r.st), m.ctypes.data) == 0


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ped_model,fmt,final_obs", [
    (abi.AUTORESET_SAME_STEP, abi.PED_NONE, abi.FIELD_U16T, False),      # T = 0: the plain form; T > 0: the featured one
    (abi.AUTORESET_SAME_STEP, abi.PED_NONE, abi.FIELD_F32, False),
    (abi.AUTORESET_NONE, abi.PED_NONE, abi.FIELD_U16T, False),
    (abi.AUTORESET_SAME_STEP, abi.PED_NONE, abi.FIELD_U16T, True),
    (abi.AUTORESET_SAME_STEP, abi.PED_SFM, abi.FIELD_U16T, True),
    (abi.AUTORESET_NEXT_STEP, abi.PED_SFM, abi.FIELD_F32, False),
    (abi.AUTORESET_NEXT_STEP, abi.PED_NONE, abi.FIELD_U16T, False)])
def test_nothing_changes_below_the_limit(gpu, mode, ped_model, fmt, final_obs):
    """A limit beyond the rollout: every output, row, terminal row and state array equals T = 0's bit for bit (for PED_NONE
    same-step calls without final_obs T = 0 runs the plain form of the kernel: featured == plain); truncated stays 0."""
    K = 45
    cfg0 = limit_config(gpu, mode, ped_model, fmt=fmt, T=0)
    cfgT = limit_config(gpu, mode, ped_model, fmt=fmt, T=10 * K)
    arrays, _ = limit_world(gpu, cfg0)
    a, b = fresh_sim(gpu, cfg0, arrays, final_obs), fresh_sim(gpu, cfgT, arrays, final_obs)
    rng = np.random.default_rng(5)
    ends = 0
    for t in range(K):
        act = gpu.torch.from_numpy(random_actions(rng, cfg0.n_envs, t)).to(gpu.dev)
        oa, outa = a.step(act)
        ob, outb = b.step(act)
        assert gpu.torch.equal(oa, ob), "obs at step %d" % t
        for k in outa:
            assert gpu.torch.equal(outa[k], outb[k]), "%s at step %d" % (k, t)
        assert int(outb["truncated"].sum()) == 0
        assert set(outb) == set(outa) | {"truncated"}             # without a limit: the outputs of ABI 6, no more
        if final_obs:
            d = outa["done"] != 0
            for k in a.final:
                assert gpu.torch.equal(a.final[k][d], b.final[k][d]), "%s at step %d" % (k, t)
        ends += int(outa["done"].sum())
    sa, sb = a.numpy_state(), b.numpy_state()
    for k in sa:
        eq(sa[k], sb[k], "state %s" % k)
    assert ends > 5


def _limited_run(gpu, mode, T, K, seed=5):
    cfg = limit_config(gpu, mode, T=T)
    arrays, _ = limit_world(gpu, cfg)
    g = fresh_sim(gpu, cfg, arrays)
    rng = np.random.default_rng(seed)
    rec = []
    for t in range(K):
        _, out = g.step(gpu.torch.from_numpy(random_actions(rng, cfg.n_envs, t)).to(gpu.dev))
        assert ("truncated" in out) == (T > 0)
        rec.append({k: out[k].cpu().numpy().copy() for k in ("done", "truncated", "is_success", "is_crash") if k in out})
    return rec


@pytest.mark.parametrize("mode", [abi.AUTORESET_SAME_STEP, abi.AUTORESET_NONE])
def test_truncation_flags(gpu, mode):
    """truncated = (steps_now >= T) & ~terminal and done = terminal | truncated for every arena and step, steps counted on the
    host; an arena that succeeds or crashes exactly at step T (T taken from an unlimited run) reports truncated = 0."""
    K = 60
    free = _limited_run(gpu, mode, 0, K)
    first = np.full(E, -1)                  # the first episode end of every arena in the unlimited run
    for t in reversed(range(K)):
        first[free[t]["done"] != 0] = t + 1
    cand = sorted(set(int(x) for x in first if 3 <= x <= 20))
    assert cand, first
    T = cand[len(cand) // 2]
    winners = np.flatnonzero(first == T)
    rec = _limited_run(gpu, mode, T, K)
    steps = np.zeros(E, np.int64)
    cut = 0
    for t, o in enumerate(rec):
        steps += 1
        term = (o["is_success"] != 0) | (o["is_crash"] != 0)
        trunc = (steps >= T) & ~term
        eq(o["truncated"], trunc.astype(np.uint8), "truncated at step %d" % t)
        eq(o["done"], (term | trunc).astype(np.uint8), "done at step %d" % t)
        if t + 1 == T:
            assert (o["done"][winners] == 1).all() and (o["truncated"][winners] == 0).all()
        cut += int(trunc.sum())
        if mode != abi.AUTORESET_NONE:
            steps[o["done"] != 0] = 0
    assert cut > E // 2


# ---------------------------------------------------------------------------------------------------------------------------
def test_compositions_hold_for_arenas_that_finish_by_themselves(gpu):
    """The oracle has no limit: the tests below apply the restart it would do at `done`.  Checked first on arenas that finish
    by themselves -- SAME_STEP (PED_NONE): a NONE-mode oracle + terminal rows + RefSim.restart equals a SAME_STEP oracle run;
    NEXT_STEP: a NONE-mode oracle + navsim_restart_cpu leaves the state a NEXT_STEP run leaves after the finishing step."""
    cfg = limit_config(gpu, abi.AUTORESET_SAME_STEP, abi.PED_NONE, S=3)
    _, host = limit_world(gpu, cfg)
    a, b = fresh_oracle(cfg, host, abi.AUTORESET_NONE), fresh_oracle(cfg, host)
    rng = np.random.default_rng(5)
    ends = crash_ends = 0
    for t in range(60):
        act = random_actions(rng, cfg.n_envs, t)
        oa, outa = a.step(act)
        ob, outb = b.step(act)
        outa = {k: v.copy() for k, v in outa.items()}
        m = outa["done"] != 0
        if m.any():
            eq(oa[m], b.final["final_obs"][m], "terminal rows at step %d" % t)
            eq(np.concatenate([outa["achieved_goal"], outa["desired_goal"]], axis=1)[m], b.final["final_goals"][m],
                "terminal goals at step %d" % t)
            oa = a.restart(m)
        eq(oa, ob, "obs at step %d" % t)
        for k in outb:
            eq(a.out[k] if k in ("achieved_goal", "desired_goal") else outa[k], outb[k], "%s at step %d" % (k, t))
        for k in set(a.a) & set(b.a):
            eq(a.a[k], b.a[k], "state %s at step %d" % (k, t))
        ends += int(m.sum()); crash_ends += int((m & (outa["is_crash"] != 0)).sum())
    assert ends > 10 and crash_ends > 2, (ends, crash_ends)

    a, b = fresh_oracle(cfg, host, abi.AUTORESET_NONE), fresh_oracle(cfg, host, abi.AUTORESET_NEXT_STEP)
    rng = np.random.default_rng(5)
    live = np.ones(E, bool)                 # arenas that have not finished before: the two runs agree on them
    checked = 0
    for t in range(60):
        act = random_actions(rng, cfg.n_envs, t)
        _, outa = a.step(act)
        b.step(act)
        m = (outa["done"] != 0) & live
        if m.any():
            _restart_state(a, m)
            for k in ("robot_pose", "robot_goal", "episode", "steps", "done_steps"):
                eq(a.a[k][live], b.a[k][live], "state %s at step %d" % (k, t))
            checked += int(m.sum())
        live &= outa["done"] == 0
    assert checked > 5


@pytest.mark.parametrize("T", [1, 9, 23])
def test_none_mode_against_the_oracle(gpu, T):
    """NAVSIM_AUTORESET_NONE: the unlimited oracle's outputs and rows, done |= truncated; arenas past T stay truncated."""
    cfg = limit_config(gpu, abi.AUTORESET_NONE, abi.PED_SFM, T=T)
    arrays, host = limit_world(gpu, cfg)
    g, r = fresh_sim(gpu, cfg, arrays), fresh_oracle(cfg, host)
    rng = np.random.default_rng(7)
    for t in range(3 * T + 6):
        act = random_actions(rng, cfg.n_envs, t)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        gout = to_numpy(gout)
        trunc = (r.a["steps"] >= T) & (rout["done"] == 0)
        for k in ("reward", "is_success", "is_crash", "distance", "achieved_goal", "desired_goal"):
            eq(gout[k], rout[k], "%s at step %d" % (k, t))
        eq(gout["done"], rout["done"] | trunc, "done at step %d" % t)
        eq(gout["truncated"], trunc.astype(np.uint8), "truncated at step %d" % t)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
    state_equal(g, r, "at the end", skip=("counters",))


@pytest.mark.parametrize("T,S,fmt", [(1, 2, abi.FIELD_U16T), (9, 3, abi.FIELD_U16T), (23, 2, abi.FIELD_F32)])
def test_same_step_against_the_oracle(gpu, T, S, fmt):
    """SAME_STEP, PED_NONE: a truncated arena's terminal row / goals are the unlimited oracle's row after the step; its next
    state and row are RefSim.restart's (navsim_restart_cpu + reset_obs); done_steps records T."""
    cfg = limit_config(gpu, abi.AUTORESET_SAME_STEP, abi.PED_NONE, S=S, fmt=fmt, T=T)
    arrays, host = limit_world(gpu, cfg)
    g, r = fresh_sim(gpu, cfg, arrays, final_obs=True), fresh_oracle(cfg, host)
    rng = np.random.default_rng(9)
    cut = 0
    for t in range(max(3 * T, 40)):
        act = random_actions(rng, cfg.n_envs, t)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        rout = {k: v.copy() for k, v in rout.items()}
        nat = rout["done"] != 0
        trunc = (r.a["steps"] >= T) & ~nat
        fin_obs, fin_goals = r.final["final_obs"].copy(), r.final["final_goals"].copy()
        fin_obs[trunc] = ro[trunc]
        fin_goals[trunc] = np.concatenate([rout["achieved_goal"], rout["desired_goal"]], axis=1)[trunc]
        if trunc.any():
            ro = r.restart(trunc)
            assert (r.a["done_steps"][trunc] == T).all()
        gout = to_numpy(gout)
        for k in ("reward", "is_success", "is_crash", "distance"):
            eq(gout[k], rout[k], "%s at step %d" % (k, t))
        for k in ("achieved_goal", "desired_goal"):
            eq(gout[k], r.out[k], "%s at step %d" % (k, t))
        eq(gout["done"], (nat | trunc).astype(np.uint8), "done at step %d" % t)
        eq(gout["truncated"], trunc.astype(np.uint8), "truncated at step %d" % t)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        d = nat | trunc
        fin = to_numpy(g.final)
        eq(fin["final_obs"][d], fin_obs[d], "terminal rows at step %d" % t)
        eq(fin["final_goals"][d], fin_goals[d], "terminal goals at step %d" % t)
        cut += int(trunc.sum())
        if t % 5 == 4:
            state_equal(g, r, "at step %d" % t, skip=("counters",))
    assert cut > E


@pytest.mark.parametrize("T,ped_model", [(1, abi.PED_NONE), (9, abi.PED_SFM), (23, abi.PED_EXTERNAL), (9, abi.PED_NONE)])
def test_next_step_against_the_oracle(gpu, T, ped_model):
    """NEXT_STEP: the call that truncates returns the terminal row (the unlimited oracle's) with done = truncated = 1 and restarts
    the state (navsim_restart_cpu); the next call resets the arena through its reset mask, truncated 0 there."""
    cfg = limit_config(gpu, abi.AUTORESET_NEXT_STEP, ped_model, S=3 if ped_model == abi.PED_SFM else 2, T=T)
    arrays, host = limit_world(gpu, cfg)
    g, r = fresh_sim(gpu, cfg, arrays), fresh_oracle(cfg, host)
    rng = np.random.default_rng(11)
    cut = 0
    for t in range(max(3 * T + 3, 40)):
        act = random_actions(rng, cfg.n_envs, t)
        if ped_model == abi.PED_EXTERNAL:
            cmd = np.stack([rng.uniform(0, 0.6, (E, N)), rng.uniform(-0.6, 0.6, (E, N))], axis=2)
            g.set_ped_cmd(cmd); r.set_ped_cmd(cmd)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        eq(g.reset_flags.cpu().numpy(), r.reset_flags, "reset flags at step %d" % t)
        trunc = (r.a["steps"] >= T) & (rout["done"] == 0)
        gout = to_numpy(gout)
        for k in ("reward", "is_success", "is_crash", "distance", "achieved_goal", "desired_goal"):
            eq(gout[k], rout[k], "%s at step %d" % (k, t))
        eq(gout["done"], rout["done"] | trunc, "done at step %d" % t)
        eq(gout["truncated"], trunc.astype(np.uint8), "truncated at step %d" % t)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        if trunc.any():
            _restart_state(r, trunc)
            r.out["done"][trunc] = 1
            r.prev_done[trunc] = 1
        cut += int(trunc.sum())
        if t % 5 == 4:
            state_equal(g, r, "at step %d" % t, skip=("counters",))
    assert cut > E // 2


def test_negative_limit_is_rejected(gpu):
    cfg = limit_config(gpu, abi.AUTORESET_SAME_STEP)
    arrays, _ = limit_world(gpu, cfg)
    g = fresh_sim(gpu, cfg, arrays)
    g.cfg.max_episode_steps = -1
    assert g.lib.navsim_step(C.byref(g.cfg), C.byref(g.st), C.byref(g.io), None) == abi.E_ARG
    assert g.lib.navsim_reset_obs(C.byref(g.cfg), C.byref(g.st), C.byref(g.io), None, None) == abi.E_ARG


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,ped_model,fmt", [(9, abi.PED_NONE, abi.FIELD_F32), (5, abi.PED_SFM, abi.FIELD_U16T)])
def test_navsim_regen_path_against_the_oracle(gpu, T, ped_model, fmt):
    """A new world per episode (navsim_regen behind every step, same-step restarts, outdoor maps): the oracle's regen with the
    truncated arenas restarted (navsim_restart_cpu: the state part of the step's restart) and added to its done flags."""
    E_, size = 40, 200
    cfg = gpu.lib.default_config(n_envs=E_, map_h=size, map_w=size, max_peds=6, ped_model=ped_model, n_spawn=6,
                                 auto_reset=abi.AUTORESET_SAME_STEP, seed=19, field_format=fmt, regen_cap=E_, min_goal_dist=3.0,
                                 max_goal_dist=8.0, spawn_clearance=0.9, ped_min_robot_dist=2.0, ped_min_goal_dist=4.0,
                                 regen_plan=0, regen_indoor_ratio=0.0, defer_reset_scan=1)
    gpu.world.lidar_1081(cfg)
    cfg.max_episode_steps = T
    arrays, host = limit_world(gpu, cfg, occ=gpu.world.make_maps(E_, size, 19), n_peds=5, min_goal_dist=10.0, max_goal_dist=20.0)
    g = gpu.sim.NavSim(cfg, arrays)
    r = ref.RefSim(cfg, host)
    eq(g.reset_obs().cpu().numpy(), r.reset_obs(), "reset obs")
    rng = np.random.default_rng(6)
    cut = 0
    for t in range(3 * T + 5):
        act = random_actions(rng, cfg.n_envs, t)
        _, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        _, rout = r.step(act)
        trunc = (r.a["steps"] >= T) & (rout["done"] == 0)
        gout = to_numpy(gout)
        for k in ("reward", "is_success", "is_crash", "distance"):
            eq(gout[k], rout[k], "%s at step %d" % (k, t))
        eq(gout["done"], rout["done"] | trunc, "done at step %d" % t)
        eq(gout["truncated"], trunc.astype(np.uint8), "truncated at step %d" % t)
        if trunc.any():
            _restart_state(r, trunc)
            r.out["done"][trunc] = 1
        eq(g.regen().cpu().numpy(), r.regen(), "obs after regen at step %d" % t)
        for k in ("achieved_goal", "desired_goal"):
            eq(g.out[k].cpu().numpy(), r.out[k], "%s after regen at step %d" % (k, t))
        cut += int(trunc.sum())
        if trunc.any() or t % 5 == 4:
            state_equal(g, r, "after regen at step %d" % t, skip=("counters",))
    assert cut > E_ // 2
    assert g.counters()["regen_unserved"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
def _same(ra, rb):
    import torch
    assert torch.equal(ra[0], rb[0])
    for t, (a, b) in enumerate(zip(ra[1:], rb[1:])):
        for k in a:
            if k == "final":
                assert torch.equal(a[k][a["done"]], b[k][b["done"]]), (k, t)
            else:
                assert torch.equal(a[k], b[k]), (k, t)


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_staged_worlds_equal_navsim_regen_with_the_limit(gpu, mode):
    """The env's default reset path for randomize_maps (worlds staged ahead, installed inside the step) is bit-identical to
    pregen_pipeline=0 (navsim_regen behind every step) over the whole rollout with the limit on; no cap binds in either."""
    T, K = 9, 30
    a = nav_env(randomize_maps=True, autoreset_mode=mode, max_episode_steps=T, use_graphs=False)
    b = nav_env(randomize_maps=True, autoreset_mode=mode, max_episode_steps=T, pregen_pipeline=0, use_graphs=False)
    assert a.pregen_pipeline > 0 and b.pregen_pipeline == 0
    acts = action_rows(K, 48)
    ra, rb = env_rollout(a, acts), env_rollout(b, acts)
    _same(ra, rb)
    assert sum(int(x["trunc"].sum()) for x in ra[1:]) > 24
    assert a.counters()["regen_unserved"] == 0 and b.counters()["regen_unserved"] == 0
    a.close(); b.close()


def test_graphs_equal_plain_launches_with_the_limit(gpu):
    T, K = 7, 24
    a = nav_env(randomize_maps=True, max_episode_steps=T, pregen_pipeline=0, use_graphs=True)
    b = nav_env(randomize_maps=True, max_episode_steps=T, pregen_pipeline=0, use_graphs=False)
    assert a.use_graphs and not b.use_graphs
    acts = action_rows(K, 48)
    ra, rb = env_rollout(a, acts), env_rollout(b, acts)
    _same(ra, rb)
    assert sum(int(x["trunc"].sum()) for x in ra[1:]) > 24
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------
def test_gym_surface_single_arena(gpu):
    """E = 1: the first T - 1 steps equal an unlimited env's; step T: done True, TimeLimit.truncated True, same reward; reset()."""
    T = 9
    a = nav_env(num_envs=1, max_episode_steps=T, pedestrian_model="none", num_humans=0)
    b = nav_env(num_envs=1, pedestrian_model="none", num_humans=0)
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa["observation"], ob["observation"])
    act = np.array([0.0, 0.3])                                 # turning on the spot: no success, no crash
    for t in range(1, T + 1):
        oa, rwa, da, ia = a.step(act)
        ob, rwb, db, ib = b.step(act)
        assert np.array_equal(oa["observation"], ob["observation"]) and rwa == rwb and db is False
        assert set(ia) == set(ib) | {"TimeLimit.truncated"} and type(ia["TimeLimit.truncated"]) is bool
        assert da is (t == T) and ia["TimeLimit.truncated"] is (t == T), t
    a.reset()
    _, _, da, ia = a.step(act)
    assert da is False and ia["TimeLimit.truncated"] is False
    a.close(); b.close()


def test_gym_surface_same_step(gpu):
    """E > 1, same-step: the final_observation rows of truncated arenas equal the unlimited env's rows at that step (until an
    arena's first truncation the two rollouts are one); no episode runs longer than T steps (counted on the host from done)."""
    import torch
    T, K = 9, 30
    a = nav_env(max_episode_steps=T, pedestrian_model="none", num_humans=0)
    b = nav_env(pedestrian_model="none", num_humans=0)
    acts = action_rows(K, 48)
    ra, rb = env_rollout(a, acts), env_rollout(b, acts)
    same = torch.ones(48, dtype=torch.bool, device=ra[0].device)
    length = torch.zeros(48, dtype=torch.int64, device=ra[0].device)
    compared = 0
    for t in range(1, K + 1):
        x, y = ra[t], rb[t]
        length += 1
        assert int(length.max()) <= T, t
        assert not bool((x["trunc"] & ~x["done"]).any()) and bool(x["done"][length >= T].all()), t
        assert bool((length[x["trunc"]] == T).all()), t
        m = x["trunc"] & same
        assert torch.equal(x["final"][m], y["obs"][m]), t
        keep = same & ~x["trunc"]
        assert torch.equal(x["obs"][keep], y["obs"][keep]) and torch.equal(x["done"][keep], y["done"][keep]), t
        compared += int(m.sum())
        same &= ~x["trunc"]
        length[x["done"]] = 0
    assert compared > 5
    a.close(); b.close()


def test_gym_surface_next_step_and_state_dict(gpu):
    """E > 1, next-step: the next call's reset_mask covers the arenas truncated in this one.  state_dict() at step k < T loaded
    into a fresh env truncates at the same steps as the uninterrupted run."""
    import torch
    T, K, k0 = 9, 30, 4
    a = nav_env(max_episode_steps=T, autoreset_mode="next_step", pedestrian_model="none", num_humans=0)
    ra = env_rollout(a, action_rows(K, 48))
    for t in range(1, K):
        assert torch.equal(ra[t + 1]["reset"], ra[t]["done"]) and bool((ra[t + 1]["reset"] | ~ra[t]["trunc"]).all()), t
        assert not bool((ra[t + 1]["trunc"] & ra[t + 1]["reset"]).any()), t
    assert sum(int(x["trunc"].sum()) for x in ra[1:]) > 24
    a.close()

    a, b = nav_env(max_episode_steps=T), nav_env(max_episode_steps=T)
    a.reset(); b.reset()
    acts = action_rows(3 * T, 48, seed=8)
    for t in range(k0):
        a.step(acts[t])
    b.load_state_dict(a.state_dict())
    cut = 0
    for t in range(k0, 3 * T):
        oa, rwa, da, ia = a.step(acts[t])
        ob, rwb, db, ib = b.step(acts[t])
        assert torch.equal(oa["observation"], ob["observation"]) and torch.equal(da, db) and torch.equal(rwa, rwb), t
        assert torch.equal(ia["TimeLimit.truncated"], ib["TimeLimit.truncated"]), t
        cut += int(ib["TimeLimit.truncated"].sum())
    assert cut > 0
    a.close(); b.close()


def test_two_shards_equal_one_world_with_the_limit(gpu):
    import torch
    T, K = 7, 20
    kw = dict(max_episode_steps=T, randomize_maps=True, pregen_pipeline=0, use_graphs=False)
    one = nav_env(**kw)
    s0, s1 = nav_env(num_envs=24, env_index_base=0, **kw), nav_env(num_envs=24, env_index_base=24, **kw)
    acts = action_rows(K, 48)
    r1 = env_rollout(one, acts)
    o0, o1 = s0.reset(), s1.reset()
    assert torch.equal(torch.cat([o0["observation"], o1["observation"]]), r1[0])
    for t in range(K):
        a, rew_a, da, ia = s0.step(acts[t][:24])
        b, rew_b, db, ib = s1.step(acts[t][24:])
        x = r1[t + 1]
        assert torch.equal(torch.cat([a["observation"], b["observation"]]), x["obs"]), t
        assert torch.equal(torch.cat([da, db]), x["done"]) and torch.equal(torch.cat([rew_a, rew_b]), x["rew"]), t
        assert torch.equal(torch.cat([ia["TimeLimit.truncated"], ib["TimeLimit.truncated"]]), x["trunc"]), t
    assert sum(int(x["trunc"].sum()) for x in r1[1:]) > 24
    for e in (one, s0, s1):
        e.close()
