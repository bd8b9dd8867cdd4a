"""GPU: navsim_ped_orca (include/navsim.h) -- ORCA pedestrians computed from the simulator's state by one kernel -- against
its specification (tests/ped_orca_spec.py, a composition of the CPU oracle's functions) bit for bit: single calls over the
shapes at which the kernel packs its wavefronts differently, closed loops through navsim_step, and the gym surface."""
import numpy as np
import pytest

import ped_orca_spec as spec
from nav_gym_amd import abi
from gpu_support import (gpu, action_rows, env_rollout, eq, fresh_oracle, fresh_sim, limit_config, limit_world, nav_env,  # noqa: F401
                         orca_pair, random_actions, small_orca_config, state_equal, to_numpy, ORCA_SENTINEL as SENTINEL)

pytestmark = pytest.mark.gpu

def _check_call(gpu, g, r, p, what):
    g.t["ped_cmd"].fill_(SENTINEL)
    r.a["ped_cmd"][...] = SENTINEL
    want_cmd, want_head, _ = spec.ped_orca(r.cfg, r.a, p)
    got = g.ped_orca({k: p[k] for k in spec.KEYS}).cpu().numpy()
    live = np.arange(r.cfg.max_peds)[None, :] < r.a["n_peds"][:, None]
    assert live.any() or r.cfg.n_envs == 0
    assert (want_cmd[~live] == SENTINEL).all() and not (want_cmd[live] == SENTINEL).any()
    eq(got, want_cmd, "ped_cmd (%s)" % what)                        # live rows, and dead rows still holding the sentinel
    eq(g.numpy_state("ped_wp_head")["ped_wp_head"], want_head, "ped_wp_head (%s)" % what)
    return want_cmd, want_head


def _two_pops(host):
    """Arena 1, pedestrian 0: a route of four waypoints whose first two lie within 1 m -- the call pops two (head 0 -> 2)."""
    x, y = host["ped_pose"][1, 0, :2]
    host["ped_waypoints"][1, 0, :4] = [[x + 0.3, y], [x, y + 0.6], [x + 2.0, y + 2.0], [x + 4.0, y]]
    host["ped_n_waypoints"][1, 0] = 4


@pytest.mark.parametrize("E,N,kw", [
    (45, 8, {}),                               # 8 arenas per wavefront, the last one partial; ragged n_peds with 0 and 1
    (45, 8, dict(robot_visible=0)),
    (7, 20, {}),                               # 3 arenas per wavefront, 4 lanes idle
    (5, 33, {}),                               # one arena per wavefront from here on
    (6, 63, {}),
    (6, 63, dict(max_neighbors=63)),           # lists of 63 entries: 160 KB of LDS per wavefront
    (5, 1, {}),                                # nobody but the robot
    (5, 1, dict(robot_visible=0)),             # lists of no entries
])
def test_single_call_vs_specification(gpu, E, N, kw):
    cfg = small_orca_config(gpu, E, N)
    n_peds = N
    if N == 8:
        n_peds = np.array([(3 * e + 2) % 9 for e in range(E)], np.int32)         # 2, 5, 8, 2, ...; arena 2 -> 8
        n_peds[1] = 6; n_peds[4] = 0; n_peds[7] = 1; n_peds[44] = 0
        assert set(n_peds) >= {0, 1, 8}
    g, r = orca_pair(gpu, cfg, n_peds, hand_made=_two_pops if N == 8 else None)
    p = spec.params(cfg, **kw)
    _, head = _check_call(gpu, g, r, p, "E %d N %d %s" % (E, N, kw))
    if N == 8:
        assert r.a["ped_wp_head"][1, 0] == 0 and head[1, 0] == 2


def test_crowded_world_closed_loop(gpu):
    """12 pedestrians per 6 m arena: they do come closer than the combined radius, so the overlapping-agents branch and the
    infeasible linear program (lp3) run.  80 steps, every call against the specification."""
    cfg = small_orca_config(gpu, 8, 12, size=120)
    g, r = orca_pair(gpu, cfg, 12, moving=False, min_goal_dist=1.0, max_goal_dist=3.0, robot_clearance=0.6)
    p = spec.params(cfg)
    comb = 2 * (p["ped_radius"] + 0.01)
    iu = np.triu_indices(12, 1)
    rng = np.random.default_rng(5)
    overlaps = 0
    for t in range(80):
        xy = r.a["ped_pose"][:, :, :2]
        d = np.sqrt(((xy[:, :, None] - xy[:, None]) ** 2).sum(-1))
        overlaps += int((d[:, iu[0], iu[1]] < comb).sum())
        cmd, head = _check_call(gpu, g, r, p, "step %d" % t)
        r.a["ped_wp_head"][...] = head
        r.set_ped_cmd(cmd)
        act = random_actions(rng, cfg.n_envs, t)
        g.step(gpu.torch.from_numpy(act).to(gpu.dev)); r.step(act)
    state_equal(g, r, "after 80 steps", skip=("counters",))
    print("crowded world: %d of %d pair-steps closer than the combined radius" % (overlaps, 8 * 66 * 80))
    assert overlaps > 0


@pytest.mark.parametrize("mode", [abi.AUTORESET_SAME_STEP, abi.AUTORESET_NEXT_STEP])
def test_closed_loop_vs_oracle(gpu, mode):
    """ped_orca(); step(act) for 40 steps of 48 arenas with 1081 beams: observations, every output and every state array equal
    specification + oracle step bit for bit, through episode ends and restarts."""
    cfg = limit_config(gpu, mode, abi.PED_EXTERNAL)
    arrays, host = limit_world(gpu, cfg, v_pref_range=(0.3, 0.6))
    g, r = fresh_sim(gpu, cfg, arrays), fresh_oracle(cfg, host)
    p = spec.params(cfg)
    rng = np.random.default_rng(5)
    ends = 0
    for t in range(40):
        cmd, head, _ = spec.ped_orca(cfg, r.a, p)
        r.a["ped_wp_head"][...] = head
        r.set_ped_cmd(cmd)
        g.ped_orca()
        act = random_actions(rng, cfg.n_envs, t)
        obs, out = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        eq(obs.cpu().numpy(), ro, "observations at step %d" % t)
        out = to_numpy(out)
        for k in rout:
            eq(out[k], rout[k], "%s at step %d" % (k, t))
        state_equal(g, r, "at step %d" % t, skip=("counters",))
        ends += int(rout["done"].sum())
    assert ends >= 5, ends


def _spec_state(env):
    names = ("ped_cmd", "ped_wp_head", "ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints", "n_peds",
             "robot_pose", "prev_action")
    return env.sim.numpy_state(*names)


def test_gym_surface_equals_external_fed_by_the_specification(gpu):
    kw = dict(num_humans=5, seed=23)
    a = nav_env(pedestrian_model="orca", **kw)
    b = nav_env(pedestrian_model="external", **kw)
    oa, ob = a.reset()["observation"], b.reset()["observation"]
    assert gpu.torch.equal(oa, ob)
    p = spec.params(a.sim.cfg)
    for t, act in enumerate(action_rows(25, 48)):
        cmd, _, _ = spec.ped_orca(b.sim.cfg, _spec_state(b), p)
        xa, xb = a.step(act), b.step(act, human_actions=cmd)
        assert gpu.torch.equal(xa[0]["observation"], xb[0]["observation"]), t
        assert gpu.torch.equal(xa[1], xb[1]) and gpu.torch.equal(xa[2], xb[2]), t
    assert gpu.torch.equal(a.sim.t["ped_pose"], b.sim.t["ped_pose"])
    # human_actions= still overrides the model
    a.step(act, human_actions=np.zeros((48, 5, 2)))
    assert float(a.sim.t["ped_cmd"].abs().max()) == 0.0
    a.close(); b.close()


def test_gym_surface_with_new_maps_per_episode(gpu):
    env = nav_env(pedestrian_model="orca", num_humans=5, randomize_maps=True, pregen_pipeline=0)
    assert env.pregen_pipeline == 0
    rec = env_rollout(env, action_rows(30, 48))
    assert not env._graphed and sum(int(x["done"].sum()) for x in rec[1:]) > 0
    assert env.counters()["regen_unserved"] == 0
    env.close()


def test_two_shards_equal_one_world(gpu):
    kw = dict(pedestrian_model="orca", num_humans=5)
    full = nav_env(**kw)
    shards = [nav_env(num_envs=24, env_index_base=24 * i, **kw) for i in (0, 1)]
    acts = action_rows(12, 48)
    rf = env_rollout(full, acts)
    rs = [env_rollout(s, [x[24 * i:24 * i + 24] for x in acts]) for i, s in enumerate(shards)]
    torch = gpu.torch
    assert torch.equal(rf[0], torch.cat([r[0] for r in rs]))
    for t in range(1, len(rf)):
        for k in ("obs", "rew", "done"):
            assert torch.equal(rf[t][k], torch.cat([r[t][k] for r in rs])), (k, t)
    assert torch.equal(full.sim.t["ped_pose"], torch.cat([s.sim.t["ped_pose"] for s in shards]))
    for e in [full] + shards:
        e.close()
