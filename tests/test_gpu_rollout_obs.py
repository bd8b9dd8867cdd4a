"""GPU: rollout observations (include/navsim.h navsim_rollout_obs) against navsim_step itself, with scan noise ON.  The entry is
called once; then, for every sequence, the saved state and observation are put back, navsim_step runs H times with that sequence's
actions -- each call's observation the next call's obs_prev -- and everything both return (row, goals, reward, pose, length,
outcome, distance) is compared bit for bit up to min(length, exact_steps).  Ends inside the horizon with the crash re-scan,
same-step terminal rows, H = 1 against navsim_lookahead_obs, noise off against navsim_rollout at range_max, the re-plan that is
left out, the shapes, the skip mask, rows='last' and NavGymEnv follow.  The worlds are shaped like
tests/test_gpu_lookahead_obs.py's four."""
import numpy as np
import pytest

import lookahead_call as lc
import lookahead_obs_call as loc
import rollout_call as rc
import rollout_obs_call as roc
from gpu_support import eq, gpu, nav_env, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

B = 67                                                                                     # two chunks, the second partial
GRID9 = np.array([(v, w) for v in (0.0, 0.25, 0.5) for w in (-0.6, 0.0, 0.6)])          # 3 linear velocities x 3 turn rates
FACE_A, FACE_B = 80, 40                                                                    # x cell of the block's face, worlds (a) / (b)


def warm(gpu, g, seed, cmds=False):
    """Five seeded random steps with scan noise on: prev_action, the waypoint heads, the leg odometry and the scan stack are live."""
    rng = np.random.default_rng(seed)
    for _ in range(5):
        if cmds:
            g.set_ped_cmd(np.stack([rng.uniform(0, 0.6, g.t["ped_cmd"].shape[:2]), rng.uniform(-0.6, 0.6, g.t["ped_cmd"].shape[:2])], axis=2))
        g.step(to_device(gpu, random_actions(rng, g.cfg.n_envs)))


def histories(g, S):
    """Arenas 1 and 2 at n_hist 0 and 1 (the stack fill), arena 5 at 0, the others where the warm-up left them: S - 1."""
    if S > 1:
        g.t["n_hist"][1] = 0; g.t["n_hist"][2] = 1; g.t["n_hist"][5] = 0
        nh = g.t["n_hist"].cpu().numpy()
        assert {0, 1, S - 1} <= set(nh.tolist()), nh


def world_a(gpu, mode=abi.AUTORESET_NONE, final_obs=False, T=0):
    """No pedestrians, E = 8, B = 97, a 96 x 120 map with its origin off zero, float32 field, full circle, stack of 3."""
    E, H, W = 8, 96, 120
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=3, seed=5,
                                 field_format=abi.FIELD_F32, origin_x=-1.0, origin_y=2.0, auto_reset=mode, n_spawn=4)
    gpu.world.lidar_full_circle(cfg, 97)
    cfg.max_episode_steps = T
    g = loc.sim_world(gpu, cfg, lc.room(E, H, W, 3, (FACE_A, FACE_A + 4, 20, 76)), 0, final_obs=final_obs)
    warm(gpu, g, 1)
    face, y = -1.0 + FACE_A * 0.05, 2.0 + 48 * 0.05
    lc.place(g, cfg, 0, face - 0.62, y)                        # beside the wall: driving on crashes, standing does not
    lc.place(g, cfg, 1, face - 0.90, y)                        # inside the discomfort zone, outside the crash zone
    lc.place(g, cfg, 2, -1.0 + 40 * 0.05, y, goal=(0.1, 0.0))  # in the open, 0.1 m from the goal
    lc.place(g, cfg, 3, -1.0 + 40 * 0.05, y, goal=(2.0, 1.0))  # in the open, the goal far
    lc.place(g, cfg, 5, face - 0.62, y)                        # as arena 0, with an empty history
    histories(g, 3)
    return g


def world_b(gpu, beams=B):
    """Social force, 8 slots with 6 present, legs mixed, a 270 degree fan (beams None: all 1081 of it -- the 256-stride passes
    with a remainder), packed field with rect records, arena 0 on the overflow plane (an almost empty 528-cell room), a time
    limit that arena 4 reaches inside the horizon, stack of 3."""
    E, S = 6, 528
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=8, ped_model=abi.PED_SFM, n_scan_stack=3, seed=7,
                                 field_format=abi.FIELD_U16T, n_spawn=4)
    gpu.world.lidar_1081(cfg)
    if beams is not None:
        cfg.n_beams = beams
    cfg.max_episode_steps = 50
    occ = lc.room(E, S, S, 5, (FACE_B, FACE_B + 10, 30, 70))
    for e in range(1, E):                                      # pillars: the field of these arenas does not saturate
        for y in range(200, S - 20, 120):
            for x in range(200, S - 20, 120):
                occ[e, y:y + 4, x:x + 4] = 1
    g = loc.sim_world(gpu, cfg, occ, 6)
    assert "field_overflow" in g.t and "rect_table" in g.t
    ovf = (g.t["field"].view(gpu.torch.int16).reshape(E, -1) == -1).any(dim=1).cpu().numpy()      # 0xFFFF: read from the plane
    assert ovf[0] and not ovf[1:].any(), ovf
    legs = g.t["ped_has_legs"][:, :6].cpu().numpy()
    assert legs.any() and not legs.all()
    warm(gpu, g, 2)
    face, y = FACE_B * 0.05, 50 * 0.05
    lc.place(g, cfg, 0, face - 0.62, y)
    lc.place(g, cfg, 1, face - 0.90, y)
    lc.place(g, cfg, 2, 7.5, 7.5, goal=(3.0, 1.0))            # beside a pedestrian
    g.t["ped_pose"][2, 0] = to_device(gpu, np.array([7.5 + 0.95, 7.5, 1.0]))
    lc.place(g, cfg, 3, 7.5, 7.5, goal=(0.1, 0.0))
    lc.place(g, cfg, 5, 7.5, 7.5, goal=(2.0, 1.0))
    g.t["steps"][4] = 46                                       # the time limit at h = 3
    histories(g, 3)
    return g


def world_b_1081(gpu):
    return world_b(gpu, beams=None)


def world_c(gpu):
    """NAVSIM_PED_EXTERNAL: the commands come as an argument that differs from the state's.  The world with a stack of 1."""
    E, S = 6, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=4, ped_model=abi.PED_EXTERNAL, n_scan_stack=1, seed=9,
                                 field_format=abi.FIELD_U16T)
    gpu.world.lidar_full_circle(cfg, B)
    g = loc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 9), 3)
    warm(gpu, g, 3, cmds=True)
    return g


def world_d(gpu):
    """Wheel speeds as actions, clamped, with a minimum turning radius; stack of 3."""
    E, S = 6, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=3, seed=11,
                                 field_format=abi.FIELD_U16T, action_kind=abi.ACTION_WHEELS, clamp_action=1, min_turning_radius=0.4)
    gpu.world.lidar_full_circle(cfg, B)
    g = loc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 11), 0)
    warm(gpu, g, 4)
    histories(g, 3)
    return g


WORLDS = [world_a, world_b, world_c, world_d]
IDS = ["a-no-peds-f32", "b-sfm-packed", "c-external", "d-wheels"]


def noisy(g):
    std = g.t["scan_noise_std"].cpu().numpy()
    assert g.cfg.add_scan_noise and (std > 0).all(), std


def sequences(g, K, H, seed):
    """[E,K,H,2] in the world's action form: random, sequence 0 driving straight on, the last sequence standing still."""
    rng = np.random.default_rng(seed)
    E = g.cfg.n_envs
    if g.cfg.action_kind == abi.ACTION_WHEELS:
        return rng.uniform(-1.0, 5.0, (E, K, H, 2))                                      # wheel speeds, some beyond the clamp
    act = np.stack([rng.uniform(-0.1, 0.6, (E, K, H)), rng.uniform(-0.8, 0.8, (E, K, H))], axis=3)
    act[:, 0] = (0.5, 0.0)
    if K > 1:
        act[:, K - 1] = 0.0
    return act


def commands(g, seed):
    if g.cfg.ped_model != abi.PED_EXTERNAL:
        return None
    rng = np.random.default_rng(seed)
    shape = tuple(g.t["ped_cmd"].shape[:2])
    return np.stack([rng.uniform(0, 0.6, shape), rng.uniform(-0.6, 0.6, shape)], axis=2)


def state_unchanged(g, saved, obs0, what):
    for k, v in lc.save_state(g).items():
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s %s" % (k, what))
    same_bits(g.obs.cpu().numpy(), obs0.cpu().numpy(), "the observation %s" % what)


# ---- 1. K = 5, H = 6, every row, against the step itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("make", [world_a, world_b_1081, world_c, world_d], ids=["a-no-peds-f32", "b-sfm-packed-1081", "c-external", "d-wheels"])
def test_six_steps_equal_the_step(gpu, make):
    g = make(gpu)
    cfg, K, H = g.cfg, 5, 6
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions, cmd = sequences(g, K, H, 31), commands(g, 12)
    roll = roc.call(gpu, cfg, g.st, actions, obs0, gamma=0.9, ped_cmd=cmd)
    state_unchanged(g, saved, obs0, "after the call")
    step = roc.steps_of(gpu, g, saved, obs0, actions, ped_cmd=cmd)
    assert (roll["exact_steps"] == H).all(), roll["exact_steps"]     # goals 10 m away: nobody reaches a last waypoint
    rows = roc.same_as_steps(roll, step, make.__name__, gamma=0.9)
    eq(roll["length"], roc.expected_length(step), "length")
    assert rows == int(roll["length"].sum())                                         # not a single row skipped
    want_len = roc.expected_length(step)
    print("%s: %d rows compared, the step's lengths %s" % (make.__name__, rows, np.bincount(want_len.ravel(), minlength=H + 1)))
    assert (want_len == H).any()                                                     # conditions on the inputs, from the STEP's results
    if make in (world_a, world_b_1081):
        ended = np.take_along_axis(step["is_crash"] != 0, (want_len - 1)[:, :, None], axis=2)[:, :, 0]
        assert ended.any() and (want_len < H).any(), "no sequence ends in a crash"
        clean = rc.call(gpu, cfg, g.st, actions, cfg.range_max, gamma=0.9, ped_cmd=cmd)
        assert not np.array_equal(roll["min_margin"], clean["min_margin"]), "the noise changed nothing"
    if make is world_b_1081:                                         # arena 4 reaches the time limit at h = 3 whatever it does
        free = (step["is_crash"][4, :, :4] == 0).all(axis=1) & (step["is_success"][4, :, :4] == 0).all(axis=1)
        assert free.any() and (roll["length"][4][free] == 4).all() and (roll["outcome"][4][free] == abi.OUTCOME_TIME_LIMIT).all()


# ---- 2. ends inside the horizon ----------------------------------------------------------------------------------------------------
def ends_inputs(gpu, **kw):
    T, H = 50, 6
    g = world_a(gpu, T=T, **kw)
    g.t["steps"][3] = T - 3                                          # arena 3, in the open: truncated at h = 2
    speeds = (0.5, 0.25, 0.1, 0.05, 0.02, 0.0)                       # straight on at six speeds
    actions = np.zeros((g.cfg.n_envs, len(speeds), H, 2))
    actions[..., 0] = np.array(speeds)[None, :, None]
    return g, actions, H


def test_ends_inside_the_horizon(gpu):
    g, actions, H = ends_inputs(gpu)
    cfg, S, NB = g.cfg, g.cfg.n_scan_stack, g.cfg.n_beams
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    roll = roc.call(gpu, cfg, g.st, actions, obs0)
    step = roc.steps_of(gpu, g, saved, obs0, actions)
    roc.same_as_steps(roll, step, "ends")                            # rows behind `length` are 0, those up to it the step's
    want_len = roc.expected_length(step)
    eq(roll["length"], want_len, "length")
    assert (roll["exact_steps"] == H).all()
    crash = step["is_crash"] != 0
    late = np.array([want_len[0, k] >= 2 and crash[0, k, want_len[0, k] - 1] for k in range(actions.shape[1])])
    print("arena 0 (0.62 m from the wall): the step's lengths %s, crash at the end %s" % (want_len[0], late))
    assert late.any(), "no sequence crashes at a step >= 1"
    assert want_len[0][-1] == H and not crash[0, -1].any()                            # standing still
    assert (want_len[2] == 1).all() and (step["is_success"][2, :, 0] != 0).all()      # 0.1 m from the goal: success at h = 0
    assert want_len[3][-1] == 3 and step["limit"][3, -1, 2] != 0 and (want_len[3] <= 3).all()    # the time limit at h = 2
    L, out = roll["length"], roll["outcome"]
    assert (out[2] == abi.OUTCOME_SUCCESS).all() and out[3][-1] == abi.OUTCOME_TIME_LIMIT
    # the crash at h >= 1 (its row equals the step's above: the re-scan under key + 1): the row's pose is the carried one
    k = int(np.argmax(late))
    h = L[0, k] - 1
    assert out[0, k] == abi.OUTCOME_CRASH and roll["min_margin"][0, k] < 0
    tail = roll["obs_all"][0, k, h, S * NB:]
    same_bits(tail[2:4], roll["pose"][0, k, h - 1, :2].astype(np.float32), "the crash row's pose is the carried one")
    same_bits(roll["goals_all"][0, k, h, :2], tail[2:4], "achieved goal of the crash row")
    assert not np.array_equal(roll["pose"][0, k, h, :2].astype(np.float32), tail[2:4])            # pose[e,k,h] stays the scan pose
    for e, kk in ((0, k), (2, 0), (3, actions.shape[1] - 1)):
        n = L[e, kk]
        assert n < H and not roll["obs_all"][e, kk, n:].any() and not roll["goals_all"][e, kk, n:].any()
        assert roll["obs_all"][e, kk, :n].any(axis=1).all()


def test_same_step_autoreset_terminal_rows(gpu):
    g, actions, H = ends_inputs(gpu, mode=abi.AUTORESET_SAME_STEP, final_obs=True)
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    roll = roc.call(gpu, g.cfg, g.st, actions, obs0)
    step = roc.steps_of(gpu, g, saved, obs0, actions)
    want_len = roc.expected_length(step)
    ended = want_len < H
    last = lambda name: np.take_along_axis(step[name], (want_len - 1)[:, :, None], axis=2)[:, :, 0] != 0
    assert (ended & last("is_crash")).any() and (ended & last("is_success")).any() and (ended & last("limit")).any()
    roc.same_as_steps(roll, step, "same-step", final=True)
    eq(roll["length"], want_len, "length")


# ---- 3. H = 1 equals navsim_lookahead_obs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [abi.LOOKOBS_NOISE_STEP, abi.LOOKOBS_NOISE_OFF], ids=["noise-step", "noise-off"])
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_horizon_one_equals_the_lookahead_observations(gpu, make, noise):
    g = make(gpu)
    cfg = g.cfg
    noisy(g)
    obs0 = g.obs.clone()
    actions = sequences(g, 9, 1, 21)
    if cfg.action_kind == abi.ACTION_TWIST:
        actions[:, :, 0] = GRID9
    cmd = commands(g, 8)
    look = loc.call(gpu, cfg, g.st, actions[:, :, 0], obs0, noise=noise, ped_cmd=cmd)
    roll = roc.call(gpu, cfg, g.st, actions, obs0, noise=noise, gamma=0.5, ped_cmd=cmd)
    same_bits(roll["obs_last"], look["obs"], "obs_last")
    same_bits(roll["goals_last"], look["goals"], "goals_last")
    same_bits(roll["obs_all"][:, :, 0], look["obs"], "obs_all")
    same_bits(roll["goals_all"][:, :, 0], look["goals"], "goals_all")
    same_bits(roll["reward"][:, :, 0], look["reward"], "reward")
    same_bits(roll["pose"][:, :, 0], look["pose"], "pose")
    same_bits(roll["ret"], look["reward"], "ret")
    same_bits(roll["distance"], look["distance"], "distance")
    same_bits(roll["min_margin"], look["margin"], "min_margin")
    succ, crash = look["is_success"] != 0, look["is_crash"] != 0
    limit = (look["done"] != 0) & ~succ & ~crash
    eq(limit.astype(np.uint8), look["truncated"], "the time limit bit against truncated")
    eq(roll["outcome"], (succ | crash << 1 | limit << 2).astype(np.uint8), "outcome")
    eq(roll["discomfort_steps"], look["discomfort"].astype(np.int32), "discomfort_steps")
    assert (roll["length"] == 1).all() and (roll["exact_steps"] == 1).all() and (roll["status"] == 1).all()
    if make in (world_a, world_b):                               # conditions on the test's inputs: every class of row occurs
        assert crash.any() and succ.any() and look["discomfort"].any() and (look["done"] == 0).any()


# ---- 4. noise off equals navsim_rollout at range_max ------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [world_a, world_b], ids=IDS[:2])
def test_noise_off_equals_the_rollout_at_range_max(gpu, make):
    g = make(gpu)
    cfg, K, H = g.cfg, 5, 6
    noisy(g)
    obs0 = g.obs.clone()
    actions = sequences(g, K, H, 31)
    off = roc.call(gpu, cfg, g.st, actions, obs0, noise=abi.LOOKOBS_NOISE_OFF, gamma=0.9)
    plain = rc.call(gpu, cfg, g.st, actions, cfg.range_max, gamma=0.9)
    for name in roc.SHARED:
        same_bits(off[name], plain[name], "noise off against navsim_rollout at range_max: %s" % name)
    assert (plain["length"] < H).any() and (plain["length"] == H).any()
    on = roc.call(gpu, cfg, g.st, actions, obs0, gamma=0.9)
    assert not np.array_equal(on["obs_last"], off["obs_last"])
    g.t["scan_noise_std"].zero_()
    zero = roc.call(gpu, cfg, g.st, actions, obs0, gamma=0.9)
    for name in roc.KEYS:
        same_bits(zero[name], off[name], "std 0 against noise off: %s" % name)


# ---- 5. the re-plan that is left out -------------------------------------------------------------------------------------------------
def test_left_out_replan_is_reported(gpu):
    g = world_b(gpu)
    cfg, K, H, e = g.cfg, 5, 6, 5
    t = g.t
    nw = int(t["ped_n_waypoints"][e, 0].item())
    last = t["ped_waypoints"][e, 0, nw - 1].cpu().numpy()
    rp = t["robot_pose"][e].cpu().numpy()
    away = (last - rp[:2]) / max(np.linalg.norm(last - rp[:2]), 1e-9)   # approach from the side the robot is on: walking away from it
    start = last - 0.58 * away                                          # 0.58 m from its last waypoint, 0.12 m a step towards it
    yaw = float(np.arctan2(away[1], away[0]) % (2 * np.pi))
    t["ped_pose"][e, 0] = to_device(gpu, np.array([start[0], start[1], yaw]))
    t["ped_vel"][e, 0] = to_device(gpu, 0.6 * away)
    t["ped_v_pref"][e, 0] = 0.6
    t["ped_wp_head"][e, 0] = nw - 1
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions = sequences(g, K, H, 41)
    off = roc.call(gpu, cfg, g.st, actions, obs0, noise=abi.LOOKOBS_NOISE_OFF)
    plain = rc.call(gpu, cfg, g.st, actions, cfg.range_max)
    eq(off["exact_steps"], plain["exact_steps"], "exact_steps against navsim_rollout's")
    roll = roc.call(gpu, cfg, g.st, actions, obs0)
    step = roc.steps_of(gpu, g, saved, obs0, actions)
    X = roll["exact_steps"]
    print("exact_steps of arena %d: %s, lengths %s" % (e, X[e], roll["length"][e]))
    assert (X[e] < H).all() and (X[e] >= 1).all()
    others = np.arange(cfg.n_envs) != e
    assert (X[others] == H).all()
    same = roll["length"] == off["length"]
    eq(X[same], plain["exact_steps"][same], "exact_steps with noise, where the noise moved no end")
    rows = roc.same_as_steps(roll, step, "replan")
    assert rows == int(np.minimum(roll["length"], X).sum()) and rows >= int(X[e].sum())
    for name in roc.KEYS:
        assert np.isfinite(roll[name][e].astype(np.float64)).all(), name


# ---- 6. shapes, the skip mask, rows='last' -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H", [(1, 3), (65, 2)], ids=["K1", "K65"])
def test_one_and_sixty_five_sequences(gpu, K, H):
    g = world_a(gpu)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions = sequences(g, K, H, 61)
    roll = roc.call(gpu, g.cfg, g.st, actions, obs0)
    step = roc.steps_of(gpu, g, saved, obs0, actions)
    rows = roc.same_as_steps(roll, step, "K = %d" % K)
    eq(roll["length"], roc.expected_length(step), "length")
    assert rows == int(roll["length"].sum())


def test_longest_horizon(gpu):
    g = world_a(gpu)
    H = abi.ROLLOUT_MAX_H
    saved, obs0 = lc.save_state(g), g.obs.clone()
    rng = np.random.default_rng(71)
    actions = np.stack([rng.uniform(0.0, 0.15, (8, 2, H)), rng.uniform(-0.8, 0.8, (8, 2, H))], axis=3)     # slow: most sequences last
    actions[:, 1] = 0.0
    roll = roc.call(gpu, g.cfg, g.st, actions, obs0, gamma=0.97)
    step = roc.steps_of(gpu, g, saved, obs0, actions)
    rows = roc.same_as_steps(roll, step, "H = %d" % H, gamma=0.97)
    eq(roll["length"], roc.expected_length(step), "length")
    assert rows == int(roll["length"].sum()) and (roc.expected_length(step) == H).any() and (roll["exact_steps"] == H).all()


def test_skip_mask_and_last_rows_only(gpu):
    g = world_a(gpu)
    actions = sequences(g, 3, 4, 51)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    skip = np.array([0, 1, 0, 0, 1, 0, 0, 1], np.uint8)
    roll = roc.call(gpu, g.cfg, g.st, actions, obs0)
    masked = roc.call(gpu, g.cfg, g.st, actions, obs0, skip=skip)
    last = roc.call(gpu, g.cfg, g.st, actions, obs0, rows="last")
    last_masked = roc.call(gpu, g.cfg, g.st, actions, obs0, rows="last", skip=skip)
    state_unchanged(g, saved, obs0, "after four calls")
    assert (roll["length"] < 4).any() and (roll["outcome"] & abi.OUTCOME_CRASH).any()
    for out, full in ((masked, roll), (last_masked, last)):
        eq(out["status"], 1 - skip, "status")
        roc.zero_rows(out, skip == 1, "skipped arenas")
        for name in out:
            same_bits(out[name][skip == 0], full[name][skip == 0], name)
    assert "obs_all" not in last and "goals_all" not in last
    for name in last:                                                # rows='last': everything else is the same
        same_bits(last[name], roll[name], "rows='last': %s" % name)


# ---- 7. through NavGymEnv -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_env_rollout_obs_then_steps_agree(gpu, mode):
    import torch
    K, H, n = 3, 4, 32
    env = nav_env(num_envs=n, n_beams=64, rollout_obs=K, rollout_obs_params=dict(horizon=H, gamma=0.95, rows="all"), autoreset_mode=mode)
    env.reset()
    rng = np.random.default_rng(4)
    rows = torch.arange(n, device="cuda:0")
    compared = finished = skipped = t = 0
    pending = np.zeros(n, bool)
    for _ in range(8):
        seq = np.stack([np.stack([random_actions(rng, n, t + h) for h in range(H)], axis=1) for _ in range(K)], axis=1)      # [E,K,H,2]
        seq_t = torch.from_numpy(seq).to("cuda:0")
        out = env.rollout_obs(seq_t)
        assert set(out["observation"]) == set(out["observations"]) == {"observation", "achieved_goal", "desired_goal"}
        eq(out["status"].cpu().numpy(), (~pending).astype(np.uint8), "status at step %d" % t)
        skipped += int(pending.sum())
        for name in ("reward", "length", "outcome"):
            assert not out[name].cpu().numpy()[pending].any(), name
        assert not out["observation"]["observation"].cpu().numpy()[pending].any()
        pick = torch.from_numpy(rng.integers(0, K, n)).to("cuda:0")
        want = {"row": out["observations"]["observation"][rows, pick].cpu().numpy(), "ach": out["observations"]["achieved_goal"][rows, pick].cpu().numpy(),
                "reward": out["reward"][rows, pick].cpu().numpy(), "length": out["length"][rows, pick].cpu().numpy(),
                "exact": out["exact_steps"][rows, pick].cpu().numpy(), "outcome": out["outcome"][rows, pick].cpu().numpy(),
                "last": out["observation"]["observation"][rows, pick].cpu().numpy()}
        live = ~pending                                                              # (next-step: a pending arena is reset, not stepped)
        for h in range(H):
            o, rew, done, info = env.step(seq_t[rows, pick, h].contiguous())
            d = done.cpu().numpy()
            row, ach = o["observation"], o["achieved_goal"]
            if mode == "same_step":                                                  # the terminal row rides in info
                m = done[:, None]
                row = torch.where(m, info["final_observation"]["observation"], row)
                ach = torch.where(m, info["final_observation"]["achieved_goal"], ach)
            now = live & (h < want["length"]) & (h < want["exact"])
            same_bits(want["row"][now, h], row.cpu().numpy()[now], "row at step %d" % t)
            same_bits(want["ach"][now, h], ach.cpu().numpy()[now], "achieved goal at step %d" % t)
            same_bits(want["reward"][now, h], rew.cpu().numpy()[now], "reward at step %d" % t)
            eq((h + 1 == want["length"])[now] & ((want["outcome"] != 0)[now]), d[now], "done at step %d" % t)
            ends = now & (h + 1 == want["length"])
            same_bits(want["last"][ends], row.cpu().numpy()[ends], "the last row at step %d" % t)
            compared += int(now.sum()); finished += int((d & now).sum())
            live = live & ~d                                                         # behind its end an arena plays another episode
            pending = d.copy() if mode == "next_step" else pending
            t += 1
    print("%s: %d arena-steps compared, %d of them ended an episode, %d arenas skipped" % (mode, compared, finished, skipped))
    assert finished > 0, "no episode ended: the terminal rows were not compared"
    assert mode != "next_step" or skipped > 0, "no arena was pending at a call: nothing was skipped"


def test_env_single_arena_gets_numpy_rows(gpu):
    K, H = 3, 4
    seq = np.zeros((K, H, 2)); seq[0, :, 0] = 0.5; seq[1, :, 1] = 0.5
    one = nav_env(num_envs=1, rollout_obs=K, rollout_obs_params=dict(horizon=H, noise="off"))
    one.reset()
    row = one.rollout_obs(seq)
    D = one.sim.obs.shape[1]
    assert "observations" not in row and isinstance(row["reward"], np.ndarray)
    assert row["reward"].shape == (K, H) and row["pose"].shape == (K, H, 3) and row["ret"].shape == (K,) and row["status"] == 1
    assert row["observation"]["observation"].shape == (K, D) and row["observation"]["observation"].dtype == np.float64
    assert row["observation"]["achieved_goal"].shape == (K, 2) and row["observation"]["desired_goal"].shape == (K, 2)
    assert one.sim.products["rollout_obs"].params.noise == abi.LOOKOBS_NOISE_OFF
    assert "rollout" not in one.sim.products and "lookahead_obs" not in one.sim.products
    full = nav_env(num_envs=1, rollout_obs=K, rollout_obs_params=dict(horizon=H, rows="all"))
    full.reset()
    row = full.rollout_obs(seq)
    assert row["observations"]["observation"].shape == (K, H, D) and row["observations"]["achieved_goal"].shape == (K, H, 2)
    L = int(row["length"][0])
    assert np.array_equal(row["observations"]["observation"][0, L - 1], row["observation"]["observation"][0])
