"""GPU: action-sequence rollout (include/navsim.h navsim_rollout) against navsim_step itself.  The rollout is called once; then,
for every sequence, the saved state is put back, navsim_step runs H times with that sequence's actions, and what both return is
compared bit for bit up to min(length, exact_steps).  With H = 1 every output is compared with navsim_lookahead's.  Ends inside
the horizon, the re-plan the rollout leaves out, the read-only state, the skip mask, next-step auto-reset and a random-shooting
controller through NavGymEnv follow.  The worlds are shaped like tests/test_gpu_lookahead.py's four."""
import numpy as np
import pytest

import lookahead_call as lc
import rollout_call as rc
from gpu_support import eq, gpu, nav_env, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

FACE_A, FACE_B = 80, 40                                                                    # x cell of the block's face, worlds (a) / (b)
GRID9 = np.array([(v, w) for v in (0.0, 0.25, 0.5) for w in (-0.6, 0.0, 0.6)])


def default_range(g):
    from nav_gym_amd import sim
    return sim.rollout_defaults(g.cfg, float(g.t["scan_discomfort"].max().item()))["range"]


def warm(gpu, g, seed, cmds=False):
    """Five seeded random steps: prev_action, the waypoint heads and the leg odometry are live afterwards."""
    rng = np.random.default_rng(seed)
    for _ in range(5):
        if cmds:
            g.set_ped_cmd(np.stack([rng.uniform(0, 0.6, g.t["ped_cmd"].shape[:2]), rng.uniform(-0.6, 0.6, g.t["ped_cmd"].shape[:2])], axis=2))
        g.step(to_device(gpu, random_actions(rng, g.cfg.n_envs)))


def world_a(gpu, T=0):
    """No pedestrians, E = 8, B = 97 (two chunks, the second partial), a 96 x 120 map with its origin off zero, float32 field."""
    E, H, W = 8, 96, 120
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=2, seed=5,
                                 field_format=abi.FIELD_F32, origin_x=-1.0, origin_y=2.0)
    gpu.world.lidar_full_circle(cfg, 97)
    cfg.max_episode_steps = T
    g = lc.sim_world(gpu, cfg, lc.room(E, H, W, 3, (FACE_A, FACE_A + 4, 20, 76)), 0)
    warm(gpu, g, 1)
    face, y = -1.0 + FACE_A * 0.05, 2.0 + 48 * 0.05
    lc.place(g, cfg, 0, face - 0.62, y)                        # beside the wall: driving on crashes, standing does not
    lc.place(g, cfg, 1, face - 0.90, y)                        # inside the discomfort zone, outside the crash zone
    lc.place(g, cfg, 2, -1.0 + 40 * 0.05, y, goal=(0.1, 0.0))  # in the open, 0.1 m from the goal
    lc.place(g, cfg, 3, -1.0 + 40 * 0.05, y, goal=(2.0, 1.0))  # in the open, the goal far
    lc.place(g, cfg, 5, -1.0 + 40 * 0.05, y, goal=(2.0, -1.0))
    return g


def world_b(gpu):
    """Social force, 8 slots with 6 present, legs mixed, the 1081-beam 270 degree lidar, E = 6, packed field with rect records,
    arena 0 on the overflow plane (an almost empty 528-cell room), a time limit that arena 4 reaches inside the horizon."""
    E, S = 6, 528
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=8, ped_model=abi.PED_SFM, n_scan_stack=2, seed=7,
                                 field_format=abi.FIELD_U16T, n_spawn=4)
    gpu.world.lidar_1081(cfg)
    cfg.max_episode_steps = 50
    occ = lc.room(E, S, S, 5, (FACE_B, FACE_B + 10, 30, 70))
    for e in range(1, E):                                      # pillars: the field of these arenas does not saturate
        for y in range(200, S - 20, 120):
            for x in range(200, S - 20, 120):
                occ[e, y:y + 4, x:x + 4] = 1
    g = lc.sim_world(gpu, cfg, occ, 6)
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
    return g


def world_c(gpu):
    """NAVSIM_PED_EXTERNAL: the commands come as an argument that differs from the state's."""
    E, S = 4, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=4, ped_model=abi.PED_EXTERNAL, n_scan_stack=1, seed=9,
                                 field_format=abi.FIELD_U16T)
    gpu.world.lidar_full_circle(cfg, 64)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 9), 3)
    warm(gpu, g, 3, cmds=True)
    return g


def world_d(gpu):
    """Wheel speeds as actions, clamped, with a minimum turning radius."""
    E, S = 4, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=1, seed=11,
                                 field_format=abi.FIELD_U16T, action_kind=abi.ACTION_WHEELS, clamp_action=1, min_turning_radius=0.4)
    gpu.world.lidar_full_circle(cfg, 64)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 11), 0)
    warm(gpu, g, 4)
    return g


WORLDS = [world_a, world_b, world_c, world_d]
IDS = ["a-no-peds-f32", "b-sfm-packed", "c-external", "d-wheels"]


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


def thresholds(g):
    return g.t["scan_threshold"].cpu().numpy(), g.t["scan_discomfort"].cpu().numpy()


# ---- 1. H = 1 equals navsim_lookahead -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_horizon_one_equals_the_lookahead(gpu, make):
    g = make(gpu)
    cfg, E, R = g.cfg, g.cfg.n_envs, default_range(g)
    actions = sequences(g, 9, 1, 21)
    if cfg.action_kind == abi.ACTION_TWIST:
        actions[:, :, 0] = GRID9
    cmd = commands(g, 8)
    look = lc.call(gpu, cfg, g.st, actions[:, :, 0], R, ped_cmd=cmd)
    roll = rc.call(gpu, cfg, g.st, actions, R, gamma=0.5, ped_cmd=cmd)
    same_bits(roll["reward"][:, :, 0], look["reward"], "reward")
    same_bits(roll["pose"][:, :, 0], look["pose"], "pose")
    same_bits(roll["ret"], look["reward"], "ret")
    same_bits(roll["distance"], look["distance"], "distance")
    same_bits(roll["min_margin"], look["margin"], "min_margin")
    succ, crash = look["is_success"] != 0, look["is_crash"] != 0
    limit = (look["done"] != 0) & ~succ & ~crash
    eq(roll["outcome"], (succ | crash << 1 | limit << 2).astype(np.uint8), "outcome")
    eq(roll["discomfort_steps"], look["discomfort"].astype(np.int32), "discomfort_steps")
    assert (roll["length"] == 1).all() and (roll["exact_steps"] == 1).all() and (roll["status"] == 1).all()
    assert roll["length"].dtype == roll["exact_steps"].dtype == roll["discomfort_steps"].dtype == np.int32
    if make in (world_a, world_b):                               # conditions on the test's inputs: every class of row occurs
        assert crash.any() and succ.any() and look["discomfort"].any() and (look["done"] == 0).any()


# ---- 2. H = 6, K = 5 against the step itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_six_steps_equal_the_step(gpu, make):
    g = make(gpu)
    cfg, E, R, K, H = g.cfg, g.cfg.n_envs, default_range(g), 5, 6
    assert cfg.add_scan_noise == 0
    saved = lc.save_state(g)
    actions, cmd = sequences(g, K, H, 31), commands(g, 12)
    roll = rc.call(gpu, cfg, g.st, actions, R, gamma=0.9, ped_cmd=cmd)
    for k, v in lc.save_state(g).items():                                            # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the call" % k)
    step = rc.steps_of(gpu, g, saved, actions, ped_cmd=cmd)
    thr, dthr = thresholds(g)
    assert (roll["exact_steps"] == H).all(), roll["exact_steps"]     # goals 10 m away: nobody reaches a last waypoint
    rows = rc.same_as_steps(roll, step, make.__name__, gamma=0.9, thr=thr, dthr=dthr, R=R)
    eq(roll["length"], rc.expected_length(step), "length")
    assert rows == int(roll["length"].sum())                                         # not a single row skipped
    print("%s: %d rows compared, lengths %s" % (make.__name__, rows, np.bincount(roll["length"].ravel(), minlength=H + 1)))
    assert (roll["length"] == H).any()
    if make is world_b:                                              # arena 4 reaches the time limit at h = 3 whatever it does
        free = (step["is_crash"][4, :, :4] == 0).all(axis=1) & (step["is_success"][4, :, :4] == 0).all(axis=1)
        assert free.any() and (roll["length"][4][free] == 4).all() and (roll["outcome"][4][free] == abi.OUTCOME_TIME_LIMIT).all()


# ---- 3. ends inside the horizon -----------------------------------------------------------------------------------------------------
def test_ends_inside_the_horizon(gpu):
    T, H = 50, 6
    g = world_a(gpu, T=T)
    cfg, R = g.cfg, default_range(g)
    g.t["steps"][5] = T - 3                                          # arena 5, in the open: truncated at h = 2
    saved = lc.save_state(g)
    speeds = (0.5, 0.25, 0.1, 0.05, 0.02, 0.0)                       # straight on at six speeds
    actions = np.zeros((cfg.n_envs, len(speeds), H, 2))
    actions[..., 0] = np.array(speeds)[None, :, None]
    roll = rc.call(gpu, cfg, g.st, actions, R)
    step = rc.steps_of(gpu, g, saved, actions)
    thr, dthr = thresholds(g)
    rc.same_as_steps(roll, step, "ends", thr=thr, dthr=dthr, R=R)    # rows behind `length` are 0, those up to it the step's
    eq(roll["length"], rc.expected_length(step), "length")
    assert (roll["exact_steps"] == H).all()
    L, out = roll["length"], roll["outcome"]
    print("arena 0 (0.62 m from the wall): lengths %s outcomes %s" % (L[0], out[0]))
    late = (out[0] == abi.OUTCOME_CRASH) & (L[0] >= 2)
    assert late.any(), "no sequence crashes at a step >= 1"
    assert (roll["min_margin"][0][out[0] == abi.OUTCOME_CRASH] < 0).all() and out[0][-1] == 0 and L[0][-1] == H
    assert (L[2] == 1).all() and (out[2] == abi.OUTCOME_SUCCESS).all()                # 0.1 m from the goal
    assert L[5][-1] == 3 and out[5][-1] == abi.OUTCOME_TIME_LIMIT                     # standing still until the time limit
    assert (L[5] <= 3).all()
    for e, k in ((0, int(np.argmax(late))), (2, 0), (5, len(speeds) - 1)):
        n = L[e, k]
        assert n < H and not roll["reward"][e, k, n:].any() and not roll["pose"][e, k, n:].any()
        assert roll["pose"][e, k, :n, :2].all()


# ---- 4. the re-plan the rollout leaves out --------------------------------------------------------------------------------------------
def test_left_out_replan_is_reported(gpu):
    g = world_b(gpu)
    cfg, R, K, H, e = g.cfg, default_range(g), 5, 6, 5
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
    saved = lc.save_state(g)
    actions = sequences(g, K, H, 41)
    roll = rc.call(gpu, cfg, g.st, actions, R)
    step = rc.steps_of(gpu, g, saved, actions)
    X = roll["exact_steps"]
    print("exact_steps of arena %d: %s, lengths %s" % (e, X[e], roll["length"][e]))
    assert (X[e] < H).all() and (X[e] >= 1).all()
    others = np.arange(cfg.n_envs) != e
    assert (X[others] == H).all()
    thr, dthr = thresholds(g)
    rows = rc.same_as_steps(roll, step, "replan", thr=thr, dthr=dthr, R=R)
    assert rows >= int(np.minimum(roll["length"], X).sum())
    for name in rc.KEYS:
        assert np.isfinite(roll[name][e].astype(np.float64)).all(), name


# ---- 5. other checks ------------------------------------------------------------------------------------------------------------------
def test_skip_mask_and_read_only_state(gpu):
    g = world_a(gpu)
    R = default_range(g)
    actions = sequences(g, 3, 4, 51)
    saved = lc.save_state(g)
    skip = np.array([0, 1, 0, 0, 1, 0, 0, 1], np.uint8)
    roll, masked = rc.call(gpu, g.cfg, g.st, actions, R), rc.call(gpu, g.cfg, g.st, actions, R, skip=skip)
    for k, v in lc.save_state(g).items():
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after two calls" % k)
    eq(masked["status"], 1 - skip, "status")
    rc.zero_rows(masked, skip == 1, "skipped arenas")
    for name in rc.KEYS:
        same_bits(masked[name][skip == 0], roll[name][skip == 0], name)


@pytest.mark.parametrize("K,H", [(1, 3), (65, 2)], ids=["K1", "K65"])
def test_one_and_sixty_five_sequences(gpu, K, H):
    g = world_a(gpu)
    saved, R = lc.save_state(g), default_range(g)
    actions = sequences(g, K, H, 61)
    roll = rc.call(gpu, g.cfg, g.st, actions, R)
    step = rc.steps_of(gpu, g, saved, actions, labels=False)
    rows = rc.same_as_steps(roll, step, "K = %d" % K)
    eq(roll["length"], rc.expected_length(step), "length")
    assert rows == int(roll["length"].sum())


def test_longest_horizon(gpu):
    g = world_a(gpu)
    H = abi.ROLLOUT_MAX_H
    saved, R = lc.save_state(g), default_range(g)
    rng = np.random.default_rng(71)
    actions = np.stack([rng.uniform(0.0, 0.15, (8, 3, H)), rng.uniform(-0.8, 0.8, (8, 3, H))], axis=3)     # slow: most sequences last
    actions[:, 2] = 0.0
    roll = rc.call(gpu, g.cfg, g.st, actions, R, gamma=0.97)
    step = rc.steps_of(gpu, g, saved, actions, labels=False)
    rows = rc.same_as_steps(roll, step, "H = %d" % H, gamma=0.97)
    eq(roll["length"], rc.expected_length(step), "length")
    assert rows == int(roll["length"].sum()) and (roll["length"] == H).any() and (roll["exact_steps"] == H).all()


def test_env_next_step_autoreset_skips_pending_arenas(gpu):
    K, H = 3, 4
    env = nav_env(num_envs=32, rollout=K, rollout_params=dict(horizon=H), autoreset_mode="next_step", num_humans=0,
                  pedestrian_model="none")
    env.reset()
    seq = np.zeros((K, H, 2)); seq[0, :, 0] = 0.5; seq[1, :, 1] = 0.5
    seen = 0
    for t in range(40):
        _, _, done, _ = env.step(np.tile([0.5, 0.0], (32, 1)))                       # straight on: arenas crash
        out = env.rollout(seq)
        pending = done.cpu().numpy()
        eq(out["status"].cpu().numpy(), (~pending).astype(np.uint8), "status at step %d" % t)
        for name in rc.KEYS:
            assert not out[name].cpu().numpy()[pending].any(), name
        assert (out["length"].cpu().numpy()[~pending] >= 1).all()
        seen += int(pending.sum())
    assert seen > 0, "no arena finished: nothing was skipped"
    one = nav_env(num_envs=1, rollout=K, rollout_params=dict(horizon=H))
    one.reset()
    row = one.rollout(seq)
    assert row["reward"].shape == (K, H) and row["pose"].shape == (K, H, 3) and row["ret"].shape == (K,) and row["status"] == 1
    assert isinstance(row["reward"], np.ndarray)


# ---- 6. through NavGymEnv: random shooting ----------------------------------------------------------------------------------------------
def shooting_run(controller, steps=150, E=64, K=8, H=6):
    from nav_gym_amd import env as envmod
    import torch
    epr = dict(envmod.DEFAULT_KWARGS["env_param_range"], scan_noise_std=([0.0, 0.0], "float"))
    env = nav_env(num_envs=E, map_size=200, n_beams=256, seed=23, num_humans=0, pedestrian_model="none", rollout=K,
                  rollout_params=dict(horizon=H, gamma=1.0), min_goal_dist=3.0, max_goal_dist=8.0, env_param_range=epr, auto_reset=False)
    env.reset()
    rng = np.random.default_rng(17)
    crashed = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    reached = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    rows = torch.arange(E, device="cuda:0")
    for _ in range(steps):
        seq = np.stack([np.stack([random_actions(rng, E) for _ in range(H)], axis=1) for _ in range(K)], axis=1)     # [E,K,H,2]
        seq[:, K - 1] = 0.0                                                          # the all-zero sequence is the last one
        seq_t = torch.from_numpy(seq).to("cuda:0")
        pick = torch.zeros(E, dtype=torch.long, device="cuda:0")
        if controller:
            out = env.rollout(seq_t)
            assert int(out["exact_steps"].min().item()) == H                         # no pedestrians: exact over the whole horizon
            safe = (out["outcome"] & abi.OUTCOME_CRASH) == 0
            pick = torch.where(safe, out["ret"], torch.full_like(out["ret"], -float("inf"))).argmax(dim=1)
            assert bool(safe[rows, pick].all())
        _, _, _, info = env.step(seq_t[rows, pick, 0].contiguous())
        crashed |= info["is_crash"] != 0
        reached |= info["is_success"] != 0
    return int(crashed.sum().item()), int(reached.sum().item())


def test_random_shooting_never_crashes(gpu):
    plain_crashed, plain_reached = shooting_run(False)
    crashed, reached = shooting_run(True)
    print("of 64 arenas within 150 steps: sequence 0's first action -- %d crash, %d reach the goal; random shooting (K = 8, H = 6) -- "
          "%d crash, %d reach the goal" % (plain_crashed, plain_reached, crashed, reached))
    assert plain_crashed >= 1, "condition: the same sequences without the controller crash somewhere"
    assert crashed == 0
