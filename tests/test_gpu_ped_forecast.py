"""GPU: pedestrian forecast (include/navsim.h navsim_ped_forecast) against navsim_step itself.  The forecast is called once; then
the saved state is put back, navsim_step runs H times with the same actions and commands, and the pedestrians and the robot
behind every step are compared with the forecast's rows bit for bit, up to exact_steps and the arena's first done step.  The
re-plan the forecast leaves out, navsim_rollout's robot, the robot modes, the independence of the horizon, the derived outputs
and the constant-velocity model against tests/ped_forecast_spec.py, the skip mask and NavGymEnv follow.  Worlds (b) and (c) are
shaped like tests/test_gpu_rollout.py's, (d) like the lookahead's wheels world with pedestrians, (e) has every pedestrian count
from none to a full wavefront in one launch, with scan noise on."""
import numpy as np
import pytest

import lookahead_call as lc
import ped_forecast_call as pf
import ped_forecast_spec as spec
import rollout_call as rc
from gpu_support import eq, gpu, nav_env, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

H6 = 6
POP = (1, 1)                                                   # world (b): the pedestrian (arena, slot) given a two-waypoint route


def warm(gpu, g, seed, cmds=False):
    """Five seeded random steps: prev_action, the velocities and the waypoint heads are live afterwards."""
    rng = np.random.default_rng(seed)
    for _ in range(5):
        if cmds:
            g.set_ped_cmd(np.stack([rng.uniform(0, 0.6, g.t["ped_cmd"].shape[:2]), rng.uniform(-0.6, 0.6, g.t["ped_cmd"].shape[:2])], axis=2))
        g.step(to_device(gpu, random_actions(rng, g.cfg.n_envs)))


def world_b(gpu):
    """Social force, 8 slots with 6 present, the 1081-beam 270 degree lidar, E = 6, packed field with rect records, arena 0 on the
    overflow plane (an almost empty 528-cell room); a time limit that arena 3 reaches at h = 1 and arena 4 at h = 3; pedestrian
    POP walks a two-waypoint route whose first waypoint it passes inside the horizon."""
    E, S = 6, 528
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=8, ped_model=abi.PED_SFM, n_scan_stack=2, seed=7,
                                 field_format=abi.FIELD_U16T, n_spawn=4)
    gpu.world.lidar_1081(cfg)
    cfg.max_episode_steps = 50
    occ = lc.room(E, S, S, 5, (40, 50, 30, 70))
    for e in range(1, E):                                      # pillars: the field of these arenas does not saturate
        for y in range(200, S - 20, 120):
            for x in range(200, S - 20, 120):
                occ[e, y:y + 4, x:x + 4] = 1
    g = lc.sim_world(gpu, cfg, occ, 6)
    assert "field_overflow" in g.t and "rect_table" in g.t
    ovf = (g.t["field"].view(gpu.torch.int16).reshape(E, -1) == -1).any(dim=1).cpu().numpy()      # 0xFFFF: read from the plane
    assert ovf[0] and not ovf[1:].any(), ovf
    warm(gpu, g, 2)
    t, (e, i) = g.t, POP
    pose = t["ped_pose"][e, i].cpu().numpy()
    last = t["ped_waypoints"][e, i, int(t["ped_n_waypoints"][e, i].item()) - 1].cpu().numpy()
    assert np.linalg.norm(last - pose[:2]) > 3.0               # (condition: the route's end is far)
    along = (last - pose[:2]) / np.linalg.norm(last - pose[:2])
    t["ped_waypoints"][e, i, 0] = to_device(gpu, pose[:2] + 1.05 * along)      # 1.05 m ahead: within 1 m after a step
    t["ped_waypoints"][e, i, 1] = to_device(gpu, last)
    t["ped_n_waypoints"][e, i] = 2
    t["ped_wp_head"][e, i] = 0
    t["ped_v_pref"][e, i] = 0.6
    t["ped_vel"][e, i] = to_device(gpu, 0.6 * along)
    t["steps"][3] = 48                                         # the time limit at h = 1
    t["steps"][4] = 46                                         # ... and at h = 3
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


def world_d(gpu, seed=15):
    """Wheel speeds as actions, clamped, with a minimum turning radius; three social-force pedestrians in four slots."""
    E, S = 4, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=4, ped_model=abi.PED_SFM, n_scan_stack=1, seed=seed,
                                 field_format=abi.FIELD_U16T, action_kind=abi.ACTION_WHEELS, clamp_action=1, min_turning_radius=0.4)
    gpu.world.lidar_full_circle(cfg, 64)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, seed), 3)
    warm(gpu, g, 4)
    return g


E_COUNTS = (0, 1, 64, 3, 20)


def world_e(gpu):
    """E = 5 (odd), 160 x 160 maps, 64 slots with 0, 1, 64, 3 and 20 pedestrians: an empty arena and a full wavefront of
    pedestrians (2080 pair terms, nine rounds of the workgroup) in one launch; float32 field; scan noise ON."""
    E, S = 5, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=64, ped_model=abi.PED_SFM, n_scan_stack=1, seed=13,
                                 field_format=abi.FIELD_F32, add_scan_noise=1)
    gpu.world.lidar_full_circle(cfg, 64)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 13, n_obstacles=4), np.array(E_COUNTS, np.int32), noise_std_range=(0.02, 0.05),
                     ped_clearance=0.3)
    eq(g.t["n_peds"].cpu().numpy(), np.array(E_COUNTS, np.int32), "n_peds")
    assert g.cfg.add_scan_noise == 1 and float(g.t["scan_noise_std"].min().item()) >= 0.02
    warm(gpu, g, 5)
    return g


WORLDS = [world_b, world_c, world_d, world_e]
IDS = ["b-sfm-packed", "c-external", "d-wheels-sfm", "e-0-to-64-noise"]
TWIST = [world_b, world_c, world_e]
TWIST_IDS = [IDS[0], IDS[1], IDS[3]]


def sequence(g, H, seed):
    """[E,H,2] in the world's action form."""
    rng = np.random.default_rng(seed)
    E = g.cfg.n_envs
    if g.cfg.action_kind == abi.ACTION_WHEELS:
        return rng.uniform(-1.0, 5.0, (E, H, 2))                                         # wheel speeds, some beyond the clamp
    return np.stack([rng.uniform(-0.1, 0.6, (E, H)), rng.uniform(-0.8, 0.8, (E, H))], axis=2)


def commands(g, seed):
    if g.cfg.ped_model != abi.PED_EXTERNAL:
        return None
    rng = np.random.default_rng(seed)
    shape = tuple(g.t["ped_cmd"].shape[:2])
    return np.stack([rng.uniform(0, 0.6, shape), rng.uniform(-0.6, 0.6, shape)], axis=2)


def counts(g):
    return np.clip(g.t["n_peds"].cpu().numpy(), 0, g.cfg.max_peds)


def all_same(a, b, what, keys=pf.KEYS):
    for k in keys:
        same_bits(a[k], b[k], "%s: %s" % (what, k))


def rows_equal_the_step(out, step, n_peds, upto, what):
    """pose, vel and robot_pose of rows h < upto[e] against the state behind step h, bit for bit -> rows compared."""
    rows = 0
    for e in range(len(n_peds)):
        n = int(n_peds[e])
        for h in range(int(upto[e])):
            tag = "%s: arena %d step %d" % (what, e, h)
            same_bits(out["pose"][e, h, :n], step["ped_pose"][e, h, :n], tag + " pose")
            same_bits(out["vel"][e, h, :n], step["ped_vel"][e, h, :n], tag + " vel")
            same_bits(out["robot_pose"][e, h], step["robot_pose"][e, h], tag + " robot_pose")
            rows += 1
    return rows


# ---- 1. against the step itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_six_steps_equal_the_step(gpu, make):
    g = make(gpu)
    cfg, E, H = g.cfg, g.cfg.n_envs, H6
    saved = lc.save_state(g)
    actions, cmd = sequence(g, H, 31), commands(g, 12)
    if cmd is not None:
        assert not np.array_equal(cmd, g.t["ped_cmd"].cpu().numpy())                 # the argument differs from the state's
    out = pf.call(gpu, cfg, g.st, H, actions=actions, ped_cmd=cmd)
    for k, v in lc.save_state(g).items():                                            # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the call" % k)
    step = pf.steps_of(gpu, g, saved, actions, ped_cmd=cmd)
    n_peds, X, done_at = counts(g), out["exact_steps"], pf.first_done(step)
    print("%s: n_peds %s exact_steps %s first done %s" % (make.__name__, n_peds, X, done_at))
    assert (out["status"] == 1).all() and X.dtype == np.int32 and ((X >= 1) & (X <= H)).all()
    # conditions on the inputs
    ended = done_at < H
    assert ended.sum() <= 2, "more than two arenas end inside the horizon"
    upto = np.minimum(X, done_at)
    crowd = n_peds > 0
    assert (upto[crowd] >= 1).all(), "an arena with pedestrians is not compared in row 0"
    assert (upto[crowd & ~ended] == H).all(), "an arena that does not end is not compared through all rows"
    rows = rows_equal_the_step(out, step, n_peds, upto, make.__name__)
    assert rows == int(upto.sum())
    if make is world_b:
        assert ended[3] and ended[4] and done_at[3] == 1 and done_at[4] == 3
        e, i = POP
        heads = step["ped_wp_head"][e, :, i]
        assert saved["ped_wp_head"][e, i].item() == 0 and heads[-1] == 1 and upto[e] == H, heads       # a pop inside the horizon
    if make is world_e:
        assert list(n_peds) == list(E_COUNTS)
    spec.unused_rows_are_empty(out, n_peds, make.__name__)


# ---- 2. the re-plan the forecast leaves out -------------------------------------------------------------------------------------------
def test_left_out_replan_is_reported(gpu):
    g = world_b(gpu)
    cfg, H, e = g.cfg, H6, 5
    t = g.t
    lc.place(g, cfg, e, 7.5, 7.5, goal=(2.0, 1.0))                      # (the rollout test's scene: the robot in the open)
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
    actions = sequence(g, H, 41)
    out = pf.call(gpu, cfg, g.st, H, actions=actions)
    step = pf.steps_of(gpu, g, saved, actions)
    X, n_peds, done_at = out["exact_steps"], counts(g), pf.first_done(step)
    print("exact_steps %s, first done %s" % (X, done_at))
    assert 1 <= X[e] < H and (X[np.arange(cfg.n_envs) != e] == H).all()
    assert done_at[e] >= X[e]
    # the real step re-plans at step X - 1 and not before: its ped_due bit, or the pedestrian's waypoint row, changes there
    before = saved["ped_waypoints"][e, 0].cpu().numpy()
    for h in range(X[e]):
        due = bool(int(step["ped_due"][e, h]) & 1) if "ped_due" in step else False
        moved = not np.array_equal(step["ped_waypoints"][e, h, 0], before) or step["ped_n_waypoints"][e, h, 0] != nw
        assert (due or moved) == (h == X[e] - 1), "step %d: due %s, route changed %s" % (h, due, moved)
        before = step["ped_waypoints"][e, h, 0]
    rows_equal_the_step(out, step, n_peds, np.minimum(X, done_at), "replan")
    # the forecast goes on without the re-plan: all H rows are filled
    n = int(n_peds[e])
    assert np.isfinite(out["pose"][e, :, :n]).all() and (out["pose"][e, :, :n, :2] != 0).all() and (out["pose"][e] != 77).all()
    assert np.isfinite(out["min_dist"][e, :n]).all() and (out["min_step"][e, :n] >= 0).all()
    moving = np.linalg.norm(out["pose"][e, H - 1, 0, :2] - out["pose"][e, X[e] - 1, 0, :2])
    assert moving > 0.0                                                 # still heading for its last waypoint


# ---- 3. against navsim_rollout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_robot_and_exactness_equal_the_rollout(gpu, make):
    from nav_gym_amd import sim
    g = make(gpu)
    cfg, H = g.cfg, H6
    R = sim.rollout_defaults(cfg, float(g.t["scan_discomfort"].max().item()))["range"]
    actions, cmd = sequence(g, H, 31), commands(g, 12)
    out = pf.call(gpu, cfg, g.st, H, actions=actions, ped_cmd=cmd)
    roll = rc.call(gpu, cfg, g.st, actions[:, None], R, ped_cmd=cmd)
    L = roll["length"][:, 0]
    print("%s: the rollout's lengths %s" % (make.__name__, L))
    assert (L >= 1).all() and (L == H).any()
    for e in range(cfg.n_envs):
        same_bits(out["robot_pose"][e, :L[e]], roll["pose"][e, 0, :L[e]], "arena %d robot_pose" % e)
    whole = L == H
    eq(out["exact_steps"][whole], roll["exact_steps"][whole, 0], "exact_steps")


# ---- 4. robot modes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", TWIST, ids=TWIST_IDS)
def test_hold_repeats_the_previous_action(gpu, make):
    g = make(gpu)
    H, cmd = 5, commands(g, 12)
    prev = g.t["prev_action"].cpu().numpy()
    assert prev.any()                                                                # (warm: live)
    hold = pf.call(gpu, g.cfg, g.st, H, robot=abi.FORECAST_HOLD, ped_cmd=cmd)
    same = pf.call(gpu, g.cfg, g.st, H, actions=np.repeat(prev[:, None], H, axis=1), ped_cmd=cmd)
    all_same(hold, same, "hold")


@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_stop_is_the_zero_action(gpu, make):
    g = make(gpu)
    H, cmd = 5, commands(g, 12)
    stop = pf.call(gpu, g.cfg, g.st, H, robot=abi.FORECAST_STOP, ped_cmd=cmd)
    zero = pf.call(gpu, g.cfg, g.st, H, actions=np.zeros((g.cfg.n_envs, H, 2)), ped_cmd=cmd)
    all_same(stop, zero, "stop")
    if not g.cfg.clamp_action:               # a robot that stands, to the rounding of the axle offset's two sums a step (ulp 4e-15)
        assert np.abs(stop["robot_pose"][:, -1, :2] - g.t["robot_pose"].cpu().numpy()[:, :2]).max() < 1e-12


# ---- 5. horizon independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_short_horizons_are_the_leading_rows(gpu, make):
    g = make(gpu)
    cfg, HM = g.cfg, abi.FORECAST_MAX_H
    actions, cmd = sequence(g, HM, 51), commands(g, 12)
    long = pf.call(gpu, cfg, g.st, HM, actions=actions, ped_cmd=cmd)
    n_peds, now = counts(g), g.t["robot_pose"].cpu().numpy()
    assert (long["pose"] != 77).all() and (long["robot_pose"] != 77).all()
    for H in (1, 3):
        short = pf.call(gpu, cfg, g.st, H, actions=actions[:, :H], ped_cmd=cmd)
        for k in ("pose", "vel", "rel", "robot_pose"):
            same_bits(short[k], np.ascontiguousarray(long[k][:, :H]), "H = %d: %s" % (H, k))
        d = spec.derived(long["pose"], long["robot_pose"], now, n_peds, horizon=H)
        same_bits(short["min_dist"], d["min_dist"], "H = %d: min_dist" % H)
        same_bits(short["min_step"], d["min_step"], "H = %d: min_step" % H)
        eq(short["exact_steps"], np.minimum(long["exact_steps"], H), "H = %d: exact_steps" % H)


# ---- 6. derived outputs and the constant-velocity model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", WORLDS, ids=IDS)
def test_derived_outputs_and_const_vel_equal_the_spec(gpu, make):
    g = make(gpu)
    cfg, H = g.cfg, 7
    actions, cmd = sequence(g, H, 61), commands(g, 12)
    n_peds, now = counts(g), g.t["robot_pose"].cpu().numpy()
    true = pf.call(gpu, cfg, g.st, H, actions=actions, ped_cmd=cmd)
    cv = pf.call(gpu, cfg, g.st, H, model=abi.FORECAST_CONST_VEL, actions=actions)
    for name, out in (("true", true), ("const_vel", cv)):
        d = spec.derived(out["pose"], out["robot_pose"], now, n_peds)
        for k in ("rel", "min_dist", "min_step"):
            same_bits(out[k], d[k], "%s %s: %s" % (make.__name__, name, k))
        spec.unused_rows_are_empty(out, n_peds, name)
        assert (out["status"] == 1).all()
    pose, vel = spec.const_vel(g.t["ped_pose"].cpu().numpy(), g.t["ped_vel"].cpu().numpy(), n_peds, cfg.time_step, H)
    same_bits(cv["pose"], pose, "const_vel pose")
    same_bits(cv["vel"], vel, "const_vel vel")
    same_bits(cv["robot_pose"], true["robot_pose"], "the robot moves by phase 0 under either model")
    assert (cv["exact_steps"] == 0).all()
    live = np.arange(cfg.max_peds)[None, :] < n_peds[:, None]
    assert (true["min_step"][live] >= 0).all() and np.isfinite(true["min_dist"][live]).all()
    if g.t["ped_vel"].cpu().numpy()[live].any():
        assert not np.array_equal(cv["pose"], true["pose"])                          # (the two models differ somewhere)


# ---- 7. skip -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [world_c, world_e], ids=[IDS[1], IDS[3]])
def test_skip_mask(gpu, make):
    g = make(gpu)
    cfg, H = g.cfg, 4
    saved = lc.save_state(g)
    actions, cmd = sequence(g, H, 71), commands(g, 12)
    skip = np.zeros(cfg.n_envs, np.uint8); skip[[1, cfg.n_envs - 1]] = 1
    plain = pf.call(gpu, cfg, g.st, H, actions=actions, ped_cmd=cmd)
    masked = pf.call(gpu, cfg, g.st, H, actions=actions, ped_cmd=cmd, skip=skip)
    for k, v in lc.save_state(g).items():
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after two calls" % k)
    eq(masked["status"], 1 - skip, "status")
    spec.skipped_rows_are_empty(masked, skip == 1, "skipped arenas")
    for k in pf.KEYS:
        same_bits(masked[k][skip == 0], plain[k][skip == 0], k)


# ---- 8. through NavGymEnv ---------------------------------------------------------------------------------------------------------------------
def test_env_info_reset_and_humans_rel(gpu):
    E, H, K = 48, 5, 2
    env = nav_env(num_envs=E, ped_forecast=H, observe_humans=K)
    env.reset()
    N = env.cfg.max_peds
    shapes = dict(pose=(E, H, N, 3), vel=(E, H, N, 2), rel=(E, H, N, 2), robot_pose=(E, H, 3), min_dist=(E, N), min_step=(E, N),
                  exact_steps=(E,), status=(E,), humans_rel=(E, H, K, 2))
    first = env.ped_forecast()                                                       # valid after reset()
    assert set(first) == set(shapes)
    for k, v in first.items():
        want = "float32" if k == "humans_rel" else abi.FORECAST_OUT[k][0]
        assert tuple(v.shape) == shapes[k] and str(v.dtype) == "torch." + want and v.is_cuda, k
    assert bool((first["status"] == 1).all())
    rng, listed = np.random.default_rng(3), 0
    for t in range(4):
        _, _, _, info = env.step(random_actions(rng, E))
        assert info["ped_forecast"] is env.ped_forecast()
        f, humans = info["ped_forecast"], info["humans"]
        rel, index = f["rel"].cpu().numpy(), humans["index"].cpu().numpy()
        want = np.zeros((E, H, K, 2), np.float32)
        for e in range(E):
            for k in range(K):
                if index[e, k] >= 0:
                    want[e, :, k] = rel[e, :, index[e, k]]
        same_bits(f["humans_rel"].cpu().numpy(), want, "humans_rel at step %d" % t)
        listed += int((index >= 0).sum())
        n_peds = np.clip(env.sim.t["n_peds"].cpu().numpy(), 0, N)
        d = spec.derived(f["pose"].cpu().numpy(), f["robot_pose"].cpu().numpy(), env.sim.t["robot_pose"].cpu().numpy(), n_peds)
        same_bits(rel, d["rel"], "rel at step %d" % t)
    assert listed > 0, "condition: some pedestrian is observed"
    # an explicit query writes into buffers of its own: what the step returned stays intact
    kept = {k: v.clone() for k, v in env.ped_forecast().items()}
    q = env.ped_forecast(actions=np.zeros((H, 2)))
    assert set(q) == set(abi.FORECAST_OUT) and q["pose"].data_ptr() != env.ped_forecast()["pose"].data_ptr()
    for k, v in env.ped_forecast().items():
        same_bits(v.cpu().numpy(), kept[k].cpu().numpy(), "info's %s after a query" % k)
    mask = np.zeros(E, bool); mask[::3] = True
    env.reset(mask)
    after = env.ped_forecast()                                                       # valid after reset(mask)
    assert bool((after["status"] == 1).all()) and tuple(after["pose"].shape) == shapes["pose"]
    now = env.sim.t["robot_pose"].cpu().numpy()
    d = spec.derived(after["pose"].cpu().numpy(), after["robot_pose"].cpu().numpy(), now, np.clip(env.sim.t["n_peds"].cpu().numpy(), 0, N))
    same_bits(after["rel"].cpu().numpy(), d["rel"], "rel after reset(mask)")


def test_env_next_step_autoreset_one_arena_and_off(gpu):
    H = 4
    env = nav_env(num_envs=32, ped_forecast=H, ped_forecast_params=dict(robot="stop"), autoreset_mode="next_step")
    env.reset()
    seen = 0
    for t in range(40):
        _, _, done, info = env.step(np.tile([0.5, 0.0], (32, 1)))                    # straight on: arenas crash
        pending = done.cpu().numpy()
        f = {k: v.cpu().numpy() for k, v in info["ped_forecast"].items()}
        eq(f["status"], (~pending).astype(np.uint8), "status at step %d" % t)
        spec.skipped_rows_are_empty(f, pending, "pending arenas at step %d" % t)
        seen += int(pending.sum())
    assert seen > 0, "no arena finished: nothing was skipped"
    one = nav_env(num_envs=1, ped_forecast=H, ped_forecast_params=dict(model="const_vel"))
    one.reset()
    row = one.ped_forecast()
    N = one.cfg.max_peds
    assert isinstance(row["pose"], np.ndarray) and row["pose"].shape == (H, N, 3) and row["rel"].shape == (H, N, 2)
    assert row["robot_pose"].shape == (H, 3) and row["min_dist"].shape == (N,) and row["status"] == 1 and row["exact_steps"] == 0
    _, _, _, info = one.step(np.array([0.2, 0.1]))
    assert isinstance(info["ped_forecast"]["vel"], np.ndarray) and info["ped_forecast"]["vel"].shape == (H, N, 2)
    q = one.ped_forecast(actions=np.zeros((H, 2)))
    assert isinstance(q["pose"], np.ndarray) and q["pose"].shape == (H, N, 3)
    # off: nothing is allocated and nothing runs
    off = nav_env(num_envs=4)
    off.reset()
    _, _, _, info = off.step(np.zeros((4, 2)))
    assert off._products == [] and "ped_forecast" not in info and not any(k.startswith("ped_forecast") for k in off.sim.products)


def test_env_plan_equals_a_query_with_the_planner_s_plan(gpu):
    E, H = 16, 6
    env = nav_env(num_envs=E, ped_forecast=H, ped_forecast_params=dict(robot="plan"), local_planner="mppi",
                  local_planner_params=dict(n_samples=8, horizon=8))
    env.reset()
    rng = np.random.default_rng(5)
    for t in range(3):
        _, _, _, info = env.step(random_actions(rng, E))
    plan = env.planner_plan()
    assert tuple(plan.shape) == (E, 8, 2) and bool((plan[:, :H] != 0).any())
    q = env.ped_forecast(actions=plan[:, :H])
    for k in abi.FORECAST_OUT:
        same_bits(info["ped_forecast"][k].cpu().numpy(), q[k].cpu().numpy(), "plan: %s" % k)
    moved = info["ped_forecast"]["robot_pose"].cpu().numpy()[:, -1, :2] - env.sim.t["robot_pose"].cpu().numpy()[:, :2]
    assert np.abs(moved).max() > 0.0
