"""GPU: lookahead observations (include/navsim.h navsim_lookahead_obs) against navsim_step itself, with scan noise ON.  The entry is
called once; then, for every candidate, the saved state and observation are put back, navsim_step runs with that action, and
everything both return -- the row, the goals, reward, done, truncated, the flags, the distance -- is compared bit for bit.  Six
arenas, 67 beams (two chunks, the second partial), a stack of 3 (one world: 1).  Same-step auto-reset, the noise switch, K = 1
and 64, the skip mask, rows='scan', the untouched state and NavGymEnv follow."""
import numpy as np
import pytest

import lookahead_call as lc
import lookahead_obs_call as loc
from gpu_support import eq, gpu, nav_env, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

E, B = 6, 67
GRID9 = np.array([(v, w) for v in (0.0, 0.25, 0.5) for w in (-0.6, 0.0, 0.6)])          # 3 linear velocities x 3 turn rates
FACE_A, FACE_B = 80, 40                                                                    # x cell of the block's face, worlds (a) / (b)


def warm(gpu, g, seed, cmds=False):
    """Five seeded random steps: prev_action, the waypoint heads, the leg odometry and the scan stack are live afterwards."""
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


def world_a(gpu, mode=abi.AUTORESET_NONE, final_obs=False):
    """No pedestrians, a 96 x 120 map with its origin off zero, float32 field, full circle, stack of 3."""
    H, W = 96, 120
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=3, seed=5,
                                 field_format=abi.FIELD_F32, origin_x=-1.0, origin_y=2.0, auto_reset=mode, n_spawn=4)
    gpu.world.lidar_full_circle(cfg, B)
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


def world_b(gpu):
    """Social force, 8 slots with 6 present, legs mixed, a 270 degree fan, packed field with rect records, arena 0 on the overflow
    plane (an almost empty 528-cell room), a time limit that arena 4 reaches on this step, stack of 3."""
    S = 528
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=8, ped_model=abi.PED_SFM, n_scan_stack=3, seed=7,
                                 field_format=abi.FIELD_U16T, n_spawn=4)
    gpu.world.lidar_1081(cfg)
    cfg.n_beams = B
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
    lc.place(g, cfg, 5, face - 0.62, y)
    g.t["steps"][4] = 49
    histories(g, 3)
    return g


def world_c(gpu):
    """NAVSIM_PED_EXTERNAL: the commands come as an argument that differs from the state's.  The world with a stack of 1."""
    S = 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=4, ped_model=abi.PED_EXTERNAL, n_scan_stack=1, seed=9,
                                 field_format=abi.FIELD_U16T)
    gpu.world.lidar_full_circle(cfg, B)
    g = loc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 9), 3)
    warm(gpu, g, 3, cmds=True)
    return g


def world_d(gpu):
    """Wheel speeds as actions, clamped, with a minimum turning radius; stack of 3."""
    S = 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=3, seed=11,
                                 field_format=abi.FIELD_U16T, action_kind=abi.ACTION_WHEELS, clamp_action=1, min_turning_radius=0.4)
    gpu.world.lidar_full_circle(cfg, B)
    g = loc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 11), 0)
    warm(gpu, g, 4)
    histories(g, 3)
    return g


def noisy(g):
    std = g.t["scan_noise_std"].cpu().numpy()
    assert g.cfg.add_scan_noise and (std > 0).all(), std
    return std


def same_as_step(look, step, what, final=False):
    """Everything navsim_step returns.  final (same-step auto-reset): a done candidate's row and goals are the terminal ones."""
    for name in loc.STEP_KEYS:
        same_bits(look[name], step[name], "%s: %s" % (what, name))
    if "truncated" in step:
        same_bits(look["truncated"], step["truncated"], "%s: truncated" % what)
    else:
        assert not look["truncated"].any(), what
    obs, goals = step["obs"], step["goals"]
    if final:
        done = step["done"] != 0
        assert done.any() and not done.all(), "%s: done %d of %d" % (what, done.sum(), done.size)
        obs = np.where(done[:, :, None], step["final_obs"], obs)
        goals = np.where(done[:, :, None], step["final_goals"], goals)
    same_bits(look["obs"], obs, "%s: row" % what)
    same_bits(look["goals"], goals, "%s: goals" % what)
    S_B = look["obs"].shape[2] - abi.OBS_TAIL
    same_bits(look["scan"], look["obs"][:, :, S_B - look["scan"].shape[2]:S_B], "%s: scan against the row's newest slot" % what)
    same_bits(look["tail"], look["obs"][:, :, S_B:], "%s: tail against the row's" % what)
    assert (look["status"] == 1).all()


@pytest.mark.parametrize("make", [world_a, world_b], ids=["a-no-peds-f32", "b-sfm-packed-overflow"])
def test_equals_the_step_with_noise(gpu, make):
    g = make(gpu)
    cfg = g.cfg
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions = np.broadcast_to(GRID9, (E, 9, 2)).copy()
    look = loc.call(gpu, cfg, g.st, actions, obs0)
    for k, v in lc.save_state(g).items():                                            # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the call" % k)
    same_bits(g.obs.cpu().numpy(), obs0.cpu().numpy(), "the observation after the call")
    step = loc.steps_of(gpu, g, saved, obs0, actions)
    # conditions on the test's inputs, from the STEP's results
    crash, succ = step["is_crash"] != 0, step["is_success"] != 0
    n_crash = crash.sum(axis=1)
    print("rows: crash %d, success %d, done %d of %d; crashing candidates per arena %s" % (crash.sum(), succ.sum(), step["done"].sum(),
                                                                                         crash.size, n_crash.tolist()))
    assert ((n_crash >= 2) & (n_crash < 9)).any(), "no arena with two crashing candidates and one that does not crash"
    assert succ.any() and (~crash & ~succ).any()
    nh = saved["n_hist"].cpu().numpy()
    assert crash[nh == 0].any() and crash[nh == 2].any(), "the re-scan must meet an empty and a full history"
    clean = lc.call(gpu, cfg, g.st, actions, cfg.range_max)                          # the noise-free lookahead
    assert not np.array_equal(look["margin"], clean["margin"]), "the noise changed nothing"
    if cfg.max_episode_steps > 0:                                                    # arena 4 truncates unless it ends otherwise
        assert step["truncated"][4].any() and step["done"][4].all()
    same_as_step(look, step, make.__name__)
    # the shared re-scan: the crashing candidates of an arena carry the same scan, the others do not
    e = int(np.flatnonzero((n_crash >= 2) & (n_crash < 9))[0])
    ks = np.flatnonzero(crash[e])
    for k in ks[1:]:
        same_bits(look["scan"][e, k], look["scan"][e, ks[0]], "re-scan of arena %d" % e)
    assert not np.array_equal(look["scan"][e, np.flatnonzero(~crash[e])[0]], look["scan"][e, ks[0]])
    # margin and discomfort, which the step does not return, from the scan the step did return (candidates that do not crash)
    thr, dthr = g.t["scan_threshold"].cpu().numpy(), g.t["scan_discomfort"].cpu().numpy()
    ok = ~crash
    newest = step["obs"][:, :, 2 * B:3 * B]
    same_bits(look["margin"][ok], (newest - thr).min(axis=2)[ok], "margin")
    eq(look["discomfort"][ok], (newest < dthr).any(axis=2)[ok].astype(np.uint8), "discomfort")
    assert (look["margin"][crash] < 0).all() and not look["discomfort"][crash].any()


def test_external_commands_and_a_stack_of_one(gpu):
    g = world_c(gpu)
    noisy(g)
    assert g.cfg.n_scan_stack == 1
    saved, obs0 = lc.save_state(g), g.obs.clone()
    rng = np.random.default_rng(8)
    cmd = np.stack([rng.uniform(0, 0.6, (E, 4)), rng.uniform(-0.6, 0.6, (E, 4))], axis=2)
    assert not np.array_equal(cmd, saved["ped_cmd"].cpu().numpy())
    actions = np.broadcast_to(GRID9, (E, 9, 2)).copy()
    look = loc.call(gpu, g.cfg, g.st, actions, obs0, ped_cmd=cmd)
    same_bits(g.t["ped_cmd"].cpu().numpy(), saved["ped_cmd"].cpu().numpy(), "the state's commands")
    same_as_step(look, loc.steps_of(gpu, g, saved, obs0, actions, ped_cmd=cmd), "external, commands given")
    same_as_step(loc.call(gpu, g.cfg, g.st, actions, None), loc.steps_of(gpu, g, saved, obs0, actions), "external, the state's commands")


def test_wheels_clamp_and_turning_radius(gpu):
    g = world_d(gpu)
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions = np.random.default_rng(10).uniform(-1.0, 5.0, (E, 9, 2))               # wheel speeds, some beyond the clamp
    look = loc.call(gpu, g.cfg, g.st, actions, obs0)
    same_as_step(look, loc.steps_of(gpu, g, saved, obs0, actions), "wheels")
    assert len(np.unique(look["pose"].reshape(-1, 3), axis=0)) > 9


def test_same_step_autoreset_terminal_rows(gpu):
    g = world_a(gpu, mode=abi.AUTORESET_SAME_STEP, final_obs=True)
    noisy(g)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    actions = np.broadcast_to(GRID9, (E, 9, 2)).copy()
    look = loc.call(gpu, g.cfg, g.st, actions, obs0)
    step = loc.steps_of(gpu, g, saved, obs0, actions)
    assert (step["is_crash"] != 0).any() and (step["is_success"] != 0).any()
    same_as_step(look, step, "same-step", final=True)


def test_noise_off_is_the_lookahead_and_the_clean_scan(gpu):
    g = world_b(gpu)
    noisy(g)
    cfg, obs0 = g.cfg, g.obs.clone()
    actions = np.broadcast_to(GRID9, (E, 9, 2)).copy()
    off = loc.call(gpu, cfg, g.st, actions, obs0, noise=abi.LOOKOBS_NOISE_OFF)
    plain = lc.call(gpu, cfg, g.st, actions, cfg.range_max)
    for name in loc.SHARED:
        same_bits(off[name], plain[name], "noise off against navsim_lookahead at range_max: %s" % name)
    on = loc.call(gpu, cfg, g.st, actions, obs0)
    assert not np.array_equal(on["scan"], off["scan"])
    g.t["scan_noise_std"].zero_()
    zero = loc.call(gpu, cfg, g.st, actions, obs0)
    for name in loc.KEYS:
        same_bits(zero[name], off[name], "std 0 against noise off: %s" % name)


def test_one_and_sixty_four_candidates_skip_and_scan_rows(gpu):
    g = world_a(gpu)
    saved, obs0 = lc.save_state(g), g.obs.clone()
    rng = np.random.default_rng(6)
    for K in (1, 64):
        actions = np.stack([rng.uniform(-0.1, 0.6, (E, K)), rng.uniform(-0.8, 0.8, (E, K))], axis=2)
        look = loc.call(gpu, g.cfg, g.st, actions, obs0)
        same_as_step(look, loc.steps_of(gpu, g, saved, obs0, actions), "K = %d" % K)
    assert (look["is_crash"] != 0).any()
    # rows='scan': no full row is asked for, and none is needed -- obs_prev may be NULL; everything else is the same
    scan = loc.call(gpu, g.cfg, g.st, actions, None, rows="scan")
    assert "obs" not in scan
    for name in scan:
        same_bits(scan[name], look[name], "rows='scan': %s" % name)
    # the skip mask
    skip = np.array([0, 1, 0, 0, 1, 1], np.uint8)
    masked = loc.call(gpu, g.cfg, g.st, actions, obs0, skip=skip)
    eq(masked["status"], 1 - skip, "status")
    for name in loc.KEYS:
        assert not masked[name][skip == 1].any(), name
        same_bits(masked[name][skip == 0], look[name][skip == 0], name)


# ---- through NavGymEnv -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_env_lookahead_obs_then_step_agree(gpu, mode):
    import torch
    K, n = 5, 16
    env = nav_env(num_envs=n, lookahead_obs=K, autoreset_mode=mode)
    env.reset()
    rng = np.random.default_rng(4)
    rows = torch.arange(n, device="cuda:0")
    compared = finished = 0
    pending = np.zeros(n, bool)
    for t in range(25):
        cand = np.stack([random_actions(rng, n, t) for _ in range(K)], axis=1)
        cand_t = torch.from_numpy(cand).to("cuda:0")
        out = env.lookahead_obs(cand_t)
        pick = torch.from_numpy(rng.integers(0, K, n)).to("cuda:0")
        want = {"row": out["observation"]["observation"][rows, pick].clone(), "ach": out["observation"]["achieved_goal"][rows, pick].clone(),
                "reward": out["reward"][rows, pick].clone(), "done": out["done"][rows, pick].clone(),
                "is_crash": out["is_crash"][rows, pick].clone()}
        eq(out["status"].cpu().numpy(), (~pending).astype(np.uint8), "status at step %d" % t)
        o, rew, done, info = env.step(cand_t[rows, pick].contiguous())
        d = done.cpu().numpy()
        live = ~pending                                                              # (next-step: a pending arena was reset, not stepped)
        row, ach = o["observation"], o["achieved_goal"]
        if mode == "same_step":                                                      # the terminal row rides in info
            m = done[:, None]
            row = torch.where(m, info["final_observation"]["observation"], row)
            ach = torch.where(m, info["final_observation"]["achieved_goal"], ach)
        same_bits(want["row"].cpu().numpy()[live], row.cpu().numpy()[live], "row at step %d" % t)
        same_bits(want["ach"].cpu().numpy()[live], ach.cpu().numpy()[live], "achieved goal at step %d" % t)
        same_bits(want["reward"].cpu().numpy()[live], rew.cpu().numpy()[live], "reward at step %d" % t)
        eq(want["done"].cpu().numpy()[live], d[live], "done at step %d" % t)
        same_bits(want["is_crash"].cpu().numpy()[live], info["is_crash"].cpu().numpy()[live], "is_crash at step %d" % t)
        compared += int(live.sum()); finished += int((d & live).sum())
        pending = d.copy() if mode == "next_step" else pending
    print("%s: %d arena-steps compared, %d of them ended an episode" % (mode, compared, finished))
    assert finished > 0, "no episode ended: the terminal rows were not compared"


def test_env_single_arena_and_scan_rows(gpu):
    one = nav_env(num_envs=1, lookahead_obs=9, lookahead_obs_params=dict(rows="scan", noise="off"))
    one.reset()
    row = one.lookahead_obs(GRID9)
    assert "observation" not in row and row["scan"].shape == (9, 256) and row["tail"].shape == (9, 7)
    assert row["reward"].shape == (9,) and row["done"].dtype == bool and row["truncated"].dtype == bool and row["status"] == 1
    assert one.sim.products["lookahead_obs"].params.noise == abi.LOOKOBS_NOISE_OFF
    full = nav_env(num_envs=1, lookahead_obs=9)
    full.reset()
    row = full.lookahead_obs(GRID9)
    D = full.sim.obs.shape[1]
    assert row["observation"]["observation"].shape == (9, D) and row["observation"]["observation"].dtype == np.float64
    assert row["observation"]["achieved_goal"].shape == (9, 2)
