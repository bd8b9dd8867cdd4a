"""The head of the fused step (kernels_step.hpp step_arena, StepHead; profiles/r22_step_head/).

A workgroup used to start with a chain of round trips: the index row one uint4 per thread at a time, then every scalar of the
arena where it was used.  Now the row is copied in batches of four uint4 per thread (row_copy), every scalar the step reads of
its arena is loaded in the same round (step_head_load), and the readers behind the phase-0 barrier -- n_hist and the noise
std on every wavefront, prev_pose / robot_goal / prev_action in the reward, the terminal row and the observation tail -- take
phase 0's copies in StepShared.  No value changed, only when it is read; so every case is a 12-step rollout of eight arenas
(one for the 1000 x 1000 map) compared bit for bit with the CPU oracle on outputs, rows and state, at the places where the
new form could go wrong:

* the row copy: rows of 136 to 2 081 uint4 (64 x 64 to 1000 x 1000 cells) under 64 to 1024 threads -- fewer elements than
  threads, exactly one batch, a ragged second batch, nine rounds in three batches;
* pointers and modes the head must respect: reset-only launches with and without a mask, the noise std absent / present
  with the noise off / on, the three restart modes, the terminal rows of a crash and of a success, the time limit, a scan
  stack of 1 and 3 across an episode boundary;
* the pedestrian kernel (the head's loads beside wavefront 0's pedestrian phase; terminal rows and next-step resets with the
  new head) and the pipelined reset path, whose kernels keep the older head.

Each case asserts on the ORACLE's outputs that the event it is named after happened.
"""
import numpy as np
import pytest

import probe_fastpaths_spec as spec
import ref
from gpu_support import gpu, device_world, eq, host_arrays, random_actions, sim_and_oracle, state_equal, to_device, to_numpy  # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

STEPS = 12


def _poses(size):
    """Eight starts in a bare room of size x size cells, by what happens to them within 12 steps of straight driving: 0 runs
    into a wall head-on, 1 and 2 obliquely, 3 turns on the spot, 4 drives along a wall inside its discomfort distance, 5 and 6
    reach a goal 0.8 m ahead, 7 starts close to a wall it then hits."""
    s, m = size, size // 2
    return [(s - 33, m, 0.0), (s - 36, m - s // 8, 0.45), (30, m - s // 8, np.pi - 0.5), (m, m, 1.0),
            (m, s - 21, 0.0), (m, m - 6, 0.5 * np.pi), (m - 6, m, np.pi), (36, 21, np.pi)]


WINNERS = (5, 6)


def _actions(E, t):
    act = np.tile(np.array([[0.5, 0.0]]), (E, 1))
    if E > 3:
        act[3] = (0.0, 0.3)
    return act


def _world(gpu, size, B, step_block, E=8, S=1, mode=abi.AUTORESET_SAME_STEP, final_obs=False, n_peds=0, T=0, noise=None, **cfg_kw):
    """One bare room for all arenas, both spawn poses of an arena its own start; goals out of reach except the winners'.
    noise: None, or (add_scan_noise, std per arena or None for no array at all).  -> (cfg, NavSim, RefSim, host)"""
    poses = _poses(size)[:E]
    occ = np.repeat(spec.room(size)[None], E, axis=0)
    ped = dict(max_peds=4, ped_model=abi.PED_SFM) if n_peds else dict(max_peds=1, ped_model=abi.PED_NONE)
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, n_scan_stack=S, auto_reset=mode, n_spawn=2, seed=22,
                                 step_block=step_block, field_format=abi.FIELD_U16T, **ped, **cfg_kw)
    spec.lidar(cfg, B)
    cfg.max_episode_steps = T
    arrays = device_world(gpu, cfg, occ, n_peds, robot_clearance=0.3)
    xy = spec.poses_xy(cfg, poses)
    goal = spec.goals_xy(cfg, poses, size)
    for e in WINNERS:
        if e < E:
            goal[e] = (xy[e, 0] + 0.8 * np.cos(xy[e, 2]), xy[e, 1] + 0.8 * np.sin(xy[e, 2]))
    spawn = np.stack([xy, xy], axis=1)
    goal2 = np.repeat(goal[:, None], 2, axis=1).copy()
    arrays["spawn_pose"] = to_device(gpu, spawn); arrays["spawn_goal"] = to_device(gpu, goal2)
    arrays["robot_pose"] = to_device(gpu, spawn[:, 0]); arrays["robot_goal"] = to_device(gpu, goal2[:, 0])
    if noise is not None:
        cfg.add_scan_noise = noise[0]
        if noise[1] is None:
            arrays.pop("scan_noise_std", None)
        else:
            arrays["scan_noise_std"] = to_device(gpu, np.asarray(noise[1], np.float32))
    host = host_arrays(arrays, occ)
    ocfg = cfg.copy()
    ocfg.max_episode_steps = 0                               # (the oracle has no time limit and no noise)
    ocfg.add_scan_noise = 0
    return cfg, gpu.sim.NavSim(cfg, arrays, final_obs=final_obs), ref.RefSim(ocfg, host), host


def _rollout(gpu, cfg, g, r, who=None, final_obs=False, steps=STEPS, between=None, skip_state=("counters",)):
    """steps steps, every output, row and (at the end) state array of the arenas `who` against the oracle.  The time limit
    (NAVSIM_AUTORESET_NONE only) is applied to the oracle's flags here.  -> what the ORACLE saw, summed over the rollout."""
    E, T = cfg.n_envs, cfg.max_episode_steps
    who = np.ones(E, bool) if who is None else who
    assert T == 0 or cfg.auto_reset == abi.AUTORESET_NONE
    first, first_ref = g.reset_obs().cpu().numpy().copy(), r.reset_obs().copy()
    eq(first[who], first_ref[who], "reset obs")
    seen = dict(crash=0, success=0, done=0, reset=0, trunc=0, crash_end=0, success_end=0, first=(first, first_ref))
    for t in range(steps):
        act = _actions(E, t)
        go, gout = g.step(to_device(gpu, act))
        ro, rout = r.step(act)
        gout = to_numpy(gout)
        done = rout["done"] != 0
        trunc = np.zeros(E, bool)
        if T > 0:
            trunc = (r.a["steps"] >= T) & ~done
            eq(gout["truncated"][who], trunc.astype(np.uint8)[who], "truncated at step %d" % t)
        for k in rout:
            want = (rout[k] | trunc) if k == "done" else rout[k]
            eq(gout[k][who], want[who], "%s at step %d" % (k, t))
        eq(go.cpu().numpy()[who], ro[who], "obs at step %d" % t)
        if final_obs and done.any():
            fin = to_numpy(g.final)
            for k in ("final_obs", "final_goals"):
                eq(fin[k][done & who], r.final[k][done & who], "%s at step %d" % (k, t))
        if cfg.auto_reset == abi.AUTORESET_NEXT_STEP:
            eq(g.reset_flags.cpu().numpy()[who], r.reset_flags[who], "reset flags at step %d" % t)
            seen["reset"] += int(r.reset_flags[who].sum())
        crash, win = (rout["is_crash"] != 0) & who, (rout["is_success"] != 0) & who
        seen["crash"] += int(crash.sum()); seen["success"] += int(win.sum()); seen["done"] += int((done & who).sum())
        seen["crash_end"] += int((crash & done).sum()); seen["success_end"] += int((win & done).sum())
        seen["trunc"] += int((trunc & who).sum())
        if between is not None:
            between(t)
    gs = g.numpy_state()
    for k, v in r.a.items():
        if k in gs and k not in ("field", "field_overflow", "rect_table", "rect_index", "scan_noise_std") + tuple(skip_state):
            per_arena = v.ndim > 0 and v.shape[0] == E and k not in ("scan_threshold", "scan_discomfort")
            eq(gs[k][who] if per_arena else gs[k], v[who] if per_arena else v, "state %s at the end" % k)
    return seen


# ------------------------------------------------------------------------------------------------ the row copy
# uint4 of a row: 128 + ceil(size / 8)^2 / 8 -> 64: 136, 200: 207 (a ragged uint4 at the end), 500: 625, 1000: 2 081
ROW_CASES = [(size, blk, 1081 if blk in (256, 1024) else 65) for size in (64, 200, 500) for blk in (64, 256, 512, 1024)]


@pytest.mark.parametrize("size,step_block,B", ROW_CASES, ids=["map%d-block%d-B%d" % c for c in ROW_CASES])
def test_row_copy_sizes_and_blocks(gpu, size, step_block, B):
    """rows shorter than the workgroup (64 x 64 everywhere above 64 threads, 500 x 500 at 1024), one exact batch, ragged batches"""
    cfg, g, r, _ = _world(gpu, size, B, step_block)
    seen = _rollout(gpu, cfg, g, r)
    assert seen["crash"] >= 2 and seen["success"] >= 1 and seen["done"] >= 3, seen       # (a restart re-scans through the same row)


def test_row_copy_nine_rounds(gpu):
    """one 1000 x 1000 arena at 256 threads: 2 081 uint4, nine per thread at most -- two full batches and a ragged third"""
    cfg, g, r, _ = _world(gpu, 1000, 1081, 256, E=1)
    seen = _rollout(gpu, cfg, g, r)
    assert seen["crash"] >= 1 and seen["done"] >= 1, seen


# ------------------------------------------------------------------------------------------------ pointers and modes
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_reset_only_launch(gpu, masked):
    """navsim_reset_obs in the middle of a rollout (no actions: the head must not read them), of all arenas and of every other
    one -- the untouched arenas carry their rows -- with a stack of three, whose history the reset clears"""
    cfg, g, r, _ = _world(gpu, 200, 65, 256, S=3, mode=abi.AUTORESET_NONE)
    mask = (np.arange(8) % 2 == 0).astype(np.uint8) if masked else None
    hits = []

    def between(t):
        if t in (4, 8):
            before = r.obs[r.cur].copy()
            rows = r.reset_obs(mask).copy()
            eq(g.reset_obs(None if mask is None else to_device(gpu, mask)).cpu().numpy(), rows, "rows after the reset at step %d" % t)
            if masked:
                assert np.array_equal(rows[mask == 0], before[mask == 0]) and not np.array_equal(rows[mask != 0], before[mask != 0])
            hits.append(t)
    seen = _rollout(gpu, cfg, g, r, between=between)
    assert hits == [4, 8] and seen["crash"] >= 1, seen


NOISE_STD = np.array([0.0, 0.03, 0.0, 0.03, 0.0, 0.0, 0.03, 0.0], np.float32)


@pytest.mark.parametrize("name,noise", [("absent-off", (0, None)), ("absent-on", (1, None)), ("present-off", (0, NOISE_STD)), ("present-on", (1, NOISE_STD))])
@pytest.mark.parametrize("step_block", [64, 256])
def test_noise_std_pointer_and_switch(gpu, name, noise, step_block):
    """scan_noise_std NULL with the noise off and on, an array with the noise off: the oracle's clean rows in every arena.  An array
    with the noise on: the arenas whose std is 0 stay the oracle's bit for bit, and the others' first rows carry noise of
    their own std (their rollouts leave the oracle's: a noisy scan decides a crash differently; tests/test_gpu_scan_noise.py
    checks every draw against its model)."""
    cfg, g, r, _ = _world(gpu, 200, 65, step_block, S=2, noise=noise)
    noisy = (NOISE_STD > 0) if name == "present-on" else np.zeros(8, bool)
    seen = _rollout(gpu, cfg, g, r, who=~noisy)
    assert seen["crash"] >= 1 and seen["done"] >= 2, seen
    if noisy.any():
        first, clean = (x[:, :2 * 65].astype(np.float64) for x in seen["first"])
        err = np.abs(first - clean)
        assert (err[noisy].max(axis=1) > 1e-4).all() and err[noisy].max() < 6 * 0.03 + 1e-6, err.max(axis=1)


@pytest.mark.parametrize("mode", [abi.AUTORESET_NONE, abi.AUTORESET_SAME_STEP, abi.AUTORESET_NEXT_STEP], ids=["none", "same_step", "next_step"])
@pytest.mark.parametrize("S", [1, 3])
def test_restart_modes_and_scan_stack(gpu, mode, S):
    """the three restart modes with one row and with a stack of three: episodes end by crash and by success inside the rollout,
    so n_hist -- now read from LDS by every wavefront -- goes 0, 1, 2, 2 ... and back to 0 where an episode starts"""
    cfg, g, r, _ = _world(gpu, 200, 1081, 256, S=S, mode=mode)
    seen = _rollout(gpu, cfg, g, r)
    assert seen["crash"] >= 2 and seen["success"] >= 1, seen
    if mode == abi.AUTORESET_NEXT_STEP:
        assert seen["reset"] >= 2, seen
    if mode != abi.AUTORESET_NONE:
        assert seen["done"] >= 4, seen                          # (restarted arenas finish again: the boundary is crossed more than once)


@pytest.mark.parametrize("B,step_block", [(65, 64), (1081, 256), (65, 512)])
def test_terminal_rows_after_a_crash_and_a_success(gpu, B, step_block):
    """io.final_obs (the FEAT twin): the terminal tail, goals and re-scan pose come from phase 0's copy of prev_pose / prev_action /
    robot_goal, while phase 4 has already written the NEXT episode's goal into the state"""
    cfg, g, r, _ = _world(gpu, 200, B, step_block, S=3, final_obs=True)
    seen = _rollout(gpu, cfg, g, r, final_obs=True)
    assert seen["crash_end"] >= 2 and seen["success_end"] >= 1, seen


@pytest.mark.parametrize("step_block", [64, 256])
def test_time_limit_hit(gpu, step_block):
    """cfg.max_episode_steps = 5 without restarts: the limit is tested on the step count the head loaded and incremented"""
    cfg, g, r, _ = _world(gpu, 200, 65, step_block, S=2, mode=abi.AUTORESET_NONE, T=5)
    seen = _rollout(gpu, cfg, g, r, skip_state=("counters", "done_steps"))
    assert seen["trunc"] >= 8, seen                            # (arena 3 turns on the spot: truncated from step 5 on)


# ------------------------------------------------------------------------------------------------ pedestrians, installs
@pytest.mark.parametrize("mode,final_obs", [(abi.AUTORESET_SAME_STEP, False), (abi.AUTORESET_SAME_STEP, True), (abi.AUTORESET_NEXT_STEP, False)],
                         ids=["same_step", "same_step-final_obs", "next_step"])
def test_pedestrian_world(gpu, mode, final_obs):
    """four social-force pedestrians at 256 threads: wavefront 0 advances them beside phase 0 (on wavefront 1) and keys their
    draws on the step count phase 0 publishes.  The pedestrian kernels always carry the terminal rows and the next-step
    reset, and they are the kernels with those paths that take the new head: the terminal tail, goals and re-scan pose of a
    crash and of a success from phase 0's copies, and an arena reset by its mask beside arenas that step."""
    cfg, g, r, _ = _world(gpu, 200, 1081, 256, S=3, n_peds=4, mode=mode, final_obs=final_obs)
    seen = _rollout(gpu, cfg, g, r, final_obs=final_obs)
    assert seen["crash_end"] >= 1 and seen["done"] >= 2, seen         # (pedestrians may stand between a winner and its goal)
    if mode == abi.AUTORESET_NEXT_STEP:
        assert seen["reset"] >= 1, seen
    assert int(r.a["n_peds"].min()) == 4


def test_pipelined_reset_world(gpu):
    """next-step restarts with worlds staged ahead (navsim_step_install): an arena that is reset installs its staged world in
    place of the step, or generates it itself.  These kernels keep the older form of the head (kNewHead in step_arena), so
    what this case guards of the change is StepShared's new layout under them and the row copy behind regen_lone; a
    -DNAVSIM_HEAD_EVERYWHERE=1 build runs their head behind that prelude through this case.  Robots 2-5 are put on their
    goals twice, so arenas finish and are reset inside 12 steps."""
    E, size, N = 8, 200, 6
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=abi.PED_SFM, n_spawn=6,
                                 auto_reset=abi.AUTORESET_NEXT_STEP, seed=31, field_format=abi.FIELD_U16T, regen_cap=E, min_goal_dist=3.0,
                                 max_goal_dist=8.0, spawn_clearance=0.9, ped_min_robot_dist=2.0, ped_min_goal_dist=4.0,
                                 regen_plan=0, regen_indoor_ratio=0.0, regen_min_steps=0, step_block=256)
    gpu.world.lidar_1081(cfg)
    occ = gpu.world.make_maps(E, size, 31)
    g, r, _ = sim_and_oracle(gpu, cfg, occ, 5)
    g.enable_pregen(pipeline=1, install=True)
    rng = np.random.default_rng(14)
    n_reset = 0
    for t in range(STEPS):
        if t in (1, 6):
            idx = gpu.torch.arange(2, 6, device=gpu.dev)
            g.t["robot_goal"][idx] = g.t["robot_pose"][idx, :2]
            r.a["robot_goal"][2:6] = r.a["robot_pose"][2:6, :2]
        act = random_actions(rng, E, t)
        go, gout = g.step(to_device(gpu, act))
        ro, rout = r.step(act)
        go = go.cpu().numpy(); gout = to_numpy(gout)
        for k in ("reward", "done", "is_success", "is_crash", "distance"):
            eq(gout[k], rout[k], "%s at step %d" % (k, t))
        flags = r.reset_flags != 0
        eq(go[~flags], ro[~flags], "obs at step %d" % t)      # (an installed arena's row is already its new world's)
        n_reset += int(flags.sum())
        eq(g.regen().cpu().numpy(), r.regen(), "obs after regen at step %d" % t)
        for k in ("achieved_goal", "desired_goal"):
            eq(g.out[k].cpu().numpy(), r.out[k], "%s after regen at step %d" % (k, t))
        if flags.any():
            gpu.torch.cuda.synchronize()
            state_equal(g, r, "after regen at step %d" % t, skip=("counters", "ped_waypoints"))
    cg, cr = g.counters(), r.counters()
    # two rounds of four arenas put on their goals: each is reset, and served with a new world, in the call after (an arena that
    # is being reset when its goal is moved finishes a call later, and may miss the rollout's end in the second round)
    assert n_reset >= 4 and cr["regen_served"] >= 4, (n_reset, cr)
    assert cg["regen_served"] == cr["regen_served"] and cg["regen_unserved"] == 0, (cg, cr)
