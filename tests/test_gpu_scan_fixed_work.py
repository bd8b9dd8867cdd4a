"""The fixed work of a scan outside its probe loop (kernels_step.hpp; profiles/r20_scan_fixed/).

Three pieces of the fused step changed form without changing a bit of its results, and each has the places where it could:

* the beam direction of a 64-beam chunk (beam_dir_fast): no TwoSum, a wider acceptance margin and a guard at |angle| = 64
  instead -- debug function 13 (the call the scan makes, against beam_dir()), laid out one wavefront per 64 elements;
* the crash / discomfort vote behind scan A (vote_flags): one LDS word and one barrier -- rollouts whose flags are raised by
  the beams of ONE chunk, i.e. by one wavefront of the arena, asserted on the oracle's own scans;
* the scan's two configuration-only quotients (step_consts_publish): computed on two lanes of phase 0 -- rollouts with
  quotients that are not round numbers, with one and two beams, and with both branches of the march limit.

Every comparison is bit for bit against the CPU oracle, noise off.
"""
import numpy as np
import pytest

import probe_fastpaths_spec as spec
import ref
from gpu_support import gpu, device_world, eq, host_arrays, state_equal, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

STEPS = 12


# ------------------------------------------------------------------------------------------------ directions
LIDAR_STEP = 1.5 * np.pi / 1080            # the 270-degree lidar's 1081 robot-frame angles
GUARD = 64.0                               # beam_dir_fast declines |lin + lth| >= 64 (navsim_device.hpp [D])


def _codes(gpu, lth, lin):
    """debug function 13 on whole wavefronts: 0 = accepted and equal to beam_dir(), 1 = not accepted, 2 = accepted and different"""
    assert len(lth) % 64 == 0 and len(lth) == len(lin)
    return gpu.sim.debug_math(13, to_device(gpu, np.asarray(lth, np.float64)), to_device(gpu, np.asarray(lin, np.float64))).cpu().numpy()


def _lidar_angles(rng, n):
    return rng.integers(0, 1081, n) * LIDAR_STEP - 0.75 * np.pi


def test_directions_of_the_step_headings(gpu):
    """(i) 4 M (heading, beam) pairs, headings in [-pi, pi], the 270-degree lidar's angles.  Nothing accepted differs from
    beam_dir(), and the fallback stays below the 5e-5 per beam that test_beam_table_direction_is_the_full_evaluation allows
    (margin 6.6e-15 against that test's 3e-15 at 1.9e-6: about 4e-6 expected)."""
    rng = np.random.default_rng(20)
    n = 64 * 65536
    code = _codes(gpu, rng.uniform(-np.pi, np.pi, n).astype(np.float32), _lidar_angles(rng, n))
    rate = float((code == 1).mean())
    print("fallback rate %.3g per beam" % rate)
    assert int((code == 2).sum()) == 0, "table direction differs from beam_dir()"
    assert rate < 5e-5, "fallback rate %g" % rate


def test_directions_on_the_axes_and_at_powers_of_two(gpu):
    """(ii) heading + beam angle on the axes (a component near 0) and at +-60 / 120 degrees (a component at a power of two), and the
    nine nearest float32 headings of each: where the acceptance interval has something to get wrong."""
    base = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 1 / 3, 2 / 3, 4 / 3, 5 / 3, -0.5, -1.0, -1 / 3, -2 / 3]) * np.pi
    lin = np.repeat(np.arange(0, 1081, 7) * LIDAR_STEP - 0.75 * np.pi, len(base) * 9)
    tgt = np.tile(np.repeat(base, 9), len(lin) // (len(base) * 9))
    lth32 = (tgt - lin).astype(np.float32)
    for j in range(9):
        sl = slice(j, None, 9)
        for _ in range(abs(j - 4)):
            lth32[sl] = np.nextafter(lth32[sl], np.float32(np.inf if j > 4 else -np.inf))
    pad = -len(lin) % 64                                                   # whole wavefronts: the last one repeats the first pairs
    code = _codes(gpu, np.concatenate([lth32, lth32[:pad]]), np.concatenate([lin, lin[:pad]]))
    assert (code != 2).all(), "special directions: %d wrong" % int((code == 2).sum())
    assert (code == 0).mean() > 0.5                                        # the fast path is not simply declining everything here


def test_one_large_heading_in_a_wavefront(gpu):
    """(iii) wavefronts in which exactly ONE lane has |lin + lth| in [8, 16), where the float64 sum's rounding error is four
    times that of a heading in [-pi, pi]: the margin covers it, and the lane's neighbours are served as ever.  (The form that
    was not kept chose first or second order by a vote of the wavefront; these wavefronts are the ones that vote changed.)"""
    rng = np.random.default_rng(21)
    G = 8192
    lin = _lidar_angles(rng, G * 64).reshape(G, 64)
    lth = rng.uniform(-np.pi, np.pi, (G, 64))
    lane = rng.integers(0, 64, G)
    big = rng.uniform(8.0, 16.0, G) * rng.choice([-1.0, 1.0], G)
    lth[np.arange(G), lane] = big - lin[np.arange(G), lane]
    lth = lth.astype(np.float32)
    ang = np.abs(lin + lth.astype(np.float64))
    keep = ((ang >= 8.0) & (ang < 16.0)).sum(axis=1) == 1                   # (float32 rounding of the heading moved a few across 8 or 16)
    assert keep.mean() > 0.99
    code = _codes(gpu, lth[keep].reshape(-1), lin[keep].reshape(-1))
    assert int((code == 2).sum()) == 0, "table direction differs from beam_dir()"
    assert (code == 0).mean() > 0.999


def test_headings_at_and_beyond_the_guard_are_declined(gpu):
    """(iv) |lin + lth| >= 64: the bound on the float64 sum's rounding error was derived below that, so every such lane reports
    1 -- at the guard itself, next to it, far beyond it, at infinity -- while the lanes just below it are still served."""
    f32 = np.float32
    at = [f32(GUARD), np.nextafter(f32(GUARD), f32(np.inf)), f32(100.0), f32(1.0e6), f32(3.0e38), f32(np.inf)]
    lth = np.array([s * v for v in at for s in (1.0, -1.0)], np.float32)
    lth = np.resize(lth, 64)
    code = _codes(gpu, lth, np.zeros(64))                                   # lin = 0: lin + lth is the heading itself
    assert (code == 1).all(), code
    # the sum crosses the guard although the heading alone does not
    lin = np.full(64, 0.75 * np.pi)
    lth = np.linspace(GUARD - 0.75 * np.pi, GUARD, 64).astype(np.float32)
    beyond = lin + lth.astype(np.float64) >= GUARD
    assert beyond.sum() >= 60
    code = _codes(gpu, lth, lin)
    assert (code[beyond] == 1).all(), code
    rng = np.random.default_rng(22)
    lth = (rng.uniform(56.0, 61.0, 64 * 256) * rng.choice([-1.0, 1.0], 64 * 256)).astype(np.float32)
    code = _codes(gpu, lth, _lidar_angles(rng, len(lth)))                   # |lin + lth| < 61 + 2.4
    assert int((code == 2).sum()) == 0
    assert (code == 0).mean() > 0.99


# ------------------------------------------------------------------------------------------------ rollouts
def _actions(E, t):
    """straight ahead at full speed; arena 3 turns on the spot in the middle of its room"""
    act = np.tile(np.array([[0.5, 0.0]]), (E, 1))
    if E > 3:
        act[3] = (0.0, 0.3)
    return act


def _world(gpu, occ1, poses, B, step_block, final_obs=False, n_peds=0, **cfg_kw):
    """One room for all arenas, every spawn pose the arena's own start pose, goals out of reach; the HIP step and the oracle."""
    E, size = len(poses), occ1.shape[0]
    occ = np.repeat(occ1[None], E, axis=0)
    ped = dict(max_peds=4, ped_model=abi.PED_SFM) if n_peds else dict(max_peds=1, ped_model=abi.PED_NONE)
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, n_scan_stack=1, auto_reset=1, n_spawn=2, seed=20,
                                 step_block=step_block, field_format=abi.FIELD_U16T, **ped, **cfg_kw)
    spec.lidar(cfg, B)
    arrays = device_world(gpu, cfg, occ, n_peds, robot_clearance=0.3)
    xy = spec.poses_xy(cfg, poses)
    spawn = np.stack([xy, xy], axis=1)
    goal = np.repeat(spec.goals_xy(cfg, poses, size)[:, None], 2, axis=1).copy()
    arrays["spawn_pose"] = to_device(gpu, spawn); arrays["spawn_goal"] = to_device(gpu, goal)
    arrays["robot_pose"] = to_device(gpu, spawn[:, 0]); arrays["robot_goal"] = to_device(gpu, goal[:, 0])
    host = host_arrays(arrays, occ)
    return cfg, gpu.sim.NavSim(cfg, arrays, final_obs=final_obs), ref.RefSim(cfg, host), host


def _rollout(gpu, cfg, g, r, host, census=True, final_obs=False):
    """STEPS steps, every output and state array against the oracle.  Returns what the oracle's scans raised: per (step, arena)
    the 64-beam chunks with a beam below the crash threshold (C) and below the discomfort threshold (D) in scan A -- taken by a
    second oracle at the pose the step integrates to, since a crash replaces the row by its re-scan -- and, for a crash, D of
    that re-scan (the row the step returns)."""
    E, B = cfg.n_envs, cfg.n_beams
    probe = ref.RefSim(cfg, host) if census else None
    thr, dthr = host["scan_threshold"], host["scan_discomfort"]
    eq(g.reset_obs().cpu().numpy(), r.reset_obs(), "reset obs")
    seen = []
    for t in range(STEPS):
        act = _actions(E, t)
        before = r.a["robot_pose"].copy()
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        for k in rout:
            eq(gout[k].cpu().numpy(), rout[k], "%s at step %d" % (k, t))
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        done = rout["done"] != 0
        if final_obs and done.any():
            fin = {k: v.cpu().numpy() for k, v in g.final.items()}
            for k in ("final_obs", "final_goals"):
                eq(fin[k][done], r.final[k][done], "%s at step %d" % (k, t))
        if not census:
            seen += [(bool(rout["is_crash"][e]), None, None, None) for e in range(E)]
            continue
        probe.a["robot_pose"][:] = ref.integrate(before, act, cfg.time_step, cfg.axle_offset)[0]
        row_a = probe.reset_obs()[:, :B]
        for e in range(E):
            C = frozenset((np.flatnonzero(row_a[e] < thr) // 64).tolist())
            D = frozenset((np.flatnonzero(row_a[e] < dthr) // 64).tolist())
            crashed = bool(rout["is_crash"][e])
            assert crashed == bool(C), "the census scan disagrees with the oracle's crash flag (arena %d, step %d)" % (e, t)
            seen.append((crashed, C, D, frozenset((np.flatnonzero(ro[e, :B] < dthr) // 64).tolist()) if crashed else None))
    state_equal(g, r, "at the end")
    return seen


# ---- the vote.  A 128-cell bare room (6.1 m inside; the robot's crash threshold is 0.6 m ahead and 0.85 m at its corners, the
# discomfort threshold 1.1 m / 1.56 m).  Arenas 0 and 4 run into a wall head-on, 1, 2 and 5 obliquely (a corner of the footprint
# arrives first: few beams, one chunk), 3 turns in the middle, 6 and 7 start inside the discomfort distance of a wall, so
# their restart's re-scan reports discomfort again.
VOTE_POSES = [(95, 64, 0.0), (92, 40, 0.45), (30, 90, np.pi - 0.5), (64, 64, 1.0), (64, 108, 0.0), (100, 30, -0.6),
              (64, 100, 0.5 * np.pi), (40, 21, np.pi)]


def _assert_vote_cases(seen):
    one_chunk = [C for crashed, C, D, D2 in seen if crashed and len(C) == 1]
    assert one_chunk, "no crash is seen by the beams of one chunk alone"
    assert any(not crashed and D and any(D - C1 for C1 in one_chunk) for crashed, C, D, D2 in seen), \
        "no step raises discomfort alone, in a chunk other than a one-chunk crash's"
    assert any(crashed and D - C for crashed, C, D, D2 in seen), "no step raises crash and discomfort in different chunks"
    assert any(not crashed and not D for crashed, C, D, D2 in seen), "no step raises neither flag"
    assert any(crashed and D2 for crashed, C, D, D2 in seen), "no crash's re-scan reports discomfort"


VOTE_CASES = [(B, blk) for B in (65, 127, 1081) for blk in (64, 256, 512, 1024)]


@pytest.mark.parametrize("B,step_block", VOTE_CASES, ids=["B%d-block%d" % c for c in VOTE_CASES])
def test_vote_of_one_chunk_reaches_the_arena(gpu, B, step_block):
    cfg, g, r, host = _world(gpu, spec.room(128), VOTE_POSES, B, step_block)
    _assert_vote_cases(_rollout(gpu, cfg, g, r, host))


@pytest.mark.parametrize("B,step_block", [(127, 256), (1081, 512)])
def test_vote_with_terminal_rows(gpu, B, step_block):
    """io.final_obs: the FEAT twin of the kernel, whose crash pass re-scans the reverted pose into the terminal row first"""
    cfg, g, r, host = _world(gpu, spec.room(128), VOTE_POSES, B, step_block, final_obs=True)
    _assert_vote_cases(_rollout(gpu, cfg, g, r, host, final_obs=True))


@pytest.mark.parametrize("B,step_block", [(127, 64), (1081, 256), (1081, 1024)])
def test_vote_with_pedestrians(gpu, B, step_block):
    """four social-force pedestrians: the flags come per lane from finish_beams and a ballot makes them one per wavefront"""
    cfg, g, r, host = _world(gpu, spec.room(128), VOTE_POSES, B, step_block, n_peds=4)
    seen = _rollout(gpu, cfg, g, r, host, census=False)
    assert any(s[0] for s in seen) and not all(s[0] for s in seen)


# ---- the constants: (angle_last - angle_min) / (n_beams - 1) and min(H W, floor(range_max / resolution) + 4)
def _poses(size):
    s = size
    return [(s // 2, s // 2, 0.3), (int(s * 0.3), s // 2, np.pi), (int(s * 0.6), int(s * 0.35), -0.5 * np.pi), (s // 2, int(s * 0.65), 0.5 * np.pi)]


#                  name            B     size  resolution  range_max  the limit is
CONST_WORLDS = [("one_beam",       1,    64,   0.05,       25.0,      "range"),
                ("two_beams",      2,    64,   0.05,       25.0,      "range"),
                ("lidar_1081",     1081, 64,   0.05,       25.0,      "range"),
                ("3.5m_at_0.07m",  127,  128,  0.07,       3.5,       "range"),      # 50.00000000000001: floor 50
                ("3.3m_at_0.07m",  1081, 128,  0.07,       3.3,       "range"),      # 47.14...: rays end at the limit inside the room
                ("map_is_limit",   127,  20,   0.2,        100.0,     "map")]        # 400 cells < 504
CONST_CASES = [w + (blk,) for w in CONST_WORLDS for blk in (64, 256)]


@pytest.mark.parametrize("name,B,size,resolution,range_max,limit,step_block", CONST_CASES, ids=["%s-block%d" % (c[0], c[6]) for c in CONST_CASES])
def test_scan_constants_from_phase_0(gpu, name, B, size, resolution, range_max, limit, step_block):
    q = range_max / resolution
    assert (limit == "map") == (size * size < np.floor(q) + 4.0)
    if name.endswith("0.07m"):
        assert q != np.rint(q)
    cfg, g, r, host = _world(gpu, spec.room(size), _poses(size), B, step_block, resolution=resolution, range_max=range_max)
    seen = _rollout(gpu, cfg, g, r, host, census=False)
    assert len(seen) == STEPS * 4
