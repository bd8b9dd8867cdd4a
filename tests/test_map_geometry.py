"""CPU: the oracle off the square, origin-zero, 5 cm grid (tests/map_geometry_scenes.py).

Three identities tie the unusual geometries back to the square map at the origin that the goldens pin, without any
reference to the device:
  * embedding   -- an H x W world equals its twin on the max(H, W)^2 map with the rest occupied, bit for bit, while every
                   position stays inside the leading min(H, W)^2 square (outside it xy_to_ij's clip differs: pinned below);
  * scaling     -- resolution x 2 with every length x 2: ranges, positions and distances exactly x 2 (0.1 = 2 x 0.05 in binary);
  * translation -- a shifted origin with shifted poses: scan rows and flags bit for bit while no pose changes its cell.
Each test asserts its own precondition and prints how many arenas and observations it covered.  Then the NumPy
specifications of the pedestrian and planning calls at shifted origins, resolutions 0.1 and 0.025, and non-square maps."""
import numpy as np
import pytest

import map_geometry_scenes as mg
import ref
from helpers import keti_thresholds
from map_geometry_runs import (ORIGINS, PED_SHIFT_BOUND, PED_TRANSLATION_SEED, SHAPES, STEPS, config, ped_shift_deviation, run,
                               scene)
from nav_gym_amd import abi

# ---- the oracle runs non-square worlds at all ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", ["closed", "open"])
def test_non_square_worlds_run_with_robots_beyond_the_leading_square(H, W, kind):
    cfg, occ, world = scene(H, W, abi.PED_SFM, inside=False, kind=kind)
    M = min(H, W)
    cells = mg.raw_cells(world["spawn_pose"], cfg, True)
    assert (cells.max(axis=-1) >= M).any(), "no spawn beyond the leading square"
    rec, _ = run(cfg, world)
    crashes, successes, restarts = mg.census(rec)
    print("%d x %d %s: %d crashes, %d successes, %d restarts" % (H, W, kind, crashes, successes, restarts))
    assert crashes > 0 and restarts > 0
    scans = np.stack([r["obs"][:, :cfg.n_scan_stack * cfg.n_beams] for r in rec])
    assert np.isfinite(scans).all() and (scans >= 0).all() and (scans <= np.float32(cfg.range_max)).all()
    if kind == "open":
        assert (scans == np.float32(cfg.range_max)).any(), "no ray left the map"


def test_the_clip_quirk_is_what_a_pose_beyond_the_leading_square_reads():
    """On an 85 x 330 map a robot at column 200 scans from column 84 (the x index is clipped against map_h), on a 330 x 85 map
    a robot at row 200 from row 84: the scan equals the one of a robot standing in the middle of that clipped cell's corner."""
    for H, W, far, clipped in ((85, 330, (200, 40), (84, 40)), (330, 85, (40, 200), (40, 84))):
        cfg = config(H, W, E=1, n_spawn=1)
        occ = mg.make_maps(1, H, W, 8, "open")
        f = ref.build_dt(occ)
        world = mg.make_world(cfg, occ, f, keti_thresholds(cfg), 8)
        for cell in (far, clipped):
            world["robot_pose"][0] = (*mg.cell_xy(cfg, np.array(cell)), 0.3)
            obs = ref.RefSim(cfg, world).reset_obs()
            if cell is far:
                first = obs[0, :cfg.n_beams].copy()
        assert np.array_equal(first, obs[0, :cfg.n_beams])
        assert tuple(ref.xy_to_ij_f32(mg.cell_xy(cfg, np.array([far])), (0, 0), 0.05, H, W)[0]) == clipped


# ---- the three identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("ped_model", [abi.PED_NONE, abi.PED_SFM, abi.PED_EXTERNAL])
def test_embedding_identity(H, W, ped_model):
    cfg, occ, world = scene(H, W, ped_model)
    big = mg.embed(occ)
    f_big = ref.build_dt(big)
    assert np.array_equal(f_big[:, :H, :W], world["field"]), "a closed ring keeps the field inside unchanged"
    cfg_e, world_e = mg.embedded_twin(cfg, world, f_big)
    rec, _ = run(cfg, world)
    rec_e, _ = run(cfg_e, world_e)
    covered = mg.check_embedding(cfg, rec, rec_e, "%d x %d model %d" % (H, W, ped_model))
    assert covered == cfg.n_envs * (STEPS + 1)
    crashes, successes, restarts = mg.census(rec)
    assert crashes > 0 and restarts > 0


def test_embedding_identity_fails_beyond_the_leading_square():
    """The precondition is not decoration: with robots beyond the square the twin reads other cells."""
    cfg, occ, world = scene(85, 330, inside=False)
    cfg_e, world_e = mg.embedded_twin(cfg, world, ref.build_dt(mg.embed(occ)))
    rec, _ = run(cfg, world, steps=2)
    rec_e, _ = run(cfg_e, world_e, steps=2)
    assert not np.array_equal(rec[0]["obs"], rec_e[0]["obs"])


@pytest.mark.parametrize("H,W", SHAPES + [(120, 120)])
def test_scaling_identity(H, W):
    cfg, occ, world = scene(H, W, min_turning_radius=0.3)
    cfg_k, world_k = mg.scaled_twin(cfg, world, 2.0)
    assert cfg_k.resolution == 0.1
    rec, _ = run(cfg, world)
    rec_k, _ = run(cfg_k, world_k, v_scale=2.0)
    covered = mg.check_scaling(cfg, rec, rec_k, 2.0, "%d x %d" % (H, W))
    assert covered == cfg.n_envs * (STEPS + 1)
    crashes, successes, restarts = mg.census(rec)
    assert crashes > 0 and restarts > 0


@pytest.mark.parametrize("H,W", [(85, 330), (203, 96), (120, 120)])
def test_scaling_identity_down_to_0_025(H, W):
    cfg, occ, world = scene(H, W)
    cfg_k, world_k = mg.scaled_twin(cfg, world, 0.5)
    assert cfg_k.resolution == 0.025
    rec, _ = run(cfg, world)
    rec_k, _ = run(cfg_k, world_k, v_scale=0.5)
    assert mg.check_scaling(cfg, rec, rec_k, 0.5, "%d x %d" % (H, W)) == cfg.n_envs * (STEPS + 1)


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("H,W", SHAPES + [(120, 120)])
def test_translation_identity(H, W, origin):
    cfg, occ, world = scene(H, W, inside=False)
    cfg_t, world_t = mg.translated_twin(cfg, world, origin)
    rec, _ = run(cfg, world)
    rec_t, _ = run(cfg_t, world_t)
    covered, dev = mg.check_translation(cfg, rec, cfg_t, rec_t, "%d x %d" % (H, W))
    assert covered == cfg.n_envs * (STEPS + 1)
    crashes, successes, restarts = mg.census(rec)
    assert crashes > 0 and restarts > 0


@pytest.mark.parametrize("origin", ORIGINS)
def test_translation_identity_with_pedestrians(origin):
    """Social-force pedestrians under translation: with every cell, flag and waypoint index equal (the preconditions; the
    seed is one that meets them), their state stays within PED_SHIFT_BOUND of the un-shifted run's."""
    cfg, occ, world = scene(96, 203, abi.PED_SFM, seed=PED_TRANSLATION_SEED)
    cfg_t, world_t = mg.translated_twin(cfg, world, origin)
    rec, _ = run(cfg, world)
    rec_t, _ = run(cfg_t, world_t)
    dev = ped_shift_deviation(cfg, rec, cfg_t, rec_t, "pedestrians, origin %s" % (origin,))
    assert max(float(np.abs(r["ped_vel"]).max()) for r in rec) > 0.1, "the pedestrians never moved"
    for k, bound in PED_SHIFT_BOUND.items():
        assert dev[k] <= bound, (k, dev[k], bound)


# ---- batch_xy_to_ij restated --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.05, 0.1, 0.025])
@pytest.mark.parametrize("origin", [(0.0, 0.0)] + ORIGINS)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_xy_to_ij_restatement_equals_the_oracle(H, W, origin, res):
    """map_geometry_scenes.xy_to_ij_f32 / _f64 (the five NumPy lines the GPU test holds the device against) and the oracle's
    functions: random positions up to a map's length outside the map, cell boundaries and their float32 neighbours."""
    rng = np.random.default_rng(H + int(1000 * res))
    L = max(H, W) * res
    b = rng.integers(-3, max(H, W) + 4, (6000, 2)) * res
    b32 = b.astype(np.float32)
    xy = np.concatenate([rng.uniform(-L, 2 * L, (20000, 2)), b, b + 0.5 * res, np.nextafter(b32, np.float32(np.inf)).astype(np.float64),
                         np.nextafter(b32, np.float32(-np.inf)).astype(np.float64)]) + np.asarray(origin)
    assert np.array_equal(mg.xy_to_ij_f64(xy, origin, res, H, W), ref.xy_to_ij(xy, origin, res, H, W))
    xy32 = xy.astype(np.float32)
    ij = mg.xy_to_ij_f32(xy32, origin, res, H, W)
    assert np.array_equal(ij, ref.xy_to_ij_f32(xy32, origin, res, H, W))
    assert ij.min() == 0 and ij[:, 0].max() == H - 1 and ij[:, 1].max() == W - 1        # x against map_h, y against map_w


# ---- the NumPy specifications at the geometries -----------------------------------------------------------------------------------
# (origin, resolution / 0.05).  A shift leaves every difference of positions within a few float64 ulps of a position (7e-15 m
# near 34 m), far below half a float32 ulp of any output, so float32 outputs move by at most ONE float32 ulp and every index,
# count and flag stays; a power-of-two scale (with every length of the parameters scaled) is exact.
GEOMETRIES = [((-16.0, 32.0), 1.0), ((-7.3, 12.9), 1.0), ((0.0, 0.0), 2.0), ((0.0, 0.0), 0.5)]


def _ulp32(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > tol
    assert not bad.any(), "%s: %d values differ by more than one float32 ulp" % (what, int(bad.sum()))


def _ped_world(H, W, N=8, seed=9):
    cfg, occ, world = scene(H, W, abi.PED_EXTERNAL, inside=(H != W), seed=seed, N=N, E=5)
    world["ped_wp_head"] = np.zeros((cfg.n_envs, N), np.int32)
    return cfg, occ, world


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_ped_observe_spec_at_the_geometries(H, W, origin, k):
    import ped_observe_spec as spec
    cfg, occ, w = _ped_world(H, W)
    obs = lambda c, f, v, p: spec.observe(c, f, v["robot_pose"], v["n_peds"], v["ped_pose"], v["ped_vel"], p)
    p = dict(sensor_range=6.0, ped_radius=0.3, max_obs=4, rays=3)
    base = obs(cfg, w["field"], w, p)
    assert base["count"].sum() > 0 and (base["visible"] == 0).any()
    cfg_t, w_t = mg.geometry_twin(cfg, w, origin, k)
    twin = obs(cfg_t, w["field"], w_t, dict(p, sensor_range=6.0 * k, ped_radius=0.3 * k))
    for key in ("count", "index", "visible"):
        assert np.array_equal(base[key], twin[key]), key
    scale = np.array([k, k, k, k, k], np.float32)
    (_ulp32 if k == 1.0 else mg._same)(base["state"] * scale, twin["state"], "state")
    if H != W:                                  # the embedding: the same world on the square map, bit for bit
        big = ref.build_dt(mg.embed(occ))
        cfg_e, w_e = mg.embedded_twin(cfg, w, big)
        emb = obs(cfg_e, big, w_e, p)
        for key in base:
            mg._same(base[key], emb[key], "embedded " + key)


@pytest.mark.parametrize("origin,k", GEOMETRIES)
def test_goal_path_spec_at_the_geometries(origin, k):
    import goal_path_spec as spec
    E, size, seed = 12, 100, 5301
    occ, w = spec.random_world(E, size, seed)
    fields = ref.build_dt(occ)
    cfg = spec.config(E, size)
    base = spec.goal_path(cfg, fields, w["robot_pose"], w["robot_goal"], {})
    assert (base["status"] & spec.OK).sum() >= 2
    cfg_t, w_t = mg.geometry_twin(cfg, w, origin, k)
    p = {n: v * k if n != "band_cost" else v for n, v in spec.DEFAULT.items()}
    twin = spec.goal_path(cfg_t, fields, w_t["robot_pose"], w_t["robot_goal"], p)
    for key in ("status", "dist"):
        assert np.array_equal(base[key], twin[key]), key
    for key in ("distance", "subgoal"):
        (_ulp32 if k == 1.0 else mg._same)(base[key] * np.float32(k), twin[key], key)


@pytest.mark.parametrize("origin,k", GEOMETRIES[:2])
def test_dwa_spec_at_a_shifted_origin(origin, k):
    """The chosen candidate, every first hit and the twist are those of the world at the origin; the scores move by the
    float64 rounding of positions near 34 m through six steps and weights of order one: below 1e-11."""
    import dwa_spec as spec
    E, N, size, seed = spec.BASE
    occ, w = spec.random_world(E, N, size, seed)
    fields = ref.build_dt(occ)
    cfg = spec.config(E, size, N)
    base = spec.plan(cfg, fields, w, spec.BASE_PARAMS)
    assert (base["first_hit"] != 0).any() and (base["first_hit"] == 0).any()
    cfg_t, w_t = mg.geometry_twin(cfg, w, origin, k)
    twin = spec.plan(cfg_t, fields, w_t, spec.BASE_PARAMS)
    for key in ("best", "status", "first_hit", "twist", "action"):
        assert np.array_equal(base[key], twin[key]), key
    _ulp32(base["clearance"], twin["clearance"], "clearance")
    ok = np.isfinite(base["scores"])
    assert np.array_equal(ok, np.isfinite(twin["scores"])) and np.abs(base["scores"][ok] - twin["scores"][ok]).max() < 1e-11


@pytest.mark.parametrize("res", [0.1, 0.025])
def test_dwa_spec_at_other_resolutions(res):
    """The same cells at another resolution with every length scaled: every candidate first hits something at the step it did."""
    import dwa_spec as spec
    E, N, size, seed = spec.BASE
    k = res / 0.05
    occ, w = spec.random_world(E, N, size, seed)
    fields = ref.build_dt(occ)
    cfg = spec.config(E, size, N)
    p = dict(spec.DEFAULT, **spec.BASE_PARAMS)
    base = spec.plan(cfg, fields, w, p)
    cfg_k, w_k = mg.geometry_twin(cfg, w, (0.0, 0.0), k)
    cfg_k.linvel_lo, cfg_k.linvel_hi = cfg.linvel_lo * k, cfg.linvel_hi * k
    lengths = ("acc_lin", "body_radius", "body_offset", "ped_radius", "margin", "clearance_cap")
    p_k = {n: (tuple(x * k for x in v) if isinstance(v, tuple) else v * k) if n in lengths else v for n, v in p.items()}
    twin = spec.plan(cfg_k, fields, w_k, p_k)
    assert np.array_equal(base["first_hit"], twin["first_hit"]) and (base["first_hit"] != 0).any()
    # (which admissible candidate wins is no part of it: the score's weights are per metre and are not scaled here)
    assert np.array_equal(np.isfinite(base["scores"]), np.isfinite(twin["scores"]))


@pytest.mark.parametrize("origin,k", [((-16.0, 32.0), 1.0), ((-7.3, 12.9), 2.0), ((-7.3, 12.9), 0.5)])
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_ped_orca_walls_spec_at_the_geometries(H, W, origin, k):
    """The specification on a hand-written rectangle list (the ring's four walls) at the geometries: pedestrians have
    walls in range, every command is finite, nothing is dropped, and on the embedding of a map that is
    not square the answer is the same bit for bit."""
    import ped_orca_spec as spec
    import ped_orca_walls_spec as wspec
    cfg, occ, w = _ped_world(H, W)
    R = mg.RING
    walls = np.array([(0, 0, W - 1, R - 1), (0, H - R, W - 1, H - 1), (0, R, R - 1, H - R - 1), (W - R, R, W - 1, H - R - 1)], np.int16)
    rects = np.zeros((cfg.n_envs, wspec.LIST_LEN, 4), np.int16)
    rects[:, 3:7] = walls
    cfg_t, w_t = mg.geometry_twin(cfg, w, origin, k)
    p = spec.params(cfg_t, time_horizon_obst=2.0, ped_radius=0.3 * k, robot_radius=0.9 * k, neighbor_dist=10.0 * k)
    cmd, head, dropped, census = wspec.ped_orca_walls(cfg_t, w_t, p, rects, 8)
    assert np.isfinite(cmd).all()
    assert census["0 edges in range"] < cfg.n_envs * cfg.max_peds and (dropped == 0).all()
    if H != W:
        cfg_e, w_e = mg.embedded_twin(cfg_t, w_t, w_t["field"])
        cmd_e, head_e, dropped_e, _ = wspec.ped_orca_walls(cfg_e, w_e, p, rects, 8)
        mg._same(cmd, cmd_e, "ped_cmd on the embedding")
        mg._same(head, head_e, "ped_wp_head on the embedding")
