"""GPU: every map-reading kernel off the square, origin-zero, 5 cm grid (tests/map_geometry_scenes.py), bit for bit against
the CPU oracle or the NumPy specifications: the builders, navsim_cast_static, the fused step and navsim_reset_obs over a
covering set of field formats, block sizes and pedestrian models, the three identities of tests/test_map_geometry.py on the
device's own outputs, and the pedestrian and planning calls."""
import ctypes as C

import numpy as np
import pytest

import dwa_call
import dwa_spec
import goal_path_call
import goal_path_spec
import map_geometry_runs as cpu
import map_geometry_scenes as mg
import ped_observe_call
import ped_orca_spec
import ped_orca_walls_spec as wspec
import ref
from gpu_support import (gpu, decode_rect_index, decode_rect_table, device_map_arrays, device_world, eq, host_arrays,  # noqa: F401
                         rollout_pair, state_equal, to_device)
from helpers import keti_thresholds
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

SHAPES = cpu.SHAPES                         # 85 x 330, 330 x 85: no side a multiple of 8 or 32; 96 x 203, 203 x 96: one side is
BUILDER_SHAPES = SHAPES + [(37, 53)]
ORIGINS = [(0.0, 0.0)] + cpu.ORIGINS
STEPS = cpu.STEPS
NO_RECTS, RECTS_GLOBAL, RECTS_LDS = "no rects", "rects from global memory", "rects from LDS"


# ---- builders ----------------------------------------------------------------------------------------------------------------
def _maps(H, W, kind="closed", E=3, seed=21):
    return mg.make_maps(E, H, W, seed + H, kind)


@pytest.mark.parametrize("H,W", BUILDER_SHAPES)
def test_build_field_both_formats(gpu, H, W):
    occ = np.concatenate([_maps(H, W), _maps(H, W, "open", 2)])
    occ[-1] = 0; occ[-1, H // 3, W // 4] = 1                      # one obstacle cell: distances up to the far corner
    want = ref.build_dt(occ)
    f32, none, nsat = gpu.sim.build_field(to_device(gpu, occ), abi.FIELD_F32)
    eq(f32.cpu().numpy(), want, "float32 field %d x %d" % (H, W))
    assert none is None and nsat == 0
    packed, plane, nsat = gpu.sim.build_field(to_device(gpu, occ), abi.FIELD_U16T)
    eq(plane.cpu().numpy(), want, "float32 plane beside the packed field")
    n, th, tw = occ.shape[0], (H + 7) // 8, (W + 7) // 8
    assert packed.numel() * 2 == gpu.lib.load().navsim_field_bytes(n, H, W, abi.FIELD_U16T) == n * th * tw * 128
    raw = packed.cpu().numpy().view(np.uint16).reshape(n, th, tw, 8, 8)          # rows of tiles, tw tiles a row
    full = raw.transpose(0, 1, 3, 2, 4).reshape(n, th * 8, tw * 8)[:, :H, :W]
    sat = np.rint(want.astype(np.float64) ** 2) >= 65535                        # stored as 0xFFFF: read from the float32 plane
    assert nsat == int(sat.sum()) and np.array_equal(full == 0xFFFF, sat)
    eq(np.sqrt(full.astype(np.float32))[~sat], want[~sat], "decoded tiles %d x %d" % (H, W))


@pytest.mark.parametrize("H,W", BUILDER_SHAPES)
def test_build_rects_and_index(gpu, H, W):
    """Every valid record is exact on every cell of its tile, its rectangles are made of occupied cells inside (map_w, map_h);
    the index rows name the records; navsim_maps_closed sees a single free cell of the ring on each of the four sides."""
    occ = np.concatenate([_maps(H, W), _maps(H, W, "open", 1)])
    n = occ.shape[0]
    occ_t = to_device(gpu, occ)
    field, f32, _ = gpu.sim.build_field(occ_t, abi.FIELD_U16T)
    table_t = gpu.sim.build_rects(occ_t, field, abi.FIELD_U16T, f32)
    table = table_t.cpu().numpy()
    T = ((H + 7) // 8) * ((W + 7) // 8)
    assert table.shape == (n, T, 4) and T * 16 == gpu.lib.load().navsim_rect_table_bytes(1, H, W)
    d2, valid = decode_rect_table(table, H, W)
    exact = np.rint(ref.build_dt(occ).astype(np.float64) ** 2).astype(np.int64)
    assert np.array_equal(d2[valid], exact[valid]), "a valid record disagrees with the exact field"
    print("%d x %d: %.3f of the cells lie in tiles with a valid record" % (H, W, valid.mean()))
    assert valid.any()
    rec = table.view(np.uint32).reshape(n, T, 4)
    for m in range(n):
        for t in np.flatnonzero((rec[m, :, 0] & 0xFFFF) != 0x7FFF):
            for lo, hi in ((rec[m, t, 0], rec[m, t, 1]), (rec[m, t, 2], rec[m, t, 3])):
                x0, y0, x1, y1 = int(lo & 0xFFFF), int(lo >> 16), int(hi & 0xFFFF), int(hi >> 16)
                assert 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H, (m, t, x0, y0, x1, y1)
                assert occ[m, y0:y1 + 1, x0:x1 + 1].all(), (m, t, x0, y0, x1, y1)
    rows, n_rects = gpu.sim.build_rect_index(table_t, H, W)
    assert rows.shape[1] == abi.rect_index_row_bytes(H, W) == gpu.lib.load().navsim_rect_index_bytes(1, H, W)
    named, has = decode_rect_index(rows.cpu().numpy(), H, W)
    tile_valid = (rec[..., 0] & 0xFFFF) != 0x7FFF
    assert (n_rects.cpu().numpy() <= 255).all() and np.array_equal(has, tile_valid), "every valid record has an index"
    eq(named[has], rec[has], "records named by the index rows")
    # closed / open: the generated maps, then one free cell in the ring's inner layer on each side in turn, and a corner
    assert gpu.sim.maps_closed(occ_t).cpu().numpy().tolist() == [1] * (n - 1) + [0]
    holes = [(2, W // 2), (H - 3, W // 2), (H // 2, 2), (H // 2, W - 3), (H - 1, W - 1), (0, W - 1), (H - 1, 0)]
    one = np.repeat(occ[:1], len(holes) + 1, axis=0)
    for k, (y, x) in enumerate(holes):
        one[k, y, x] = 0
    assert gpu.sim.maps_closed(to_device(gpu, one)).cpu().numpy().tolist() == [0] * len(holes) + [1]


@pytest.mark.parametrize("H,W", [(85, 330), (203, 96)])
@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_world_closed_sees_one_free_cell_on_each_side(gpu, H, W, fmt):
    """navsim_world_closed reads the ring from the distance field in the world's format."""
    holes = [(2, W // 2), (H - 3, W // 2), (H // 2, 2), (H // 2, W - 3), (H - 1, W - 1)]
    occ = np.repeat(_maps(H, W, E=1), len(holes) + 2, axis=0)
    for k, (y, x) in enumerate(holes):
        occ[k, y, x] = 0
    E = occ.shape[0]
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, field_format=fmt)
    field, plane, _ = gpu.sim.build_field(to_device(gpu, occ), fmt)
    st = abi.NavsimState()
    st.field = field.data_ptr()
    n_open = gpu.torch.zeros(1, dtype=gpu.torch.int32, device=gpu.dev)
    assert gpu.lib.load().navsim_world_closed(C.byref(cfg), C.byref(st), n_open.data_ptr(), None) == 0
    gpu.torch.cuda.synchronize()
    assert int(n_open.item()) == len(holes)


@pytest.mark.parametrize("H,W", BUILDER_SHAPES)
def test_costmap(gpu, H, W):
    occ = np.concatenate([_maps(H, W), _maps(H, W, "open", 2)])
    occ[-1] = 0; occ[-1, 0, 0] = 1                     # one sampled obstacle cell in a corner: the inflation leaves free cells at any size
    got = gpu.sim.costmap(to_device(gpu, occ)).cpu().numpy()
    assert got.shape == (occ.shape[0], H // 5, W // 5)
    eq(got, ref.costmap(occ), "costmap %d x %d" % (H, W))
    assert 0 < got[-1].mean() < 1


@pytest.mark.parametrize("res", [0.05, 0.1, 0.025])
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_xy_to_ij(gpu, H, W, origin, res):
    """Both forms of the device's batch_xy_to_ij against the NumPy restatement (map_geometry_scenes.xy_to_ij_f32 / _f64) and
    the oracle: positions all over the map and a map's length beyond it on every side -- the x index clipped against map_h,
    the y index against map_w --, cell corners, and the float32 neighbours of cell boundaries."""
    rng = np.random.default_rng(H + int(1000 * res))
    L = max(H, W) * res
    xy = rng.uniform(-L, 2 * L, (20000, 2))
    b = rng.integers(-3, max(H, W) + 4, (6000, 2)) * res                        # cell boundaries
    b32 = b.astype(np.float32)
    xy = np.concatenate([xy, b, b + 0.5 * res, np.nextafter(b32, np.float32(np.inf)).astype(np.float64),
                         np.nextafter(b32, np.float32(-np.inf)).astype(np.float64)]) + np.asarray(origin)
    cfg = gpu.lib.default_config(map_h=H, map_w=W, origin_x=origin[0], origin_y=origin[1], resolution=res)
    got = gpu.sim.debug_xy_to_ij(cfg, to_device(gpu, xy), False).cpu().numpy()
    eq(got, mg.xy_to_ij_f64(xy, origin, res, H, W), "float64 form")
    eq(got, ref.xy_to_ij(xy, origin, res, H, W).astype(np.int32), "float64 form against the oracle")
    xy32 = xy.astype(np.float32)
    got = gpu.sim.debug_xy_to_ij(cfg, to_device(gpu, xy32.astype(np.float64)), True).cpu().numpy()
    eq(got, mg.xy_to_ij_f32(xy32, origin, res, H, W), "float32 form")
    eq(got, ref.xy_to_ij_f32(xy32, origin, res, H, W).astype(np.int32), "float32 form against the oracle")
    if H != W:                                  # the clip quirk is live: indices the map's own side would not allow
        assert (got[:, 0] >= W).any() if H > W else (got[:, 1] >= H).any()
    assert got.min() == 0 and got[:, 0].max() == H - 1 and got[:, 1].max() == W - 1


# ---- navsim_cast_static --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", abi.MARCH_RULES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_cast_static(gpu, H, W, rule):
    rng = np.random.default_rng(H)
    occ = np.concatenate([_maps(H, W, E=2), _maps(H, W, "open", 2)])
    field = ref.build_dt(occ)
    E, n = occ.shape[0], 2048
    q = np.zeros((E, n, 3), np.float32)
    for e in range(E):
        free = np.argwhere(occ[e] == 0)
        pick = free[rng.integers(0, len(free), n)]
        q[e, :, 0] = pick[:, 1] + rng.uniform(0, 1, n); q[e, :, 1] = pick[:, 0] + rng.uniform(0, 1, n)
    q[:, :, 2] = rng.uniform(-np.pi, 3 * np.pi, (E, n))
    # outside the map on all four sides (and in the corner cells), looking in and looking away
    out = [[-3, H / 2], [W + 2, H / 2], [W / 2, -1], [W / 2, H], [W, H / 2], [W / 2, H + 7.5], [-0.5, -0.5], [0, 0],
           [W - 1, H - 1], [W - 0.5, H - 0.5], [H + 3, W + 3], [max(H, W) - 1, min(H, W) - 1], [min(H, W) - 1, max(H, W) - 1]]
    for e in range(E):
        for k, p in enumerate(out):
            q[e, 2 * k, :2] = p; q[e, 2 * k + 1, :2] = p
            q[e, 2 * k, 2] = np.arctan2(H / 2 - p[1], W / 2 - p[0]); q[e, 2 * k + 1, 2] = q[e, 2 * k, 2] + np.pi
    max_range = float(H * W)
    want = ref.cast_static(field, q, max_range, rule)
    got = gpu.sim.cast_static(to_device(gpu, field), to_device(gpu, q), max_range, rule).cpu().numpy()
    eq(got, want, "cast_static %d x %d rule %d" % (H, W, rule))
    assert (want[2:] == max_range).mean() > 0.01, "no ray left the open maps"
    assert (want[:2, 2 * len(out):] < max_range).all(), "a ray left a closed map"


# ---- the fused step and navsim_reset_obs ---------------------------------------------------------------------------------------
def _device_run(gpu, cfg, occ, world, form=NO_RECTS, steps=STEPS, seed=5, v_scale=1.0):
    cfg = cfg.copy()
    arrays = device_map_arrays(gpu, cfg, occ, world, form != NO_RECTS)
    if form == RECTS_LDS:
        assert cfg.closed_maps == 1, "the LDS form marches without a bounds test: closed maps only"
    g = gpu.sim.NavSim(cfg, arrays)
    assert ("rect_table" in g.t) == (form in (RECTS_GLOBAL, RECTS_LDS))
    cmd = None
    if cfg.ped_model == abi.PED_EXTERNAL:
        def cmd(t, rng):
            g.set_ped_cmd(np.stack([rng.uniform(0, 0.6, (cfg.n_envs, cfg.max_peds)),
                                    rng.uniform(-0.6, 0.6, (cfg.n_envs, cfg.max_peds))], axis=2))
    names = [k for k in mg.STATE if k in g.t]

    def step(act):
        obs, out = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        return obs.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}
    rec = mg.rollout(lambda: g.reset_obs().cpu().numpy(), step, lambda: g.numpy_state(*names), cfg.n_envs, steps, seed, v_scale, cmd)
    return rec, g


def _equal_runs(dev, want, label):
    assert len(dev) == len(want)
    for t, (a, b) in enumerate(zip(dev, want)):
        eq(a["obs"], b["obs"], "%s: observation %d" % (label, t))
        if b["out"] is not None:
            for k in b["out"]:
                eq(a["out"][k], b["out"][k], "%s: %s at step %d" % (label, k, t))
        for k in mg.STATE:
            if k in b:
                eq(a[k], b[k], "%s: state %s at observation %d" % (label, k, t))


def _both(gpu, cfg, occ, world, form, label, **kw):
    """The same world through the device and the oracle, every observation, output and state array compared."""
    dev, g = _device_run(gpu, cfg, occ, world, form, **kw)
    want, r = cpu.run(cfg, world, **kw)
    _equal_runs(dev, want, label)
    return dev, g, r


def _scene(gpu, H, W, ped_model, fmt, form, block, kind="closed", n_beams=181, inside=False, seed=3, **kw):
    rect_lds = {NO_RECTS: 0, RECTS_GLOBAL: 1, RECTS_LDS: 2}[form]
    return cpu.scene(H, W, ped_model, inside=inside, kind=kind, seed=seed, n_beams=n_beams, field_format=fmt, step_block=block,
                     rect_lds=rect_lds, lidar_legs=1, **kw)


# field format and form, threads per arena, pedestrian model, beams: every format, block size and model at least once on a
# wide and on a tall map; robots and pedestrians stand beyond the leading square in every second arena
F32, U16T = abi.FIELD_F32, abi.FIELD_U16T
STEP_CASES = [
    (85, 330, F32, NO_RECTS, 64, abi.PED_NONE, 127), (330, 85, F32, NO_RECTS, 1024, abi.PED_SFM, 181),
    (330, 85, U16T, NO_RECTS, 256, abi.PED_SFM, 181), (96, 203, U16T, NO_RECTS, 512, abi.PED_NONE, 127),
    (96, 203, U16T, RECTS_GLOBAL, 512, abi.PED_EXTERNAL, 181), (330, 85, U16T, RECTS_GLOBAL, 64, abi.PED_NONE, 127),
    (203, 96, U16T, RECTS_LDS, 1024, abi.PED_SFM, 1081), (85, 330, U16T, RECTS_LDS, 256, abi.PED_NONE, 181),
    (330, 85, U16T, RECTS_LDS, 512, abi.PED_EXTERNAL, 127), (85, 330, U16T, RECTS_GLOBAL, 256, abi.PED_SFM, 181),
]


@pytest.mark.parametrize("H,W,fmt,form,block,ped_model,n_beams", STEP_CASES)
def test_step_on_closed_maps(gpu, H, W, fmt, form, block, ped_model, n_beams):
    origin = ORIGINS[(H + block) % 3]
    cfg, occ, world = _scene(gpu, H, W, ped_model, fmt, form, block, n_beams=n_beams)
    cfg, world = mg.translated_twin(cfg, world, origin)
    cells = mg.raw_cells(world["spawn_pose"], cfg, True)
    assert (cells.max(axis=-1) >= min(H, W)).any(), "no spawn beyond the leading square"
    dev, g, r = _both(gpu, cfg, occ, world, form, "%d x %d %s" % (H, W, form))
    assert g.cfg.closed_maps == (0 if form == NO_RECTS else 1)
    crashes, successes, restarts = mg.census(dev)
    assert crashes > 0 and restarts > 0
    if ped_model != abi.PED_NONE:
        eq(g.ped_scans().cpu().numpy(), r.ped_scans(), "pedestrian scans")


@pytest.mark.parametrize("H,W,fmt,form,block,ped_model", [
    (85, 330, F32, NO_RECTS, 256, abi.PED_SFM), (330, 85, U16T, NO_RECTS, 512, abi.PED_NONE),
    (96, 203, U16T, RECTS_GLOBAL, 1024, abi.PED_EXTERNAL), (203, 96, U16T, RECTS_GLOBAL, 64, abi.PED_SFM),
    (330, 85, F32, NO_RECTS, 64, abi.PED_NONE), (85, 330, U16T, RECTS_GLOBAL, 256, abi.PED_NONE)])
def test_step_on_open_maps(gpu, H, W, fmt, form, block, ped_model):
    """Gaps in the ring on all four sides: the forms of the march that test the bounds (cfg.closed_maps comes out 0, so a
    record table is read from global memory)."""
    cfg, occ, world = _scene(gpu, H, W, ped_model, fmt, form, block, kind="open")
    cfg, world = mg.translated_twin(cfg, world, ORIGINS[(W + block) % 3])
    dev, g, r = _both(gpu, cfg, occ, world, form, "open %d x %d %s" % (H, W, form))
    assert g.cfg.closed_maps == 0
    B = cfg.n_scan_stack * cfg.n_beams
    assert sum(int((d["obs"][:, :B] == np.float32(cfg.range_max)).sum()) for d in dev) > 0, "no ray left the map"
    if ped_model != abi.PED_NONE:
        eq(g.ped_scans().cpu().numpy(), r.ped_scans(), "pedestrian scans")


@pytest.mark.parametrize("H,W", [(85, 330), (330, 85)])
@pytest.mark.parametrize("fmt,form", [(F32, NO_RECTS), (U16T, NO_RECTS), (U16T, RECTS_GLOBAL)])
def test_first_observation_of_robots_outside_the_map(gpu, H, W, fmt, form):
    """Robots standing outside an open map on each of its four sides, and in the middle of it.  xy_to_ij clips the x index
    against map_h and the y index against map_w, so on a non-square map the origin cell of such a robot can lie beyond the
    map's own side: calc_range's first sample leaves the map and every beam reads range_max.  (On a square map the clip
    always lands in the map; the step's first probe relied on that and read the field at that cell.)"""
    places = [(W // 2, H // 2), (-4, H // 2), (W + 3, H // 2), (W // 2, -4), (W // 2, H + 3), (max(H, W) - 2, max(H, W) - 2),
              (min(H, W) + 40, min(H, W) // 2), (min(H, W) // 2, min(H, W) + 40)]
    E = len(places) + 1                                   # (the last arena stays inside: nothing is read behind the last field)
    cfg = cpu.config(H, W, E=E, n_beams=127, field_format=fmt, step_block=64, rect_lds=1 if form == RECTS_GLOBAL else 0,
                     auto_reset=0, n_spawn=1)
    occ = mg.make_maps(E, H, W, 4, "open")
    world = mg.make_world(cfg, occ, ref.build_dt(occ), keti_thresholds(cfg), 4, inside=False)
    for e, cell in enumerate(places):
        world["robot_pose"][e, :2] = mg.cell_xy(cfg, np.array(cell))
    dev, g = _device_run(gpu, cfg, occ, world, form, steps=0)
    want, r = cpu.run(cfg, world, steps=0)
    _equal_runs(dev, want, "robots outside a %d x %d map" % (H, W))
    rows = want[0]["obs"][:, :cfg.n_beams]
    ij = ref.xy_to_ij_f32(world["robot_pose"][:, :2].astype(np.float32), (0, 0), cfg.resolution, H, W)
    beyond = (ij[:, 0] >= W) | (ij[:, 1] >= H)
    assert beyond.sum() >= 2 and (rows[beyond] == np.float32(cfg.range_max)).all()
    assert not (rows[~beyond] == np.float32(cfg.range_max)).all(axis=1).any()


# ---- the three identities on the device's own outputs --------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,fmt,form,block,ped_model", [
    (85, 330, U16T, RECTS_LDS, 256, abi.PED_SFM), (330, 85, F32, NO_RECTS, 512, abi.PED_EXTERNAL),
    (96, 203, U16T, RECTS_GLOBAL, 1024, abi.PED_NONE), (203, 96, U16T, NO_RECTS, 64, abi.PED_SFM)])
def test_embedding_identity_on_the_device(gpu, H, W, fmt, form, block, ped_model):
    cfg, occ, world = _scene(gpu, H, W, ped_model, fmt, form, block, inside=True)
    big = mg.embed(occ)
    cfg_e, world_e = mg.embedded_twin(cfg, world, ref.build_dt(big))
    dev, g, _ = _both(gpu, cfg, occ, world, form, "%d x %d" % (H, W))
    dev_e, g_e, _ = _both(gpu, cfg_e, big, world_e, form, "embedded %d x %d" % (H, W))
    covered = mg.check_embedding(cfg, dev, dev_e, "device, %d x %d %s" % (H, W, form))
    assert covered == cfg.n_envs * (STEPS + 1)


@pytest.mark.parametrize("H,W,fmt,form,block", [
    (85, 330, U16T, RECTS_LDS, 512), (330, 85, U16T, NO_RECTS, 64), (96, 203, F32, NO_RECTS, 256),
    (120, 120, U16T, RECTS_GLOBAL, 1024)])
def test_scaling_identity_on_the_device(gpu, H, W, fmt, form, block):
    """Resolution 0.1 and 0.025 beside 0.05: each run equals the oracle's, and the device's own outputs scale exactly."""
    cfg, occ, world = _scene(gpu, H, W, abi.PED_NONE, fmt, form, block, min_turning_radius=0.3)
    dev, _, _ = _both(gpu, cfg, occ, world, form, "%d x %d at 0.05" % (H, W))
    for k in (2.0, 0.5):
        cfg_k, world_k = mg.scaled_twin(cfg, world, k)
        assert cfg_k.resolution == 0.05 * k
        dev_k, _, _ = _both(gpu, cfg_k, occ, world_k, form, "%d x %d at %g" % (H, W, cfg_k.resolution), v_scale=k)
        covered = mg.check_scaling(cfg, dev, dev_k, k, "device, %d x %d %s" % (H, W, form))
        assert covered == cfg.n_envs * (STEPS + 1)


@pytest.mark.parametrize("H,W,fmt,form,block", [
    (85, 330, U16T, RECTS_GLOBAL, 64), (330, 85, U16T, RECTS_LDS, 1024), (203, 96, F32, NO_RECTS, 512),
    (120, 120, U16T, NO_RECTS, 256)])
def test_translation_identity_on_the_device(gpu, H, W, fmt, form, block):
    cfg, occ, world = _scene(gpu, H, W, abi.PED_NONE, fmt, form, block)
    dev, _, _ = _both(gpu, cfg, occ, world, form, "%d x %d at the origin" % (H, W))
    for origin in cpu.ORIGINS:
        cfg_t, world_t = mg.translated_twin(cfg, world, origin)
        dev_t, _, _ = _both(gpu, cfg_t, occ, world_t, form, "%d x %d at %s" % (H, W, origin))
        covered, _ = mg.check_translation(cfg, dev, cfg_t, dev_t, "device, %d x %d %s" % (H, W, form))
        assert covered == cfg.n_envs * (STEPS + 1)


def test_translation_identity_with_pedestrians_on_the_device(gpu):
    """tests/test_map_geometry.py's pedestrian case and bound on the device's own state."""
    cfg, occ, world = _scene(gpu, 96, 203, abi.PED_SFM, U16T, RECTS_LDS, 256, inside=True, seed=cpu.PED_TRANSLATION_SEED)
    dev, _, _ = _both(gpu, cfg, occ, world, RECTS_LDS, "pedestrians at the origin")
    for origin in cpu.ORIGINS:
        cfg_t, world_t = mg.translated_twin(cfg, world, origin)
        dev_t, _, _ = _both(gpu, cfg_t, occ, world_t, RECTS_LDS, "pedestrians at %s" % (origin,))
        worst = cpu.ped_shift_deviation(cfg, dev, cfg_t, dev_t, "device, pedestrians, origin %s" % (origin,))
        for k, bound in cpu.PED_SHIFT_BOUND.items():
            assert worst[k] <= bound, (k, worst[k], bound)


# ---- pedestrian and planning calls -----------------------------------------------------------------------------------------------
# (origin, resolution / 0.05): a shifted origin alone, then both unrepresentable origins with the coarser and the finer grid
GEOMETRIES = [((-16.0, 32.0), 1.0), ((-7.3, 12.9), 2.0), ((-7.3, 12.9), 0.5), ((0.0, 0.0), 2.0)]


def _scaled(params, k, keys):
    return {name: (tuple(x * k for x in v) if isinstance(v, tuple) else v * k) if name in keys else v for name, v in params.items()}


def ped_world(H, W, origin, k, N=8, seed=9, **kw):
    """A world of tests/map_geometry_scenes.py with N walking pedestrians, beyond the leading square in every second arena."""
    cfg, occ, world = cpu.scene(H, W, abi.PED_EXTERNAL, inside=False, seed=seed, N=N, E=5, **kw)
    cfg, world = mg.geometry_twin(cfg, world, origin, k)
    world["ped_wp_head"] = np.zeros((cfg.n_envs, N), np.int32)
    return cfg, occ, world


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_ped_observe(gpu, H, W, origin, k, fmt):
    dev = ped_observe_call
    cfg, occ, w = ped_world(H, W, origin, k, field_format=fmt)
    st, keep = dev.device_state(gpu, cfg, occ, w)
    seen = hidden = 0
    for p in (dict(sensor_range=6.0 * k, ped_radius=0.3 * k, max_obs=4, rays=3), dict(sensor_range=3.0 * k, ped_radius=0.3 * k, max_obs=8, rays=1, fov=0)):
        want = dev.answer(cfg, w["field"], w, p)
        dev.same(dev.call(gpu, cfg, st, p), want, "%d x %d origin %s resolution %g %s" % (H, W, origin, cfg.resolution, p))
        seen += int(want["count"].sum()); hidden += int((want["visible"] == 0).sum())
    assert seen > 0 and hidden > 0


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_ped_scans(gpu, H, W, origin, k):
    cfg, occ, w = ped_world(H, W, origin, k, field_format=U16T, rect_lds=1)
    del w["ped_wp_head"]
    dev, g = _device_run(gpu, cfg, occ, w, RECTS_GLOBAL, steps=2)
    want, r = cpu.run(cfg, w, steps=2)
    _equal_runs(dev, want, "two steps")
    scans = r.ped_scans()
    eq(g.ped_scans().cpu().numpy(), scans, "pedestrian scans %d x %d origin %s resolution %g" % (H, W, origin, cfg.resolution))
    assert (scans < np.float32(cfg.ped_range_max)).any() and (scans > 0).any()


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85), (120, 120)])
def test_ped_orca_walls(gpu, H, W, origin, k):
    """max_obst_rects = 8, time_horizon_obst = 2 on the rectangles the device listed for the map."""
    spec = ped_orca_spec
    cfg, occ, w = ped_world(H, W, origin, k, field_format=U16T, rect_lds=1)
    arrays = device_map_arrays(gpu, cfg, occ, {n: v for n, v in w.items() if n != "ped_wp_head"}, True)
    g = gpu.sim.NavSim(cfg, arrays)
    g.reset_obs()
    rects = wspec.decode_rows(g.t["rect_index"].cpu().numpy())
    listed = np.zeros(occ.shape, np.uint8)
    for e in range(cfg.n_envs):
        for x0, y0, x1, y1 in (r for r in rects[e] if r.any()):
            assert 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H
            listed[e, y0:y1 + 1, x0:x1 + 1] = 1
    assert not (listed & ~occ & 1).any(), "a listed rectangle covers a free cell"
    a = dict(w, ped_cmd=np.full(w["ped_cmd"].shape, -7.25))
    g.t["ped_cmd"].fill_(-7.25)
    p = spec.params(cfg, time_horizon_obst=2.0, ped_radius=0.3 * k, robot_radius=0.9 * k, neighbor_dist=10.0 * k)
    dropped = gpu.torch.full((cfg.n_envs, cfg.max_peds), -1, dtype=gpu.torch.int32, device=gpu.dev)
    got = g.ped_orca_walls({n: p[n] for n in spec.KEYS}, 8, dropped).cpu().numpy()
    want_cmd, want_head, want_dropped, census = wspec.ped_orca_walls(cfg, a, p, rects, 8)
    what = "%d x %d origin %s resolution %g" % (H, W, origin, cfg.resolution)
    eq(got, want_cmd, "ped_cmd " + what)
    eq(g.t["ped_wp_head"].cpu().numpy(), want_head, "ped_wp_head " + what)
    eq(dropped.cpu().numpy(), want_dropped, "dropped " + what)
    print(what, dict(census))
    assert census["0 edges in range"] < cfg.n_envs * cfg.max_peds, "no pedestrian has a wall in range"


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_goal_path(gpu, origin, k, fmt):
    spec, dev = goal_path_spec, goal_path_call
    E, size, seed = 12, 100, 5301
    occ, w = spec.random_world(E, size, seed)
    cfg, w = mg.geometry_twin(spec.config(E, size, field_format=fmt), w, origin, k)
    st, keep = dev.device_state(gpu, cfg, occ, w)
    fields = ref.build_dt(occ)
    for p in ({}, dict(hard_clearance=0.2, clearance=1.5, band_cost=16, lookahead=6.0)):
        p = _scaled(dict(spec.DEFAULT, **p), k, ("hard_clearance", "clearance", "lookahead"))
        want = dev.answer(cfg, fields, w, p)
        assert (want["status"] & spec.OK).sum() >= 2 and ((want["dist"] != spec.INF) & (want["dist"] > 0)).sum() > 200
        dev.same(dev.call(gpu, cfg, st, p), want, "origin %s resolution %g %s" % (origin, cfg.resolution, p))


@pytest.mark.parametrize("origin,k", GEOMETRIES)
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_dwa(gpu, origin, k, fmt):
    spec, dev = dwa_spec, dwa_call
    E, N, size, seed = spec.BASE
    occ, w = spec.random_world(E, N, size, seed)
    cfg = spec.config(E, size, N, field_format=fmt)
    cfg.linvel_lo, cfg.linvel_hi = cfg.linvel_lo * k, cfg.linvel_hi * k
    cfg, w = mg.geometry_twin(cfg, w, origin, k)
    p = _scaled(dict(spec.DEFAULT, **spec.BASE_PARAMS), k, ("acc_lin", "body_radius", "body_offset", "ped_radius", "margin", "clearance_cap"))
    st, keep = dev.device_state(gpu, cfg, occ, w)
    want = spec.plan(cfg, ref.build_dt(occ), w, p)
    assert (want["first_hit"] != 0).any() and (want["first_hit"] == 0).any()
    dev.same(dev.call(gpu, cfg, st, p), want, "origin %s resolution %g" % (origin, cfg.resolution))


@pytest.mark.parametrize("H,W", [(330, 85), (85, 330)])
def test_replan_inside_the_step_on_a_costmap_that_is_not_square(gpu, H, W):
    """navsim_step_replan (one launch: the arenas with a waiting pedestrian re-plan first) on 66 x 17 and 17 x 66 costmaps at a
    shifted origin: the oracle's serial step, replan, step, ... bit for bit, and navsim_replan on its own behind it."""
    E, N, cap = 6, 4, 64
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, max_peds=N, ped_model=abi.PED_SFM, n_spawn=4, auto_reset=0, seed=29,
                                 field_format=U16T, ped_min_goal_dist=1.5, origin_x=-7.3, origin_y=12.9)
    gpu.world.lidar_full_circle(cfg, 127)
    occ = mg.make_maps(E, H, W, 29, n_boxes=1)
    arrays = device_world(gpu, cfg, occ, N, plan_paths=True, v_pref_range=(0.5, 0.6), min_goal_dist=1.0, max_goal_dist=3.0,
                          robot_clearance=0.6)
    assert tuple(arrays["costmap"].shape) == (E, H // 5, W // 5)
    eq(arrays["costmap"].cpu().numpy(), ref.costmap(occ), "costmap")
    g = gpu.sim.NavSim(cfg, arrays)
    g.replan_in_step = True
    r = ref.RefSim(cfg, host_arrays(arrays, occ))
    eq(g.reset_obs().cpu().numpy(), r.reset_obs(), "reset obs")
    assert (r.a["ped_n_waypoints"] > 1).any(), "no pedestrian started with a planned path"
    rng = np.random.default_rng(3)
    for t in range(60):
        act = np.stack([rng.uniform(0.0, 0.2, E), rng.uniform(-0.64, 0.64, E)], axis=1)
        if t > 0:
            r.replan(cap)
        ro, rout = r.step(act)
        go, gout = g.step_overlapped(gpu.torch.from_numpy(act).to(gpu.dev), cap)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        for k in rout:
            eq(gout[k].cpu().numpy(), rout[k], "%s at step %d" % (k, t))
    g.replan(cap); r.replan(cap)
    state_equal(g, r, "at the end", live_waypoints_only=True)
    assert g.counters() == r.counters() and r.counters()["replan_served"] >= 1, r.counters()


def test_regen_at_a_shifted_origin_and_resolution(gpu):
    """navsim_regen on square maps of 0.1 m cells whose origin is (-7.3, 12.9): new maps, tables, pedestrians and first
    observations equal the oracle's."""
    E, size = 8, 120
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=3, ped_model=abi.PED_SFM, n_spawn=4, auto_reset=1, seed=29,
                                 field_format=U16T, regen_cap=4, min_goal_dist=2.0, max_goal_dist=6.0, spawn_clearance=0.8,
                                 ped_min_robot_dist=1.5, ped_min_goal_dist=3.0, resolution=0.1, origin_x=-7.3, origin_y=12.9)
    gpu.world.lidar_full_circle(cfg, 90)
    occ = gpu.world.make_maps(E, size, 29)
    regenerated = 0
    for t, go, gout, ro, rout, g, r in rollout_pair(gpu, cfg, occ, n_peds=3, steps=30, seed=3, min_goal_dist=2.0, max_goal_dist=6.0,
                                                     robot_clearance=0.8):
        eq(go, ro, "obs at step %d" % t)
        regenerated += min(int(rout["done"].sum()), 4)
        eq(g.regen().cpu().numpy(), r.regen(), "obs after regen at step %d" % t)
    state_equal(g, r, "at the end")
    assert regenerated >= 2
    lo, hi = np.array([-7.3, 12.9]), np.array([-7.3, 12.9]) + size * 0.1
    assert ((r.a["spawn_pose"][..., :2] > lo) & (r.a["spawn_pose"][..., :2] < hi)).all(), "a spawn outside the shifted map"


def test_regen_refuses_a_map_that_is_not_square(gpu):
    """navsim_regen draws square maps: NAVSIM_E_UNSUPPORTED for map_h != map_w, and nothing is written."""
    cfg, occ, world = _scene(gpu, 85, 330, abi.PED_SFM, U16T, RECTS_GLOBAL, 256)
    dev, g = _device_run(gpu, cfg, occ, world, RECTS_GLOBAL, steps=1)
    torch = gpu.torch
    g.out["done"].fill_(1)
    watched = list(g.t.values()) + g.obs_buf
    before = [t.clone() for t in watched]
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=gpu.dev)
    io = g._io_copy(obs=g.obs)
    rc = g.lib.navsim_regen(C.byref(g.cfg), C.byref(g.st), C.byref(io), C.c_void_p(ws.data_ptr()), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == abi.E_UNSUPPORTED
    assert all(torch.equal(a, b) for a, b in zip(watched, before)) and not ws.any()
