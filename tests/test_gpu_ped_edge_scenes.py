"""GPU: the device against the CPU oracle, bit for bit, on the pedestrian edge scenes of tests/ped_edge_scenes.py (which
tests/test_ped_edge_scenes.py holds against independent float64 references): the first observation, two steps -- observation,
every output, the state -- and the pedestrian scans.  The near scenes crash, so the revert and the second scan with its own
prims_prepare are inside.

Forms: 64, 256, 512 and 1024 threads per arena; the float32 field, the packed field, the packed field with rect records read
from global memory and from LDS; pedestrians inside the step's launch (ped_split 0) and ahead of it (2); the three march rules
once each at step_block = 0.  The reference lidar and both social-force worlds (max_peds 64 and 11) run every block size with
every field form resp. pedestrian form; every other lidar runs one form, taken in turn.  The oracle runs once per world and
march rule, whatever the device's form.  Nothing here faults by design: every pose is finite, and poses outside the map are
ones xy_to_ij clips, which the oracle has run on the CPU first."""
import functools

import numpy as np
import pytest

import map_geometry_scenes as mg
import ped_edge_runs as cpu
import ped_edge_scenes as ps
from gpu_support import gpu, device_map_arrays, eq, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

BLOCKS = (64, 256, 512, 1024)
FIELDS = ("f32", "u16t", "rects", "rects_lds")
FORMS = [(b, f) for b in BLOCKS for f in FIELDS]
STATE = mg.STATE + ("ped_goal", "n_peds", "ped_due")


def _device_arrays(gpu, cfg, occ, world, field):
    """The world's arrays with the field (and the rect records) the device builds from occ; sets the configuration's
    field_format, rect_lds and closed_maps."""
    cfg.field_format = abi.FIELD_F32 if field == "f32" else abi.FIELD_U16T
    cfg.rect_lds = {"f32": 0, "u16t": 0, "rects": 1, "rects_lds": 2}[field]
    rects = field in ("rects", "rects_lds")
    a = device_map_arrays(gpu, cfg, occ, world, rects)
    assert not rects or cfg.closed_maps == 1
    return a


def _device_run(gpu, cfg, occ, world, action, steps, block, field, split, march_rule=None):
    cfg = cfg.copy()
    cfg.step_block, cfg.ped_split = block, split
    if march_rule is not None:
        cfg.march_rule = march_rule
    g = gpu.sim.NavSim(cfg, _device_arrays(gpu, cfg, occ, world, field))
    assert ("rect_table" in g.t) == (field in ("rects", "rects_lds"))
    names = [k for k in STATE if k in g.t or k == "ped_due"]
    rec = [dict(obs=g.reset_obs().cpu().numpy(), out=None, state=g.numpy_state(*names))]
    act = to_device(gpu, np.tile(np.asarray(action, np.float64), (cfg.n_envs, 1)))
    for _ in range(steps):
        obs, out = g.step(act)
        rec.append(dict(obs=obs.cpu().numpy(), out={k: v.cpu().numpy() for k, v in out.items()}, state=g.numpy_state(*names)))
    scans = g.ped_scans().cpu().numpy() if cfg.ped_model != abi.PED_NONE else None
    return rec, scans


def _equal(dev, want, names, label):
    assert len(dev) == len(want)
    for t, (a, b) in enumerate(zip(dev, want)):
        for e in np.flatnonzero((a["obs"] != b["obs"]).any(axis=1))[:1]:           # name the scene of the first row that differs
            eq(a["obs"][e], b["obs"][e], "%s: observation %d of scene '%s'" % (label, t, names[e]))
        if b["out"] is not None:
            assert set(a["out"]) == set(b["out"])
            for k in b["out"]:
                eq(a["out"][k], b["out"][k], "%s: %s at step %d" % (label, k, t))
        compared = 0
        for k in STATE:
            if k in b["state"] and k in a["state"]:
                eq(a["state"][k], b["state"][k], "%s: state %s at observation %d" % (label, k, t))
                compared += 1
        assert compared >= 12, compared


@functools.lru_cache(maxsize=None)
def _oracle_lidar(name, march_rule=None):
    cfg, occ, world, names = cpu.lidar_world(name)
    rec, r = cpu.run(cfg, world, (0.0, 0.0), cpu.STEPS, march_rule)
    return rec, r.ped_scans()


@functools.lru_cache(maxsize=None)
def _oracle_sfm(max_peds, march_rule=None):
    cfg, occ, world, scenes = cpu.sfm_world(max_peds)
    rec, r = cpu.run(cfg, world, ps.SFM_ACTION, cpu.STEPS, march_rule)
    return rec, r.ped_scans()


def _lidar_case(gpu, name, block, field, split, march_rule=None):
    cfg, occ, world, names = cpu.lidar_world(name)
    want, want_scans = _oracle_lidar(name, march_rule)
    dev, scans = _device_run(gpu, cfg, occ, world, (0.0, 0.0), cpu.STEPS, block, field, split, march_rule)
    label = "%s, %d threads, %s, ped_split %d" % (name, block, field, split)
    _equal(dev, want, names, label)
    for e in np.flatnonzero((scans != want_scans).any(axis=(1, 2)))[:1]:
        eq(scans[e], want_scans[e], "%s: pedestrian scans of scene '%s'" % (label, names[e]))
    B = cfg.n_beams
    assert sum(int(x["out"]["is_crash"].sum()) for x in want[1:]) > 0, "the near scenes crash"
    assert (want[0]["obs"][:, -7 - B:-7] < np.float32(cfg.range_max)).any() and (want_scans < np.float32(cfg.ped_range_max)).any()


@pytest.mark.parametrize("block,field", FORMS)
def test_reference_lidar_in_every_form(gpu, block, field):
    _lidar_case(gpu, "reference_1081", block, field, 2 if (BLOCKS.index(block) + FIELDS.index(field)) % 2 else 0)


OTHERS = [n for n in cpu.LIDAR_WORLDS if n != "reference_1081"]


@pytest.mark.parametrize("k,name", list(enumerate(OTHERS)), ids=OTHERS)
def test_every_lidar(gpu, k, name):
    block, field = FORMS[(5 * k + 3) % len(FORMS)]            # (5 and 16 are coprime: the forms are taken in turn, blocks and fields mixed)
    _lidar_case(gpu, name, block, field, 2 if k % 3 == 1 else 0)


@pytest.mark.parametrize("march_rule", abi.MARCH_RULES)
def test_march_rules_on_the_lidar_scenes(gpu, march_rule):
    _lidar_case(gpu, "circle_4000" if march_rule == abi.MARCH_F32_FMA else "reference_1081", 0, FIELDS[march_rule % len(FIELDS)], 0, march_rule)


def _sfm_case(gpu, max_peds, block, field, split, march_rule=None):
    cfg, occ, world, scenes = cpu.sfm_world(max_peds)
    names = [s["name"] for s in scenes]
    want, want_scans = _oracle_sfm(max_peds, march_rule)
    dev, scans = _device_run(gpu, cfg, occ, world, ps.SFM_ACTION, cpu.STEPS, block, field, split, march_rule)
    label = "social force, max_peds %d, %d threads, %s, ped_split %d" % (max_peds, block, field, split)
    _equal(dev, want, names, label)
    eq(scans, want_scans, label + ": pedestrian scans")
    moved = np.abs(want[-1]["state"]["ped_pose"] - world["ped_pose"]).max(axis=(1, 2)) > 0
    assert moved.sum() >= len(scenes) - 1                   # (every arena but the one with n_peds = 0)


@pytest.mark.parametrize("split", [0, 2])
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("max_peds", [64, 11])
def test_social_force_scenes(gpu, max_peds, block, split):
    _sfm_case(gpu, max_peds, block, FIELDS[(BLOCKS.index(block) + split // 2 + (max_peds == 11)) % len(FIELDS)], split)


@pytest.mark.parametrize("march_rule", abi.MARCH_RULES)
def test_march_rules_on_the_social_force_scenes(gpu, march_rule):
    _sfm_case(gpu, 11 if march_rule == abi.MARCH_F64 else 64, 0, FIELDS[(march_rule + 1) % len(FIELDS)], 2 * (march_rule % 2), march_rule)


@pytest.mark.parametrize("name", list(ps.WIDE_LIDARS))
@pytest.mark.parametrize("block,field", [(256, "rects_lds"), (1024, "f32")])
def test_a_lidar_above_one_turn_without_pedestrians(gpu, name, block, field):
    """include/navsim.h angle_last: with pedestrians such a lidar is refused (tests/test_gpu_step_refusals.py); without them
    nothing is culled and it is served -- robots at rest and driving, walls in range."""
    lidar = ps.WIDE_LIDARS[name]
    scenes = ps.lidar_scenes(lidar, crowd=False)
    cfg = cpu.config(lidar, len(scenes), abi.PED_NONE, range_max=25.0)
    world = ps.lidar_world(cfg, scenes)
    occ = cpu.with_map(cfg, world)
    assert cfg.angle_last - cfg.angle_min > 2 * np.pi
    want, _ = cpu.run(cfg, world, (0.3, 0.2))
    dev, _ = _device_run(gpu, cfg, occ, world, (0.3, 0.2), cpu.STEPS, block, field, 0)
    _equal(dev, want, [s["name"] for s in scenes], "%s without pedestrians, %d threads, %s" % (name, block, field))
    rows = want[-1]["obs"][:, :cfg.n_beams]
    assert (rows < np.float32(25.0)).all() and len(np.unique(rows)) > 100, "the walls are in range"
