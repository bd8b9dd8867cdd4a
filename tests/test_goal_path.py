"""CPU: the goal path (include/navsim.h navsim_goal_path) -- the specification of tests/goal_path_spec.py pinned before any GPU
run (Dijkstra against plain relaxation, hand-made grids with known answers, the properties of the walk), the entry's place in the
C ABI, its argument refusals, the keywords on NavGymEnv, and the population of the random worlds the device test uses.  The
device against that specification is tests/test_gpu_goal_path.py."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import goal_path_spec as spec
import ref
from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = spec.INF


# ---- the field ----------------------------------------------------------------------------------------------------------------
def test_dijkstra_equals_relaxation_to_the_fixed_point():
    """200 random 12 x 12 class arrays (walls, band cells of multiplier 1 .. 16, clear cells), the goal anywhere -- also on a
    wall: two algorithms, one field."""
    reached = walls_as_goal = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        band = int(rng.integers(1, 17))
        kind = rng.choice(3, size=(12, 12), p=(0.3, 0.3, 0.4))
        m = np.where(kind == 0, 0, np.where(kind == 1, band, 1)).astype(np.uint8)
        goal = (int(rng.integers(12)), int(rng.integers(12)))
        a = spec.field_from_classes(m, goal)
        b, sweeps = spec.relax_from_classes(m, goal)
        assert (a == b).all(), seed
        assert a[goal[1], goal[0]] == 0 and (a[(m == 0) & (a != 0)] == INF).all()
        reached += int(((a != INF) & (a != 0)).sum())
        walls_as_goal += int(m[goal[1], goal[0]] == 0)
    assert reached > 2000 and walls_as_goal > 20


def test_empty_room_is_the_chamfer_metric():
    m = np.ones((15, 17), np.uint8)
    g = (5, 9)
    d = spec.field_from_classes(m, g)
    jc, ic = np.mgrid[0:15, 0:17]
    di, dj = np.abs(ic - g[0]), np.abs(jc - g[1])
    assert (d == 7 * np.minimum(di, dj) + 5 * np.abs(di - dj)).all()


def test_wall_with_one_gap():
    """Every path to the far side passes the gap: dist = dist[gap] + the chamfer distance to the gap, at least."""
    m = np.ones((15, 15), np.uint8)
    m[:, 7] = 0
    m[11, 7] = 1
    g = (2, 3)
    d = spec.field_from_classes(m, g).astype(np.int64)
    gap = d[11, 7]
    assert gap == 7 * 4 + 5 * 4 + 5                                   # to (6, 11) beside the gap, then straight in: no corner is cut
    jc, ic = np.mgrid[0:15, 8:15]
    di, dj = np.abs(ic - 7), np.abs(jc - 11)
    # beyond the gap the first hop cannot be diagonal (the wall cells beside the gap are corners): at least one straight hop
    assert (d[:, 8:] >= gap + 7 * np.minimum(di, dj) + 5 * np.abs(di - dj)).all()
    assert d[11, 8] == gap + 5 and d[10, 8] == gap + 10 and d[12, 9] == gap + 12
    assert (d[:, 7][np.arange(15) != 11] == INF).all()


def test_thin_diagonal_wall_is_watertight():
    """A one-cell-thick diagonal wall of MAP cells at hard_clearance = 3 resolution: every nav cell whose block the wall touches is
    impassable, and a staircase of such blocks cannot be crossed without cutting a corner -- the far side stays 0xFFFF."""
    size = 100
    occ = np.zeros((size, size), np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    for t in range(size):
        occ[t, size - 1 - t] = 1                                       # the anti-diagonal, 8-connected only
    cfg = spec.config(1, size)
    p = dict(hard_clearance=3 * cfg.resolution, clearance=3 * cfg.resolution)
    d = ref.build_dt(occ)[0]
    m = spec.classes(cfg, d, p)
    touched = occ.reshape(20, 5, 20, 5).max(axis=(1, 3)) != 0
    assert (m[touched] == 0).all()                                     # the sample is at most 2.83 < 3 cells from the wall
    f = spec.field_from_classes(m, spec.nav_cell(cfg, 1.0, 1.0))
    jc, ic = np.mgrid[0:20, 0:20]
    assert (f[(ic + jc > 19) & (m != 0)] == INF).all() and ((ic + jc > 19) & (m != 0)).sum() > 100
    assert (f[(ic + jc < 19) & (m != 0)] != INF).all()


def test_band_hop_costs_band_cost_times_the_clear_one():
    m = np.ones((3, 8), np.uint8)
    m[:, 3:6] = 4
    m[0, :] = m[2, :] = 0                                               # a corridor one cell wide
    d = spec.field_from_classes(m, (0, 1))
    assert d[1].tolist() == [0, 5, 10, 30, 50, 70, 75, 80]            # leaving a band cell costs 4 x 5
    d = spec.field_from_classes(m, (7, 1))
    assert d[1].tolist() == [80, 75, 70, 65, 45, 25, 5, 0]            # ... whichever way the path runs


def test_saturating_snake():
    m, goal, order = spec.snake_classes()
    d = spec.field_from_classes(m, goal)
    want = np.minimum(80 * np.arange(len(order)), INF)
    got = np.array([d[jc, ic] for ic, jc in order])
    assert (got == want).all() and (want == INF).sum() > 100 and want[819] == 65520 and want[820] == INF
    b, _ = spec.relax_from_classes(m[:12, :], goal)                     # (the relaxation agrees on a piece of it)
    assert (b == spec.field_from_classes(m[:12, :], goal)).all()


# ---- the walk -----------------------------------------------------------------------------------------------------------------
def _world(E, size, seed):
    occ, w = spec.random_world(E, size, seed)
    cfg = spec.config(E, size)
    return cfg, ref.build_dt(occ), w


def test_walk_properties_and_population_of_the_random_worlds():
    """On the random worlds of the device test: the walk never enters an impassable cell, never cuts a corner, dist falls at every
    hop, and walked <= lookahead_cells.  And the conditions on the test's own inputs: at least half of the arenas OK, at least one
    walk that ends on the goal cell, at least one robot off the field, at least one path across the band."""
    ok = reached = off = band = total = 0
    for E, size, seed in spec.RANDOM_WORLDS:
        cfg, fields, w = _world(E, size, seed)
        o = spec.goal_path(cfg, fields, w["robot_pose"], w["robot_goal"], {}, detail=True)
        L = spec.lookahead_cells(cfg, {})
        for e in range(E):
            total += 1
            m, dist, cells = o["classes"][e], o["dist"][e].astype(np.int64), o["cells"][e]
            g = spec.nav_cell(cfg, *w["robot_goal"][e])
            st = int(o["status"][e])
            if st == spec.OFF_FIELD:
                off += 1
                assert len(cells) == 1 and dist[cells[0][1], cells[0][0]] == INF
                continue
            assert st & spec.OK
            ok += 1
            reached += int(bool(st & spec.REACHED))
            walked = 0
            for (ai, aj), (bi, bj) in zip(cells, cells[1:]):
                assert max(abs(ai - bi), abs(aj - bj)) == 1
                assert m[bj, bi] != 0 or (bi, bj) == g
                if ai != bi and aj != bj:
                    assert (m[aj, bi] != 0 or (bi, aj) == g) and (m[bj, ai] != 0 or (ai, bj) == g)
                assert dist[bj, bi] < dist[aj, ai]
                walked += 5 if (ai == bi or aj == bj) else 7
            assert walked <= L and bool(st & spec.REACHED) == (cells[-1] == g)
            band += int(any(m[j, i] > 1 for i, j in cells))
    print(dict(total=total, ok=ok, reached=reached, off=off, band=band))
    assert 2 * ok >= total and reached >= 1 and off >= 1 and band >= 1


def test_inside_the_lookahead_the_distance_is_the_straight_line():
    cfg = spec.config(1, 100)
    d = ref.build_dt(spec.scale5(spec.room(20)))[0]
    m = spec.classes(cfg, d, {})
    goal = (2.31, 2.77)
    f = spec.field_from_classes(m, spec.nav_cell(cfg, *goal))
    for pose in ((1.52, 2.13, 0.7), (2.9, 3.4, -2.0), (2.31, 2.77, 1.0), (2.3, 2.8, 0.0)):
        dist, sub, status = spec.query(cfg, m, f, pose, goal, {})
        dx, dy = np.float64(goal[0]) - np.float64(pose[0]), np.float64(goal[1]) - np.float64(pose[1])
        assert status == spec.OK | spec.REACHED
        assert dist.view(np.uint32) == np.float32(np.sqrt(dx * dx + dy * dy)).view(np.uint32)
        assert abs(float(np.hypot(*sub)) - float(dist)) < 1e-6
    far = (0.6, 0.6, 0.0)                                                # ~2.8 m away: beyond the 2 m look-ahead
    dist, sub, status = spec.query(cfg, m, f, far, goal, {})
    assert status == spec.OK and float(dist) > 0.99 * float(np.hypot(goal[0] - far[0], goal[1] - far[1]))   # (a diagonal hop weighs 7 < 5 sqrt 2)
    dist0, sub0, status0, cells = spec.query(cfg, m, f, far, goal, dict(lookahead=0.0), detail=True)
    assert status0 == spec.OK and len(cells) == 1                        # look-ahead 0: the sub-goal is the robot's own cell centre
    cx, cy = spec.centre(*cells[0])
    assert abs(float(sub0[0]) - (cx - far[0])) < 1e-6 and abs(float(sub0[1]) - (cy - far[1])) < 1e-6


def test_spiral_needs_the_whole_corridor():
    nav = spec.spiral()
    cfg = spec.config(1, 5 * nav.shape[0])
    m = spec.classes(cfg, ref.build_dt(spec.scale5(nav))[0], {})
    lane = int((m != 0).sum())
    assert (m[m != 0] == 3).mean() > 0.95 and lane > 500                # only the centre lane, in the band (but for the middle)
    f = spec.field_from_classes(m, (2, 2))
    far = f[m != 0].max()
    # one cell after the other at 15 a hop (no corner is cut); the lane's dead ends and its wider turns are off that path: a tenth
    assert far != INF and far >= 15 * 0.9 * lane


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()         # no structure changed its size
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert re.search(r"\bint navsim_goal_path\(", header) and re.search(r"\bsize_t navsim_goal_field_bytes\(", header)
    for name in ("navsim_goal_path", "navsim_goal_field_bytes", "navsim_debug_goal_path_sweeps"):
        assert name in abi.EXPORTS and hasattr(L, name), name
    fields = struct_fields(header, "navsim_goal_path_params")
    assert fields == ["hard_clearance", "clearance", "lookahead", "band_cost"]
    assert [n for n, _ in abi.NavsimGoalPathParams._fields_] == fields
    assert C.sizeof(abi.NavsimGoalPathParams) == 32
    assert struct_fields(header, "navsim_goal_field") == [n for n, _ in abi.NavsimGoalField._fields_] == ["dist", "key", "rebuilds"]
    assert struct_fields(header, "navsim_goal_path_out") == [n for n, _ in abi.NavsimGoalPathOut._fields_] == list(abi.GOAL_PATH_OUT)
    for name, value in (("OK", 1), ("REACHED_GOAL_CELL", 2), ("OFF_FIELD", 4)):
        assert re.search(r"#define NAVSIM_GOAL_PATH_%s\s+%d\b" % (name, value), header) and getattr(abi, "GOAL_PATH_" + name) == value
    assert (spec.OK, spec.REACHED, spec.OFF_FIELD) == (1, 2, 4)
    cfg = lib.default_config(n_envs=3, map_h=103, map_w=57)
    assert L.navsim_goal_field_bytes(C.byref(cfg)) == 3 * 20 * 11 * 2
    cfg.map_w = 4
    assert L.navsim_goal_field_bytes(C.byref(cfg)) == 0 and L.navsim_goal_field_bytes(None) == 0


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, map_h=100, map_w=100)
    st_fields = ("robot_pose", "robot_goal", "episode", "field")

    def state(skip=(), **extra):
        st = abi.NavsimState()
        for k in st_fields + tuple(extra):
            setattr(st, k, None if k in skip else ptr)
        return st

    def field(skip=()):
        return abi.NavsimGoalField(**{k: (None if k in skip else ptr) for k in ("dist", "key", "rebuilds")})

    def outputs(skip=()):
        return abi.NavsimGoalPathOut(**{k: (None if k in skip else ptr) for k in abi.GOAL_PATH_OUT})

    def params(**kw):
        p = abi.NavsimGoalPathParams(hard_clearance=0.3, clearance=0.75, lookahead=2.0, band_cost=3)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    ref_ = lambda x: None if x is None else C.byref(x)
    call = lambda c=cfg, s=state(), p=params(), f=field(), o=outputs(): L.navsim_goal_path(ref_(c), ref_(s), ref_(p), None, None,
                                                                                             ref_(f), ref_(o), None)
    assert call(c=None) == call(s=None) == call(p=None) == call(f=None) == call(o=None) == abi.E_ARG
    for k in ("dist", "key"):
        assert call(f=field(skip=(k,))) == abi.E_ARG, k
    for k in abi.GOAL_PATH_OUT:
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    for k in st_fields:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
    nan, inf = float("nan"), float("inf")
    for k, bad in (("hard_clearance", nan), ("hard_clearance", inf), ("hard_clearance", np.nextafter(3 * cfg.resolution, 0.0)),
                   ("hard_clearance", -1.0), ("clearance", nan), ("clearance", inf), ("clearance", np.nextafter(0.3, 0.0)),
                   ("band_cost", 0), ("band_cost", 17), ("band_cost", -3), ("lookahead", -0.1), ("lookahead", nan),
                   ("lookahead", inf)):
        assert call(p=params(**{k: bad})) == abi.E_ARG, (k, bad)
    for k, bad in (("n_envs", -1), ("map_h", 4), ("map_w", 4)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        assert call(c=c2) == abi.E_ARG, (k, bad)
    shared = cfg.copy(); shared.shared_field = 1
    assert call(c=shared, s=state(map_slot=1)) == abi.E_ARG
    fmt = cfg.copy(); fmt.field_format = 7
    assert call(c=fmt) == abi.E_UNSUPPORTED
    big = cfg.copy(); big.map_h = big.map_w = 1200                          # 240 x 240 nav cells: 175 KB, more than a workgroup has
    assert call(c=big) == abi.E_UNSUPPORTED
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted
    empty = cfg.copy(); empty.n_envs = 0; empty.map_h = empty.map_w = 1000   # (the reference's 200 x 200 nav cells fit)
    assert call(c=empty, p=params(hard_clearance=3 * cfg.resolution, clearance=3 * cfg.resolution, band_cost=16, lookahead=0.0)) == abi.OK
    assert call(c=empty, p=params(band_cost=1), f=field(skip=("rebuilds",))) == abi.OK     # (rebuilds may be NULL)


# ---- host wiring --------------------------------------------------------------------------------------------------------------
def test_parameter_defaults_and_unknown_keys():
    from nav_gym_amd import lib, sim
    cfg = lib.default_config()
    p = sim.goal_path_params(cfg)
    assert (p.hard_clearance, p.clearance, p.band_cost, p.lookahead) == (0.3, 0.75, 3, 2.0)
    assert sim.goal_path_defaults(cfg) == spec.DEFAULT and tuple(sim.GOAL_PATH_KEYS) == tuple(spec.DEFAULT)
    p = sim.goal_path_params(cfg, dict(hard_clearance=0.2, clearance=0.5, band_cost=5, lookahead=1.0))
    assert (p.hard_clearance, p.clearance, p.band_cost, p.lookahead) == (0.2, 0.5, 5, 1.0)
    with pytest.raises(ValueError, match="hard_clearance, clearance, band_cost, lookahead"):
        sim.goal_path_params(cfg, dict(look_ahead=3.0))
    lay = sim.goal_path_layout(5)
    assert [(k, d, shape) for k, d, _, _, shape in lay[:-1]] == [("distance", "float32", (5,)), ("subgoal", "float32", (5, 2)),
                                                                 ("status", "uint8", (5,))]
    assert [hi - lo for _, _, lo, hi, _ in lay[:-1]] == [20, 40, 5]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:]))


def test_env_keywords():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, goal_path=True, goal_path_params=dict(lookahead=1.0, band_cost=2))
    assert env.goal_path_on and env.goal_path_params == dict(lookahead=1.0, band_cost=2)
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.goal_path_on and twin.goal_path_params == dict(lookahead=1.0, band_cost=2) and twin.num_envs == 3
    with pytest.raises(RuntimeError):
        env.goal_path()                                    # before reset()
    with pytest.raises(RuntimeError):
        env.goal_field()
    with pytest.raises(ValueError, match="goal_path=True"):                        # parameters without the feature
        nav_gym_env.make("NavGym-v0", num_envs=3, goal_path_params=dict(lookahead=1.0))
    with pytest.raises(ValueError, match="hard_clearance, clearance, band_cost, lookahead"):    # an unknown key names the known ones
        nav_gym_env.make("NavGym-v0", num_envs=3, goal_path=True, goal_path_params=dict(range=1.0))
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert not plain.goal_path_on
    with pytest.raises(RuntimeError):
        plain.goal_path()
    with pytest.raises(RuntimeError):
        plain.goal_field()
    assert "goal_path" not in registry.spec("NavGym-v0")["kwargs"] and "goal_path_params" not in registry.spec("NavGym-v0")["kwargs"]
