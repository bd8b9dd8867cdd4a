"""CPU: ORCA pedestrians that avoid the arena's listed rectangles (include/navsim.h navsim_ped_orca_walls) -- the entry's place in
the C ABI and its refusals, and the specification (tests/ped_orca_walls_spec.py: the selection in numpy float32 + the oracle's
navsim_crowd_orca_cpu with one polygon set per query) on the oracle alone: the selection rule on hand-made lists, the axes, a
closed loop through boxes, the float64 swept-clearance check and the census of the shared scenes.  The device against that
specification is tests/test_gpu_ped_orca_walls.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import ped_orca_spec as spec
import ped_orca_walls_scenes as ws
import ped_orca_walls_spec as wspec
import ref
from helpers import keti_thresholds
from nav_gym_amd import abi


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_stays_7_with_one_new_export():
    from nav_gym_amd import lib
    L = lib.load()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 and C.sizeof(abi.NavsimPedOrcaParams) == 56
    assert "navsim_ped_orca_walls" in abi.EXPORTS and hasattr(L, "navsim_ped_orca_walls")
    assert "navsim_ped_orca" in abi.EXPORTS and hasattr(L, "navsim_ped_orca")


def test_argument_refusals_without_gpu():
    from nav_gym_amd import lib, sim
    L = lib.load()
    cfg = lib.default_config(n_envs=2, max_peds=5, ped_model=abi.PED_EXTERNAL)
    st = abi.NavsimState()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    for name in ("n_peds", "ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head",
                 "robot_pose", "prev_action", "rect_index"):
        setattr(st, name, ptr)

    def call(c, p, K, out=ptr, state=st):
        return L.navsim_ped_orca_walls(C.byref(c), C.byref(state), None if p is None else C.byref(p), K, out, None, None)
    good = sim.ped_orca_params(cfg)
    for K in (-1, 33, 1 << 20):
        assert call(cfg, good, K) == abi.E_ARG, K
    bare = abi.NavsimState()
    C.memmove(C.byref(bare), C.byref(st), C.sizeof(st))
    bare.rect_index = None
    assert call(cfg, good, 1, state=bare) == abi.E_ARG                            # rectangles wanted, no list
    for tho in (0.0, -5.0):
        assert call(cfg, sim.ped_orca_params(cfg, {"time_horizon_obst": tho}), 8) == abi.E_ARG, tho
    # the lists of one wavefront beyond a CU's LDS: refused before any launch (63 pedestrians, lists of 63, 32 rectangles)
    big = cfg.copy(); big.max_peds = 63
    assert call(big, sim.ped_orca_params(big, {"max_neighbors": 63}), 32) == abi.E_UNSUPPORTED
    # navsim_ped_orca's refusals, at K = 0 and at K = 8
    for K in (0, 8):
        assert call(cfg, good, K, None) == abi.E_ARG and call(cfg, None, K) == abi.E_ARG
        for model in (abi.PED_NONE, abi.PED_SFM):
            c2 = cfg.copy(); c2.ped_model = model
            assert call(c2, good, K) == abi.E_ARG, model
        c2 = cfg.copy(); c2.max_peds = abi.ORCA_MAX_AGENTS
        assert call(c2, good, K) == abi.E_ARG
        for key, bad in (("ped_radius", 0.0), ("robot_radius", 0.0), ("time_step", 0.0), ("time_horizon", -5.0), ("max_neighbors", -1)):
            assert call(cfg, sim.ped_orca_params(cfg, {key: bad}), K) == abi.E_ARG, (key, bad)
    # the key and its default
    assert "max_obst_rects" in sim.PED_ORCA_KEYS and sim.ped_orca_defaults(cfg)["max_obst_rects"] == 0
    assert sim.ped_orca_params(cfg, {"max_obst_rects": 8}).orca.time_horizon_obst == 5.0


def test_env_keyword():
    import nav_gym_env
    env = nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", orca_params=dict(max_obst_rects=8))
    assert env._orca_rects == 8 and env.orca_params == dict(max_obst_rects=8)
    assert nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca")._orca_rects == 0
    with pytest.raises(ValueError):                                  # a world of corridor maps per episode has no rect_index
        nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", randomize_maps=True, indoor_ratio=0.5,
                         orca_params=dict(max_obst_rects=8))
    with pytest.raises(ValueError):                                  # nor has a float32 field
        nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", field_format=abi.FIELD_F32,
                         orca_params=dict(max_obst_rects=8))
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", orca_params=dict(max_obst_rects=33))


# ---- the shared scenes, answered once -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _answers(shape):
    E, N, cs = ws.calls(shape)
    cfg = ws.config(E, N)
    out = []
    for s, K, kw in cs:
        p = spec.params(cfg, **kw)
        out.append((cfg, p, s, K) + wspec.ped_orca_walls(cfg, ws.state(s, cfg), p, ws.hand_list(E), K))
    return out


@pytest.mark.parametrize("shape", list(ws.SHAPES))
def test_no_rectangles_is_ped_orca(shape):
    E, N, cs = ws.calls(shape)
    cfg = ws.config(E, N)
    for s, _, kw in cs[:3]:
        p, a = spec.params(cfg, **kw), ws.state(s, cfg)
        a["ped_cmd"][...] = -7.25
        cmd, head, dropped, _ = wspec.ped_orca_walls(cfg, a, p, ws.hand_list(E), 0)
        want_cmd, want_head, _ = spec.ped_orca(cfg, a, p)
        assert np.array_equal(cmd, want_cmd) and np.array_equal(head, want_head) and not dropped.any()


def test_census_of_the_scenes():
    ws.census_of([(shape, item[-1]) for shape in ws.SHAPES for item in _answers(shape)], 20, "oracle composition", lanes=False)


# ---- the selection alone ------------------------------------------------------------------------------------------------------
def _list(entries):
    rects = np.zeros((wspec.LIST_LEN, 4), np.int16)
    for k, r in entries.items():
        rects[k] = r
    return rects


def test_selection_rule():
    cfg = ws.config(1, 1)
    f = np.float32
    sel = lambda rects, px, py, reach, K: wspec.select(cfg, rects, px, py, f(f(reach) * f(reach)), K)
    # cells of 0.05 m; the pedestrian at (3, 3); squares of 2 cells whose near faces are 0.5, 1.0, 1.5, 2.0 m to its right
    right = lambda d, y=59: (60 + int(round(d / 0.05)), y, 61 + int(round(d / 0.05)), y + 1)
    # zero entries in the middle are skipped, list order does not matter, kept indices come back ascending
    rects = _list({3: right(1.5), 7: right(0.5), 100: right(1.0), 254: right(2.0)})
    assert sel(rects, 3.0, 3.0, 5.0, 8) == ([3, 7, 100, 254], 4)
    assert sel(rects, 3.0, 3.0, 5.0, 2) == ([7, 100], 4)                          # the nearest two; dropped = 4 - 2
    assert sel(rects, 3.0, 3.0, 1.25, 8) == ([7, 100], 2)                         # the range rejects the others
    assert sel(rects, 3.0, 3.0, 5.0, 0) == ([], 4)
    # a nearer rectangle behind a full list displaces the farthest; an equally near one does not (ties go to the lower index)
    rects = _list({1: right(1.0), 2: right(1.5), 3: right(0.5)})
    assert sel(rects, 3.0, 3.0, 5.0, 2) == ([1, 3], 3)
    left = (60 - 20 - 2, 59, 60 - 20 - 1, 60)                                     # near face 1.0 m to the LEFT: as far as right(1.0)
    tie = _list({5: right(1.0), 9: left})
    d = [wspec.select(cfg, _list({0: r}), 3.0, 3.0, f(25.0), 1) for r in (right(1.0), left)]
    assert d[0] == ([0], 1) and d[1] == ([0], 1)
    assert sel(tie, 3.0, 3.0, 5.0, 1) == ([5], 2)
    assert sel(_list({5: left, 9: right(1.0)}), 3.0, 3.0, 5.0, 1) == ([5], 2)
    # exactly at the range: rejected (strict <).  The face at x = 4.0 from px = 3.0: d2 = 1.0 exactly
    assert sel(_list({4: right(1.0)}), 3.0, 3.0, 1.0, 8) == ([], 0)
    assert sel(_list({4: right(1.0)}), 3.0, 3.0, float(np.nextafter(f(1.0), f(2.0))), 8) == ([4], 1)
    # the lone cell (0, 0) is an all-zero entry: no obstacle; a rectangle that starts at cell (0, 0) is one
    assert sel(_list({0: (0, 0, 0, 0), 1: (0, 0, 119, 2)}), 0.5, 0.5, 5.0, 8) == ([1], 1)


def _one_ped(pos, waypoint, vel=(0.0, 0.0), v_pref=0.8, heading=0.0):
    s = dict(ped_pose=np.array([[[pos[0], pos[1], heading]]]), ped_vel=np.array([[vel]], np.float64),
             ped_v_pref=np.array([[v_pref]]), waypoint=np.array([[waypoint]], np.float64), robot_pose=np.array([[0.6, 0.6, 0.0]]),
             prev_action=np.zeros((1, 2)), n_peds=np.ones(1, np.int32))
    return s


def test_pedestrian_inside_a_rectangle_keeps_it_and_gets_no_edge():
    cfg = ws.config(1, 1)
    p = spec.params(cfg, robot_visible=0, time_horizon_obst=2.0)
    x0, y0, x1, y1 = ws.BOXES[1]
    centre = ((x0 + x1 + 1) / 2 * ws.RES, (y0 + y1 + 1) / 2 * ws.RES)
    a = ws.state(_one_ped(centre, (centre[0] + 3.0, centre[1])), cfg)
    cmd, _, dropped, census = wspec.ped_orca_walls(cfg, a, p, _list({6: ws.BOXES[1]})[None], 8)
    free, _, _ = spec.ped_orca(cfg, a, p)
    assert census.query["n_obst"][0] == 1 and census["0 edges in range"] == 1 and dropped[0, 0] == 0
    assert np.array_equal(cmd, free)                                 # ... so it walks out as if the rectangle were not there


def test_axes():
    """A pedestrian heading at the off-diagonal box is deflected; at the transposed place, heading the transposed way, it is not."""
    cfg = ws.config(1, 1)
    p = spec.params(cfg, robot_visible=0, time_horizon_obst=2.0)
    x0, y0, x1, y1 = ws.OFF_DIAGONAL
    cx, cy = (x0 + x1 + 1) / 2 * ws.RES + 0.1, (y0 + y1 + 1) / 2 * ws.RES        # (slightly off the axis: no symmetric stall)
    rects = ws.hand_list(1)
    for transposed in (False, True):
        pos, goal, vel = (cx, cy - 1.0), (cx, cy + 1.5), (0.0, 0.8)
        if transposed:
            pos, goal, vel = pos[::-1], goal[::-1], vel[::-1]
        a = ws.state(_one_ped(pos, goal, vel, heading=np.arctan2(vel[1], vel[0])), cfg)
        cmd, _, _, census = wspec.ped_orca_walls(cfg, a, p, rects, 8)
        free, _, _ = spec.ped_orca(cfg, a, p)
        print("transposed %s: command %s, without walls %s" % (transposed, cmd[0, 0], free[0, 0]))
        assert census["walls bind"] == (0 if transposed else 1)
        assert np.array_equal(cmd, free) == transposed


# ---- closed loop on the oracle composition -------------------------------------------------------------------------------------
def _through_boxes():
    """Six pedestrians, one per box: a route of two waypoints on opposite sides of the box, the pedestrian at the first."""
    import torch  # noqa: F401  (world.make_world is not used: the state is written by hand)
    n = len(ws.BOXES)
    cfg = ws.config(1, n, auto_reset=abi.AUTORESET_NONE, n_spawn=0, n_beams=64)
    from nav_gym_amd import world
    world.lidar_full_circle(cfg, 64)
    P = cfg.max_waypoints
    wp, pose = np.zeros((1, n, P, 2)), np.zeros((1, n, 3))
    for i, (x0, y0, x1, y1) in enumerate(ws.BOXES):
        cx, cy = (x0 + x1 + 1) / 2 * ws.RES, (y0 + y1 + 1) / 2 * ws.RES
        along_x = i % 2 == 0
        d = np.array([1.0, 0.07] if along_x else [0.07, 1.0])        # (not through the centre: no symmetric stall)
        wp[0, i, 0], wp[0, i, 1] = (cx, cy) - 0.9 * d, (cx, cy) + 0.9 * d
        pose[0, i, :2] = wp[0, i, 0]
        pose[0, i, 2] = 0.0 if along_x else np.pi / 2
    occ = ws.occupancy(1)
    thr, dthr = keti_thresholds(cfg)
    r = ref.RefSim(cfg, dict(
        field=ref.build_dt(occ), scan_noise_std=np.zeros(1, np.float32),
        scan_threshold=thr, scan_discomfort=dthr,
        robot_pose=np.array([[2.25, 3.75, 0.0]]), robot_goal=np.array([[3.75, 2.25]]), prev_action=np.zeros((1, 2)),
        prev_pose=np.zeros((1, 3)), n_hist=np.zeros(1, np.int32), episode=np.zeros(1, np.int64), steps=np.zeros(1, np.int64),
        n_peds=np.full(1, n, np.int32), ped_pose=pose, ped_vel=np.zeros((1, n, 2)), ped_prev_yaw=np.zeros((1, n)),
        ped_dist=np.zeros((1, n, 3)), ped_v_pref=np.full((1, n), 0.6), ped_has_legs=np.ones((1, n), np.uint8),
        ped_waypoints=wp, ped_n_waypoints=np.full((1, n), 2, np.int32), ped_cmd=np.zeros((1, n, 2))))
    r.reset_obs()
    return cfg, r


def _rect_distance(xy):
    """distance of every point [n,2] to the nearest of the map's rectangles (0 inside), float64"""
    r = np.array(ws.WALLS + ws.BOXES, np.float64)
    lo, hi = r[:, :2] * ws.RES, (r[:, 2:] + 1) * ws.RES
    d = np.maximum(np.maximum(lo[None] - xy[:, None], xy[:, None] - hi[None]), 0.0)
    return np.sqrt((d ** 2).sum(-1)).min(1)


@pytest.mark.parametrize("K", [8, 0])
def test_closed_loop_through_boxes(K):
    cfg, r = _through_boxes()
    p = spec.params(cfg, robot_visible=0, time_horizon_obst=2.0)
    rects = ws.hand_list(1)
    radius = float(np.float32((p["ped_radius"] + 0.01) + p["safety_space"]))
    nearest = np.inf
    for _ in range(200):
        cmd, head, _, _ = wspec.ped_orca_walls(cfg, r.a, p, rects, K)
        r.a["ped_wp_head"][...] = head
        r.set_ped_cmd(cmd)
        r.step(np.zeros((1, 2)))
        nearest = min(nearest, float(_rect_distance(r.a["ped_pose"][0, :, :2]).min()))
    print("max_rects %d: a pedestrian centre comes within %.9f m of a rectangle (radius %.4f)" % (K, nearest, radius))
    if K:
        assert nearest >= radius - ws.B
    else:
        assert nearest == 0.0                                        # without walls a centre enters a box: the scenario bites


# ---- the independent check ----------------------------------------------------------------------------------------------------
def test_swept_clearance():
    """The disc swept for time_horizon_obst along the oracle's answer against the kept rectangles, by tests/orca_f64.py: every
    query of every call that starts clear by 1 mm with nothing dropped.  Measured with the oracle on these scenes (3 197 queries
    compared, 295 = 8.4 % left out): worst entry 8.94e-8 m at 0.5 s, 6.86e-7 m at 2 s -> B = orca_scenes.CLEAR_BOUND; 0.253 m at
    5 s (2 of 90 queries of the 3 x 33, max_rects 32 call; every other call <= 2.0e-6 m) -> 4 x worst = 1 m, more than the
    radius: at that horizon nothing is bounded (ped_orca_walls_scenes.B_LONG says why)."""
    def answer(shape, c):
        cfg, p, _, _, cmd, _, _, census = _answers(shape)[c]
        return cmd, census, cfg, p
    ws.swept_check(answer, "oracle composition")
