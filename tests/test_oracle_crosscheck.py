"""CPU: independent cross-checks of the UNPINNED oracle rows (a3-a6), SURVEY.md section 8c:
SciPy EDT vs the oracle's distance transform, unit-step ray walk vs sphere trace, closed-form
ray/rectangle and ray/circle cases, and the deterministic math against numpy."""
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import ref
from helpers import keti_thresholds, outdoor_map
from nav_gym_amd import abi


def _ulp(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(b), 1e-300)))


def test_navmath_against_numpy():
    rng = np.random.default_rng(0)
    x = rng.uniform(-40, 40, 200000)
    assert _ulp(ref.math_fn(0, x), np.sin(x)) <= 2
    assert _ulp(ref.math_fn(1, x), np.cos(x)) <= 2
    y, xx = rng.normal(size=200000), rng.normal(size=200000)
    assert _ulp(ref.math_fn(2, y, xx), np.arctan2(y, xx)) <= 2
    e = -rng.uniform(0, 60, 200000)
    assert _ulp(ref.math_fn(3, e), np.exp(e)) <= 2
    assert np.array_equal(ref.math_fn(5, x), np.mod(x, 2 * np.pi))
    # axes and quadrants of atan2
    ys = np.array([0.0, 1.0, -1.0, 0.0, 1e-300, -2.0])
    xs = np.array([1.0, 0.0, 0.0, -1.0, -1.0, -2.0])
    np.testing.assert_allclose(ref.math_fn(2, ys, xs), np.arctan2(ys, xs), rtol=0, atol=1e-15)


@pytest.mark.parametrize("size,seed", [(100, 1), (400, 2), (500, 3)])
def test_distance_transform_vs_scipy(size, seed):
    rng = np.random.default_rng(seed)
    occ = outdoor_map(rng, size)
    f = ref.build_dt(occ)[0]
    d2 = ndi.distance_transform_edt(occ == 0) ** 2
    d2 = np.rint(d2).astype(np.int64)
    assert np.array_equal(f, np.sqrt(d2.astype(np.float32)))
    assert (f[occ != 0] == 0).all() and (f[occ == 0] > 0).all()


def test_distance_transform_random_and_ragged():
    rng = np.random.default_rng(5)
    occ = (rng.random((3, 37, 53)) < 0.02).astype(np.uint8)
    occ[1] = 0
    occ[1, 0, 0] = 1                              # a single obstacle in a corner
    f = ref.build_dt(occ)
    for m in range(3):
        d2 = np.rint(ndi.distance_transform_edt(occ[m] == 0) ** 2).astype(np.int64)
        assert np.array_equal(f[m], np.sqrt(d2.astype(np.float32)))
    empty = ref.build_dt(np.zeros((1, 8, 8), np.uint8))
    assert (empty >= 32768).all()                 # documented "no obstacle" value


def _random_queries(rng, occ, n):
    free = np.argwhere(occ == 0)
    pick = free[rng.integers(0, len(free), n)]
    q = np.zeros((n, 3), np.float32)
    q[:, 0] = pick[:, 1]
    q[:, 1] = pick[:, 0]
    q[:, 2] = rng.uniform(-np.pi, 3 * np.pi, n)
    return q


def test_sphere_trace_vs_unit_steps():
    """Same sampling rule with unit steps.  The two walks sample different points t along the ray,
    so a grazing ray can catch (or miss) a corner cell in one and not the other -- the documented
    corner-skip of sphere tracing.  On outdoor maps ~89 % of rays agree exactly and > 99 % to
    within 1.5 cells; neither walk dominates the other."""
    rng = np.random.default_rng(7)
    occ = outdoor_map(rng, 200)
    f = ref.build_dt(occ)
    q = _random_queries(rng, occ, 20000)
    a = ref.cast_static(f, q[None], 200.0 * 200.0)[0]
    b = ref.cast_unit_steps(occ, q, 200.0 * 200.0)
    frac_equal = np.mean(a == b)
    assert frac_equal > 0.85, frac_equal
    assert np.mean(np.abs(a - b) <= 1.5) > 0.99
    # both report exact cell-centre distances: every finite range is sqrt(integer)
    fin = a < 200.0 * 200.0
    assert np.allclose(np.rint(a[fin].astype(np.float64) ** 2), a[fin].astype(np.float64) ** 2, atol=2e-2)


def march_rule_sensitivity(n_rays, size=500, n_maps=8, seed=3, keep=None):
    """How many rays of calc_range change their result between the candidate roundings of include/navsim.h
    (NAVSIM_MARCH_F64: fl32(fl64(d) * 0.999); NAVSIM_MARCH_F32: d * 0.999f; NAVSIM_MARCH_F32_FMA: the latter with the
    sample position contracted into an FMA), on outdoor maps of the bench's shape with origins on free integer cells
    (env.py:419) and uniform headings.  Ranges are exact cell-centre distances, so a changed range IS a changed hit
    cell.  -> (n_rays, [n_changed F64 vs F32, n_changed F32 vs F32_FMA], [max |delta| cells of each]);
    `keep` (a list) collects (occ, queries, ranges_f64, ranges_f32, ranges_f32_fma) of the maps holding changed rays
    of both kinds."""
    rng = np.random.default_rng(seed)
    per = n_rays // n_maps
    changed, worst = [0, 0], [0.0, 0.0]
    for _ in range(n_maps):
        occ = outdoor_map(rng, size)
        f = ref.build_dt(occ[None])
        q = _random_queries(rng, occ, per)
        a = ref.cast_static(f, q[None], float(size * size), abi.MARCH_F64)[0]
        b = ref.cast_static(f, q[None], float(size * size), abi.MARCH_F32)[0]
        c = ref.cast_static(f, q[None], float(size * size), abi.MARCH_F32_FMA)[0]
        diffs = (a != b, b != c)
        for k, (diff, x, y) in enumerate(((diffs[0], a, b), (diffs[1], b, c))):
            changed[k] += int(diff.sum())
            if diff.any():
                worst[k] = max(worst[k], float(np.abs(x[diff] - y[diff]).max()))
        if keep is not None and diffs[0].any() and diffs[1].any():
            # the changed rays (at most 64 of each kind) + a few unchanged
            pick = np.concatenate([np.where(diffs[0])[0][:64], np.where(diffs[1])[0][:64], np.arange(8)])
            keep.append((occ, q[pick], a[pick], b[pick], c[pick]))
    return per * n_maps, changed, worst


def direction_rounding_sensitivity(n_rays, size=500, n_maps=8, seed=5, rule=abi.MARCH_F32):
    """The FOURTH family of last-bit differences (round-5 verdict): upstream's calc_range takes its ray direction from the C
    library's cosf / sinf of the float heading, the specification from fl32(cos64(fl64(heading))) -- the correctly rounded
    value; glibc's float functions are accurate to < 1 ulp but not correctly rounded for every argument.  Measured here:
    (a) how many headings THIS machine's libm rounds differently (either component), (b) how many rays then change their hit
    cell, (c) the conditional sensitivity -- rays that change when dx resp. dy is moved by one ulp up or down.
    -> dict(rays, libm_differs, libm_changed, ulp_changed = [dx+, dx-, dy+, dy-], worst_cells)"""
    rng = np.random.default_rng(seed)
    per = n_rays // n_maps
    out = dict(rays=0, libm_differs=0, libm_changed=0, ulp_changed=[0, 0, 0, 0], worst_cells=0.0)
    for _ in range(n_maps):
        occ = outdoor_map(rng, size)
        f = ref.build_dt(occ[None])[0]
        q = _random_queries(rng, occ, per)
        d0 = ref.beam_dirs(q[:, 2])
        base = ref.cast_dirs(f, np.concatenate([q[:, :2], d0], axis=1), float(size * size), rule)
        assert np.array_equal(base, ref.cast_static(f[None], q[None], float(size * size), rule)[0])
        d1 = ref.beam_dirs(q[:, 2], libm=True)
        differs = (d0 != d1).any(axis=1)
        r1 = ref.cast_dirs(f, np.concatenate([q[:, :2], d1], axis=1), float(size * size), rule)
        out["rays"] += per
        out["libm_differs"] += int(differs.sum())
        out["libm_changed"] += int((r1 != base).sum())
        if (r1 != base).any():
            out["worst_cells"] = max(out["worst_cells"], float(np.abs(r1 - base)[r1 != base].max()))
        for k, (col, toward) in enumerate(((0, np.inf), (0, -np.inf), (1, np.inf), (1, -np.inf))):
            d = d0.copy()
            d[:, col] = np.nextafter(d[:, col], np.float32(toward))
            r = ref.cast_dirs(f, np.concatenate([q[:, :2], d], axis=1), float(size * size), rule)
            out["ulp_changed"][k] += int((r != base).sum())
    return out


def test_direction_rounding_sensitivity_is_of_the_order_of_the_other_roundings():
    """A reduced run of the measurement quoted in DESIGN.md section 2 (10^7 rays: `python tests/test_oracle_crosscheck.py`):
    moving a ray's direction by one ulp changes its hit cell for a few rays in 10^5 -- the same order as the step-rule
    families -- and this machine's libm differs from the correctly rounded direction on a small fraction of headings only."""
    s = direction_rounding_sensitivity(400_000, n_maps=4)
    per_1e5 = [c * 1e5 / s["rays"] for c in s["ulp_changed"]]
    assert all(0.0 < x < 60.0 for x in per_1e5), per_1e5
    assert s["libm_differs"] < 0.2 * s["rays"]
    assert s["libm_changed"] <= max(s["ulp_changed"])


def test_march_rule_cases(golden_dir):
    """The unpinned roundings of range_libc's march (oracle/navsim_ref.c, row a4; include/navsim.h NAVSIM_MARCH_*) are
    a documented switch.  The step rules give different probe sequences for about 3 rays in 10^6, the contracted
    sample position for more (`python tests/test_oracle_crosscheck.py` measures 10^7 and writes this fixture); a
    changed ray lands on another cell (0.05 m >> 1e-5 m), which is why the rule has to be a switch and not a
    tolerance.  The fixture holds rays where the rules DO differ: the oracle reproduces all recorded answers
    (tests/test_gpu_parity.py asks the same of the device)."""
    d = np.load(os.path.join(golden_dir, "march_rule_cases.npz"))
    n_maps = int(d["n_maps"])
    changed_step = changed_pos = 0
    for m in range(n_maps):
        H, W = [int(x) for x in d["shape_%d" % m]]
        occ = np.unpackbits(d["occ_%d" % m])[: H * W].reshape(H, W)
        f = ref.build_dt(occ[None])
        q = d["q_%d" % m]
        a = ref.cast_static(f, q[None], float(H * W), abi.MARCH_F64)[0]
        b = ref.cast_static(f, q[None], float(H * W), abi.MARCH_F32)[0]
        c = ref.cast_static(f, q[None], float(H * W), abi.MARCH_F32_FMA)[0]
        assert np.array_equal(a, d["r64_%d" % m]) and np.array_equal(b, d["r32_%d" % m])
        assert np.array_equal(c, d["r32fma_%d" % m])
        changed_step += int((a != b).sum())
        changed_pos += int((b != c).sum())
    assert changed_step >= 3 and changed_pos >= 3


def test_cast_static_edges():
    occ = np.zeros((1, 20, 30), np.uint8)
    occ[0, :, 25] = 1
    f = ref.build_dt(occ)
    q = np.array([[[3.0, 10.0, 0.0], [3.0, 10.0, np.pi], [3.0, 10.0, np.pi / 2], [25.0, 4.0, 1.0]]], np.float32)
    r = ref.cast_static(f, q, 600.0)[0]
    assert r[0] == 22.0                           # wall at x = 25
    assert r[1] == 600.0 and r[2] == 600.0        # leaves the map -> max_range (env.py:337)
    assert r[3] == 0.0                            # starts inside an occupied cell
    assert ref.cast_static(f, np.zeros((1, 0, 3), np.float32), 600.0).shape == (1, 0)   # empty query set


def test_render_polys_rectangle_closed_form():
    B = 720
    ang = np.linspace(-np.pi, np.pi, B, endpoint=False)
    hx, hy = 1.1, 0.6
    verts = np.array([[[0, hx, hy], [0, -0.7, hy], [0, -0.7, -hy], [0, hx, -hy]]], np.float32)   # un-closed
    got = ref.render_polys(np.full((1, B), 25.0, np.float32), ang[None], verts, [4], [[0.0, 0.0]])[0]
    c, s = np.cos(ang), np.sin(ang)
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, hx / c, np.where(c < 0, -0.7 / c, np.inf))
        ty = np.where(s > 0, hy / s, np.where(s < 0, -hy / s, np.inf))
    np.testing.assert_allclose(got, np.minimum(tx, ty), rtol=0, atol=2e-6)
    # two contours, second nearer; ids separate them (no edge between contours)
    verts2 = np.array([[[0, 5, -1], [0, 5, 1], [1, 2, -1], [1, 2, 1]]], np.float32)
    got2 = ref.render_polys(np.full((1, 1), 25.0, np.float32), np.zeros((1, 1)), verts2, [4], [[0.0, 0.0]])[0]
    assert abs(got2[0] - 2.0) < 1e-6
    # a beam pointing away keeps its range; zero vertices is a no-op
    got3 = ref.render_polys(np.full((1, 1), 25.0, np.float32), np.full((1, 1), np.pi), verts2, [4], [[0.0, 0.0]])[0]
    assert got3[0] == 25.0
    got4 = ref.render_polys(np.full((1, 3), 7.0, np.float32), np.zeros((1, 3)), verts2, [0], [[0.0, 0.0]])[0]
    assert (got4 == 7.0).all()


def test_render_legs_circle_closed_form():
    # agent at (3, 0) heading 0, no travel: front = 0.3, side = 0.1 -> right (3.3, 0.2), left (2.7, -0.2)
    agent = np.array([[[3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]], np.float32)
    cc = ref.leg_centres(agent[0, 0])
    np.testing.assert_allclose(cc, [3.3, 0.2, 2.7, -0.2], rtol=0, atol=1e-6)
    B = 2048
    ang = np.linspace(-0.2, 0.2, B)
    got = ref.render_legs(np.full((1, B), 25.0, np.float32), ang[None], agent, [1], [[0.0, 0.0]])[0]
    exp = np.full(B, 25.0)
    for cx, cy in ((3.3, 0.2), (2.7, -0.2)):
        b = cx * np.cos(ang) + cy * np.sin(ang)
        x = cx * np.sin(ang) - cy * np.cos(ang)
        disc = 0.03 ** 2 - x ** 2
        t = b - np.sqrt(np.maximum(disc, 0))
        exp = np.where((disc >= 0) & (t >= 0), np.minimum(exp, t), exp)
    hit = exp < 25.0
    assert hit.sum() > 50
    # away from the tangent rays the float32 evaluation is tight; at grazing incidence sqrt(disc)
    # amplifies the float32 rounding of centre and direction, so compare hit/miss sets loosely there
    interior = np.zeros(B, bool)
    for cx, cy in ((3.3, 0.2), (2.7, -0.2)):
        x = cx * np.sin(ang) - cy * np.cos(ang)
        interior |= np.abs(x) < 0.025
    np.testing.assert_allclose(got[interior], exp[interior], rtol=0, atol=2e-5)
    assert np.mean((got < 25.0) == hit) > 0.995
    # travel animates the legs: dist_x = 0.3*pi/2 -> front = 0.3*cos(pi) = -0.3
    agent2 = agent.copy()
    agent2[0, 0, 3] = 0.3 * np.pi / 2
    np.testing.assert_allclose(ref.leg_centres(agent2[0, 0]), [2.7, 0.2, 3.3, -0.2], rtol=0, atol=1e-6)


def test_leg_odometry_matches_numpy():
    rng = np.random.default_rng(3)
    n = 64
    pose = np.stack([rng.uniform(0, 20, n), rng.uniform(0, 20, n), rng.uniform(0, 2 * np.pi, n)], 1)
    vel = rng.uniform(-0.6, 0.6, (n, 2))
    prev_yaw = rng.uniform(-np.pi, np.pi, n)
    dist0 = rng.uniform(-1, 1, (n, 3))
    got = ref.leg_odometry(pose, vel, prev_yaw, 0.2, dist0)
    th = -pose[:, 2]
    bx = np.cos(th) * vel[:, 0] - np.sin(th) * vel[:, 1]
    by = np.sin(th) * vel[:, 0] + np.cos(th) * vel[:, 1]
    exp = dist0 + np.stack([bx, by, (pose[:, 2] - prev_yaw) / 0.2], 1) * 0.2
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-12)


def test_costmap_and_planner_properties():
    """costmap = 4-cell dilation of the 5x-subsampled map (env.py:312-332); planner = shortest
    4-connected path: its length equals the BFS distance, every cell is free and consecutive cells
    are neighbours; blocked or unreachable queries return no path."""
    from collections import deque
    rng = np.random.default_rng(3)
    occ = outdoor_map(rng, 400)[None]
    cost = ref.costmap(occ)
    assert cost.shape == (1, 80, 80)
    sub = occ[0, ::5, ::5]
    exp = ndi.binary_dilation(np.pad(sub, 4, mode="reflect"), structure=np.ones((9, 9)))[4:-4, 4:-4]
    assert np.array_equal(cost[0].astype(bool), exp)
    free = np.argwhere(cost[0] == 0)
    n = 40
    a = free[rng.integers(0, len(free), n)]; b = free[rng.integers(0, len(free), n)]
    start = np.stack([(a[:, 1] + 0.5) * 0.25, (a[:, 0] + 0.5) * 0.25], 1)
    goal = np.stack([(b[:, 1] + 0.5) * 0.25, (b[:, 0] + 0.5) * 0.25], 1)
    wp, n_wp, cells, plen = ref.plan(np.repeat(cost, n, 0), start, goal, interval=2.0, max_wp=64)
    for q in range(n):
        dist = -np.ones((80, 80), int); dist[b[q, 0], b[q, 1]] = 0
        dq = deque([(b[q, 0], b[q, 1])])
        while dq:
            j, i = dq.popleft()
            for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                jj, ii = j + dj, i + di
                if 0 <= jj < 80 and 0 <= ii < 80 and cost[0, jj, ii] == 0 and dist[jj, ii] < 0:
                    dist[jj, ii] = dist[j, i] + 1; dq.append((jj, ii))
        if dist[a[q, 0], a[q, 1]] < 0:
            assert n_wp[q] == 0
            continue
        assert cells[q] == dist[a[q, 0], a[q, 1]] + 1
        assert n_wp[q] >= 1 and np.allclose(wp[q, n_wp[q] - 1], goal[q])          # last waypoint = goal
        d = np.linalg.norm(np.diff(np.vstack([start[q], wp[q, : n_wp[q]]]), axis=0), axis=1)
        assert abs(d.sum() - plen[q]) < 1e-9 and plen[q] >= np.linalg.norm(goal[q] - start[q]) - 1e-9
    blocked = np.argwhere(cost[0] != 0)[0]
    _, n0, _, _ = ref.plan(cost, [[(blocked[1] + 0.5) * 0.25, (blocked[0] + 0.5) * 0.25]], goal[:1], 2.0)
    assert n0[0] == 0


def test_regen_with_planning_properties():
    """cfg.regen_plan = 1 (env.py:342-383, 756-804): the new robot start and goal are centres of free
    costmap cells joined by a path no longer than twice the straight line; pedestrians start at least
    ped_min_robot_dist from the robot and their waypoints are exactly what the planner returns for
    (start, last waypoint) at a 2 m interval."""
    from nav_gym_amd import abi, robots
    from helpers import finished_world
    E, size, N = 8, 300, 6
    cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=abi.PED_SFM, n_spawn=6,
                             auto_reset=1, seed=5, regen_cap=8, min_goal_dist=3.0, max_goal_dist=8.0,
                             ped_min_robot_dist=2.0, ped_min_goal_dist=4.0, regen_plan=1, obstacle_number=6)
    rng = np.random.default_rng(0)
    occ = np.stack([outdoor_map(rng, size) for _ in range(E)])
    thr, dthr = keti_thresholds(cfg)
    r = ref.RefSim(cfg, finished_world(cfg, occ, ref.build_dt(occ), 5, (thr, dthr)))
    r.reset_obs()
    _, out = r.step(np.zeros((E, 2)))
    assert out["done"].all()
    r.regen()
    cost = ref.costmap((r.a["field"] == 0).astype(np.uint8))
    cell = lambda xy: (int(xy[1] / 0.25), int(xy[0] / 0.25))
    robots_ok = planned_peds = 0
    for e in range(E):
        s, g = r.a["robot_pose"][e, :2], r.a["robot_goal"][e]
        wp, n_wp, _, plen = ref.plan(cost[e:e + 1], [s], [g], 5.0, max_wp=cfg.max_waypoints)
        if n_wp[0] > 0 and plen[0] <= 2.0 * np.linalg.norm(g - s):
            robots_ok += 1
            assert cost[e][cell(s)] == 0 and cost[e][cell(g)] == 0
            assert 3.0 < np.linalg.norm(g - s) < 8.0
        for i in range(5):
            p, n = r.a["ped_pose"][e, i, :2], r.a["ped_n_waypoints"][e, i]
            w = r.a["ped_waypoints"][e, i]
            if n > 1 or cost[e][cell(w[0])] == 0:
                wp, n_wp, _, _ = ref.plan(cost[e:e + 1], [p], [w[n - 1]], 2.0, max_wp=cfg.max_waypoints)
                if n_wp[0] == n and n < cfg.max_waypoints:
                    assert np.array_equal(wp[0, :n], w[:n])
                    planned_peds += 1
                    assert np.linalg.norm(p - s) >= 2.0 and np.linalg.norm(w[n - 1] - p) > 4.0
        assert (r.a["ped_n_waypoints"][e, 5:] == 1).all()
    assert robots_ok >= E - 1 and planned_peds >= 3 * E


def test_wheel_speed_actions_equal_the_converted_twists():
    """NAVSIM_ACTION_WHEELS on the oracle (round 4, build-defined): stepping with wheel speeds (left, right) equals
    stepping with the twist robots.husky_twist_from_wheels makes of them, bit for bit; with clamp_action the twist is
    clipped to linvel_range x rotvel_range first, and the observation's `vel` slots carry the clipped twist."""
    from nav_gym_amd import robots
    E, size = 6, 120
    rng = np.random.default_rng(8)
    occ = np.stack([outdoor_map(rng, size, n_obstacles=3) for _ in range(E)])
    field = ref.build_dt(occ)
    outs = {}
    for kind, clamp in ((abi.ACTION_WHEELS, 0), (abi.ACTION_TWIST, 0), (abi.ACTION_WHEELS, 1), (abi.ACTION_TWIST, 1)):
        cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, n_beams=64, axle_offset=0.0, action_kind=kind,
                                 clamp_action=clamp, linvel_lo=0.0, linvel_hi=1.0, rotvel_lo=-2.0, rotvel_hi=2.0)
        thr = ref.scan_threshold(cfg, robots.footprint_array("husky", "threshold_footprint"))
        dthr = ref.scan_threshold(cfg, robots.footprint_array("husky", "discomfort_threshold_footprint"))
        pose = np.zeros((E, 3))
        for e in range(E):
            j, i = np.unravel_index(np.argmax(field[e]), field[e].shape)
            pose[e] = ((i + 0.5) * 0.05, (j + 0.5) * 0.05, 0.3 * e)
        r = ref.RefSim(cfg, dict(field=field, scan_threshold=thr, scan_discomfort=dthr, scan_noise_std=np.zeros(E, np.float32),
                                 robot_pose=pose, robot_goal=pose[:, :2] + 30.0, prev_action=np.zeros((E, 2)),
                                 prev_pose=np.zeros((E, 3)), n_hist=np.zeros(E, np.int32), episode=np.zeros(E, np.int64),
                                 steps=np.zeros(E, np.int64)))
        r.reset_obs()
        rr = np.random.default_rng(3)
        rows = []
        for t in range(12):
            wheels = rr.uniform(-3.0, 9.0, (E, 2))
            act = wheels
            if kind == abi.ACTION_TWIST:
                act = robots.husky_twist_from_wheels(wheels[:, 0], wheels[:, 1])
            obs, out = r.step(act)
            rows.append(obs.copy())
        outs[(kind, clamp)] = np.stack(rows)
    assert np.array_equal(outs[(abi.ACTION_WHEELS, 0)], outs[(abi.ACTION_TWIST, 0)])
    assert np.array_equal(outs[(abi.ACTION_WHEELS, 1)], outs[(abi.ACTION_TWIST, 1)])
    assert not np.array_equal(outs[(abi.ACTION_WHEELS, 0)], outs[(abi.ACTION_WHEELS, 1)])
    vel = outs[(abi.ACTION_WHEELS, 1)][2:, :, -3:-1]                 # `vel` = the previous action as integrated
    assert vel[..., 0].min() >= 0.0 and vel[..., 0].max() <= 1.0 and np.abs(vel[..., 1]).max() <= 2.0
    assert outs[(abi.ACTION_WHEELS, 0)][2:, :, -3].max() > 1.0


def test_regen_indoor_maps_are_one_corridor_tree():
    """cfg.regen_indoor_ratio = 1: every regenerated map is a corridor map (create_indoor_map,
    map_generator.py:97-123): free space is ONE 4-connected component (a tree of L-shaped corridors grown
    from the centre), corridors are 3.5-4.5 m wide, walls fill the rest; robot and goal lie in free space."""
    from nav_gym_amd import abi, robots
    from helpers import finished_world
    E, size = 6, 400
    cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, max_peds=1, ped_model=abi.PED_NONE, n_spawn=6,
                             auto_reset=1, seed=9, regen_cap=8, min_goal_dist=3.0, max_goal_dist=8.0,
                             regen_indoor_ratio=1.0)
    rng = np.random.default_rng(0)
    occ = np.stack([outdoor_map(rng, size) for _ in range(E)])
    thr, dthr = keti_thresholds(cfg)
    r = ref.RefSim(cfg, finished_world(cfg, occ, ref.build_dt(occ), 0, (thr, dthr)))
    r.reset_obs()
    _, out = r.step(np.zeros((E, 2)))
    assert out["done"].all()
    r.regen()
    fracs = []
    for e in range(E):
        free = r.a["field"][e] > 0
        lab, n = ndi.label(free)
        assert n == 1, "free space of arena %d falls into %d pieces" % (e, n)
        fracs.append(free.mean())
        # sample() keeps 2 coarse cells of wall at the low end and 1 at the high end; rows are flipped afterwards
        assert not free[:10].any() and not free[-20:].any() and not free[:, :20].any() and not free[:, -10:].any()
        i, j = int(r.a["robot_pose"][e, 0] / 0.05), int(r.a["robot_pose"][e, 1] / 0.05)
        assert free[j, i]
    assert 0.05 < min(fracs) and max(fracs) < 0.9 and len({round(f, 4) for f in fracs}) > 1


if __name__ == "__main__":          # the figure quoted in DESIGN.md section 2 + tests/golden/march_rule_cases.npz
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kept = []
    n, changed, worst = march_rule_sensitivity(10_000_000, n_maps=20, keep=kept)
    print("march rule F64 vs F32: %d of %d rays change their hit cell (%.4f %%), largest change %.2f cells"
          % (changed[0], n, 100.0 * changed[0] / n, worst[0]))
    print("march rule F32 vs F32_FMA: %d of %d rays change their hit cell (%.4f %%), largest change %.2f cells"
          % (changed[1], n, 100.0 * changed[1] / n, worst[1]))
    s = direction_rounding_sensitivity(10_000_000, n_maps=20)
    print("ray direction, correctly rounded vs this machine's cosf / sinf: %d of %d headings differ in dx or dy (%.3f %%), %d rays "
          "change their hit cell (%.4f %%), largest change %.2f cells; one ulp on dx up / down, dy up / down: %s rays per 10^7"
          % (s["libm_differs"], s["rays"], 100.0 * s["libm_differs"] / s["rays"], s["libm_changed"], 100.0 * s["libm_changed"] / s["rays"],
             s["worst_cells"], [int(round(c * 1e7 / s["rays"])) for c in s["ulp_changed"]]))
    out = {"n_maps": np.int32(min(len(kept), 3))}
    for m, (occ, q, a, b, c) in enumerate(kept[:3]):
        out["r32fma_%d" % m] = c
        out["shape_%d" % m] = np.array(occ.shape, np.int32)
        out["occ_%d" % m] = np.packbits(occ.astype(np.uint8).reshape(-1))
        out["q_%d" % m] = q
        out["r64_%d" % m] = a
        out["r32_%d" % m] = b
    np.savez_compressed(os.path.join(_root, "tests", "golden", "march_rule_cases.npz"), **out)


def test_short_episodes_restart_in_place():
    """cfg.regen_min_steps (build-defined; the reference draws a map at every reset): an arena whose episode ended after
    fewer steps keeps its map -- the step's restart from the spawn table stands -- and is counted; one that lasted long
    enough is regenerated.  The step records the length of the episode that ended (done_steps)."""
    from helpers import finished_world
    E, size = 6, 200
    cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, max_peds=1, ped_model=abi.PED_NONE, n_spawn=4, auto_reset=1,
                             seed=3, regen_cap=E, min_goal_dist=3.0, max_goal_dist=8.0, regen_min_steps=3)
    rng = np.random.default_rng(0)
    occ = np.stack([outdoor_map(rng, size) for _ in range(E)])
    thr, dthr = keti_thresholds(cfg)
    r = ref.RefSim(cfg, finished_world(cfg, occ, ref.build_dt(occ), 0, (thr, dthr)))
    r.reset_obs()
    # every arena ends its episode in this step; pretend half of them had been running for a while
    r.a["steps"][:] = [0, 7, 1, 2, 0, 40]
    _, out = r.step(np.zeros((E, 2)))
    assert out["done"].all()
    assert r.a["done_steps"].tolist() == [1, 8, 2, 3, 1, 41] and (r.a["steps"] == 0).all()
    field0, pose0, ep0 = r.a["field"].copy(), r.a["robot_pose"].copy(), r.a["episode"].copy()
    r.regen()
    lng = r.a["done_steps"] >= 3
    assert lng.tolist() == [False, True, False, True, False, True]
    for e in range(E):
        same_map = np.array_equal(r.a["field"][e], field0[e])
        assert same_map == (not lng[e]), e
        if not lng[e]:
            assert np.array_equal(r.a["robot_pose"][e], pose0[e])           # the restart in place stands
    assert np.array_equal(r.a["episode"], ep0)                              # the step advanced them, regen does not
    c = r.counters()
    assert c["regen_short"] == 3 and c["regen_served"] == 3 and c["regen_unserved"] == 0
    # without the buffer the rule cannot be applied: refused, not ignored
    r.st.done_steps = None
    r.out["done"][:] = 1
    with pytest.raises(Exception):
        r.regen()


def test_native_thread_pool_equals_sequential_steps():
    """bench.py's CPU baseline (navsim_step_threads_cpu: POSIX threads inside the oracle, arenas split statically, no
    barrier between steps) computes exactly what step() after step() computes: observations, outputs and state."""
    from nav_gym_amd import lib, world
    E, size, N = 13, 120, 4
    cfg = lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=abi.PED_SFM, n_spawn=4, auto_reset=1,
                             n_scan_stack=2, seed=8)
    world.lidar_full_circle(cfg, 90)
    occ = world.make_maps(E, size, 8)
    import torch
    arrays = world.make_world(cfg, occ, n_peds=3, device="cpu", field=torch.from_numpy(ref.build_dt(occ)), min_goal_dist=2.0,
                              max_goal_dist=4.0, robot_clearance=0.8)
    host = {k: v.numpy() for k, v in arrays.items()}
    host["scan_threshold"], host["scan_discomfort"] = keti_thresholds(cfg)
    a, b = ref.RefSim(cfg, host), ref.RefSim(cfg, host)
    assert np.array_equal(a.reset_obs(), b.reset_obs())
    rng = np.random.default_rng(1)
    for n_steps, n_threads in ((5, 3), (4, 13), (1, 40)):
        acts = np.stack([rng.uniform(0, 0.5, (n_steps, E)), rng.uniform(-0.64, 0.64, (n_steps, E))], axis=2)
        for s in range(n_steps):
            oa, outa = a.step(acts[s])
        ob, outb = b.step_native_threads(acts, n_threads)
        assert np.array_equal(oa, ob)
        for k in outa:
            assert np.array_equal(outa[k], outb[k]), k
        for k in a.a:
            assert np.array_equal(a.a[k], b.a[k]), k
