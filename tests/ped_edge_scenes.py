"""TEST INFRASTRUCTURE: hand-made pedestrian scenes at the edges of the two shortcuts the device takes with pedestrians (NumPy
only; shared by tests/test_ped_edge_scenes.py on the oracle and tests/test_gpu_ped_edge_scenes.py on the device).

  * the bearing-culled merge of pedestrian primitives into a scan (csrc/kernels_step.hpp prim_in_range,
    merge_prims_culled_core): lidars inside and next to a primitive, primitives at the clip range, on the first and last
    beam's bearing and on the +-pi fold of the relative bearing, sides seen under almost pi, 256 primitives at once;
  * the social force in its two device forms (half a pair table on wavefront 0; one list of pair terms per pack of arenas):
    coincident agents, a vanishing interaction vector, theta == 0, a pedestrian on its waypoint, v_pref = 0, the speed clamp,
    the gradient's clamped cells, every pedestrian count at which the pair table's indexing changes shape.

One scene is one arena; all scenes of a world share its configuration (one lidar, one origin).  A world is a dict of host
arrays named like abi.STATE_LAYOUT -- what ref.RefSim takes -- plus the list of its scenes' names, so that a failure names
the case.  The map is a 160 x 160 hall of the default 5 cm cells, empty inside the 5-cell ring; with range_max = 3 m the
clip range lies inside the hall for a lidar at its centre.  The distance field and the scan thresholds are the caller's."""
import math

import numpy as np

SIZE, RING, RES = 160, 5, 0.05
RANGE_MAX = 3.0
RCULL = float(np.float32(RANGE_MAX) * np.float32(1.0001) + np.float32(0.01))     # kernels_step.hpp prim_cull_range
LEG_R = 0.03
HALF = (0.22, 0.19)                                     # human.py:5-10: the rectangle's half sides (body x, body y)
LEGS = ((0.3, 0.2), (-0.3, -0.2))                       # DESIGN.md section 2 row a6 at ped_dist = 0: right leg, left leg
CENTRE = (4.013, 3.987)                                 # the lidar of every lidar scene, before the origin's shift
# Larger headings are left to a later change.  A float32 heading near 30 000 rad has an ulp of 1.95e-3 rad, more than the
# 1.57e-3 rad between the beams of the 4000-beam lidar: only there does the merge's two-beam margin decide a hit (with 4000
# beams and |heading| <= 50 rad a margin of zero loses nothing: floor / ceil already round the interval outwards, and the
# bearing errors are a thousandth of a beam).  But at 30 000 rad the device's beam directions themselves leave the oracle's
# by an ulp (fan_77, 'a side under 2.90 rad': two ranges differ by 3.7e-9 m), which is another matter than the merge.
HEADINGS = (0.0, 0.5 * math.pi, -0.5 * math.pi, math.pi, -math.pi, 1.5 * math.pi, 50.0, -50.0)
MAX_PEDS = 64

# name -> (angle_min, angle_last, n_beams)
LIDARS = dict(
    reference_1081=(-0.75 * math.pi, 0.75 * math.pi, 1081),
    circle_8=(-math.pi, math.pi - 2 * math.pi / 8, 8),          # step 0.785: 2 pi - 2 step < 4.8, the alias m = -1 is walked
    circle_9=(-math.pi, math.pi - 2 * math.pi / 9, 9),          # step 0.698: it is not
    circle_10=(-math.pi, math.pi - 2 * math.pi / 10, 10),
    circle_33=(-math.pi, math.pi - 2 * math.pi / 33, 33),
    fan_77=(-2.0, 2.5, 77),
    circle_4000=(-math.pi, math.pi - 2 * math.pi / 4000, 4000),
    one_beam=(-0.3, 0.3, 1),
    two_beams=(-2.5, 2.5, 2),
    three_beams=(-2.0, 2.0, 3),
    half_plane=(-0.5 * math.pi, 0.5 * math.pi, 181),
    fan_02=(0.4, 0.6, 21),
    exactly_2pi=(-math.pi, math.pi, 90),
    reversed_33=(1.0, -1.0, 33),                                # step < 0: every primitive takes all beams
)
WIDE_LIDARS = dict(wide_7=(-3.5, 3.5, 90), wide_94=(-3.2, 6.2, 90))        # above 2 pi: served without pedestrians only
PED_LIDARS = dict(ped_9=9, ped_512=512)                                     # cfg.ped_n_beams over the default half plane
OFFSETS = dict(origin_m16_32=(-16.0, 32.0), origin_40_40=(40.0, 40.0))


def hall():
    """uint8 [SIZE, SIZE]: the 5-cell ring, nothing inside."""
    m = np.ones((SIZE, SIZE), np.uint8)
    m[RING:SIZE - RING, RING:SIZE - RING] = 0
    return m


def _rot(a, v):
    c, s = math.cos(a), math.sin(a)
    return np.array([c * v[0] - s * v[1], s * v[0] + c * v[1]])


def ped_with_lidar_at(L, yaw, body):
    """The pose (x, y, yaw) of a pedestrian in whose body frame the point L has the coordinates `body`."""
    p = np.asarray(L, np.float64) - _rot(yaw, body)
    return (p[0], p[1], yaw)


def ped_at(L, bearing, dist, yaw):
    return (L[0] + dist * math.cos(bearing), L[1] + dist * math.sin(bearing), yaw)


def _scene(name, robot, peds):
    """peds: list of ((x, y, yaw), has_legs)."""
    return dict(name=name, robot=tuple(robot), peds=[(tuple(p), int(l)) for p, l in peds])


def lidar_scenes(lidar, crowd=True):
    """The scenes of one lidar (angle_min, angle_last, n_beams): robot and pedestrians at rest."""
    amin, alast, _ = lidar
    L = CENTRE
    out = []
    hd = lambda k: HEADINGS[k % len(HEADINGS)]
    # ---- near: the lidar inside a rectangle, next to a side and to a vertex (vertex threshold 1e-3 m), inside a leg disc
    # and at 1.04 / 1.06 radii from its centre (threshold 1.05), sides seen under 2.9, 3.05 and 3.13 rad (threshold 3.0)
    near = [("inside a rectangle", 0.7, (0.05, -0.03), 0),
            ("0.5 mm from a side", 2.1, (0.1, HALF[1] + 0.0005), 0),
            ("2 mm from a side", -1.3, (-0.07, -HALF[1] - 0.002), 0),
            ("0.5 mm from a vertex", 0.4, (HALF[0] + 0.0005 * math.sqrt(0.5), HALF[1] + 0.0005 * math.sqrt(0.5)), 0),
            ("2 mm from a vertex", 3.9, (-HALF[0] - 0.002 * math.sqrt(0.5), HALF[1] + 0.002 * math.sqrt(0.5)), 0),
            ("inside a leg disc", 1.1, (LEGS[0][0] + 0.01, LEGS[0][1] - 0.005), 1),
            ("1.04 radii from a leg", -2.2, (LEGS[1][0] + 1.04 * LEG_R * math.cos(0.8), LEGS[1][1] + 1.04 * LEG_R * math.sin(0.8)), 1),
            ("1.06 radii from a leg", 2.9, (LEGS[0][0] + 1.06 * LEG_R * math.cos(-2.0), LEGS[0][1] + 1.06 * LEG_R * math.sin(-2.0)), 1)]
    for d in (2.9, 3.05, 3.13):                         # on the side's bisector, 3 cm off its middle: d = 2 atan(0.22 / h) roughly
        near.append(("a side under %.2f rad" % d, 0.9 + d, (0.03, HALF[1] + HALF[0] / math.tan(0.5 * d)), 0))
    for k, (name, yaw, body, legs) in enumerate(near):
        out.append(_scene("near: " + name, (L[0], L[1], hd(k)), [(ped_with_lidar_at(L, yaw, body), legs)]))
    # ---- far: the nearest point of a side / of a leg disc at range_max - 1 cm, range_max, rcull -+ 1 mm, rcull + 0.5 m
    # (towards the hall's corners, where the walls are 5 m away).  A pedestrian facing away along its bearing shows the
    # side x = -0.22 at dist - 0.22 and its left leg nearest.
    for k, (name, D) in enumerate((("range_max - 1 cm", RANGE_MAX - 0.01), ("range_max", RANGE_MAX), ("rcull - 1 mm", RCULL - 0.001),
                                   ("rcull + 1 mm", RCULL + 0.001), ("rcull + 0.5 m", RCULL + 0.5))):
        yaw = hd(k + 3)
        b1, b2 = amin + yaw + 0.25 * (alast - amin), amin + yaw + 0.8 * (alast - amin)     # both inside the field of view
        rect = ped_at(L, b1, D + HALF[0], b1)
        leg = ped_at(L, b2, -LEGS[1][0] + math.sqrt((D + LEG_R) ** 2 - LEGS[1][1] ** 2), b2)
        out.append(_scene("far: a side and a leg at " + name, (L[0], L[1], yaw), [(rect, 0), (leg, 1)]))
    # ---- bearing: for every heading, primitives on the first and the last beam's bearing, opposite to the first beam (the
    # [-pi, pi) fold of the relative bearing), straddling each end of the field of view, and wholly inside the blind sector
    fov = alast - amin
    blind = amin + 0.5 * (fov + 2 * math.pi) if 0 < fov < 2 * math.pi - 0.5 else amin + math.pi + 0.3
    for k, yaw in enumerate(HEADINGS):
        rel = [amin, alast, amin + math.pi, amin - 0.06, alast + 0.06, blind, amin + math.pi - 1e-4]
        peds = [(ped_at(L, yaw + r, 1.1 + 0.27 * i, 0.3 + 1.7 * i + k), (i + k) % 2) for i, r in enumerate(rel)]
        out.append(_scene("bearing: heading %.4f" % yaw, (L[0], L[1], yaw), peds))
    # ---- crowd: 64 pedestrians in two rings, every second one with legs -> 128 sides and 64 discs with cfg.lidar_legs, 256 sides without
    if crowd:
        peds = [(ped_at(L, 0.013 + 2 * math.pi * i / 32, 1.3 if i < 32 else 2.2, 0.37 * i), i % 2) for i in range(64)]
        out.append(_scene("crowd: two rings of 32", (L[0], L[1], 0.4), peds))
    return out


def lidar_world(cfg, scenes, origin=(0.0, 0.0)):
    """Host arrays of the lidar scenes: everything at rest, NAVSIM_PED_EXTERNAL with zero commands.  cfg supplies n_envs
    (= len(scenes)), max_peds, max_waypoints, n_spawn = 1; `origin` shifts every position (set cfg.origin_x / _y to it)."""
    E, N, P = cfg.n_envs, cfg.max_peds, cfg.max_waypoints
    assert E == len(scenes) and cfg.n_spawn == 1
    o = np.asarray(origin, np.float64)
    a = _blank(E, N, P)
    for e, sc in enumerate(scenes):
        x, y, yaw = sc["robot"]
        a["robot_pose"][e] = (x + o[0], y + o[1], yaw)
        a["robot_goal"][e] = (x + o[0] + 2.0, y + o[1] + 1.0)
        assert len(sc["peds"]) <= N
        a["n_peds"][e] = len(sc["peds"])
        for i, ((px, py, pyaw), legs) in enumerate(sc["peds"]):
            a["ped_pose"][e, i] = (px + o[0], py + o[1], pyaw)
            a["ped_has_legs"][e, i] = legs
            a["ped_waypoints"][e, i, 0] = (px + o[0], py + o[1])
    return _finish(a)


def _blank(E, N, P):
    return dict(scan_noise_std=np.zeros(E, np.float32), robot_pose=np.zeros((E, 3)), robot_goal=np.zeros((E, 2)),
                prev_action=np.zeros((E, 2)), prev_pose=np.zeros((E, 3)), n_hist=np.zeros(E, np.int32),
                episode=np.zeros(E, np.int64), steps=np.zeros(E, np.int64), spawn_pose=np.zeros((E, 1, 3)),
                spawn_goal=np.zeros((E, 1, 2)), n_peds=np.zeros(E, np.int32), ped_pose=np.zeros((E, N, 3)),
                ped_vel=np.zeros((E, N, 2)), ped_prev_yaw=np.zeros((E, N)), ped_dist=np.zeros((E, N, 3)),
                ped_v_pref=np.full((E, N), 0.4), ped_has_legs=np.zeros((E, N), np.uint8),
                ped_waypoints=np.zeros((E, N, P, 2)), ped_n_waypoints=np.ones((E, N), np.int32),
                ped_cmd=np.zeros((E, N, 2)), ped_goal=np.zeros((E, N, 2)))


def _finish(a):
    a["prev_pose"][:] = a["robot_pose"]
    a["spawn_pose"][:, 0] = a["robot_pose"]             # one entry, the robot's own place: within 10 m of every pedestrian, so
    a["spawn_goal"][:, 0] = a["robot_goal"]             # a pedestrian at its final waypoint draws no new goal from the table
    a["ped_goal"][:] = a["ped_waypoints"][:, :, 0]
    return a


# ---- social-force scenes -------------------------------------------------------------------------------------------------------
# A pedestrian: dict(p=(x, y), v=(vx, vy), yaw=, v_pref=, wp=(x, y)).  expect: the branches the scene is there for, as
# (kind, i, j) with j = n for the robot and j = None for a branch of pedestrian i alone; kinds as ped_edge_f64.sfm_step reports
# them.  nudge: the pedestrian whose y moves by 1e-6 m in the perturbed twin, which must take none of the expected branches.
def _p(p, v=(0.0, 0.0), v_pref=0.4, wp=None, yaw=0.3):
    wp = (p[0] + 2.0, p[1] + 1.5) if wp is None else wp
    return dict(p=tuple(p), v=tuple(v), v_pref=v_pref, wp=tuple(wp), yaw=yaw)


def _cell(i, j, fx=0.37, fy=0.61):
    """a point inside cell (column i, row j)"""
    return ((i + fx) * RES, (j + fy) * RES)


def _cloud(n, seed, lo=1.2, hi=6.8):
    """n walking pedestrians on a jittered 8 x 8 grid: no two near each other by accident, none at rest"""
    rng = np.random.default_rng(seed)
    slots = rng.permutation(64)[:n]
    out = []
    for s in slots:
        gx, gy = s % 8, s // 8
        p = (lo + (hi - lo) * (gx + rng.uniform(0.2, 0.8)) / 8, lo + (hi - lo) * (gy + rng.uniform(0.2, 0.8)) / 8)
        a, sp = rng.uniform(0, 2 * math.pi), rng.uniform(0.1, 0.5)
        out.append(_p(p, (sp * math.cos(a), sp * math.sin(a)), v_pref=rng.uniform(0.2, 0.6),
                      wp=(rng.uniform(lo, hi), rng.uniform(lo, hi)), yaw=rng.uniform(0, 2 * math.pi)))
    return out


ROBOT = (6.5125, 3.0, 0.6)          # on the row y = 3 of the scenes whose pedestrians stand still: dy is an exact 0 there


# seeds of the clouds whose default leaves a pair within 1e-3 rad of theta = 0 as placed (searched upwards from 1000; with
# 64 pedestrians there are 4 160 ordered pairs and about one seed in four is clear of it)
CLOUD_SEEDS = {"63 of 64 pedestrians": 1012, "64 of 64 pedestrians": 1012, "n_peds above max_peds (64)": 1012,
               "7 of 11 pedestrians (ragged)": 1000}


def sfm_scenes(max_peds, seeds=None):
    N = max_peds
    S = []

    def add(name, peds, expect=(), nudge=None, robot=ROBOT, n_peds=None):
        S.append(dict(name=name, robot=robot, peds=peds, expect=list(expect), nudge=nudge,
                      n_peds=len(peds) if n_peds is None else n_peds))
    walk = _p((2.3, 5.1), (0.2, 0.15))
    # the same velocity, preferred speed and waypoint too: the two stay one point for all three steps.  (With different
    # velocities they part along v_j - v_i, so in the second step the interaction vector lambda (v_i - v_j) + d is parallel
    # to d by construction: theta = 0 up to rounding, exactly the discontinuity no scene may sit on.)
    add("two pedestrians at one point", [_p((3.0, 4.2), (0.3, 0.1)), _p((3.0, 4.2), (0.3, 0.1)), walk],
        [("coincident", 0, 1), ("coincident", 1, 0)], nudge=1)
    add("a pedestrian at the robot's point", [_p(ROBOT[:2], (0.1, 0.3)), walk], [("coincident", 0, 2)], nudge=0)
    # lambda (v_i - v_j) + d = 0 exactly: d = (1, 0), v_i = 0, v_j = (0.5, 0); seen from j, d = (-1, 0) and the sum is 0 again
    add("vanishing interaction vector", [_p((3.0, 3.0)), _p((4.0, 3.0), (0.5, 0.0))],
        [("il0", 0, 1), ("il0", 1, 0), ("theta0", 0, 2), ("theta0", 1, 2)], nudge=1)
    add("head-on pair", [_p((2.0, 3.0), (0.4, 0.0)), _p((4.0, 3.0), (-0.4, 0.0))],
        [("theta0", 0, 1), ("theta0", 1, 0), ("theta0", 0, 2), ("theta0", 1, 2)], nudge=1)
    # (no perturbed twin: between two agents at rest lambda (v_i - v_j) + d is d itself, theta is 0 wherever they stand, and
    # off the row only the rounding of a cross product would decide its sign)
    add("pair at rest", [_p((2.5, 3.0)), _p((3.75, 3.0))],
        [("theta0", 0, 1), ("theta0", 1, 0), ("theta0", 0, 2), ("theta0", 1, 2)])
    add("a pedestrian on its waypoint", [_p((3.1, 4.4), (0.2, 0.1), wp=(3.1, 4.4)), walk], [("at_waypoint", 0, None)], nudge=0)
    add("v_pref = 0", [_p((3.3, 4.1), (0.2, -0.3), v_pref=0.0), walk], [("clamp", 0, None), ("heading_kept", 0, None)])
    add("a speed that must clamp", [_p((3.3, 4.6), (2.0, 1.0), v_pref=0.3), walk], [("clamp", 0, None)])
    lo, hi = RING, SIZE - RING - 1
    add("first and last free cells of a row and of a column",
        [_p(_cell(lo, 80), (0.1, 0.2)), _p(_cell(hi, 81), (-0.1, 0.2)), _p(_cell(79, lo), (0.2, 0.1)), _p(_cell(82, hi), (0.2, -0.1))],
        [("saturated", i, None) for i in range(4)])
    add("pedestrians in wall cells", [_p(_cell(0, 80), (0.1, 0.2)), _p(_cell(2, 3), (0.2, 0.1)), _p(_cell(SIZE - 1, SIZE - 1), (-0.2, 0.1)),
                                      _p(_cell(RING - 1, 40), (0.1, -0.2)), _p(_cell(100, SIZE - RING), (0.15, 0.1))],
        [("flat_field", 0, None), ("flat_field", 1, None), ("flat_field", 2, None), ("saturated", 3, None), ("saturated", 4, None)])
    add("pedestrians outside the map on each side", [_p((-1.0, 4.1), (0.1, 0.2)), _p((9.0, 3.7), (-0.1, 0.2)), _p((4.2, -1.0), (0.2, 0.1)),
                                                     _p((3.6, 9.0), (0.2, -0.1)), _p((-0.7, -0.4), (0.1, 0.1)), _p((8.6, 8.9), (0.1, -0.1))],
        [("flat_field", i, None) for i in range(6)])
    counts = [c for c in (1, 2, 3, N - 1, N) if 1 <= c <= N]
    seed = lambda name, default: (seeds or CLOUD_SEEDS).get(name, default)
    for c in sorted(set(counts)):
        name = "%d of %d pedestrians" % (c, N)
        add(name, _cloud(c, seed(name, 100 + c)))
    add("n_peds = 0", _cloud(min(3, N), 7), n_peds=0)
    name = "n_peds above max_peds (%d)" % N
    add(name, _cloud(N, seed(name, 8)), n_peds=N + 6)
    if N < 20:                                              # ragged counts in one pack of arenas
        for c in (5, N - 4, 4, N - 1, 6):
            name = "%d of %d pedestrians (ragged)" % (c, N)
            add(name, _cloud(c, seed(name, 200 + c)))
    return S


def sfm_world(cfg, scenes, nudge=False):
    """Host arrays of the social-force scenes (NAVSIM_PED_SFM).  nudge=True: the perturbed twin, the scene's `nudge`
    pedestrian moved by 1e-6 m in y (scenes without one unchanged)."""
    E, N, P = cfg.n_envs, cfg.max_peds, cfg.max_waypoints
    assert E == len(scenes) and cfg.n_spawn == 1
    a = _blank(E, N, P)
    for e, sc in enumerate(scenes):
        a["robot_pose"][e] = sc["robot"]
        a["robot_goal"][e] = (sc["robot"][0] - 3.0, sc["robot"][1] + 2.0)
        a["n_peds"][e] = sc["n_peds"]
        assert len(sc["peds"]) <= N
        for i, p in enumerate(sc["peds"]):
            a["ped_pose"][e, i] = (p["p"][0], p["p"][1], p["yaw"])
            a["ped_vel"][e, i] = p["v"]
            a["ped_v_pref"][e, i] = p["v_pref"]
            a["ped_waypoints"][e, i, 0] = p["wp"]
            a["ped_has_legs"][e, i] = i % 2
        if nudge and sc["nudge"] is not None:
            a["ped_pose"][e, sc["nudge"], 1] += 1e-6
    return _finish(a)


SFM_ACTION = (0.2, 0.1)             # the robot drives on: from the second step on it has a velocity in the social force
