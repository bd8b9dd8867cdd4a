"""Inputs and comparisons shared by tests/test_orca_reference.py (the CPU oracle) and tests/test_gpu_orca_reference.py (both
kernels): the random worlds, the obstacle scene, the degenerate table, arenas of pedestrians made of the same scenes, and
the comparison of an ORCA answer with the float64 reference of tests/orca_f64.py.  numpy + orca_f64 only."""
import numpy as np

import orca_f64 as f64

ORCA_P = dict(time_step=0.25, neighbor_dist=10.0, time_horizon=5.0, time_horizon_obst=5.0, max_neighbors=10)   # orca.py:62-65
RADIUS = 0.301
QUERIES = 1500
# box side (m), agents per query, seed, parameters that differ from ORCA_P.  The 6 m world looks 1.5 m far and keeps 3
# neighbours: that is where neighbor_dist rejects, the list is truncated and a later, nearer neighbour displaces an entry.
WORLDS = ((12.0, 8, 101, {}),
          (6.0, 12, 102, dict(neighbor_dist=1.5, max_neighbors=3)),
          (3.0, 12, 103, {}),
          (2.0, 16, 104, {}))

# ---- bounds: four times the worst value the float32 CPU oracle showed against the float64 reference over the committed
# inputs (the four worlds, the obstacle scene, the pedestrian arenas), rounded up to one digit.  The figures themselves are
# in the docstrings of tests/test_orca_reference.py and in DESIGN.md section 5.
VEL_BOUND = 2e-5               # feasible: |velocity - optimum|, m/s (worst seen 3.03e-6)
PEN_BOUND = 4e-5               # infeasible, well-conditioned: largest penetration - minimax value, m/s (7.94e-6)
SPEED_BOUND = 4e-3             # infeasible, well-conditioned: speed - max_speed, m/s (8.28e-4)
CLEAR_BOUND = 3e-6             # obstacles: how far the swept disc may enter a polygon, m (5.97e-7)
MIN_DET = 0.01                 # well-conditioned: smallest |det| over pairs of half-plane directions
MIN_MARGIN = 1e-5              # a query nearer than this to a discrete decision is not compared
MAX_SKIP_FEASIBLE = 0.01       # share of feasible queries the margin may exclude
MAX_SKIP_INFEASIBLE = 0.40     # share of infeasible queries the conditioning may exclude

BOXES = np.array([[[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]],
                  [[4.0, 1.0], [3.0, 1.0], [3.0, 0.0], [4.0, 0.0]]])                   # counter-clockwise


def world(box, n, seed, queries=QUERIES):
    """-> agents [Q,n,6], pref_vel [Q,2]"""
    rng = np.random.default_rng(seed)
    ag = np.zeros((queries, n, 6))
    ag[..., :2] = rng.uniform(0.0, box, (queries, n, 2))
    ag[..., 2:4] = rng.uniform(-0.6, 0.6, (queries, n, 2))
    ag[..., 4] = RADIUS
    ag[..., 5] = rng.uniform(0.3, 1.0, (queries, 1))
    return ag, rng.uniform(-1.2, 1.2, (queries, 2))


def params(**kw):
    return dict(ORCA_P, **kw)


def obstacle_scene(n, seed, queries):
    """Agent 0 around the two boxes with more than 1 mm of clearance, n - 1 other agents near it -> agents, pref_vel"""
    rng = np.random.default_rng(seed)
    ag = np.zeros((0, n, 6)); pv = np.zeros((0, 2))
    while len(ag) < queries:
        a = np.zeros((queries, n, 6))
        a[:, 0, :2] = rng.uniform([-2.5, -2.5], [5.5, 2.5], (queries, 2))
        a[:, 1:, :2] = a[:, :1, :2] + rng.uniform(-3.0, 3.0, (queries, n - 1, 2))
        a[..., 2:4] = rng.uniform(-0.6, 0.6, (queries, n, 2))
        a[..., 4] = RADIUS
        a[..., 5] = rng.uniform(0.3, 1.0, (queries, 1))
        p = rng.uniform(-1.2, 1.2, (queries, 2))
        a32 = a.astype(np.float32).astype(np.float64)
        inside = ((a32[:, 0, None, :2] > BOXES.min(1)[None]) & (a32[:, 0, None, :2] < BOXES.max(1)[None])).all(-1).any(-1)
        keep = ~inside & (f64.swept_clearance(a32[:, 0, :2], np.zeros((queries, 2)), RADIUS, 0.0, BOXES) > 1e-3)
        ag = np.concatenate([ag, a[keep]]); pv = np.concatenate([pv, p[keep]])
    return ag[:queries], pv[:queries]


def clipped(pref_vel, max_speed):
    sp = np.sqrt((pref_vel ** 2).sum(1))
    return pref_vel * np.where(sp > max_speed, max_speed / np.maximum(sp, 1e-300), 1.0)[:, None]


# name, agents [2,6] (px, py, vx, vy, radius, max_speed), pref_vel
DEGENERATE = (
    ("coincident agents, equal velocity", [[0, 0, 0.2, 0.1, 0.3, 1.0], [0, 0, 0.2, 0.1, 0.3, 1.0]], [0.5, 0.25]),
    ("coincident agents, different velocity", [[0, 0, 0.3, 0.0, 0.3, 1.0], [0, 0, -0.2, 0.0, 0.3, 1.0]], [0.5, 0.25]),
    ("exactly touching agents", [[0, 0, 0.0, 0.0, 0.25, 1.0], [0.5, 0, 0.0, 0.0, 0.25, 1.0]], [0.5, 0.0]),
    ("relative velocity on the apex (w = 0)", [[0, 0, 0.5, 0.0, 0.25, 1.0], [2.5, 0, 0.0, 0.0, 0.25, 1.0]], [0.5, 0.0]),
    ("nothing moves, far apart", [[0, 0, 0.0, 0.0, 0.3, 1.0], [4.0, 1.0, 0.0, 0.0, 0.3, 1.0]], [0.0, 0.0]),
    ("max_speed 0", [[0, 0, 0.2, 0.1, 0.3, 0.0], [1.0, 0.25, -0.2, 0.0, 0.3, 0.0]], [0.5, 0.25]),
)


# what the oracle answers today (the float32 values, exactly)
DEGENERATE_ANSWERS = np.array([[0.5, 0.25], [1.0, 0.0], [0.0, 0.0], [float.fromhex("0x1.f5c29p-2"), float.fromhex("-0x1.91530ap-5")],
                               [0.0, 0.0], [0.0, 0.0]])


def degenerate_batch():
    return (np.array([d[1] for d in DEGENERATE], np.float64), np.array([d[2] for d in DEGENERATE], np.float64))


def tie_batch(third, queries=200):
    """Agent 0 at the origin between two agents at +d and -d, exactly equally far in float32, with different velocities.
    third False: a list of one entry -- the tie goes to the first of the list.  third True: a list of two entries and a
    third, nearer agent behind them, which pushes the second of the two out.  -> parameters, agents, pref_vel"""
    rng = np.random.default_rng(105 + third)
    n = 4 if third else 3
    ag = np.zeros((queries, n, 6))
    d = rng.uniform(-2.0, 2.0, (queries, 2)).astype(np.float32).astype(np.float64)
    ag[:, 1, :2] = d; ag[:, 2, :2] = -d
    if third:
        ag[:, 3, :2] = 0.75 * d[:, ::-1] * [1.0, -1.0]
    ag[..., 2:4] = rng.uniform(-0.6, 0.6, (queries, n, 2))
    ag[..., 4] = RADIUS
    ag[..., 5] = rng.uniform(0.3, 1.0, (queries, 1))
    return params(max_neighbors=n - 2), ag, rng.uniform(-1.2, 1.2, (queries, 2))


def tie_check(answer):
    for third in (False, True):
        p, ag, pv = tie_batch(third)
        swapped = ag.copy(); swapped[:, [1, 2]] = ag[:, [2, 1]]
        first, second = f64.solve(p, ag, pv), f64.solve(p, swapped, pv)
        v = answer(p, ag, pv, None)
        with np.errstate(invalid="ignore"):
            told = first["feasible"] & second["feasible"] & (np.sqrt(((first["vel"] - second["vel"]) ** 2).sum(1)) > 1e-3)
            err = np.sqrt(((v - first["vel"]) ** 2).sum(1))[told]
        print("ties, %s: %d of %d queries tell the two neighbours apart; worst |v - optimum with the first of the list| %.3g"
              % ("a nearer third agent follows" if third else "room for one", told.sum(), len(v), err.max()))
        assert told.sum() >= 20 and err.max() <= VEL_BOUND


# ---- the comparison -----------------------------------------------------------------------------------------------------
def measure(res, vel):
    """An implementation's velocities vel [Q,2] against the float64 reference's result res -> per-query figures."""
    vel = np.asarray(vel, np.float64)
    feas = res["feasible"]
    wide = res["margin"] >= MIN_MARGIN
    well = ~feas & wide & (res["min_det"] >= MIN_DET)
    with np.errstate(invalid="ignore"):
        m = dict(finite=np.isfinite(vel).all(1), feasible=feas, compared=feas & wide, well=well, ill=~feas & ~well,
                 err=np.sqrt(((vel - res["vel"]) ** 2).sum(1)), pen=f64.penetration(res, vel) - res["minimax"],
                 over=np.sqrt((vel ** 2).sum(1)) - res["max_speed"],
                 off=np.sqrt(((vel - res["minimax_vel"]) ** 2).sum(1)))
    return m


def judge(measures, what, caps=True):
    """Prints the worst figures and the shares left out over a list of measure() results and asserts the bounds above (and,
    with caps, how much may be left out).  -> the figures"""
    m = {k: np.concatenate([x[k] for x in measures]) for k in measures[0]}
    assert m["finite"].all(), what
    worst = lambda v, s, init=0.0: float(v[s].max(initial=init))
    fig = dict(n_feasible=int(m["feasible"].sum()), n_infeasible=int((~m["feasible"]).sum()),
               feasible_compared=int(m["compared"].sum()), infeasible_compared=int(m["well"].sum()),
               vel_err=worst(m["err"], m["compared"]), pen_excess=worst(m["pen"], m["well"]),
               overspeed=worst(m["over"], m["well"], -np.inf), ill_overspeed=worst(m["over"], m["ill"], -np.inf),
               ill_distance=worst(m["off"], m["ill"]), ill_pen_excess=worst(m["pen"], m["ill"]))
    skip_f = 1.0 - fig["feasible_compared"] / max(fig["n_feasible"], 1)
    skip_i = 1.0 - fig["infeasible_compared"] / max(fig["n_infeasible"], 1)
    print("%s: feasible %d (compared %d, %.2f %% left out), worst |v - optimum| %.3g; infeasible %d (compared %d, %.1f %% left "
          "out), worst penetration above the minimax value %.3g, worst speed - max_speed %.3g; ill-conditioned, not compared: "
          "speed - max_speed up to %.3g, %.3g from the optimum, penetration %.3g above it"
          % (what, fig["n_feasible"], fig["feasible_compared"], 100 * skip_f, fig["vel_err"], fig["n_infeasible"],
             fig["infeasible_compared"], 100 * skip_i, fig["pen_excess"], fig["overspeed"], fig["ill_overspeed"],
             fig["ill_distance"], fig["ill_pen_excess"]))
    if caps:
        assert skip_f <= MAX_SKIP_FEASIBLE and skip_i <= MAX_SKIP_INFEASIBLE, what
    assert fig["vel_err"] <= VEL_BOUND, what
    assert fig["pen_excess"] <= PEN_BOUND and fig["overspeed"] <= SPEED_BOUND, what
    return fig


def crowd_batches(name):
    """The batches navsim_crowd_orca is given -> [(parameters, agents, pref_vel, n_agents or None)].
    'worlds': the first 500 queries of each of the four worlds.  'ragged': the first 1000 of the 6 m and of the 3 m world
    with 1 .. 12 agents per query, a list of 3 and a range of 2.5 m."""
    if name == "worlds":
        return [(params(**kw),) + tuple(x[:500] for x in world(box, n, seed)) + (None,) for box, n, seed, kw in WORLDS]
    assert name == "ragged"
    out = []
    for box, n, seed, _ in WORLDS[1:3]:
        ag, pv = world(box, n, seed)
        na = np.random.default_rng(seed + 50).integers(1, n + 1, 1000).astype(np.int32)
        na[:3] = 1
        out.append((params(neighbor_dist=2.5, max_neighbors=3), ag[:1000], pv[:1000], na))
    return out


def crowd_check(name, answer, least=10):
    """answer(parameters, agents, pref_vel, n_agents) -> velocities, for every batch of `name`; then bounds and census."""
    measures, total = [], {}
    for p, ag, pv, na in crowd_batches(name):
        res = f64.solve(p, ag, pv, na)
        measures.append(measure(res, answer(p, ag, pv, na)))
        total = add_census(total, census(res))
    fig = judge(measures, "navsim_crowd_orca " + name)
    check_census(total, least, "navsim_crowd_orca " + name)
    return fig


CENSUS_KEYS = tuple("class: " + c for c in f64.CLASS_NAMES) + tuple("optimum: " + w for w in f64.WHERE_NAMES) + \
    ("list truncated", "list entry displaced", "neighbor_dist rejects", "infeasible")


def census(res, select=None):
    """How often each half-plane class, optimum location and list event occurs among the queries (select: a mask)."""
    s = np.ones(len(res["feasible"]), bool) if select is None else select
    c = {}
    for k, name in enumerate(f64.CLASS_NAMES):
        c["class: " + name] = int((res["cls"][s] == k).sum())
    for k, name in enumerate(f64.WHERE_NAMES):
        c["optimum: " + name] = int((res["where"][s] == k).sum())
    c["list truncated"] = int(res["truncated"][s].sum())
    c["list entry displaced"] = int(res["displaced"][s].sum())
    c["neighbor_dist rejects"] = int(res["rejected"][s].sum())
    c["infeasible"] = int((~res["feasible"][s]).sum())
    return c


def add_census(a, b):
    return {k: a.get(k, 0) + b.get(k, 0) for k in CENSUS_KEYS}


def check_census(c, least, what):
    print("%s census: %s" % (what, ", ".join("%s %d" % kv for kv in c.items())))
    short = {k: v for k, v in c.items() if v < least}
    assert not short, "%s: fewer than %d of %s" % (what, least, short)


# ---- arenas of pedestrians -----------------------------------------------------------------------------------------------
def ped_arenas(E, N, boxes, seed, n_peds=None, centre=(6.0, 6.0), speed=0.6):
    """One scene per arena: N pedestrians and the robot uniform in a square around `centre` whose side is boxes[e mod
    len(boxes)], velocities U(-speed, speed)^2, v_pref U(0.3, 1.0), one waypoint each at U(-1.2, 1.2)^2 from the pedestrian.
    -> the state arrays navsim_ped_orca reads, as a dict (`waypoint` [E,N,2]: ped_waypoints[:, :, 0] with ped_wp_head 0 and
    ped_n_waypoints 1)."""
    rng = np.random.default_rng(seed)
    box = np.asarray(boxes, np.float64)[np.arange(E) % len(boxes)]
    lo = np.asarray(centre) - box[:, None] / 2
    pose = np.zeros((E, N, 3))
    pose[..., :2] = lo[:, None] + rng.uniform(0.0, 1.0, (E, N, 2)) * box[:, None, None]
    pose[..., 2] = rng.uniform(-np.pi, np.pi, (E, N))
    robot = np.zeros((E, 3))
    robot[:, :2] = lo + rng.uniform(0.0, 1.0, (E, 2)) * box[:, None]
    robot[:, 2] = rng.uniform(-np.pi, np.pi, E)
    return dict(ped_pose=pose, ped_vel=rng.uniform(-speed, speed, (E, N, 2)), ped_v_pref=rng.uniform(0.3, 1.0, (E, N)),
                waypoint=pose[..., :2] + rng.uniform(-1.2, 1.2, (E, N, 2)), robot_pose=robot,
                prev_action=np.stack([rng.uniform(0.0, speed, E), rng.uniform(-0.64, 0.64, E)], 1),
                n_peds=np.full(E, N, np.int32) if n_peds is None else np.asarray(n_peds, np.int32))


def ragged(E, N):
    """n_peds with 0, 1 and N among them (N = 8: what tests/test_gpu_ped_orca.py uses)"""
    n = np.array([(3 * e + 2) % (N + 1) for e in range(E)], np.int32)
    n[1] = N - 2; n[4] = 0; n[7] = 1; n[E - 1] = 0
    return n


_VARIANTS = ({}, dict(robot_visible=0), dict(max_neighbors=0), dict(max_neighbors=1), dict(max_neighbors=3),
             dict(neighbor_dist=1.5), dict(max_neighbors=3, neighbor_dist=1.5, robot_visible=0))
# shape -> E, N, ragged n_peds, the box sides the arenas cycle through, and one dict of parameters per call (every call draws
# new scenes and starts the cycle of boxes one further)
PED_CASES = {
    "45x8": (45, 8, True, (2.0, 3.0, 6.0, 10.0), _VARIANTS),
    "11x12": (11, 12, False, (2.5, 3.5, 6.0, 10.0), _VARIANTS + _VARIANTS),
    "7x20": (7, 20, False, (3.0, 5.0, 8.0, 11.0), ({},) * 7 + (dict(neighbor_dist=2.0),) * 2),
    "5x33": (5, 33, False, (4.0, 6.0, 9.0, 11.0), ({},) * 7 + (dict(neighbor_dist=2.0),) * 2),
    "4x63": (4, 63, False, (5.0, 7.0, 9.0, 11.0), (dict(max_neighbors=10),) * 4 + (dict(max_neighbors=10, neighbor_dist=1.2),) * 3),
}


def ped_calls(name):
    """-> E, N, [(scene, parameters that differ)] of one shape"""
    E, N, rag, boxes, variants = PED_CASES[name]
    calls = []
    for c, kw in enumerate(variants):
        b = tuple(boxes[(c + k) % len(boxes)] for k in range(len(boxes)))
        calls.append((ped_arenas(E, N, b, 7000 + 100 * N + c, ragged(E, N) if rag else None), kw))
    return E, N, calls


def ped_state(s, max_waypoints):
    """The arrays of a scene as the simulator holds them (what differs from `s`: the routes)."""
    E, N = s["ped_v_pref"].shape
    wp = np.zeros((E, N, max_waypoints, 2))
    wp[:, :, 0] = s["waypoint"]
    a = {k: v for k, v in s.items() if k != "waypoint"}
    a.update(ped_waypoints=wp, ped_n_waypoints=np.ones((E, N), np.int32), ped_wp_head=np.zeros((E, N), np.int32))
    return a


def lane_sets(E, N, env):
    """Which queries (by their arena `env`) sit behind the first arena of their wavefront, and which in a last, partly
    filled wavefront (kernels_ped_orca.hpp: a wavefront serves 64 / N whole arenas, one when N > 32)."""
    G = 64 // N if N <= 32 else 1
    return (env % G) > 0, (env >= (E // G) * G) if E % G else np.zeros(len(env), bool)


def ped_queries(s, p):
    """The ORCA queries of the arenas s (include/navsim.h navsim_ped_orca, steps 2 and 3), in float64 with libm's cos / sin.
    p: ped_radius, robot_radius, safety_space, robot_visible.  -> env [Q], ped [Q], agents [Q,A,6], n_agents [Q],
    pref_vel [Q,2], theta [Q]"""
    E, N = s["ped_v_pref"].shape
    A = N + (1 if p["robot_visible"] else 0)
    r_ped, r_rob = (p["ped_radius"] + 0.01) + p["safety_space"], (p["robot_radius"] + 0.01) + p["safety_space"]
    env, ped, agents, n_agents = [], [], [], []
    for e in range(E):
        n = int(min(max(s["n_peds"][e], 0), N))
        rows = np.zeros((n + 1, 6))
        rows[:n, :2] = s["ped_pose"][e, :n, :2]; rows[:n, 2:4] = s["ped_vel"][e, :n]; rows[:n, 4] = r_ped
        rows[n, :2] = s["robot_pose"][e, :2]
        rows[n, 2:4] = s["prev_action"][e, 0] * np.array([np.cos(s["robot_pose"][e, 2]), np.sin(s["robot_pose"][e, 2])])
        rows[n, 4] = r_rob
        m = n + (1 if p["robot_visible"] else 0)
        for i in range(n):
            q = np.zeros((A, 6))
            q[:m] = rows[[i] + [j for j in range(m) if j != i]]
            q[:, 5] = s["ped_v_pref"][e, i]
            env.append(e); ped.append(i); agents.append(q); n_agents.append(m)
    env, ped = np.asarray(env, np.int64), np.asarray(ped, np.int64)
    g = s["waypoint"][env, ped] - s["ped_pose"][env, ped, :2]
    gl = np.sqrt((g ** 2).sum(1))
    pref = np.where((gl > 1.0)[:, None], g / np.maximum(gl, 1e-300)[:, None], g)
    return env, ped, np.asarray(agents).reshape(-1, A, 6), np.asarray(n_agents, np.int64), pref, s["ped_pose"][env, ped, 2]


def cmd_velocity(cmd, theta, time_step):
    """The velocity a command (speed, omega) turns a pedestrian of heading theta into: speed (cos, sin)(theta + omega dt)."""
    ang = theta + cmd[:, 1] * time_step
    return cmd[:, :1] * np.stack([np.cos(ang), np.sin(ang)], 1)


def ped_reference(s, p):
    """The float64 reference for every live pedestrian of the scene s under the parameters p of navsim_ped_orca
    -> env [Q], ped [Q], theta [Q], the result of orca_f64.solve"""
    env, ped, agents, n_agents, pref, theta = ped_queries(s, p)
    return env, ped, theta, f64.solve(p, agents, pref, n_agents)


def ped_check(name, answer, least=10):
    """Every call of the shape `name`: answer(scene, parameters that differ) -> (ped_cmd [E,N,2], time_step, the full
    parameters) is compared with the float64 reference; then the bounds, the census and the lanes' census of the shape."""
    E, N, calls = ped_calls(name)
    G = 64 // N if N <= 32 else 1
    measures, total = [], {}
    lanes = {"infeasible behind the wavefront's first arena": 0, "displaced behind the wavefront's first arena": 0,
             "infeasible in the last, partial wavefront": 0, "displaced in the last, partial wavefront": 0}
    for s, kw in calls:
        cmd, time_step, p = answer(s, kw)
        env, ped, theta, res = ped_reference(s, p)
        measures.append(measure(res, cmd_velocity(cmd[env, ped], theta, time_step)))
        total = add_census(total, census(res))
        behind, last = lane_sets(E, N, env)
        lanes["infeasible behind the wavefront's first arena"] += int((~res["feasible"] & behind).sum())
        lanes["displaced behind the wavefront's first arena"] += int((res["displaced"] & behind).sum())
        lanes["infeasible in the last, partial wavefront"] += int((~res["feasible"] & last).sum())
        lanes["displaced in the last, partial wavefront"] += int((res["displaced"] & last).sum())
    fig = judge(measures, "pedestrians " + name)
    check_census(total, least, "pedestrians " + name)
    if G == 1:
        lanes = {k: v for k, v in lanes.items() if "behind" not in k}
    if E % G == 0:
        lanes = {k: v for k, v in lanes.items() if "last" not in k}
    print("pedestrians %s lanes: %s" % (name, ", ".join("%s %d" % kv for kv in lanes.items())))
    short = {k: v for k, v in lanes.items() if v < least}
    assert not short, "pedestrians %s: fewer than %d of %s" % (name, least, short)
    return fig


def ped_full_lists(answer, sample=200):
    """4 arenas of 63 slow pedestrians over 7 m with max_neighbors 63: every list holds all 63 others.  The float64
    reference enumerates 39 711 triples of half-planes per query, so `sample` queries are compared; among 1 953 pairs of
    directions the smallest |det| is below MIN_DET for nearly every query, so how many infeasible queries the conditioning
    leaves out is printed and not capped here."""
    s = ped_arenas(4, 63, (7.0,), 7963, speed=0.15)
    cmd, time_step, p = answer(s, dict(max_neighbors=63))
    env, ped, agents, n_agents, pref, theta = ped_queries(s, p)
    pick = np.random.default_rng(63).choice(len(env), sample, replace=False)
    res = f64.solve(p, agents[pick], pref[pick], n_agents[pick])
    assert (np.isfinite(res["b"]).sum(1) == 63).all()
    fig = judge([measure(res, cmd_velocity(cmd[env[pick], ped[pick]], theta[pick], time_step))], "pedestrians 4x63, lists of 63",
                caps=False)
    print("pedestrians 4x63, lists of 63 census: %s" % census(res))
    assert fig["feasible_compared"] >= 50
    return fig


def ped_degenerate():
    """Four arenas of three pedestrians: two at one pose with zero velocity (what a reset leaves if two spawn on one spot);
    two at one pose with different velocities; a pedestrian exactly on the robot; a pedestrian whose v_pref is 0."""
    s = ped_arenas(4, 3, (4.0,), 7903)
    s["ped_pose"][0, 1] = s["ped_pose"][0, 0]; s["ped_vel"][0] = 0.0
    s["ped_pose"][1, 1] = s["ped_pose"][1, 0]
    s["ped_pose"][2, 0, :2] = s["robot_pose"][2, :2]
    s["ped_v_pref"][3, 0] = 0.0
    return s
