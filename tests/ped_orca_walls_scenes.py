"""Inputs and checks shared by tests/test_ped_orca_walls.py (the oracle composition) and tests/test_gpu_ped_orca_walls.py (the
kernel): the 6 m map, its rectangle list written by hand, arenas of pedestrians on it, the calls both sides answer, the census
over them and the swept-clearance check against tests/orca_f64.py.  numpy + orca_f64 + orca_scenes + the specification."""
import numpy as np

import orca_f64 as f64
import orca_scenes as scenes
import ped_orca_walls_spec as wspec

SIZE, RES = 120, 0.05                                              # 120 x 120 cells of 0.05 m: 6 m
RING = 3
# x0, y0, x1, y1 in cells, inclusive: three boxes on the diagonal, a box and its transpose, and one box whose transposed
# place is free -- what tells x from y
BOXES = ((24, 24, 35, 35), (54, 54, 65, 65), (84, 84, 95, 95), (20, 60, 29, 71), (60, 20, 71, 29), (84, 36, 99, 45))
OFF_DIAGONAL = BOXES[5]
WALLS = ((0, 0, SIZE - 1, RING - 1), (0, SIZE - RING, SIZE - 1, SIZE - 1), (0, RING, RING - 1, SIZE - RING - 1),
         (SIZE - RING, RING, SIZE - 1, SIZE - RING - 1))
# B, how far a swept disc may enter a kept rectangle, by the rule "orca_scenes.CLEAR_BOUND if the worst the oracle shows on
# these scenes is below it, else 4 x the worst seen, to one digit" -- per obstacle horizon, because the oracle's answer to
# that rule depends on it:
#   time_horizon_obst 0.5 and 2 (36 calls, every max_rects): worst 6.86e-7 m -> B = CLEAR_BOUND = 3e-6
#   time_horizon_obst 5 (8 calls, all ten rectangles of the 6 m map in range): the oracle sends 2 of 90 queries of the 3 x 33
#     call INTO a box -- clearance -0.13 and -0.25 m; other seeds give -0.30, the radius itself, in half of their calls -- a
#     box more than 1.2 m away gets no binding half-plane (rvo2's `covered` shortcut over up to 20 obstacle half-planes; the
#     same with max_neighbors = 0).  4 x 0.3 -> B_LONG = 1 m: more than the radius, so at this horizon the check bounds
#     NOTHING and says so; the figures are printed, and include/navsim.h and DESIGN.md section 5 call the case NOT bounded.
B = scenes.CLEAR_BOUND
B_LONG = 1.0


def bound(horizon):
    return B if horizon <= 2.0 else B_LONG


MAX_LEFT_OUT = 0.10


def occupancy(E=1):
    """uint8 [E, SIZE, SIZE] indexed [y][x] like every map of the simulator: the closed ring and the boxes"""
    occ = np.zeros((SIZE, SIZE), np.uint8)
    for x0, y0, x1, y1 in WALLS + BOXES:
        occ[y0:y1 + 1, x0:x1 + 1] = 1
    return np.repeat(occ[None], E, 0)


def hand_list(E=1, order=None):
    """int16 [E, 255, 4]: the ring's four walls and the boxes, zero entries in front, in the middle and behind"""
    rects = np.zeros((E, wspec.LIST_LEN, 4), np.int16)
    slots = (1, 2, 4, 5, 9, 10, 11, 40, 200, 254) if order is None else order
    for s, r in zip(slots, WALLS + BOXES):
        rects[:, s] = r
    return rects


def config(E, N, **kw):
    import ref
    from nav_gym_amd import abi
    return ref.default_config(n_envs=E, map_h=SIZE, map_w=SIZE, max_peds=N, ped_model=abi.PED_EXTERNAL, resolution=RES,
                              origin_x=0.0, origin_y=0.0, time_step=0.2, **kw)


def arenas(E, N, seed, n_peds=None, overlap_share=0.15):
    """orca_scenes.ped_arenas over the free 5.7 m of the map; a pedestrian whose disc of 0.301 m would touch a rectangle is
    drawn again, except a share of them (the census wants discs that overlap a wall)."""
    s = scenes.ped_arenas(E, N, (5.6, 5.0, 4.0, 5.6), seed, n_peds, centre=(3.0, 3.0))
    rng = np.random.default_rng(seed + 1)
    polys = np.array([[[x0 * RES, y0 * RES], [(x1 + 1) * RES, y0 * RES], [(x1 + 1) * RES, (y1 + 1) * RES], [x0 * RES, (y1 + 1) * RES]]
                      for x0, y0, x1, y1 in WALLS + BOXES])
    xy = s["ped_pose"][..., :2].reshape(-1, 2)
    keep = rng.uniform(size=len(xy)) < overlap_share
    for _ in range(200):
        inside = ((xy[:, None] > polys[None, :, 0]) & (xy[:, None] < polys[None, :, 2])).all(-1).any(-1)
        bad = (inside | (f64.swept_clearance(xy, np.zeros_like(xy), 0.301, 0.0, polys) < 0.02)) & ~keep
        if not bad.any():
            break
        xy[bad] = rng.uniform(0.3, 5.7, (int(bad.sum()), 2))
    s["ped_pose"][..., :2] = xy.reshape(E, N, 2)
    s["waypoint"] = s["ped_pose"][..., :2] + rng.uniform(-1.2, 1.2, (E, N, 2))
    return s


# ---- the calls ---------------------------------------------------------------------------------------------------------
# shape -> E, N, ragged n_peds: every lane layout of the kernel (8 arenas per wavefront with a partial last one, 3 per
# wavefront with idle lanes, one per wavefront, 64 per wavefront)
SHAPES = {"7x8": (7, 8, True), "5x20": (5, 20, False), "3x33": (3, 33, False), "64x1": (64, 1, False)}
# max_rects, parameters that differ from ped_orca_spec.params.  Small lists go with short horizons: the swept-clearance check
# leaves a query with dropped > 0 out and may leave out 10 % of all queries, so rectangles are dropped in a minority of the
# queries only (max_rects 1 and 3 at 0.5 s, 8 at 2 s: where two or more, four or more, nine or more rectangles are in range)
VARIANTS = ((8, dict(time_horizon_obst=2.0)), (1, dict(time_horizon_obst=0.5)), (3, dict(time_horizon_obst=0.5)),
            (32, dict(time_horizon_obst=5.0)), (8, dict(time_horizon_obst=0.5)), (32, dict(time_horizon_obst=0.5)),
            (8, dict(time_horizon_obst=2.0, robot_visible=0)), (8, dict(time_horizon_obst=2.0, max_neighbors=0)),
            (32, dict(time_horizon_obst=2.0)), (3, dict(time_horizon_obst=0.5, robot_visible=0)),
            (32, dict(time_horizon_obst=5.0, robot_visible=0)), (1, dict(time_horizon_obst=0.5, max_neighbors=3)))
SEED = 8100


def ragged(E, N):
    n = np.array([(3 * e + 2) % (N + 1) for e in range(E)], np.int32)
    n[1] = N; n[2] = 0; n[E - 1] = 3                               # 0 and N among them; the last, partial wavefront is live
    return n


def calls(shape):
    """-> E, N, [(scene, max_rects, parameters that differ)]"""
    E, N, rag = SHAPES[shape]
    return E, N, [(arenas(E, N, SEED + 100 * N + c, ragged(E, N) if rag else None), K, kw) for c, (K, kw) in enumerate(VARIANTS)]


def state(s, cfg):
    a = scenes.ped_state(s, cfg.max_waypoints)
    a["ped_cmd"] = np.zeros(s["ped_pose"].shape[:2] + (2,))
    return a


def lane_masks(E, N, env):
    behind, last = scenes.lane_sets(E, N, env)
    G = 64 // N if N <= 32 else 1
    return (behind if G > 1 else None), (last if E % G else None)


def census_of(records, least, what, lanes=True):
    """records: [(shape, census of one call)] over every shape -> asserts `least` of every class over all queries and, with
    lanes, over the lanes behind the first arena of their wavefront and over the lanes of a last, partly filled wavefront"""
    total = {}
    for shape, census in records:
        E, N, _ = SHAPES[shape]
        behind, last = lane_masks(E, N, census.query["env"])
        add(total, census.masks)
        if lanes and behind is not None:
            add(total, census.masks, behind, "behind the wavefront's first arena: ")
        if lanes and last is not None:
            add(total, census.masks, last, "in the partial wavefront: ")
    check_census(total, least, what)
    return total


def check_census(total, least, what):
    print("%s census: %s" % (what, ", ".join("%s %d" % kv for kv in total.items())))
    short = {k: v for k, v in total.items() if v < least}
    assert not short, "%s: fewer than %d of %s" % (what, least, short)


def add(total, masks, select=None, prefix=""):
    for k, m in masks.items():
        total[prefix + k] = total.get(prefix + k, 0) + int((m if select is None else m & select).sum())
    return total


# ---- the independent check ----------------------------------------------------------------------------------------------
def swept(census, velocity, horizon):
    """The kept rectangles against the disc swept along `velocity` [Q,2] for `horizon` s, in float64 (orca_f64.swept_clearance)
    -> clearance of the compared queries, how many there are, how many were left out (start clearance <= 1 mm or dropped)"""
    q = census.query
    out, left = [], 0
    for j in range(len(q["env"])):
        polys = q["verts"][j, :q["n_obst"][j]].astype(np.float32).astype(np.float64)
        if len(polys) == 0:
            out.append(np.inf)
            continue
        pos = q["pos"][j:j + 1]
        inside = ((pos > polys[:, 0]) & (pos < polys[:, 2])).all(-1).any()
        start = f64.swept_clearance(pos, np.zeros((1, 2)), q["radius"][j], 0.0, polys)[0]
        if inside or start <= 1e-3 or q["dropped"][j] > 0:
            left += 1
            continue
        out.append(f64.swept_clearance(pos, velocity[j:j + 1], q["radius"][j], float(np.float32(horizon)), polys)[0])
    return np.asarray(out), left


def swept_check(answer, what):
    """answer(shape, call index) -> (ped_cmd [E,N,2], census of the specification, cfg, full parameters) for every call of
    every shape: every query that starts clear by more than 1 mm with nothing dropped holds bound(time_horizon_obst), and at
    most MAX_LEFT_OUT of all queries are left out by those two conditions"""
    worst, n, left = {}, 0, 0
    for shape in SHAPES:
        for c, (K, kw) in enumerate(VARIANTS):
            cmd, census, cfg, p = answer(shape, c)
            q = census.query
            vel = scenes.cmd_velocity(cmd[q["env"], q["ped"]], q["theta"], cfg.time_step)
            h = p["time_horizon_obst"]
            cl, lo = swept(census, vel, h)
            w = float(cl.min(initial=np.inf))
            print("%s %s max_rects %d %s: %d queries, worst %.3g m, %d below -%.1g, %d left out"
                  % (what, shape, K, kw, len(cl), w, int((cl < -B).sum()), B, lo))
            assert w >= -bound(h), (what, shape, K, kw, w)
            worst[h], n, left = min(worst.get(h, np.inf), w), n + len(cl), left + lo
    print("%s: swept clearance of %d queries, worst by time_horizon_obst %s; %d left out (%.1f %%)"
          % (what, n, ", ".join("%g s: %.3g m (bound -%.1g)" % (h, w, bound(h)) for h, w in sorted(worst.items())), left,
             100.0 * left / max(n + left, 1)))
    assert left <= MAX_LEFT_OUT * (n + left), what
    assert n >= 200, what
    return worst
