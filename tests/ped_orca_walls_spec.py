"""The specification of navsim_ped_orca_walls (include/navsim.h) as a composition of the oracle's existing functions: the query
of tests/ped_orca_spec.py (imported, not restated), the selection of the arena's listed rectangles in numpy float32 scalars, and
ref.crowd_orca with one polygon set per query.  numpy + ref + ped_orca_spec only."""
import numpy as np

import ped_orca_spec as spec
import ref

LIST_LEN = 255                                                     # entries 0 .. 254 of a rect_index row are rectangles
CENSUS_KEYS = ("0 edges in range", "1 edge in range", "2 edges in range", "3 or more edges in range", "disc overlaps a wall",
               "nearest feature a corner", "nearest feature a face", "dropped > 0", "walls bind", "walls and an agent bind")


def decode_rows(rows):
    """uint8 [E, R] rect_index rows as read back from the device -> int16 [E, 255, 4] = x0, y0, x1, y1 of every list entry."""
    rows = np.ascontiguousarray(np.asarray(rows, np.uint8)[:, :LIST_LEN * 8])
    return rows.view("<i2").reshape(rows.shape[0], LIST_LEN, 4).copy()


def vertices(cfg, rect):
    """xa, ya, xb, yb of one list entry, float64"""
    x0, y0, x1, y1 = (int(v) for v in rect)
    return (cfg.origin_x + float(x0) * cfg.resolution, cfg.origin_y + float(y0) * cfg.resolution,
            cfg.origin_x + float(x1 + 1) * cfg.resolution, cfg.origin_y + float(y1 + 1) * cfg.resolution)


def select(cfg, rects, px, py, range_sq, max_rects):
    """The max_rects nearest rectangles of the list `rects` [255, 4] strictly inside the range around (px, py), all float32:
    Agent::insertAgentNeighbor's rule over ascending k.  -> (kept list indices in ascending k, in-range count)"""
    f = np.float32
    px, py, range_sq, zero = f(px), f(py), f(range_sq), f(0.0)
    range0 = range_sq
    kept, n_in = [], 0                                             # kept: (d2, k) in ascending distance, ties in list order
    for k in np.flatnonzero(np.asarray(rects[:LIST_LEN]).any(1)):  # all-zero entries are skipped wherever they stand
        x0, y0, x1, y1 = (int(v) for v in rects[k])
        if x1 < x0 or y1 < y0:                                     # (no builder writes one)
            continue
        xa, ya, xb, yb = (f(v) for v in vertices(cfg, rects[k]))
        dx = max(max(f(xa - px), f(px - xb)), zero)
        dy = max(max(f(ya - py), f(py - yb)), zero)
        d2 = f(f(dx * dx) + f(dy * dy))
        n_in += bool(d2 < range0)
        if max_rects > 0 and d2 < range_sq:
            if len(kept) == max_rects:
                kept.pop()
            i = len(kept)
            while i != 0 and d2 < kept[i - 1][0]:
                i -= 1
            kept.insert(i, (d2, int(k)))
            if len(kept) == max_rects:
                range_sq = kept[-1][0]
    return sorted(k for _, k in kept), n_in


class _Recorder(object):
    """Stands in for the module `ref` inside ped_orca_spec for one call: keeps the query ped_orca_spec.ped_orca assembles and
    the oracle's answer to it."""

    def __init__(self):
        self.query = None

    def __getattr__(self, name):
        return getattr(ref, name)

    def crowd_orca(self, params, agents, pref_vel, **kw):
        vel, act = ref.crowd_orca(params, agents, pref_vel, **kw)
        self.query = dict(params=params, agents=np.asarray(agents, np.float64), pref=np.asarray(pref_vel, np.float64),
                          n_agents=np.asarray(kw["n_agents"], np.int32), theta=np.asarray(kw["theta"], np.float64), vel=vel)
        return vel, act


def query(cfg, a, p):
    """ped_orca_spec.ped_orca's own query and answer: -> (cmd, head, the recorded query or None without live pedestrians).
    The module attribute ped_orca_spec.ref is the recorder for the length of the call (ped_orca_spec itself is not edited):
    not re-entrant, and it records nothing if ped_orca_spec ever binds ref.crowd_orca at import -- the assert catches that."""
    rec = _Recorder()
    spec.ref = rec
    try:
        cmd, head, _ = spec.ped_orca(cfg, a, p)
    finally:
        spec.ref = ref
    assert rec.query is not None or not (np.asarray(a["n_peds"]) > 0).any(), "ped_orca_spec no longer calls ref.crowd_orca"
    if rec.query is not None:
        E, N = cfg.n_envs, cfg.max_peds
        live = [(e, i) for e in range(E) for i in range(int(min(max(a["n_peds"][e], 0), N)))]
        rec.query["env"], rec.query["ped"] = (np.asarray(live, np.int64).reshape(-1, 2).T)
    return cmd, head, rec.query


class Census(dict):
    """counts by CENSUS_KEYS; .masks: the same as bool arrays over the queries; .query: env, ped, pos, radius, max_speed, vel
    (the answer), theta, verts [Q, K, 4, 2] and n_obst [Q] (the kept rectangles), dropped [Q]"""


def _census(q, verts, n_obst, dropped, horizon, vel, vel_alone):
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    pos, radius, ms = f32(q["agents"][:, 0, :2]), f32(q["agents"][:, 0, 4]), f32(q["agents"][:, 0, 5])
    Q = len(pos)
    rng = float(np.float32(horizon)) * ms + radius
    edges, near, corner, face = np.zeros(Q, np.int64), np.full(Q, np.inf), np.zeros(Q, bool), np.zeros(Q, bool)
    for j in range(Q):
        for o in range(int(n_obst[j])):
            v = f32(verts[j, o])
            for k in range(4):
                a, b = v[k], v[(k + 1) % 4]
                ab, ap = b - a, pos[j] - a
                if ab[0] * ap[1] - ab[1] * ap[0] < 0.0:                          # strictly on the outer side of a -> b
                    t = min(max(float(ap @ ab) / float(ab @ ab), 0.0), 1.0)
                    edges[j] += bool(np.hypot(*(ap - t * ab)) < rng[j])
            dx = max(v[0, 0] - pos[j, 0], pos[j, 0] - v[2, 0], 0.0)
            dy = max(v[0, 1] - pos[j, 1], pos[j, 1] - v[2, 1], 0.0)
            d = float(np.hypot(dx, dy))
            if d < near[j]:
                near[j], corner[j], face[j] = d, dx > 0.0 and dy > 0.0, (dx > 0.0) != (dy > 0.0)
    walls = np.sqrt(((vel - q["vel"]) ** 2).sum(1)) > 1e-3
    agent = np.sqrt(((vel - vel_alone) ** 2).sum(1)) > 1e-3
    masks = dict(zip(CENSUS_KEYS, (edges == 0, edges == 1, edges == 2, edges >= 3, near < radius, corner, face, dropped > 0,
                                   walls, walls & agent)))
    c = Census((k, int(m.sum())) for k, m in masks.items())
    c.masks = masks
    c.query = dict(env=q["env"], ped=q["ped"], pos=pos, radius=radius, max_speed=ms, vel=vel, theta=q["theta"], verts=verts,
                   n_obst=n_obst, dropped=dropped)
    return c


def ped_orca_walls(cfg, a, p, rects, max_rects):
    """cfg: navsim_config; a: the arrays of a RefSim (r.a); p: ped_orca_spec.params(); rects: int16 [E, 255, 4], the list of
    every arena's rect_index row (decode_rows of the device's bytes, or written by hand); max_rects: 0 .. 32.
    Returns (ped_cmd [E,N,2] -- rows of dead slots copied from a["ped_cmd"] --, ped_wp_head [E,N], dropped [E,N] int32 -- 0 in
    dead slots --, census).  Nothing in `a` is written."""
    E, N = cfg.n_envs, cfg.max_peds
    assert 0 <= max_rects <= 32 and np.asarray(rects).shape == (E, LIST_LEN, 4)
    cmd, head, q = query(cfg, a, p)
    dropped = np.zeros((E, N), np.int32)
    if q is None or max_rects == 0:
        empty = Census((k, 0) for k in CENSUS_KEYS)
        empty.masks, empty.query = None, None
        return cmd, head, dropped, empty
    f = np.float32
    Q = len(q["env"])
    verts, n_obst, drop = np.zeros((Q, max_rects, 4, 2)), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    tho = f(p["time_horizon_obst"])
    for j in range(Q):
        e = int(q["env"][j])
        px, py, radius, ms = (f(q["agents"][j, 0, c]) for c in (0, 1, 4, 5))
        reach = f(f(tho * ms) + radius)
        kept, n_in = select(cfg, rects[e], px, py, f(reach * reach), max_rects)
        for o, k in enumerate(kept):
            xa, ya, xb, yb = vertices(cfg, rects[e][k])
            verts[j, o] = [[xa, ya], [xb, ya], [xb, yb], [xa, yb]]
        n_obst[j], drop[j] = len(kept), n_in - len(kept)
    op = q["params"]
    answer = lambda n_agents: ref.crowd_orca(op, q["agents"], q["pref"], verts=verts, n_agents=n_agents, n_obst=n_obst,
                                             obst_set=np.arange(Q, dtype=np.int32), theta=q["theta"])
    vel, act = answer(q["n_agents"])
    vel_alone, _ = answer(np.ones(Q, np.int32))
    cmd[q["env"], q["ped"], 0] = act[:, 0]
    cmd[q["env"], q["ped"], 1] = act[:, 1] / cfg.time_step
    dropped[q["env"], q["ped"]] = drop
    return cmd, head, dropped, _census(q, verts, n_obst, drop, p["time_horizon_obst"], vel, vel_alone)
