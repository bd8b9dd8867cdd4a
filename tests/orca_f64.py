"""ORCA for one agent per query as a brute-force float64 evaluation of its definition -- the reference navsim_crowd_orca and
navsim_ped_orca are checked against beyond their bit-for-bit oracle.  numpy only; nothing of the
oracle, of the kernels or of RVO2's incremental linear programs is used or restated here.

What is computed (van den Berg, Guy, Lin, Manocha: "Reciprocal n-body collision avoidance", section 4; the operation-level
statement of include/navsim.h navsim_crowd_orca):
  neighbours   the other agents strictly closer than neighbor_dist, the max_neighbors nearest of them, ties by list order.
  half-planes  one per neighbour.  With p = p_B - p_A, v = v_A - v_B, R = r_A + r_B and tau = time_horizon, the velocity
               obstacle is the union over 0 < t <= tau of the discs of radius R / t around p / t: a cone with its apex at
               the origin, truncated by the disc around p / tau.  u leads from v to the nearest point of its boundary (the
               arc facing the origin, or the line carrying the nearer leg), n is the outward normal there, and A takes half
               of the correction: n . (x - (v_A + u / 2)) >= 0.  Agents that already overlap (|p| <= R) use the disc
               around p / time_step alone.
  feasible     among the velocities of the speed disc that satisfy every half-plane, the one nearest to the preferred
               velocity: the best of a finite list of candidates (the preferred velocity clipped to the disc, its
               projection on every line, every line-line and every line-circle intersection).
  infeasible   if there is none, the smallest possible value of the largest penetration max_i n_i . (point_i - x) over the
               speed disc: the best of the candidates r n_i, the points of the circle where two penetrations are equal, and
               the points where three are.  That value is unique; it is negative exactly when the program is feasible.
Obstacle polygons get no half-planes here: swept_clearance() measures what their constraints are for."""
from itertools import combinations

import numpy as np

CUTOFF, LEFT_LEG, RIGHT_LEG, COLLIDING = 0, 1, 2, 3                    # class of a half-plane
CLASS_NAMES = ("cut-off", "left leg", "right leg", "colliding")
INTERIOR, CIRCLE, LINE, VERTEX, LINE_CIRCLE = 0, 1, 2, 3, 4            # where the feasible optimum sits
WHERE_NAMES = ("interior", "speed circle", "one line", "vertex of two lines", "line and circle")
EPS = 1e-9                                                             # a candidate may miss a constraint by this (float64 noise)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _dot(a, b):
    return (a * b).sum(-1)


def _det(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _rot(a, c, s):
    return np.stack([a[..., 0] * c - a[..., 1] * s, a[..., 0] * s + a[..., 1] * c], -1)


def neighbours(agents, n_agents, neighbor_dist, max_neighbors):
    """-> index [Q,L] into the agent list (0 where absent), have [Q,L], and the list events and margin of the selection."""
    Q, A = agents.shape[:2]
    L = max(min(int(max_neighbors), A - 1), 0)
    k = np.arange(1, A)
    valid = k[None, :] < n_agents[:, None]
    d = np.sqrt(((agents[:, 1:, :2] - agents[:, :1, :2]) ** 2).sum(-1))
    inside = valid & (d < neighbor_dist)
    key = np.where(inside, d, np.inf)
    order = np.argsort(key, axis=1, kind="stable")                     # nearest first, ties by list order
    sd = np.take_along_axis(key, order, 1)
    n_in = inside.sum(1)
    have = np.arange(L)[None, :] < np.minimum(n_in, L)[:, None]
    index = np.where(have, order[:, :L] + 1, 0)
    truncated = n_in > L
    kept = np.zeros((Q, A - 1), bool)
    np.put_along_axis(kept, order[:, :L], have, 1)
    first = inside & (np.cumsum(inside, 1) <= L)                       # what the list holds before anyone is displaced
    displaced = truncated & (kept != first).any(1)
    rejected = (valid & ~inside).any(1)
    gap = np.full(Q, np.inf)
    if 0 < L < A - 1:
        with np.errstate(invalid="ignore"):
            gap = np.where(truncated, sd[:, L] - sd[:, L - 1], np.inf)
    edge = np.where(valid, np.abs(d - neighbor_dist), np.inf).min(1) if A > 1 else np.full(Q, np.inf)
    return index, have, dict(truncated=truncated, displaced=displaced, rejected=rejected), np.minimum(gap, edge)


def half_planes(agents, index, have, time_horizon, time_step):
    """-> n [Q,L,2] outward unit normals, b [Q,L] (the half-plane is n . x >= b), cls [Q,L] (-1: absent), margin [Q]."""
    me = agents[:, :1]
    ot = np.take_along_axis(agents, index[:, :, None], 1)
    p = ot[..., :2] - me[..., :2]
    v = me[..., 2:4] - ot[..., 2:4]
    R = me[..., 4] + ot[..., 4]
    dist = np.sqrt(_dot(p, p))
    with np.errstate(all="ignore"):
        # agents apart: the truncated cone
        c = p / time_horizon
        w = v - c
        wl = np.sqrt(_dot(w, w))
        cos_w = _dot(w, -p) / (wl * dist)                              # angle of w against the direction centre -> apex
        on_arc = cos_w > R / dist                                      # ... is inside the arc between the tangent points
        alpha = np.arcsin(np.clip(R / dist, -1.0, 1.0))                # half opening angle of the cone
        ph = p / dist[..., None]
        left = _det(p, v) > 0.0                                        # v on the left of the cone's axis
        t_left, t_right = _rot(ph, np.cos(alpha), np.sin(alpha)), _rot(ph, np.cos(alpha), -np.sin(alpha))
        tang = np.where(left[..., None], t_left, t_right)              # unit vector along the nearer leg, away from the apex
        n_leg = np.where(left[..., None], _rot(t_left, 0.0, 1.0), _rot(t_right, 0.0, -1.0))     # pointing out of the cone
        u_leg = _dot(v, tang)[..., None] * tang - v
        n_arc = w / wl[..., None]
        u_arc = (R / time_horizon - wl)[..., None] * n_arc
        # agents overlapping: out of the disc around p / time_step within one step
        w2 = v - p / time_step
        w2l = np.sqrt(_dot(w2, w2))
        n_col = w2 / w2l[..., None]
        u_col = (R / time_step - w2l)[..., None] * n_col
        apart = dist > R
        arc = apart & on_arc
        n = np.where(apart[..., None], np.where(on_arc[..., None], n_arc, n_leg), n_col)
        u = np.where(apart[..., None], np.where(on_arc[..., None], u_arc, u_leg), u_col)
        cls = np.where(apart, np.where(on_arc, CUTOFF, np.where(left, LEFT_LEG, RIGHT_LEG)), COLLIDING)
        b = _dot(n, me[..., 2:4] + 0.5 * u)
        side = np.abs(_det(p, w)) / (dist * wl)
    ok = have & np.isfinite(n).all(-1) & np.isfinite(b)                # a NaN half-plane constrains nothing
    cls = np.where(ok, cls, -1)
    m = np.minimum(np.where(ok, np.abs(dist - R), np.inf), np.where(ok & apart & ~arc, side, np.inf))
    return np.where(ok[..., None], n, 0.0), np.where(ok, b, -np.inf), cls, m.min(1, initial=np.inf)


def _pairs(L, k):
    c = np.array(list(combinations(range(L), k)), np.int64).reshape(-1, k)
    return [c[:, i] for i in range(k)]


def _solve2(a1, c1, a2, c2):
    """x with a1 . x = c1 and a2 . x = c2 (nan where the rows are parallel)."""
    with np.errstate(all="ignore"):
        dt = _det(a1, a2)
        x = np.stack([c1 * a2[..., 1] - c2 * a1[..., 1], a1[..., 0] * c2 - a2[..., 0] * c1], -1) / dt[..., None]
    return x


def _line_circle(a, c, r):
    """The two points of the circle |x| = r on the line a . x = c (a need not be a unit vector; nan where there are none)."""
    with np.errstate(all="ignore"):
        al = np.sqrt(_dot(a, a))
        h = c / al
        an = a / al[..., None]
        s = np.sqrt(r[:, None] ** 2 - h ** 2)
        foot = h[..., None] * an
        t = np.stack([an[..., 1], -an[..., 0]], -1) * s[..., None]
    return foot + t, foot - t


def _penetration(n, b, x):
    """max over the half-planes of b - n . x, for candidates x [Q,M,2] -> [Q,M] (-inf without half-planes)."""
    with np.errstate(invalid="ignore"):
        pen = b[:, None, :] - (x[:, :, None, 0] * n[:, None, :, 0] + x[:, :, None, 1] * n[:, None, :, 1])
    pen = np.where(np.isneginf(b)[:, None, :], -np.inf, pen)
    return pen.max(-1, initial=-np.inf)


def _solve_chunk(n, b, pref, r):
    Q, L = b.shape
    present = np.isfinite(b)
    bb = np.where(present, b, 0.0)
    nan = np.where(present, 0.0, np.nan)                               # poisons candidates made of absent lines
    i2, j2 = _pairs(L, 2)
    # ---- the feasible program
    sp = np.sqrt(_dot(pref, pref))
    with np.errstate(all="ignore"):
        clipped = np.where((sp > r)[:, None], pref * (r / sp)[:, None], pref)
    proj = pref[:, None, :] - (_dot(n, pref[:, None, :]) - bb + nan)[..., None] * n
    vert = _solve2(n[:, i2], bb[:, i2] + nan[:, i2], n[:, j2], bb[:, j2] + nan[:, j2])
    lc1, lc2 = _line_circle(n, bb + nan, r)
    cand = np.concatenate([clipped[:, None, :], proj, vert, lc1, lc2], 1)
    kind = np.concatenate([[INTERIOR], np.full(L, LINE), np.full(len(i2), VERTEX), np.full(2 * L, LINE_CIRCLE)])
    with np.errstate(invalid="ignore"):
        ok = (_penetration(n, b, cand) <= EPS) & (_dot(cand, cand) <= (r[:, None] + EPS) ** 2)
        cost = np.where(ok, ((cand - pref[:, None, :]) ** 2).sum(-1), np.inf)
    best = cost.argmin(1)
    feasible = ok.any(1)
    vel = np.where(feasible[:, None], cand[np.arange(Q), best], np.nan)
    where = np.where(feasible, kind[best], -1)
    where = np.where(feasible & (best == 0) & (sp > r), CIRCLE, where)
    # ---- the smallest largest penetration over the disc
    i3, j3, k3 = _pairs(L, 3)
    single = r[:, None, None] * n + nan[..., None]
    bis = n[:, j2] - n[:, i2]
    e1, e2 = _line_circle(bis, bb[:, j2] - bb[:, i2] + nan[:, i2] + nan[:, j2], r)
    tri = _solve2(n[:, j3] - n[:, i3], bb[:, j3] - bb[:, i3] + nan[:, i3] + nan[:, j3],
                  n[:, k3] - n[:, i3], bb[:, k3] - bb[:, i3] + nan[:, k3])
    cand = np.concatenate([single, e1, e2, tri], 1)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(cand).all(-1) & (_dot(cand, cand) <= (r[:, None] * (1.0 + 1e-12)) ** 2)
    value = np.where(inside, _penetration(n, b, np.where(inside[..., None], cand, 0.0)), np.inf)
    if value.shape[1] == 0:
        value, cand = np.full((Q, 1), -np.inf), np.zeros((Q, 1, 2))
    best = value.argmin(1)
    minimax = value[np.arange(Q), best]
    minimax = np.where(present.any(1), minimax, -np.inf)
    return vel, where, feasible, minimax, cand[np.arange(Q), best]


def solve(params, agents, pref_vel, n_agents=None, budget=1e7):
    """params: time_step, neighbor_dist, time_horizon, max_neighbors (rounded to float32 like every input); agents [Q,A,6] =
    px, py, vx, vy, radius, max_speed with agent 0 the one solved for; pref_vel [Q,2]; n_agents [Q] or None.
    Returns a dict of arrays over the queries:
      feasible, vel (the optimum, nan where infeasible), where (INTERIOR .. LINE_CIRCLE, -1 where infeasible),
      minimax (the smallest largest penetration over the speed disc; -inf without half-planes), minimax_vel (a velocity with
      that penetration), n [Q,L,2] / b [Q,L] (half-plane l is n . x >= b; b = -inf where absent), cls [Q,L] (CUTOFF ..
      COLLIDING, -1 where absent), truncated, displaced, rejected (list events), min_det (smallest |det| over pairs of
      half-plane directions, inf below two), margin (how far the nearest discrete decision is from flipping: neighbour
      selection, overlapping or apart, left or right leg, feasible or not), max_speed."""
    agents = _f32(agents)
    pref = _f32(pref_vel).reshape(-1, 2)
    Q, A = agents.shape[:2]
    n_agents = np.full(Q, A, np.int64) if n_agents is None else np.minimum(np.asarray(n_agents, np.int64), A)
    f = {k: float(np.float32(params[k])) for k in ("time_step", "neighbor_dist", "time_horizon")}
    index, have, events, m_sel = neighbours(agents, n_agents, f["neighbor_dist"], params["max_neighbors"])
    n, b, cls, m_cls = half_planes(agents, index, have, f["time_horizon"], f["time_step"])
    r = agents[:, 0, 5]
    L = b.shape[1]
    per_query = max(1, L * (L * (L - 1) * (L - 2) // 6 + 3 * L * L))
    step = max(1, int(budget // per_query))
    parts = [_solve_chunk(n[s:s + step], b[s:s + step], pref[s:s + step], r[s:s + step]) for s in range(0, max(Q, 1), step)]
    vel, where, feasible, minimax, mvel = (np.concatenate(x) for x in zip(*parts))
    min_det = np.full(Q, np.inf)
    if L >= 2:
        i2, j2 = _pairs(L, 2)
        both = np.isfinite(b[:, i2]) & np.isfinite(b[:, j2])
        min_det = np.where(both, np.abs(_det(n[:, i2], n[:, j2])), np.inf).min(1)
    margin = np.minimum(np.minimum(m_sel, m_cls), np.abs(minimax))
    out = dict(feasible=feasible, vel=vel, where=where, minimax=minimax, minimax_vel=mvel, n=n, b=b, cls=cls, min_det=min_det,
               margin=margin, max_speed=r)
    out.update(events)
    return out


def penetration(res, vel):
    """The largest penetration of res's half-planes by the velocities vel [Q,2] (-inf without half-planes)."""
    return _penetration(res["n"], res["b"], np.asarray(vel, np.float64)[:, None, :])[:, 0]


def _point_segment(p, a, b):
    ab = b - a
    with np.errstate(all="ignore"):
        t = np.clip(np.nan_to_num(_dot(p - a, ab) / _dot(ab, ab)), 0.0, 1.0)
    q = a + t[..., None] * ab
    return np.sqrt(_dot(p - q, p - q))


def swept_clearance(pos, vel, radius, horizon, polys):
    """The clearance of the disc of `radius` swept from pos [Q,2] along vel [Q,2] for `horizon` seconds from the polygons
    polys [O,V,2]: distance of the segment pos .. pos + vel horizon from the nearest edge minus the radius (the segment
    crossing an edge counts as distance 0).  Negative: the disc enters a polygon by that much.  Meant for starts outside."""
    pos = np.asarray(pos, np.float64)[:, None, :]
    end = pos + np.asarray(vel, np.float64)[:, None, :] * horizon
    polys = np.asarray(polys, np.float64)
    a = polys.reshape(-1, 2)[None]
    bq = np.roll(polys, -1, axis=1).reshape(-1, 2)[None]
    d = np.minimum(np.minimum(_point_segment(pos, a, bq), _point_segment(end, a, bq)),
                   np.minimum(_point_segment(a, pos, end), _point_segment(bq, pos, end)))
    cross = (_det(end - pos, a - pos) * _det(end - pos, bq - pos) < 0) & (_det(bq - a, pos - a) * _det(bq - a, end - a) < 0)
    return np.where(cross, 0.0, d).min(1) - radius
