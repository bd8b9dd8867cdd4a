"""navsim_local_map (include/navsim.h) restated in NumPy: ref.math_fn for sin / cos, ref.build_dt for the float32 field.  Every
float64 operation is one NumPy operation, so each is rounded on its own.  The rule is written out as the header words it, step by
step, over all cells of an arena at once.  Also: the worlds and the parameter sets the CPU and the GPU tests share."""
import numpy as np

import dwa_spec
import ref

SIN, COS = 0, 1
# sim.local_map_defaults(cfg) in a world with pedestrians
DEFAULT = dict(cell=0.1, ahead=0.0, cap=2.0, ped_radius=0.3, channels=4)


def _f(fn, x):
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(x, np.float64)))
    return np.asarray(ref.math_fn(fn, x), np.float64)


def centres(pose, G, cell, ahead):
    """Steps 2 and 3 -> (wx [G,G], wy [G,G], s, c): the world position of the centre of cell (r, q)."""
    rx, ry, th = (np.float64(x) for x in pose)
    s, c = _f(SIN, th)[0], _f(COS, th)[0]
    k = np.arange(G, dtype=np.float64)
    half = np.float64(G) * np.float64(0.5)
    u = (((k + np.float64(0.5)) - half) * np.float64(cell) + np.float64(ahead))[:, None]       # by r
    v = (((k + np.float64(0.5)) - half) * np.float64(cell))[None, :]                           # by q
    wx = rx + (c * u - s * v)
    wy = ry + (s * u + c * v)
    return wx, wy, s, c


def local_map(cfg, fields, w, params, size, visible=None, skip=None, map_slot=None, detail=False):
    """fields [M,H,W] float32 (ref.build_dt); arena e reads fields[0] if cfg.shared_field, else fields[map_slot[e]] (None: e).
    w: robot_pose [E,3] and, with more than one channel, n_peds [E], ped_pose [E,N,3], ped_vel [E,N,2].  visible [E,N] or None,
    skip [E] or None.  -> float32 [E,C,G,G]; detail=True: (that, dict of 'inside' [E,G,G] bool, 'covered' [E,G,G] bool, 'tied'
    [E,G,G] bool: the least d2 is held by more than one counted pedestrian, 'counted' [E] pedestrians that count)."""
    p = dict(DEFAULT, **params)
    E, N, H, W = cfg.n_envs, cfg.max_peds, cfg.map_h, cfg.map_w
    G, C = int(size), int(p["channels"])
    cap, pr, res = np.float64(p["cap"]), np.float64(p["ped_radius"]), np.float64(cfg.resolution)
    ox, oy = np.float64(cfg.origin_x), np.float64(cfg.origin_y)
    out = np.zeros((E, C, G, G), np.float32)
    info = dict(inside=np.zeros((E, G, G), bool), covered=np.zeros((E, G, G), bool), tied=np.zeros((E, G, G), bool),
                counted=np.zeros(E, np.int64))
    for e in range(E):
        if skip is not None and skip[e]:                                        # step 1
            continue
        wx, wy, s, c = centres(w["robot_pose"][e], G, p["cell"], p["ahead"])     # steps 2, 3
        # step 4
        fi, fj = ((wx - ox) / res).astype(np.float32), ((wy - oy) / res).astype(np.float32)
        inside = (fi >= np.float32(0)) & (fi < np.float32(W)) & (fj >= np.float32(0)) & (fj < np.float32(H))
        i = np.where(inside, fi, np.float32(0)).astype(np.int32)
        j = np.where(inside, fj, np.float32(0)).astype(np.int32)
        field = fields[0 if cfg.shared_field else (e if map_slot is None else int(map_slot[e]))]
        clr = np.minimum(field[j, i].astype(np.float64) * res, cap)
        out[e, 0] = np.where(inside, clr, np.float64(0)).astype(np.float32)
        info["inside"][e] = inside
        if C == 1:
            continue
        # step 5
        n = min(max(int(w["n_peds"][e]), 0), N)
        who = [k for k in range(n) if visible is None or visible[e][k] != 0]
        info["counted"][e] = len(who)
        if not who:
            out[e, 1] = np.float32(cap)
            continue                                                            # (channels 2 and 3 stay 0)
        px = np.asarray(w["ped_pose"], np.float64)[e, who, 0][:, None, None]
        py = np.asarray(w["ped_pose"], np.float64)[e, who, 1][:, None, None]
        ex, ey = px - wx[None], py - wy[None]
        d2 = ex * ex + ey * ey
        near = np.argmin(d2, axis=0)                                            # the first of equal minima: the least (d2, i)
        d2n = np.take_along_axis(d2, near[None], axis=0)[0]
        dist = np.sqrt(d2n)
        out[e, 1] = np.minimum(np.maximum(dist - pr, np.float64(0)), cap).astype(np.float32)
        info["tied"][e] = (d2 == d2n[None]).sum(axis=0) > 1
        covered = dist <= pr
        info["covered"][e] = covered
        if C == 4:                                                              # step 6
            vx = np.asarray(w["ped_vel"], np.float64)[e, who, 0][near]
            vy = np.asarray(w["ped_vel"], np.float64)[e, who, 1][near]
            out[e, 2] = np.where(covered, c * vx + s * vy, np.float64(0)).astype(np.float32)
            out[e, 3] = np.where(covered, c * vy - s * vx, np.float64(0)).astype(np.float32)
    return (out, info) if detail else out


def config(E, size, N=0, **kw):
    return dwa_spec.config(E, size, N, **kw)


# ---- the shared world: dwa_spec.random_world's maps and pedestrians, the robots and the counts placed for this rule -------------
BASE = (5, 6, 100, 8101)             # E, N, cells a side (5 m x 5 m at 0.05 m), seed
TIE_ARENA, TIE_G, TIE_OFFSET = 3, 16, 0.25


def base_world():
    """E = 5 arenas of 100 x 100 cells, six pedestrian slots each, all of them holding poses.
    arena 0: the robot 0.4 m from the map's x = 0 side, heading 0.3 -- its window lies partly outside the map --; arena 1: no pedestrians;
    arena 2: three of the six slots count; arena 3: heading 0 at (2.5, 2.5), pedestrians 0 and 1 placed TIE_OFFSET metres either
    side (along x) of the centre of cell (TIE_G / 2, TIE_G / 2) of the TIE_G-cell map with 0.1 m cells and ahead = 0 -- the sums
    are exact, so their squared distances to that centre are equal -- with different velocities, the others far away; arena 4:
    the robot in the far corner."""
    E, N, size, seed = BASE
    occ, w = dwa_spec.random_world(E, N, size, seed)
    w = {k: np.array(v, copy=True) for k, v in w.items()}
    w["robot_pose"][0] = (0.4, 2.5, 0.3)
    w["robot_pose"][4, :2] = (4.8, 4.7)
    w["n_peds"] = np.array([6, 0, 3, 6, 6], np.int32)
    w["robot_pose"][TIE_ARENA] = (2.5, 2.5, 0.0)
    wx, wy, s, c = centres(w["robot_pose"][TIE_ARENA], TIE_G, 0.1, 0.0)
    x, y = wx[TIE_G // 2, TIE_G // 2], wy[TIE_G // 2, TIE_G // 2]
    w["ped_pose"][TIE_ARENA, 0, :2] = (x + TIE_OFFSET, y)
    w["ped_pose"][TIE_ARENA, 1, :2] = (x - TIE_OFFSET, y)
    assert (x + TIE_OFFSET) - x == TIE_OFFSET and (x - TIE_OFFSET) - x == -TIE_OFFSET
    w["ped_pose"][TIE_ARENA, 2:, :2] = ((0.3, 0.3), (0.3, 4.7), (4.7, 0.3), (4.7, 4.7))
    w["ped_vel"][TIE_ARENA, 0], w["ped_vel"][TIE_ARENA, 1] = (0.5, -0.25), (-0.375, 0.125)
    return occ, w


# the single calls of the device test: (G, cell, ahead, channels); cap = 0.6 m so that both clearances saturate in a 5 m map
CAP = 0.6
CALLS = [(1, 0.1, 0.0, 4), (7, 0.33, 0.0, 4), (7, 0.05, 1.5, 2), (16, 0.1, 0.0, 4), (16, 0.05, 0.0, 1), (16, 0.33, 1.5, 2),
         (64, 0.1, 0.0, 4), (64, 0.05, 1.5, 1), (64, 0.33, 0.0, 2), (128, 0.05, 0.0, 4), (128, 0.1, 1.5, 2), (128, 0.33, 0.0, 1),
         (30, 0.1, 0.0, 4), (12, 0.1, 1.5, 4)]


def call_params(cell, ahead, channels, **kw):
    return dict(dict(cell=cell, ahead=ahead, cap=CAP, ped_radius=0.3, channels=channels), **kw)
