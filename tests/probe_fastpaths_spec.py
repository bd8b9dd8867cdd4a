"""Scenes for tests/test_gpu_probe_fastpaths.py and a NumPy march that says which form each probe round of a wavefront takes.

A probe round of the step kernel's march (kernels_step.hpp probe_round, RECT = 2, no pedestrians) has a wave-uniform short form:
it leaves out the second rectangle's distance when no LIVE lane stands in a tile whose index pair names two different
rectangles (ia != ib).
`round_forms` marches the scans of a rollout the way a wavefront does -- 64 adjacent beams per chunk, a chunk left at
`park` live lanes and the parked rays marched 64 at a time, float32 t, t += max(0.999 sqrt(d2), 1) -- from the exact
integer field and the index pairs the step stages in LDS, and counts the rounds by form.  It is a census of the conditions,
not a second oracle: results are compared with oracle/ref.py, and the census only has to show that a scene exercises the
path it is there for.
"""
import numpy as np

RING = 3            # occupied cells around every map (closed maps: what the LDS form of the march needs)


def room(size):
    occ = np.ones((size, size), np.uint8)
    occ[RING:size - RING, RING:size - RING] = 0
    return occ


def scene(kind):
    """occ [H, W] uint8 and the start poses (cell i, cell j, heading) of the scene's four arenas."""
    if kind == "bare_room":                 # (a) nothing but the walls, every distance below 32 cells
        occ = room(64)
        poses = [(32, 32, 0.3), (17, 32, np.pi), (40, 18, -0.5 * np.pi), (30, 45, 0.5 * np.pi)]
    elif kind == "box_grid":                # (b) 3-cell boxes on a 9-cell pitch: most tiles need two rectangles
        occ = room(120)
        poses = [(60, 60, 0.2), (58, 62, 2.0), (62, 58, -2.5), (60, 56, -1.4)]
        for y in range(9, 108, 9):
            for x in range(9, 108, 9):
                if abs(x + 1 - 60) > 16 or abs(y + 1 - 60) > 16:      # a clearing for the robot
                    occ[y:y + 3, x:x + 2 + (x + y) // 9 % 2] = 1
    elif kind == "one_box":                 # (c) one box: a fan of 64 beams straddles the bisector between it and a wall
        occ = room(96)
        occ[40:52, 60:70] = 1
        poses = [(30, 46, 0.0), (34, 30, 0.6), (40, 70, -0.7), (75, 20, -0.5 * np.pi)]
    else:
        raise KeyError(kind)
    return occ, poses


SCENES = ("bare_room", "box_grid", "one_box")


def lidar(cfg, B):
    """1081 beams over 270 degrees (a chunk of 64 spans 16), or B beams over 1.2 rad ahead of the robot: a chunk then looks at
    one side of a room, where the full circle's chunks of 180 degrees always see two walls"""
    cfg.n_beams = B
    cfg.angle_min, cfg.angle_last = (-0.75 * np.pi, 0.75 * np.pi) if B == 1081 else (-0.6, 0.6)
    return cfg


def goals_xy(cfg, poses, size):
    """the centre of the corner of the room farthest from each pose: no arena reaches its goal within a test"""
    far = [(size - 9 if i < size // 2 else 8, size - 9 if j < size // 2 else 8, 0.0) for i, j, _ in poses]
    return poses_xy(cfg, far)[:, :2]


def poses_xy(cfg, poses):
    """cell centres in metres (ij_to_xy) + heading, float64 [n, 3]"""
    return np.array([[(i + 0.5) * cfg.resolution + cfg.origin_x, (j + 0.5) * cfg.resolution + cfg.origin_y, th] for i, j, th in poses])


def _march(d2, two, x0, y0, dx, dy, t, active, limit, stop, out):
    """all chunks [G, 64] at once; a chunk is left when at most `stop` of its lanes are live"""
    H, W = d2.shape
    while True:
        running = active.sum(axis=1) > stop
        if not running.any():
            return t, active
        x = np.clip((x0 + dx * t).astype(np.int32), 0, W - 1); y = np.clip((y0 + dy * t).astype(np.int32), 0, H - 1)
        dd = d2[y, x]
        pair = (two[y >> 3, x >> 3] & active).any(axis=1)                           # the live lanes vote
        live = active & running[:, None]
        out["rounds"] += int(running.sum())
        out["one_rect"] += int((running & ~pair).sum()); out["two_rect"] += int((running & pair).sum())
        for g in np.flatnonzero(running):
            out["by_chunk"].setdefault(out["scan"] * 4096 + int(g) + out["group_base"], set()).add(bool(pair[g]))
        occ = live & (dd == 0)
        step = np.maximum(np.float32(0.999) * np.sqrt(dd.astype(np.float32)), np.float32(1.0))
        go = live & ~occ
        tn = (t + step).astype(np.float32)
        t = np.where(go, tn, t).astype(np.float32)
        active = np.where(running[:, None], go & (tn < limit), active)


def round_forms(cfg, field, index_pairs, poses, park, dirs_of):
    """Census over the scans taken from `poses` [n, 4] = (arena, x, y, heading).  field: float32 distances [E, H, W];
    index_pairs: uint16 [E, tiles_y, tiles_x] (ia | ib << 8); dirs_of(float32 headings) -> float32 [n, 2]."""
    B = cfg.n_beams
    out = dict(rounds=0, one_rect=0, two_rect=0, by_chunk={}, scan=0, group_base=0)
    step = (cfg.angle_last - cfg.angle_min) / (B - 1)
    lin = np.arange(B) * step + cfg.angle_min
    lin[-1] = cfg.angle_last
    limit = np.float32(np.floor(cfg.range_max / cfg.resolution) + 4.0)
    G = (B + 63) // 64
    k = np.minimum(np.arange(G * 64), B - 1)
    valid = (np.arange(G * 64) < B).reshape(G, 64)
    for e, px, py, th in poses:
        e = int(e)
        d2 = np.rint(field[e].astype(np.float64) ** 2).astype(np.int64)
        p = index_pairs[e]
        two = (p & 0xFF) != (p >> 8)                                                # (no index: both bytes 0xFF, equal)
        lx, ly, lth = np.float32(px), np.float32(py), np.float32(th)
        i0 = int(np.floor((lx - np.float32(cfg.origin_x)) / np.float32(cfg.resolution)))
        j0 = int(np.floor((ly - np.float32(cfg.origin_y)) / np.float32(cfg.resolution)))
        if d2[j0, i0] == 0:
            continue
        d = dirs_of((lin + float(lth)).astype(np.float32))
        dx, dy = d[k, 0].reshape(G, 64), d[k, 1].reshape(G, 64)
        t1 = np.maximum(np.float32(0.999) * np.sqrt(np.float32(d2[j0, i0])), np.float32(1.0))
        t = np.full((G, 64), t1, np.float32)
        out["scan"] += 1; out["group_base"] = 0
        t, act = _march(d2, two, np.float32(i0), np.float32(j0), dx, dy, t, valid & bool(t1 < limit), limit, park, out)
        if park and act.any():                                                      # the parked rays, 64 at a time
            sel = np.flatnonzero(act.reshape(-1))
            n = len(sel); G2 = (n + 63) // 64
            idx = np.where(np.arange(G2 * 64) < n, sel[np.minimum(np.arange(G2 * 64), n - 1)], 0).reshape(G2, 64)
            first = idx[:, :1]
            v2 = (np.arange(G2 * 64) < n).reshape(G2, 64)
            idx = np.where(v2, idx, first)                                          # lanes past the last ray: the group's first
            out["group_base"] = 2048
            _march(d2, two, np.float32(i0), np.float32(j0), dx.reshape(-1)[idx], dy.reshape(-1)[idx], t.reshape(-1)[idx], v2, limit, 0, out)
    return out
