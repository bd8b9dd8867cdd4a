"""navsim_scan_labels (include/navsim.h) restated in NumPy, composed from the CPU oracle's exported functions: ref.math_fn for
sin / cos, ref.xy_to_ij_f32 for the scan's origin cell, ref.cast_static for the static ray (queries (i0, j0, heading),
max_range = H W: the full march; it evaluates beam_dir itself), ref.beam_dirs for the directions the merges use and
ref.leg_centres for the leg discs.  seg_merge / circle_merge are written out here in float32 NumPy arrays over the beams, one
operation per line of the C, so each is rounded on its own.  Candidates are taken ONE AFTER THE OTHER in the rule's order: the
sequential rule itself, not a minimum.  Also: the hand-made scenes and the random worlds the CPU and the GPU tests share."""
import numpy as np

import ped_edge_scenes
import ref
from helpers import keti_thresholds
from nav_gym_amd import abi, world

SIN, COS = 0, 1
NONE, WALL, BODY, LEG = abi.BEAM_NONE, abi.BEAM_WALL, abi.BEAM_PED_BODY, abi.BEAM_PED_LEG
FOOTPRINT = ((0.22, 0.19), (-0.22, 0.19), (-0.22, -0.19), (0.22, -0.19))        # human.py:5-10
LEG_RADIUS = np.float32(0.03)


def _f(fn, x):
    return np.asarray(ref.math_fn(fn, np.ascontiguousarray(np.atleast_1d(np.asarray(x, np.float64)))), np.float64)


def beam_angles(cfg):
    """np.linspace(angle_min, angle_last, B) as the rule states it: k * step + angle_min, the last beam angle_last itself."""
    B = cfg.n_beams
    if B == 1:
        return np.array([cfg.angle_min], np.float64)
    step = (np.float64(cfg.angle_last) - np.float64(cfg.angle_min)) / np.float64(B - 1)
    lin = np.arange(B, dtype=np.float64) * step + np.float64(cfg.angle_min)
    lin[B - 1] = cfg.angle_last
    return lin


def candidates(cfg, n, ped_pose, ped_dist, ped_has_legs):
    """The pedestrians' primitives of one arena in the rule's order -> [(kind, pedestrian, float32 parameters), ...]: first the
    four sides of every pedestrian without (legs and cfg.lidar_legs), then the two discs of every one with."""
    segs, discs = [], []
    for i in range(n):
        px, py, th = (np.float64(v) for v in ped_pose[i])
        if ped_has_legs[i] and cfg.lidar_legs:
            a = np.zeros(8, np.float32)
            a[0:3] = np.asarray(ped_pose[i], np.float64).astype(np.float32)
            a[3:6] = np.asarray(ped_dist[i], np.float64).astype(np.float32)
            cc = ref.leg_centres(a)
            discs.append((LEG, i, (cc[0], cc[1])))
            discs.append((LEG, i, (cc[2], cc[3])))
        else:
            s, c = _f(SIN, th)[0], _f(COS, th)[0]
            v = [(np.float32((c * np.float64(x) - s * np.float64(y)) + px), np.float32((s * np.float64(x) + c * np.float64(y)) + py))
                 for x, y in FOOTPRINT]
            for k in range(4):
                w = (k + 1) & 3
                segs.append((BODY, i, (v[k][0], v[k][1], v[w][0], v[w][1])))
    return segs + discs


def _seg_t(ox, oy, c, s, px, py, qx, qy):
    """seg_merge's t per beam, +inf where it declines (float32 arrays c, s; float32 scalars otherwise)."""
    ex, ey = qx - px, qy - py
    wx, wy = px - ox, py - oy
    denom = c * ey - s * ex
    with np.errstate(all="ignore"):
        t = (wx * ey - wy * ex) / denom
        u = (wx * s - wy * c) / denom
    ok = (denom != 0) & (t >= 0) & (u >= 0) & (u <= 1)
    return np.where(ok, t, np.float32(np.inf)).astype(np.float32)


def _disc_t(ox, oy, c, s, cx, cy, rad):
    wx, wy = cx - ox, cy - oy
    b = wx * c + wy * s
    x = wx * s - wy * c
    disc = rad * rad - x * x
    with np.errstate(all="ignore"):
        t = b - np.sqrt(disc)
    ok = ~(disc < 0) & (t >= 0)
    return np.where(ok, t, np.float32(np.inf)).astype(np.float32)


def scan_labels(cfg, fields, robot_pose, n_peds=None, ped_pose=None, ped_dist=None, ped_has_legs=None, skip=None, map_slot=None):
    """fields [M,H,W] float32 (ref.build_dt); arena e reads fields[0] if cfg.shared_field, else fields[map_slot[e]] (None: e).
    -> {'range' [E,B] float32, 'label' [E,B] uint8, 'index' [E,B] int8, 'hits' [E,N] int32}."""
    E, N, B, H, W = cfg.n_envs, cfg.max_peds, cfg.n_beams, cfg.map_h, cfg.map_w
    out = dict(range=np.zeros((E, B), np.float32), label=np.zeros((E, B), np.uint8), index=np.full((E, B), -1, np.int8),
               hits=np.zeros((E, N), np.int32))
    res32, rmax = np.float32(cfg.resolution), np.float32(cfg.range_max)
    lin = beam_angles(cfg)
    for e in range(E):
        if skip is not None and skip[e]:
            continue
        n = 0 if cfg.ped_model == abi.PED_NONE else min(int(n_peds[e]), N)
        lx, ly, lth = (np.float32(v) for v in np.asarray(robot_pose[e], np.float64))
        i0, j0 = ref.xy_to_ij_f32(np.array([[lx, ly]], np.float32), (cfg.origin_x, cfg.origin_y), cfg.resolution, H, W)[0]
        heading = (lin + np.float64(lth)).astype(np.float32)
        slot = 0 if cfg.shared_field else (e if map_slot is None else int(map_slot[e]))
        q = np.stack([np.full(B, i0, np.float32), np.full(B, j0, np.float32), heading], axis=1)[None]
        r = ref.cast_static(fields[slot][None], q, float(np.float32(H * W)), cfg.march_rule)[0] * res32       # candidate 0
        d = ref.beam_dirs(heading)
        c, s = d[:, 0], d[:, 1]
        kind, who = np.full(B, WALL, np.uint8), np.full(B, -1, np.int8)
        for k_, i, p in (candidates(cfg, n, ped_pose[e], ped_dist[e], ped_has_legs[e]) if n > 0 else ()):
            t = _seg_t(lx, ly, c, s, *p) if k_ == BODY else _disc_t(lx, ly, c, s, p[0], p[1], LEG_RADIUS)
            low = t < r                                                # strict: an equal candidate does not replace
            r = np.where(low, t, r).astype(np.float32)
            kind[low], who[low] = k_, i
        r = np.where(r < 0, np.float32(0), r)
        r = np.where(r > rmax, rmax, r).astype(np.float32)
        none = r == rmax
        kind[none], who[none] = NONE, -1
        out["range"][e], out["label"][e], out["index"][e] = r, kind, who
        for i in range(n):
            out["hits"][e, i] = int((who == i).sum())
    return out


def answer(cfg, fields, a, **kw):
    """scan_labels of a world's arrays (a RefSim's .a or the dict a world function returns)."""
    return scan_labels(cfg, fields, a["robot_pose"], a.get("n_peds"), a.get("ped_pose"), a.get("ped_dist"), a.get("ped_has_legs"),
                       **kw)


def newest_scan(cfg, obs):
    """The newest scan slot of observation rows [E, S B + 7]."""
    B, S = cfg.n_beams, cfg.n_scan_stack
    return obs[:, (S - 1) * B:S * B]


# ---- worlds -------------------------------------------------------------------------------------------------------------------
def room(size, boxes=0, seed=0, wall=True):
    """A size x size map with `boxes` random boxes of 4 .. 12 cells a side, closed by a 3-cell wall unless wall is False (rays
    then leave the map: no return)."""
    occ = np.zeros((size, size), np.uint8)
    if wall:
        occ[:3] = 1; occ[-3:] = 1; occ[:, :3] = 1; occ[:, -3:] = 1
    rng = np.random.default_rng(seed)
    for _ in range(boxes):
        w, h = rng.integers(4, 13, 2)
        x, y = rng.integers(6, size - 18, 2)
        occ[y:y + h, x:x + w] = 1
    return occ


def config(E, N, size, lidar=None, ped_model=abi.PED_EXTERNAL, **kw):
    """lidar: None = 1081 beams over 270 degrees, an int = that many beams over the full circle, (270, B) = B beams over 270
    degrees."""
    cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=ped_model, n_spawn=1, **kw)
    if lidar is None or isinstance(lidar, tuple):
        world.lidar_1081(cfg)
        if lidar is not None:
            cfg.n_beams = lidar[1]
        return cfg
    return world.lidar_full_circle(cfg, lidar)


def random_scenes(E, N, size, seed, n_peds=None, boxes=5, res=0.05, wall=True):
    """E scenes for ped_edge_scenes.lidar_world: the robot in the middle third of a room(size), N pedestrians 0.5 .. 5 m from it
    (inside the room), every second one in expectation with legs.  -> (occ [E,size,size], scenes)"""
    rng = np.random.default_rng(seed)
    occ = np.stack([room(size, boxes, seed + 100 + e, wall) for e in range(E)])
    scenes = []
    for e in range(E):
        while True:
            rc = rng.integers(size // 3, 2 * size // 3, 2)
            if not occ[e, rc[1] - 2:rc[1] + 3, rc[0] - 2:rc[0] + 3].any():
                break
        rx, ry = (rc + rng.uniform(0.0, 1.0, 2)) * res
        n = N if n_peds is None else int(n_peds[e])
        peds = []
        while len(peds) < N:                                     # (the slots behind n hold poses too: they must be ignored)
            b, dist = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(0.5, 5.0)
            px, py = rx + dist * np.cos(b), ry + dist * np.sin(b)
            if 0.4 < px < size * res - 0.4 and 0.4 < py < size * res - 0.4:
                peds.append(((px, py, rng.uniform(0.0, 2.0 * np.pi)), int(rng.uniform() < 0.5)))
        scenes.append(dict(robot=(rx, ry, rng.uniform(0.0, 2.0 * np.pi)), peds=peds, n=n))
    return occ, scenes


def scene_world(cfg, scenes):
    """Host arrays of the scenes (ped_edge_scenes.lidar_world: NAVSIM_PED_EXTERNAL, everything at rest) with the Keti
    thresholds; a scene's 'n' (optional) is its live count."""
    a = ped_edge_scenes.lidar_world(cfg, scenes)
    for e, sc in enumerate(scenes):
        a["n_peds"][e] = sc.get("n", len(sc["peds"]))
    a["scan_threshold"], a["scan_discomfort"] = keti_thresholds(cfg)
    if cfg.ped_model == abi.PED_NONE:
        a = {k: v for k, v in a.items() if not k.startswith("ped_") and k != "n_peds"}
    return a


# (E, size, N, lidar, seed) of the four worlds of the CPU comparison with the oracle's own scan (the 64-beam world has four arenas:
# its pedestrians are few and its beams 5.6 degrees apart)
ORACLE_WORLDS = ((2, 160, 8, None, 7101), (2, 200, 64, None, 7102), (4, 120, 5, 64, 7103), (2, 600, 20, None, 7104))

# (E, N, B, seed, live counts) of the device's single calls, each over 270 degrees and over the full circle: the shapes at which
# the kernel's lane and interval logic changes -- one wavefront's worth of beams and one more, several beams per thread, every
# pedestrian slot, a single beam; pedestrian counts that vary per arena, 0 among them
DEVICE_WORLDS = ((1, 1, 64, 7201, None), (3, 5, 65, 7202, (0, 5, 2)), (5, 21, 1081, 7203, (21, 0, 7, 20, 1)),
                 (2, 64, 1081, 7204, None), (4, 8, 1, 7205, (8, 3, 0, 8)))
DEVICE_SIZE = 160


def device_world(E, N, B, seed, n_peds, full, size=DEVICE_SIZE, **kw):
    """-> (cfg, occ, host arrays) of one of DEVICE_WORLDS; full: the beams over the full circle, else over 270 degrees."""
    cfg = config(E, N, size, lidar=B if full else (270, B), **kw)
    occ, scenes = random_scenes(E, N, size, seed, n_peds)
    return cfg, occ, scene_world(cfg, scenes)


# ---- hand-made scenes: an empty walled room of 200 cells (10 m), the robot at its centre looking along +x ---------------------
ROOM = 200
ROBOT = (5.0125, 5.0125, 0.0)


def hand_scene(peds, lidar=65, robot=ROBOT, skip=None, **kw):
    """-> (cfg, fields, arrays, result) of one arena with pedestrians `peds` = [((x, y, yaw), legs), ...] relative to nothing:
    world coordinates.  lidar: beams over the full circle (odd: one looks straight ahead), None = 1081 over 270 degrees."""
    cfg = config(1, max(len(peds), 1), ROOM, lidar=lidar, **kw)
    a = scene_world(cfg, [dict(robot=robot, peds=peds)])
    fields = ref.build_dt(room(ROOM)[None])
    return cfg, fields, a, answer(cfg, fields, a, skip=skip)


def ahead(dist, side=0.0, yaw=0.0, legs=0):
    return ((ROBOT[0] + dist, ROBOT[1] + side, yaw), legs)
