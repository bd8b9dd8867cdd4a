"""TEST INFRASTRUCTURE: hand-made worlds off the square, origin-zero, 5 cm grid (NumPy only; shared by
tests/test_map_geometry.py on the oracle and tests/test_gpu_map_geometry.py on the device).

A world is a dict of host arrays named like abi.STATE_LAYOUT (what ref.RefSim takes); the distance field is the
caller's (ref.build_dt on the CPU, sim.build_field on the device), because building it is one of the things under test.

Conventions restated from the oracle (oracle/navsim_ref.c xy_to_ij, trace_ray):
  * x is the COLUMN of the map (bounded by map_w), y the ROW (bounded by map_h);
  * xy_to_ij clips the x index against map_h and the y index against map_w, so on a non-square map a pose outside the
    leading min(H, W) x min(H, W) square is read at a clipped cell.  `inside=True` keeps every spawn, goal, pedestrian
    and waypoint so far inside that square that a short rollout cannot leave it; `inside=False` deliberately places
    some beyond it.
"""
import numpy as np

RING = 5            # create_outdoor_map's border wall, in cells


def closed_map(rng, H, W, n_boxes=6):
    """uint8 [H, W]: a 5-cell ring of occupied cells and `n_boxes` boxes of 3 .. 9 cells a side."""
    m = np.ones((H, W), np.uint8)
    m[RING:H - RING, RING:W - RING] = 0
    for _ in range(n_boxes):
        hh, hw = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        cy = int(rng.integers(RING + hh, H - RING - hh))
        cx = int(rng.integers(RING + hw, W - RING - hw))
        m[cy - hh:cy + hh + 1, cx - hw:cx + hw + 1] = 1
    return m


def open_map(rng, H, W, n_boxes=4):
    """closed_map with a gap through the ring on each of the four sides: rays leave the map through every side, so
    the march's bounds test decides their ranges."""
    m = closed_map(rng, H, W, n_boxes)
    gy, gx = max(H // 6, 4), max(W // 6, 4)
    y0, x0 = int(rng.integers(RING + 1, H - RING - gy)), int(rng.integers(RING + 1, W - RING - gx))
    y1, x1 = int(rng.integers(RING + 1, H - RING - gy)), int(rng.integers(RING + 1, W - RING - gx))
    m[:RING, x0:x0 + gx] = 0            # row 0 side
    m[H - RING:, x1:x1 + gx] = 0        # last-row side
    m[y0:y0 + gy, :RING] = 0            # column 0 side
    m[y1:y1 + gy, W - RING:] = 0        # last-column side
    return m


def make_maps(E, H, W, seed, kind="closed", n_boxes=6):
    rng = np.random.default_rng(seed)
    f = closed_map if kind == "closed" else open_map
    return np.stack([f(rng, H, W, n_boxes) for _ in range(E)])


def embed(occ, S=None):
    """The [E, H, W] maps in the low corner of S x S maps (S = max(H, W)), the rest occupied."""
    E, H, W = occ.shape
    S = max(H, W) if S is None else S
    out = np.ones((E, S, S), np.uint8)
    out[:, :H, :W] = occ
    return out


def cell_xy(cfg, cells):
    """ij_to_xy (env.py:1214-1220): centres of the cells [..., 2] = (column i, row j), float64 metres."""
    c = np.asarray(cells, np.float64)
    return np.stack([(c[..., 0] + 0.5) * cfg.resolution + cfg.origin_x, (c[..., 1] + 0.5) * cfg.resolution + cfg.origin_y], -1)


def _pick(rng, ok, n):
    """n cells (column i, row j) among the True cells of ok [H, W]."""
    jj, ii = np.nonzero(ok)
    assert len(jj) >= 1, "no cell satisfies the placement rule: change the map seed"
    k = rng.integers(0, len(jj), n)
    return np.stack([ii[k], jj[k]], -1)


def make_world(cfg, occ, field, thresholds, seed, n_peds=0, inside=True, travel_m=1.5):
    """Host arrays for cfg.n_envs arenas on the maps occ [E, H, W] with their float32 distance field (cells).

    Robots: cfg.n_spawn start / goal pairs per arena.  Entry 0 faces the nearest obstacle from 0.95 .. 1.1 m away (a
    straight drive crashes within a few steps), entry 1 has its goal 0.637 m ahead (it succeeds), the others are free cells
    with goals 1 .. 3 m away.  Pedestrians walk between two waypoints.
    inside: every cell used lies travel_m metres inside the leading square (plus the ring); False: in every second arena
    the cells come from BEYOND the leading square on the long axis (and from anywhere in the others)."""
    E, N, K, P = cfg.n_envs, cfg.max_peds, max(cfg.n_spawn, 1), cfg.max_waypoints
    H, W = occ.shape[1:]
    M = min(H, W)
    rng = np.random.default_rng(seed)
    res = cfg.resolution
    margin = int(np.ceil(travel_m / res))
    jj, ii = np.mgrid[0:H, 0:W]
    a = dict(field=field, scan_threshold=thresholds[0], scan_discomfort=thresholds[1],
             scan_noise_std=np.zeros(E, np.float32),
             robot_pose=np.zeros((E, 3)), robot_goal=np.zeros((E, 2)),
             prev_action=np.zeros((E, 2)), prev_pose=np.zeros((E, 3)),
             n_hist=np.zeros(E, np.int32), episode=np.zeros(E, np.int64), steps=np.zeros(E, np.int64),
             spawn_pose=np.zeros((E, K, 3)), spawn_goal=np.zeros((E, K, 2)))
    if N and n_peds:
        a.update(n_peds=np.full(E, n_peds, np.int32), ped_pose=np.zeros((E, N, 3)), ped_vel=np.zeros((E, N, 2)),
                 ped_prev_yaw=np.zeros((E, N)), ped_dist=np.zeros((E, N, 3)),
                 ped_v_pref=rng.uniform(0.2, 0.6, (E, N)), ped_has_legs=(np.arange(E * N).reshape(E, N) % 2).astype(np.uint8),
                 ped_waypoints=np.zeros((E, N, P, 2)), ped_n_waypoints=np.full((E, N), min(2, P), np.int32),
                 ped_cmd=np.zeros((E, N, 2)), ped_goal=np.zeros((E, N, 2)))
    for e in range(E):
        f = field[e]
        if inside:
            region = (ii < M - margin) & (jj < M - margin)
        elif e % 2 == 0:
            region = (ii >= M) | (jj >= M)              # beyond the leading square (empty on a square map)
            if not region.any():
                region = np.ones((H, W), bool)
        else:
            region = np.ones((H, W), bool)
        clr = 1.0 / res                                 # clear of the robot's threshold footprint (its corners: 0.92 m)
        free = region & (f >= clr)
        cells = _pick(rng, free, K)
        near = region & (f >= 0.95 / res) & (f < 1.1 / res)
        if near.any():
            cells[0] = _pick(rng, near, 1)[0]
        th = rng.uniform(0, 2 * np.pi, K)
        # entry 0 faces down the field's gradient: towards its nearest obstacle
        i0, j0 = cells[0]
        gx = float(f[j0, min(i0 + 1, W - 1)]) - float(f[j0, max(i0 - 1, 0)])
        gy = float(f[min(j0 + 1, H - 1), i0]) - float(f[max(j0 - 1, 0), i0])
        th[0] = np.arctan2(-gy, -gx) % (2 * np.pi)
        xy = cell_xy(cfg, cells)
        goal_cells = _pick(rng, free, K)
        goal = cell_xy(cfg, goal_cells)
        d = goal - xy
        L = np.maximum(np.linalg.norm(d, axis=1), 1e-9)
        scale = np.minimum(1.0, rng.uniform(1.0, 3.0, K) * (res / 0.05) / L)     # goals 1 .. 3 m (20 .. 60 cells) away
        goal = xy + d * scale[:, None]
        goal[0] = xy[0] + 4.0 * (res / 0.05) * np.array([np.cos(th[0]), np.sin(th[0])])     # behind the wall: never reached
        if K > 1:
            # (0.637, not 0.6: straight steps of 0.1 m would put the robot exactly distance_threshold = 0.5 m from the goal,
            # where the last bit of a position decides `distance < threshold`)
            goal[1] = xy[1] + 0.637 * (res / 0.05) * np.array([np.cos(th[1]), np.sin(th[1])])
        a["spawn_pose"][e, :, :2] = xy
        a["spawn_pose"][e, :, 2] = th
        a["spawn_goal"][e] = goal
        k0 = e % K
        a["robot_pose"][e] = a["spawn_pose"][e, k0]
        a["robot_goal"][e] = goal[k0]
        if "ped_pose" in a:
            pfree = region & (f >= 0.5 / res)
            pc = _pick(rng, pfree, N)
            a["ped_pose"][e, :, :2] = cell_xy(cfg, pc)
            a["ped_pose"][e, :, 2] = rng.uniform(0, 2 * np.pi, N)
            # walking already: between agents at rest the social force's angle is exactly 0, and its sign(theta) term then
            # hangs on the last bit of a position -- a discontinuity of the model, not a matter of geometry
            a["ped_vel"][e] = rng.uniform(-0.3, 0.3, (N, 2)) * (res / 0.05)
            for w in range(min(2, P)):
                a["ped_waypoints"][e, :, w] = cell_xy(cfg, _pick(rng, pfree, N))
            a["ped_goal"][e] = a["ped_waypoints"][e, :, min(2, P) - 1]
    return a


def actions(rng, E, t, v_scale=1.0):
    """The rollout's action of step t, float64 [E, 2]: random twists with bursts of straight driving."""
    act = np.stack([rng.uniform(0.0, 0.5, E), rng.uniform(-0.64, 0.64, E)], axis=1)
    if t % 3 != 2:
        act[::2, 0] = 0.5; act[::2, 1] = 0.0
    act[:, 0] *= v_scale
    return act


# ---- twins ---------------------------------------------------------------------------------------------------------------
_XY = ("robot_pose", "robot_goal", "prev_pose", "spawn_pose", "spawn_goal", "ped_pose", "ped_waypoints", "ped_goal")


def _copy(world):
    return {k: np.array(v, copy=True) for k, v in world.items()}


def embedded_twin(cfg, world, field_SS):
    """The same world on the S x S embedding of its maps (field_SS: the distance field of embed(occ))."""
    c = cfg.copy()
    c.map_h = c.map_w = field_SS.shape[1]
    w = _copy(world)
    w["field"] = field_SS
    return c, w


def scaled_twin(cfg, world, k=2.0):
    """The same cells at k times the resolution: every length of the configuration and of the state multiplied by k.
    (The caller multiplies the linear action by k as well; the reward's forward and rotation terms do not scale.)"""
    c = cfg.copy()
    for name in ("resolution", "range_max", "axle_offset", "min_turning_radius", "distance_threshold", "origin_x", "origin_y"):
        setattr(c, name, getattr(cfg, name) * k)
    w = _copy(world)
    for name in _XY + ("ped_vel", "ped_v_pref"):
        if name in w:
            if name == "ped_v_pref":
                w[name] *= k
            else:
                w[name][..., :2] *= k
    if "prev_action" in w:
        w["prev_action"][..., 0] *= k
    for name in ("scan_threshold", "scan_discomfort"):
        if name in w:
            w[name] = (w[name] * np.float32(k)).astype(np.float32)
    return c, w


def geometry_twin(cfg, world, origin, k):
    """scaled_twin, then translated_twin: the same cells at resolution k x cfg.resolution on a map whose origin is `origin`."""
    c, w = scaled_twin(cfg, world, k)
    return translated_twin(c, w, origin)


def translated_twin(cfg, world, origin):
    """The same world with the map's origin at `origin` and every position shifted by the same amount."""
    c = cfg.copy()
    sx, sy = origin[0] - cfg.origin_x, origin[1] - cfg.origin_y
    c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
    w = _copy(world)
    for name in _XY:
        if name in w:
            w[name][..., 0] += sx
            w[name][..., 1] += sy
    return c, w


def xy_to_ij_f32(xy, origin, resolution, map_h, map_w):
    """batch_xy_to_ij on float32 inputs (env.py:1228-1253 under NumPy 2): subtraction and division in float32, the x index
    clipped against map_h and the y index against map_w, truncated."""
    xy = np.asarray(xy, np.float32)
    f = (xy - np.asarray(origin, np.float64).astype(np.float32)) / np.float32(resolution)
    hi = np.array([map_h, map_w], np.float32)
    f = np.where(f >= hi, hi - np.float32(1), f)
    return np.where(f < 0, np.float32(0), f).astype(np.int32)


def xy_to_ij_f64(xy, origin, resolution, map_h, map_w):
    """batch_xy_to_ij on float64 inputs: float64 subtraction and division, stored to float32, clipped, truncated."""
    f = ((np.asarray(xy, np.float64) - np.asarray(origin, np.float64)) / float(resolution)).astype(np.float32)
    hi = np.array([map_h, map_w], np.float32)
    f = np.where(f >= hi, hi - np.float32(1), f)
    return np.where(f < 0, np.float32(0), f).astype(np.int32)


# ---- rollouts and the three identities (run on the oracle and on the device's own outputs alike) --------------------------
STATE = ("robot_pose", "robot_goal", "prev_pose", "prev_action", "n_hist", "episode", "steps", "ped_pose", "ped_vel",
         "ped_dist", "ped_prev_yaw", "ped_waypoints", "ped_n_waypoints", "ped_wp_head")


def rollout(reset_obs, step, state, E, steps, seed, v_scale=1.0, cmd=None):
    """reset_obs() -> obs; step(action) -> (obs, out); state() -> dict of NumPy state arrays; all NumPy.  cmd(t, action)
    is called ahead of every step (PED_EXTERNAL).  -> one record per observation: dict(obs=, out= (None for the first), plus
    the state arrays)."""
    rng = np.random.default_rng(seed)
    rec = [dict(obs=np.array(reset_obs()), out=None, **{k: np.array(v) for k, v in state().items()})]
    for t in range(steps):
        act = actions(rng, E, t, v_scale)
        if cmd is not None:
            cmd(t, rng)
        obs, out = step(act)
        rec.append(dict(obs=np.array(obs), out={k: np.array(v) for k, v in out.items()},
                        **{k: np.array(v) for k, v in state().items()}))
    return rec


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d of %d differ, max |diff| %.3e, first at %s" % (
            what, len(bad), a.size, np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))), bad[0]))


def raw_cells(xy, cfg, f32):
    """The cell indices of positions [..., 2] as xy_to_ij forms them, WITHOUT the clip against the map's sides."""
    big = 1 << 30
    org = (cfg.origin_x, cfg.origin_y)
    return (xy_to_ij_f32 if f32 else xy_to_ij_f64)(np.asarray(xy)[..., :2], org, cfg.resolution, big, big)


def _positions(r):
    """every position whose cell a step reads: the robot's pose and its pre-step pose (a crash reverts to it), the pedestrians"""
    out = [(r["robot_pose"], True), (r["prev_pose"], True)]
    if "ped_pose" in r:
        out += [(r["ped_pose"], True), (r["ped_pose"], False)]       # the pedestrian scans read float32, the social force float64
    return out


def check_embedding(cfg, rec, rec_emb, label):
    """The H x W world and its twin on the S x S embedding: every observation, output and state array bit for bit.
    Precondition (asserted): no position's cell index reaches min(H, W) on either axis, at any observation."""
    M = min(cfg.map_h, cfg.map_w)
    assert len(rec) == len(rec_emb)
    worst, covered = 0, 0
    for t, (a, b) in enumerate(zip(rec, rec_emb)):
        for xy, f32 in _positions(a):
            worst = max(worst, int(raw_cells(xy, cfg, f32).max()))
        assert worst < M, "%s: observation %d uses cell index %d beyond the leading square of %d" % (label, t, worst, M)
        _same(a["obs"], b["obs"], "%s: observation %d" % (label, t))
        if a["out"] is not None:
            assert set(a["out"]) == set(b["out"])
            for k in a["out"]:
                _same(a["out"][k], b["out"][k], "%s: %s at step %d" % (label, k, t))
        for k in STATE:
            if k in a:
                _same(a[k], b[k], "%s: state %s at observation %d" % (label, k, t))
        covered += a["obs"].shape[0]
    print("%s: embedding identity over %d arenas x %d observations = %d rows (largest cell index %d of %d)" % (
        label, rec[0]["obs"].shape[0], len(rec), covered, worst, M))
    return covered


def check_scaling(cfg, rec, rec_k, k, label):
    """The world and its twin at k times the resolution (k a power of two, no pedestrians): scans, positions, the linear
    velocity and `distance` exactly k times, yaw, the angular velocity and every flag equal.  `reward` is no part of it."""
    B = cfg.n_scan_stack * cfg.n_beams
    f, covered = np.float32(k), 0
    assert len(rec) == len(rec_k)
    for t, (a, b) in enumerate(zip(rec, rec_k)):
        _same(a["obs"][:, :B] * f, b["obs"][:, :B], "%s: scans at observation %d" % (label, t))
        _same(a["obs"][:, B:B + 5] * f, b["obs"][:, B:B + 5], "%s: prev xy, xy, v at observation %d" % (label, t))
        _same(a["obs"][:, B + 5:], b["obs"][:, B + 5:], "%s: omega, yaw at observation %d" % (label, t))
        if a["out"] is not None:
            for key in ("done", "is_success", "is_crash"):
                _same(a["out"][key], b["out"][key], "%s: %s at step %d" % (label, key, t))
            _same(a["out"]["distance"] * k, b["out"]["distance"], "%s: distance at step %d" % (label, t))
            for key in ("achieved_goal", "desired_goal"):
                _same(a["out"][key] * f, b["out"][key], "%s: %s at step %d" % (label, key, t))
        for key in ("robot_pose", "prev_pose"):
            _same(a[key][:, :2] * k, b[key][:, :2], "%s: %s xy at observation %d" % (label, key, t))
            _same(a[key][:, 2], b[key][:, 2], "%s: %s yaw at observation %d" % (label, key, t))
        _same(a["robot_goal"] * k, b["robot_goal"], "%s: goal at observation %d" % (label, t))
        for key in ("n_hist", "episode", "steps"):
            _same(a[key], b[key], "%s: %s at observation %d" % (label, key, t))
        covered += a["obs"].shape[0]
    print("%s: scaling identity (x %g) over %d arenas x %d observations = %d rows" % (
        label, k, rec[0]["obs"].shape[0], len(rec), covered))
    return covered


def check_translation(cfg, rec, cfg_t, rec_t, label, scans=True):
    """The world and its translated twin: scan rows and flags bit for bit (ranges come from integer cell offsets).
    Precondition (asserted): every position lies in the same cell in both runs, at every observation.
    scans=False (pedestrians in sight: the scan renders them from float32 primitives at another magnitude, so the rows are
    no part of the identity): the flags become a precondition too, and only the deviations are returned.
    -> (rows covered, worst deviation of the un-shifted pedestrian state: positions [m], velocities [m/s], yaw [rad])."""
    B = cfg.n_scan_stack * cfg.n_beams
    sx, sy = cfg_t.origin_x - cfg.origin_x, cfg_t.origin_y - cfg.origin_y
    covered, dev = 0, dict(ped_xy=0.0, ped_vel=0.0, ped_yaw=0.0, robot_xy=0.0)
    assert len(rec) == len(rec_t)
    for t, (a, b) in enumerate(zip(rec, rec_t)):
        for (xa, f32), (xb, _) in zip(_positions(a), _positions(b)):
            ca, cb = raw_cells(xa, cfg, f32), raw_cells(xb, cfg_t, f32)
            assert np.array_equal(ca, cb), "%s: a pose changed its cell under the shift at observation %d: %s" % (
                label, t, np.argwhere(ca != cb)[0])
        if scans:
            _same(a["obs"][:, :B], b["obs"][:, :B], "%s: scans at observation %d" % (label, t))
        if a["out"] is not None:
            for key in ("done", "is_success", "is_crash"):
                _same(a["out"][key], b["out"][key], "%s: %s at step %d" % (label, key, t))
        for key in ("n_hist", "episode", "steps", "ped_wp_head", "ped_n_waypoints"):
            if key in a:
                _same(a[key], b[key], "%s: %s at observation %d" % (label, key, t))
        un = b["robot_pose"][:, :2] - (sx, sy)
        dev["robot_xy"] = max(dev["robot_xy"], float(np.abs(un - a["robot_pose"][:, :2]).max()))
        if "ped_pose" in a:
            un = b["ped_pose"][..., :2] - (sx, sy)
            dev["ped_xy"] = max(dev["ped_xy"], float(np.abs(un - a["ped_pose"][..., :2]).max()))
            dev["ped_vel"] = max(dev["ped_vel"], float(np.abs(b["ped_vel"] - a["ped_vel"]).max()))
            dy = np.abs(b["ped_pose"][..., 2] - a["ped_pose"][..., 2])
            dev["ped_yaw"] = max(dev["ped_yaw"], float(np.minimum(dy, 2 * np.pi - dy).max()))
        covered += a["obs"].shape[0]
    print("%s: translation identity (origin %g, %g) over %d arenas x %d observations = %d rows; worst deviations %s" % (
        label, cfg_t.origin_x, cfg_t.origin_y, rec[0]["obs"].shape[0], len(rec), covered,
        ", ".join("%s %.3e" % kv for kv in sorted(dev.items()))))
    return covered, dev


def census(rec):
    """(crashes, successes, restarts) of a rollout's outputs"""
    outs = [r["out"] for r in rec if r["out"] is not None]
    return (int(sum(o["is_crash"].sum() for o in outs)), int(sum(o["is_success"].sum() for o in outs)),
            int(sum(o["done"].sum() for o in outs)))
