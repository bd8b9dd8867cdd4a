"""TEST INFRASTRUCTURE: independent float64 references for pedestrians in a scan and for the social force (NumPy and math
only: no import of the oracle, of ref or of nav_gym_amd; configurations are read by attribute).

Lidar.  Beam k of a lidar at pose (x, y, yaw) looks along
fl32(linspace(angle_min, angle_last, B)[k] + fl32(yaw)) from (fl32(x), fl32(y)).  Pedestrians are 0.44 x 0.38 m rectangles, or
with legs two discs of 3 cm radius; their float32 vertices and centres are formed as row a6 states.  Every primitive is then
taken into the BEAM'S frame (the beam is the +x axis) in float64: a side is hit where it crosses y = 0 at x >= 0, a disc
where |y_c| <= r, at x_c - sqrt(r^2 - y_c^2) >= 0.  The walls' ranges are an input (they come from the oracle's march).
A beam is a SILHOUETTE beam when it passes within 1e-5 rad of a vertex's bearing or of a disc's tangent: there a hit
appears or vanishes with the last bit of a product, in any arithmetic.

Social force (written from the model's definition with angles): desired force (v_pref e - v) / tau;
Moussaid's interaction with every other pedestrian and the robot -- t = lambda (v_i - v_j) + d, B = gamma |t|, theta the angle
from t to d, -exp(-dist / B - (n' B theta)^2) along t and -sign(theta) exp(-dist / B - (n B theta)^2) along t's left normal;
exp(-(d_wall - r) / sigma), saturating at 1 for d_wall <= r, along the distance field's central-difference gradient; weights 1 / 2.1 / 10; v += a dt, clamped to
v_pref; x += v dt; heading = direction of motion above 1e-6 m/s.  sfm_step reports every degenerate branch it takes."""
import math

import numpy as np

FOOTPRINT = np.array([[0.22, 0.19], [-0.22, 0.19], [-0.22, -0.19], [0.22, -0.19]])      # human.py:5-10
LEG_RADIUS = float(np.float32(0.03))
SILHOUETTE = 1e-5           # rad


# ---- lidar -----------------------------------------------------------------------------------------------------------------------
def beam_headings(angle_min, angle_last, n_beams, yaw):
    """float32 [B]: where env.py:424 rounds the beam angle"""
    lin = np.linspace(angle_min, angle_last, n_beams) if n_beams > 1 else np.array([angle_min])
    return (lin + float(np.float32(yaw))).astype(np.float32)


def rectangle(pose, footprint=FOOTPRINT):
    """float32 [4, 2]: the footprint through T(x, y) R(yaw), float64 arithmetic on the float64 pose"""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    fp = np.asarray(footprint, np.float64).reshape(4, 2)
    return np.stack([c * fp[:, 0] - s * fp[:, 1] + pose[0], s * fp[:, 0] + c * fp[:, 1] + pose[1]], 1).astype(np.float32)


def leg_centres(pose, dist):
    """float32 [2, 2]: row a6 on the float32 pose and leg odometry"""
    px, py, th = (float(np.float32(v)) for v in pose)
    dx, dy, dth = (float(np.float32(v)) for v in dist)
    front = 0.3 * math.cos(dx * 2.0 / 0.3 + dth)
    side = 0.1 * math.cos(dy * 2.0 / 0.1 + dth)
    c, s = math.cos(th), math.sin(th)
    legs = [(front, side + 0.1), (-front, -side - 0.1)]
    return np.array([[c * x - s * y + px, s * x + c * y + py] for x, y in legs]).astype(np.float32)


def scan(origin_xy, headings, segs, discs, wall, clip):
    """ranges float64 [B] and the silhouette mask [B]: float32 inputs, float64 arithmetic.
    segs [S, 2, 2] (end points), discs [D, 2] (centres), wall [B] the walls' ranges in metres, clip = range_max."""
    L = np.asarray(origin_xy, np.float32).astype(np.float64)
    ang = np.asarray(headings, np.float32).astype(np.float64)
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    r = np.asarray(wall, np.float64).copy()
    sil = np.zeros(len(ang), bool)
    segs = np.asarray(segs, np.float32).astype(np.float64).reshape(-1, 2, 2)
    discs = np.asarray(discs, np.float32).astype(np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        if len(segs):
            w = segs - L                                                # [S, 2, 2]
            x = c[:, :, None] * w[None, :, :, 0] + s[:, :, None] * w[None, :, :, 1]      # [B, S, 2]: along the beam
            y = c[:, :, None] * w[None, :, :, 1] - s[:, :, None] * w[None, :, :, 0]      # to its left
            yp, yq, xp, xq = y[..., 0], y[..., 1], x[..., 0], x[..., 1]
            cross = (yp * yq <= 0.0) & (yp != yq)                       # the side meets the beam's line (end points included)
            t = xp + (xq - xp) * (yp / (yp - yq))
            hit = cross & (t >= 0.0)
            r = np.minimum(r, np.where(hit, t, np.inf).min(axis=1))
            sil |= ((np.abs(np.arctan2(y, x)) < SILHOUETTE) & (np.hypot(x, y) > 0)).any(axis=(1, 2))
        if len(discs):
            w = discs - L
            x = c * w[None, :, 0] + s * w[None, :, 1]                   # [B, D]
            y = c * w[None, :, 1] - s * w[None, :, 0]
            h2 = LEG_RADIUS * LEG_RADIUS - y * y
            t = x - np.sqrt(h2)
            hit = (h2 >= 0.0) & (t >= 0.0)
            r = np.minimum(r, np.where(hit, t, np.inf).min(axis=1))
            d = np.hypot(x, y)
            half = np.arcsin(np.minimum(1.0, LEG_RADIUS / d))
            b = np.arctan2(y, x)
            sil |= ((d > LEG_RADIUS) & ((np.abs(b - half) < SILHOUETTE) | (np.abs(b + half) < SILHOUETTE))).any(axis=1)
    return np.clip(r, 0.0, clip), sil


def robot_scan(cfg, state, e, wall):
    """The robot's scan of arena e from the state arrays (robot_pose, n_peds, ped_pose, ped_dist, ped_has_legs)."""
    n = min(int(state["n_peds"][e]), cfg.max_peds) if "n_peds" in state else 0
    segs, discs = [], []
    for i in range(n):
        pose = state["ped_pose"][e, i]
        if state["ped_has_legs"][e, i] and cfg.lidar_legs:
            discs.extend(leg_centres(pose, state["ped_dist"][e, i]))
        else:
            v = rectangle(pose)
            segs.extend([(v[k], v[(k + 1) % 4]) for k in range(4)])
    rp = state["robot_pose"][e]
    return scan(rp[:2], beam_headings(cfg.angle_min, cfg.angle_last, cfg.n_beams, rp[2]), segs, discs, wall, cfg.range_max)


def ped_scan(cfg, state, e, i, wall):
    """Pedestrian i's scan (env.py:685-693): the other pedestrians and the robot as rectangles, no legs."""
    n = min(int(state["n_peds"][e]), cfg.max_peds)
    segs = []
    for a in range(n + 1):
        if a == i:
            continue
        v = rectangle(state["ped_pose"][e, a]) if a < n else rectangle(state["robot_pose"][e], list(cfg.robot_seen_footprint))
        segs.extend([(v[k], v[(k + 1) % 4]) for k in range(4)])
    pp = state["ped_pose"][e, i]
    return scan(pp[:2], beam_headings(cfg.ped_angle_min, cfg.ped_angle_last, cfg.ped_n_beams, pp[2]), segs, [], wall, cfg.ped_range_max)


def origin_cell(cfg, xy):
    """batch_xy_to_ij on a float32 position (env.py:419 under NumPy 2): float32 arithmetic, clipped, truncated -> (i, j)"""
    f = (np.asarray(xy, np.float32) - np.array([cfg.origin_x, cfg.origin_y]).astype(np.float32)) / np.float32(cfg.resolution)
    hi = np.array([cfg.map_h, cfg.map_w], np.float32)
    f = np.where(f >= hi, hi - np.float32(1), f)
    return np.where(f < 0, np.float32(0), f).astype(np.int32)


# ---- social force ------------------------------------------------------------------------------------------------------------------
def _cell64(cfg, x, y):
    """batch_xy_to_ij on a float64 position: float64 arithmetic stored to float32, clipped, truncated"""
    out = []
    for v, o, hi in ((x, cfg.origin_x, cfg.map_h), (y, cfg.origin_y, cfg.map_w)):
        f = np.float32((v - o) / cfg.resolution)
        f = np.float32(hi - 1) if f >= np.float32(hi) else f
        out.append(int(np.float32(0) if f < 0 else f))
    return out


def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def sfm_step(cfg, field, robot_pose, robot_speed, pos, vel, yaw, v_pref, wp, n):
    """One social-force step of the first n pedestrians of an arena.  field float32 [H, W] (cells); robot_speed = the linear
    velocity of its previous action; pos [N, 2], vel [N, 2], yaw [N], v_pref [N], wp [N, 2] (current waypoints), float64.
    -> (pos, vel, yaw) of the n pedestrians, report: list of (kind, i, j), j = n for the robot, None for a branch of i alone;
    kinds: coincident, il0 (pair skipped), theta0 (no angular term), at_waypoint, flat_field, saturated, clamp, heading_kept;
    and min_theta: the smallest non-zero |theta| met."""
    H, W = field.shape
    dt = cfg.time_step
    A = [(pos[i][0], pos[i][1], vel[i][0], vel[i][1]) for i in range(n)]
    A.append((robot_pose[0], robot_pose[1], robot_speed * math.cos(robot_pose[2]), robot_speed * math.sin(robot_pose[2])))
    report, min_theta = [], math.inf
    new = []
    for i in range(n):
        xi, yi, vxi, vyi = A[i]
        # desired
        ex, ey = wp[i][0] - xi, wp[i][1] - yi
        L = math.hypot(ex, ey)
        if L > 1e-9:
            ex, ey = ex / L, ey / L
        else:
            ex = ey = 0.0
            report.append(("at_waypoint", i, None))
        fx = cfg.sfm_k_desired * (v_pref[i] * ex - vxi) / cfg.sfm_tau
        fy = cfg.sfm_k_desired * (v_pref[i] * ey - vyi) / cfg.sfm_tau
        # social
        sx = sy = 0.0
        for j in range(n + 1):
            if j == i:
                continue
            xj, yj, vxj, vyj = A[j]
            dx, dy = xj - xi, yj - yi
            dist = math.hypot(dx, dy)
            if dist < 1e-9:
                report.append(("coincident", i, j))
                continue
            tx = cfg.sfm_lambda * (vxi - vxj) + dx / dist
            ty = cfg.sfm_lambda * (vyi - vyj) + dy / dist
            tl = math.hypot(tx, ty)
            if tl < 1e-9:
                report.append(("il0", i, j))
                continue
            theta = math.atan2(tx * dy - ty * dx, tx * dx + ty * dy)        # from t to d, both unnormalised
            Bq = cfg.sfm_gamma * tl
            if theta == 0.0:
                report.append(("theta0", i, j))
            else:
                min_theta = min(min_theta, abs(theta))
            decel = -math.exp(-dist / Bq - (cfg.sfm_n_prime * Bq * theta) ** 2)
            turn = -math.copysign(1.0, theta) * math.exp(-dist / Bq - (cfg.sfm_n * Bq * theta) ** 2) if theta != 0.0 else 0.0
            ux, uy = tx / tl, ty / tl
            sx += decel * ux - turn * uy
            sy += decel * uy + turn * ux
        # obstacles
        ci, cj = _cell64(cfg, xi, yi)
        ci, cj = min(ci, W - 1), min(cj, H - 1)
        gx = float(field[cj, min(ci + 1, W - 1)]) - float(field[cj, max(ci - 1, 0)])
        gy = float(field[min(cj + 1, H - 1), ci]) - float(field[max(cj - 1, 0), ci])
        gl = math.hypot(gx, gy)
        ox = oy = 0.0
        if gl > 0.0:
            depth = -(float(field[cj, ci]) * cfg.resolution - cfg.sfm_agent_radius) / cfg.sfm_sigma_obstacle
            if depth > 0.0:                                 # nearer to the wall than the agent's radius: the force saturates
                report.append(("saturated", i, None))
            mag = math.exp(min(depth, 0.0))
            ox, oy = mag * gx / gl, mag * gy / gl
        else:
            report.append(("flat_field", i, None))
        vx = vxi + (fx + cfg.sfm_k_social * sx + cfg.sfm_k_obstacle * ox) * dt
        vy = vyi + (fy + cfg.sfm_k_social * sy + cfg.sfm_k_obstacle * oy) * dt
        sp = math.hypot(vx, vy)
        if sp > v_pref[i]:
            k = v_pref[i] / sp if sp > 0.0 else 0.0
            vx, vy = vx * k, vy * k
            report.append(("clamp", i, None))
        th = yaw[i]
        if math.hypot(vx, vy) > 1e-6:
            th = math.atan2(vy, vx) % (2 * math.pi)
        else:
            report.append(("heading_kept", i, None))
        new.append((xi + vx * dt, yi + vy * dt, vx, vy, th))
    new = np.array(new, np.float64).reshape(n, 5)
    return new[:, 0:2], new[:, 2:4], new[:, 4], report, min_theta
