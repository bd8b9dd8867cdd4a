"""navsim_ped_forecast (include/navsim.h) restated in NumPy where the rule is not the step's own: the constant-velocity model
(rule 4), rel / min_dist / min_step given pose and robot_pose (rules 6 and 7), the rows of unused slots (rule 8) and of skipped
arenas (rule 1).  Every float64 operation is one NumPy operation, so each is rounded on its own; sin / cos are the CPU oracle's
(ref.math_fn), as in tests/ped_observe_spec.py.  The social force is NOT restated: navsim_step is the reference for it
(tests/test_gpu_ped_forecast.py)."""
import numpy as np

import ref

SIN, COS = 0, 1


def _f(fn, x):
    return np.asarray(ref.math_fn(fn, np.ascontiguousarray(np.atleast_1d(np.asarray(x, np.float64)))), np.float64)


def const_vel(ped_pose, ped_vel, n_peds, dt, H):
    """Rule 4 -> (pose [E,H,N,3], vel [E,H,N,2]); slots i >= n_peds[e] are 0 (rule 8)."""
    ped_pose, ped_vel = np.asarray(ped_pose, np.float64), np.asarray(ped_vel, np.float64)
    E, N = ped_pose.shape[:2]
    pose, vel = np.zeros((E, H, N, 3)), np.zeros((E, H, N, 2))
    for h in range(H):
        span = np.float64(h + 1) * np.float64(dt)
        pose[:, h, :, 0] = ped_pose[:, :, 0] + ped_vel[:, :, 0] * span
        pose[:, h, :, 1] = ped_pose[:, :, 1] + ped_vel[:, :, 1] * span
        pose[:, h, :, 2] = ped_pose[:, :, 2]
        vel[:, h] = ped_vel
    live = np.arange(N)[None, :] < np.clip(np.asarray(n_peds), 0, N)[:, None]
    pose[~live[:, None, :].repeat(H, axis=1)] = 0.0
    vel[~live[:, None, :].repeat(H, axis=1)] = 0.0
    return pose, vel


def derived(pose, robot_pose, robot_now, n_peds, horizon=None):
    """Rules 6 - 8 over the first `horizon` rows (None: all) -> {'rel' [E,h,N,2] float32, 'min_dist' [E,N] float64, 'min_step'
    [E,N] int32}.  pose [E,H,N,3], robot_pose [E,H,3]: the forecast's own; robot_now [E,3]: the state's robot_pose."""
    pose, robot_pose, robot_now = (np.asarray(a, np.float64) for a in (pose, robot_pose, robot_now))
    E, H, N = pose.shape[:3]
    H = H if horizon is None else int(horizon)
    rel = np.zeros((E, H, N, 2), np.float32)
    min_dist, min_step = np.full((E, N), np.inf), np.full((E, N), -1, np.int32)
    for e in range(E):
        n = int(min(max(int(n_peds[e]), 0), N))
        rx, ry, th = robot_now[e]
        c, s = _f(COS, th)[0], _f(SIN, th)[0]
        for h in range(H):
            ax, ay = pose[e, h, :n, 0] - rx, pose[e, h, :n, 1] - ry
            rel[e, h, :n, 0] = (c * ax + s * ay).astype(np.float32)
            rel[e, h, :n, 1] = (c * ay - s * ax).astype(np.float32)
            dx, dy = pose[e, h, :n, 0] - robot_pose[e, h, 0], pose[e, h, :n, 1] - robot_pose[e, h, 1]
            d = np.sqrt(dx * dx + dy * dy)
            less = d < min_dist[e, :n]                                  # strictly: the FIRST step that attains the minimum
            min_dist[e, :n][less] = d[less]
            min_step[e, :n][less] = h
    return dict(rel=rel, min_dist=min_dist, min_step=min_step)


def unused_rows_are_empty(out, n_peds, what=""):
    """Rule 8: the rows of slots i >= n are 0, min_dist +inf, min_step -1."""
    E, H, N = out["pose"].shape[:3]
    for e in range(E):
        n = int(min(max(int(n_peds[e]), 0), N))
        for k in ("pose", "vel", "rel"):
            assert not out[k][e, :, n:].any(), "%s: %s of arena %d behind slot %d" % (what, k, e, n)
        assert np.isposinf(out["min_dist"][e, n:]).all() and (out["min_step"][e, n:] == -1).all(), "%s: arena %d" % (what, e)


def skipped_rows_are_empty(out, arenas, what=""):
    """Rule 1: every array of a skipped arena's rows is 0, status included."""
    for k, v in out.items():
        assert not np.asarray(v)[arenas].any(), "%s: %s" % (what, k)
