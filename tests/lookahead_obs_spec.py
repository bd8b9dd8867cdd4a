"""TEST INFRASTRUCTURE (CPU): rules 6 - 8 of navsim_lookahead_obs (include/navsim.h) restated in NumPy -- the row pose behind a
crash, the tail, the goals, the shared crash re-scan copied into the crashing candidates, and the row assembled from the previous
observation.  tests/test_lookahead_obs.py holds it to the reference's recorded traces."""
import numpy as np


def wrap_pi(a):
    return np.arctan2(np.sin(a), np.cos(a))                                  # env.py:454


def row_pose(crash, prev_pose, pose):
    """Rule 6: behind a crash the row describes prev_pose (env.py:707-717), else the candidate's pose.  [K,3] float64."""
    crash = np.asarray(crash, bool)
    return np.where(crash[:, None], np.asarray(prev_pose, np.float64)[None, :], np.asarray(pose, np.float64))


def tails(prev_pose, poses, prev_action):
    """Rule 7: [K,7] float32 of (prev_pose xy, row pose xy, prev_action, wrapped row yaw); poses: row_pose()'s [K,3]."""
    K = len(poses)
    t = np.empty((K, 7), np.float64)
    t[:, 0:2] = np.asarray(prev_pose, np.float64)[:2]
    t[:, 2:4] = poses[:, :2]
    t[:, 4:6] = np.asarray(prev_action, np.float64)
    t[:, 6] = wrap_pi(poses[:, 2])
    return t.astype(np.float32)


def goals(poses, goal):
    """Rule 7: [K,4] float32 of (row pose xy, robot_goal)."""
    return np.concatenate([poses[:, :2], np.broadcast_to(np.asarray(goal, np.float64), (len(poses), 2))], axis=1).astype(np.float32)


def crash_copy(scans, crash, rescan):
    """Rule 6: the one re-scan of the arena in the place of every crashing candidate's scan.  scans [K,B], rescan [B]."""
    crash = np.asarray(crash, bool)
    return np.where(crash[:, None], np.asarray(rescan, np.float32)[None, :], np.asarray(scans, np.float32))


def rows(obs_prev, n_hist, scans, tail, S):
    """Rule 8: [K, S*B+7] float32.  Slot S - 1 is the candidate's scan; slot j < S - 1 is slot j + 1 of obs_prev where
    S - 1 - j <= n_hist, else the scan (env.py:257-279)."""
    scans = np.asarray(scans, np.float32)
    K, B = scans.shape
    prev = np.asarray(obs_prev, np.float32)[:S * B].reshape(S, B)
    out = np.empty((K, S * B + 7), np.float32)
    for j in range(S):
        old = j < S - 1 and S - 1 - j <= n_hist
        out[:, j * B:(j + 1) * B] = prev[j + 1][None, :] if old else scans
    out[:, S * B:] = tail
    return out


def next_n_hist(n_hist, S):
    return min(n_hist + 1, S - 1)                                            # the step's phase 6


def first_n_hist(S):
    return min(1, S - 1)                                                     # ... and behind a reset
