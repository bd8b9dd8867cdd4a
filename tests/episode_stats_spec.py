"""Episode statistics (include/navsim.h navsim_episode_stats_update / _clear) in plain NumPy: float64, the header's
operation order, one arena at a time.  The yardstick of tests/test_episode_stats.py and tests/test_gpu_episode_stats.py."""
import math

import numpy as np

AUTORESET_NONE, AUTORESET_SAME_STEP, AUTORESET_NEXT_STEP = 0, 1, 2
SUCCESS, CRASH, TIME_LIMIT = 1, 2, 4
TOTALS = ("episodes", "successes", "crashes", "time_limits", "steps")
ACCUMULATORS = (("ret", np.float64), ("length", np.int32), ("path_length", np.float64), ("min_clearance", np.float64),
                ("discomfort_steps", np.int32))
PUBLISHED = (("ep_return", np.float64), ("ep_length", np.int32), ("ep_path_length", np.float64),
             ("ep_min_clearance", np.float64), ("ep_discomfort_steps", np.int32), ("ep_outcome", np.uint8))


class EpisodeStats(object):
    def __init__(self, n_envs, n_beams, n_scan_stack, auto_reset, scan_threshold, scan_discomfort):
        self.E, self.B, self.S, self.auto_reset = int(n_envs), int(n_beams), int(n_scan_stack), int(auto_reset)
        self.thr = np.asarray(scan_threshold, dtype=np.float32).reshape(self.B)
        self.dthr = np.asarray(scan_discomfort, dtype=np.float32).reshape(self.B)
        for k, d in ACCUMULATORS + PUBLISHED:
            setattr(self, k, np.zeros(self.E, dtype=d))
        self.totals = np.zeros(len(TOTALS), dtype=np.uint64)
        self.clear()

    def clear(self, mask=None):
        for e in range(self.E):
            if mask is None or mask[e]:
                self.ret[e], self.length[e], self.path_length[e] = 0.0, 0, 0.0
                self.min_clearance[e], self.discomfort_steps[e] = np.inf, 0

    def update(self, obs, reward, done, is_success, is_crash, truncated=None, final_obs=None, reset_mask=None):
        """One call behind a step.  Returns the arenas that finished, as a list."""
        B, S = self.B, self.S
        if self.auto_reset == AUTORESET_SAME_STEP:
            assert final_obs is not None
        if self.auto_reset == AUTORESET_NEXT_STEP:
            assert reset_mask is not None
        finished = []
        for e in range(self.E):
            if self.auto_reset == AUTORESET_NEXT_STEP and reset_mask[e]:
                continue                                    # the call reset the arena: reward 0 is no step of an episode
            row = final_obs[e] if (self.auto_reset == AUTORESET_SAME_STEP and done[e]) else obs[e]
            row = np.asarray(row, dtype=np.float32)
            scan, tail = row[(S - 1) * B: S * B], row[S * B:]
            self.length[e] += 1
            self.ret[e] = np.float64(self.ret[e]) + np.float64(reward[e])
            dx = float(tail[2]) - float(tail[0])
            dy = float(tail[3]) - float(tail[1])
            self.path_length[e] = float(self.path_length[e]) + math.sqrt(dx * dx + dy * dy)
            clear = (scan.astype(np.float64) - self.thr.astype(np.float64)).min()
            if clear < self.min_clearance[e]:
                self.min_clearance[e] = clear
            crash_row = bool((scan < self.thr).any())
            if bool((scan < self.dthr).any()) and not crash_row:
                self.discomfort_steps[e] += 1
            if done[e]:
                limit = truncated is not None and bool(truncated[e])
                outcome = (SUCCESS if is_success[e] != 0 else 0) | (CRASH if is_crash[e] != 0 else 0) | (TIME_LIMIT if limit else 0)
                self.ep_return[e], self.ep_length[e], self.ep_path_length[e] = self.ret[e], self.length[e], self.path_length[e]
                self.ep_min_clearance[e], self.ep_discomfort_steps[e] = self.min_clearance[e], self.discomfort_steps[e]
                self.ep_outcome[e] = outcome
                self.totals += np.array([1, bool(outcome & SUCCESS), bool(outcome & CRASH), bool(outcome & TIME_LIMIT),
                                         int(self.length[e])], dtype=np.uint64)
                self.clear([i == e for i in range(self.E)])
                finished.append(e)
        return finished

    def published(self):
        return {k: getattr(self, k).copy() for k, _ in PUBLISHED}

    def accumulators(self):
        return {k: getattr(self, k).copy() for k, _ in ACCUMULATORS}

    def totals_dict(self):
        return {k: int(self.totals[i]) for i, k in enumerate(TOTALS)}
