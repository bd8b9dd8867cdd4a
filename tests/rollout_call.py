"""TEST INFRASTRUCTURE (GPU): navsim_rollout through the C ABI into sentinel-filled outputs, and the step itself as its reference:
the saved state put back, H navsim_step calls with sequence k, what they wrote stacked.  The small worlds, the state's save and
restore and the placement helpers are tests/lookahead_call.py's."""
import ctypes as C

import numpy as np

import lookahead_call as lc
import scan_labels_call
from gpu_support import eq, same_bits, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.ROLLOUT_OUT)
PER_STEP = ("reward", "pose")


def call(gpu, cfg, st, actions, R, gamma=1.0, ped_cmd=None, skip=None):
    """navsim_rollout into sentinel-filled outputs -> NumPy arrays.  actions: [E,K,H,2] float64."""
    torch, E = gpu.torch, cfg.n_envs
    actions = np.ascontiguousarray(actions, np.float64)
    K, H = actions.shape[1:3]
    out = {}
    for k, (dtype, tail) in abi.ROLLOUT_OUT.items():
        shape = (E,) + tuple({"K": K, "H": H}.get(s, s) for s in tail)
        out[k] = torch.full(shape, 77, dtype=getattr(torch, dtype), device=gpu.dev)
    o = abi.NavsimRolloutOut(**{k: v.data_ptr() for k, v in out.items()})
    p = abi.NavsimRolloutParams(n_seq=K, horizon=H, range=float(R), gamma=float(gamma))
    t_act = to_device(gpu, actions)
    t_cmd = None if ped_cmd is None else to_device(gpu, np.ascontiguousarray(ped_cmd, np.float64))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_rollout(C.byref(cfg), C.byref(st), C.byref(p), t_act.data_ptr(),
                                       None if t_cmd is None else t_cmd.data_ptr(), None if t_skip is None else t_skip.data_ptr(),
                                       C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def steps_of(gpu, g, saved, actions, ped_cmd=None, labels=True):
    """For every sequence k: the saved state put back, then H navsim_step calls with actions[:, k, h] -> what they wrote, stacked
    [E,K,H]: reward, done, is_success, is_crash, distance, limit (io.truncated, or done without success and crash), pose (the
    state's robot_pose behind the step: the scan pose unless the step crashed) and, with labels, navsim_scan_labels' range
    behind each step [E,K,H,B]."""
    E, K, H = actions.shape[:3]
    names = ("reward", "done", "is_success", "is_crash", "distance", "limit", "pose") + (("range",) if labels else ())
    out = {k: [] for k in names}
    for k in range(K):
        lc.load_state(g, saved)
        if ped_cmd is not None:
            g.set_ped_cmd(ped_cmd)
        seq = {name: [] for name in names}
        for h in range(H):
            _, o = g.step(to_device(gpu, actions[:, k, h]))
            o = {name: v.cpu().numpy().copy() for name, v in o.items()}
            for name in lc.STEP_KEYS:
                seq[name].append(o[name])
            seq["limit"].append(o["truncated"] if "truncated" in o
                                else o["done"] & (o["is_success"] == 0).astype(np.uint8) & (o["is_crash"] == 0).astype(np.uint8))
            seq["pose"].append(g.t["robot_pose"].cpu().numpy().copy())
            if labels:
                seq["range"].append(scan_labels_call.call(gpu, g.cfg, g.st, hits=g.cfg.ped_model != abi.PED_NONE)["range"])
        for name in names:
            out[name].append(np.stack(seq[name], axis=1))
    lc.load_state(g, saved)
    return {name: np.stack(v, axis=1) for name, v in out.items()}


def expected_length(step):
    """[E,K]: index of the first done step + 1, else H."""
    done = step["done"] != 0
    H = done.shape[2]
    return np.where(done.any(axis=2), done.argmax(axis=2) + 1, H).astype(np.int32)


def same_as_steps(roll, step, what, gamma=1.0, thr=None, dthr=None, R=None):
    """Rule by rule against the step's own results, for every row h < min(length, exact_steps) -- and never fewer rows than the
    step's own first done index allows.  Returns the number of rows compared."""
    E, K, H = step["reward"].shape
    want_len = expected_length(step)
    exact = roll["exact_steps"]
    assert (roll["status"] == 1).all() and ((exact >= 1) & (exact <= H)).all()
    rows = 0
    for e in range(E):
        for k in range(K):
            L, X = int(roll["length"][e, k]), int(exact[e, k])
            n = min(L, X)
            if X >= want_len[e, k]:
                assert L == want_len[e, k], "%s: length[%d,%d] = %d, the step's %d" % (what, e, k, L, want_len[e, k])
            else:
                assert L >= X or L == want_len[e, k]
            tag = "%s: [%d,%d]" % (what, e, k)
            same_bits(roll["reward"][e, k, :n], step["reward"][e, k, :n], tag + " reward")
            crash = step["is_crash"][e, k, :n] != 0
            same_bits(roll["pose"][e, k, :n][~crash], step["pose"][e, k, :n][~crash], tag + " pose")
            assert not roll["reward"][e, k, L:].any() and not roll["pose"][e, k, L:].any(), tag + " rows behind length"
            rows += n
            if L - 1 < X:                                          # the last evaluated step is an exact one
                h = L - 1
                want = int(step["is_success"][e, k, h] != 0) | int(step["is_crash"][e, k, h] != 0) << 1 | int(step["limit"][e, k, h] != 0) << 2
                assert int(roll["outcome"][e, k]) == want, "%s outcome %d, the step's %d" % (tag, roll["outcome"][e, k], want)
                same_bits(roll["distance"][e, k], step["distance"][e, k, h], tag + " distance")
                ret, g_ = 0.0, 1.0                                 # float64, in the stated order
                for r in roll["reward"][e, k, :L]:
                    ret = ret + g_ * float(r)
                    g_ = g_ * float(gamma)
                same_bits(roll["ret"][e, k], np.float64(ret), tag + " ret")
                if thr is not None and "range" in step:
                    rng = step["range"][e, k, :L]
                    cr = step["is_crash"][e, k, :L] != 0
                    disc = (rng < dthr).any(axis=1) & ~cr
                    assert int(roll["discomfort_steps"][e, k]) == int(disc.sum()), tag + " discomfort_steps"
                    if not cr.any():
                        margin = (np.minimum(rng, np.float32(R)) - thr).min()
                        same_bits(roll["min_margin"][e, k], np.float32(margin), tag + " min_margin")
                    assert (roll["min_margin"][e, k] < 0) == bool(cr.any()), tag + " margin's sign"
    return rows


def zero_rows(out, arenas, what):
    """Every array of the arenas' rows is 0 (status included)."""
    for name in KEYS:
        assert not out[name][arenas].any(), "%s: %s" % (what, name)


__all__ = ["call", "steps_of", "same_as_steps", "expected_length", "zero_rows", "KEYS", "eq"]
