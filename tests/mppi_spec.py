"""navsim_mppi (include/navsim.h) restated in NumPy, rule by rule.  The Gaussian draws g [E,K,H,2] and navsim_rollout's outputs
are INPUTS: everything else -- the warm start, the AR(1) chain and the clamp, the cost, the weights and the new plan -- is float64
NumPy with one operation per rounding, exp_neg from the oracle (ref math fn 3) and the goal-field lookup from
tests/goal_path_spec.py.  Also: the streams of rule 4 (scan_noise_f64.hash4) and, from them, the draws of the float64 model and
the words navsim_debug_math fn 17 takes to return the device's own."""
import numpy as np

import goal_path_spec as gps
import ref
import scan_noise_f64 as noise

EXP_NEG = 3
PURPOSE = 0x6D707069
CRASH = 2                                    # bit 1 of navsim_rollout's outcome
OK, ALL_CRASH = 1, 2
DEFAULT = dict(n_samples=4, horizon=3, iterations=1, stop_sample=1, select=0, sigma=(0.1, 0.2), lo=(0.0, -0.64), hi=(0.5, 0.64),
               init_action=(0.0, 0.0), beta=0.0, lam=0.05, w_goal=1.0, w_crash=100.0, off_field_cost=10.0)


def params(**kw):
    """A parameter dict with alpha = sqrt(1 - beta^2) as the host computes it."""
    p = dict(DEFAULT, **kw)
    for k in ("sigma", "lo", "hi", "init_action"):
        p[k] = np.asarray(p[k], np.float64)
    p["beta"] = np.float64(p["beta"])
    p["alpha"] = np.sqrt(np.float64(1.0) - p["beta"] * p["beta"])
    for k in ("lam", "w_goal", "w_crash", "off_field_cost"):
        p[k] = np.float64(p[k])
    return p


def clamp(v, lo, hi):
    """min(max(v, lo), hi) as the device writes it: two selects"""
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


# ---- rule 2 ---------------------------------------------------------------------------------------------------------------------
def warm_start(plan, plan_key, episode, steps, p, skip=None):
    """-> (plan [E,H,2], plan_key [E,2], mode [E]: 0 kept, 1 shifted, 2 fresh, -1 skipped); the inputs are not modified."""
    plan, key = np.array(plan, np.float64), np.array(plan_key, np.int64)
    mode = np.full(len(plan), -1)
    for e in range(len(plan)):
        if skip is not None and skip[e]:
            continue
        ep, s = int(episode[e]), int(steps[e])
        if (int(key[e, 0]), int(key[e, 1])) == (ep, s):
            mode[e] = 0
        elif (int(key[e, 0]), int(key[e, 1])) == (ep, s - 1):
            mode[e] = 1
            plan[e, :-1] = plan[e, 1:].copy()
        else:
            mode[e] = 2
            plan[e] = p["init_action"]
        key[e] = (ep, s)
    return plan, key, mode


# ---- rule 4 ---------------------------------------------------------------------------------------------------------------------
def streams(seed, env_index_base, episode, steps, it, K):
    """uint64 [E,K]: stream_k of every arena"""
    out = np.zeros((len(episode), K), np.uint64)
    purpose = np.array([(PURPOSE + (k << 32)) & noise.M64 for k in range(K)], np.uint64)
    for e in range(len(episode)):
        key = ((int(episode[e]) << 32) + (int(steps[e]) << 3) + int(it)) & noise.M64
        out[e] = noise.hash4((int(seed) ^ key) & noise.M64, int(env_index_base) + e, key, purpose)
    return out


def draws_model(stream, H):
    """g [E,K,H,2] of the float64 model: beam 2 h + c of stream_k"""
    return noise.gauss(stream, np.arange(2 * H)).reshape(stream.shape + (H, 2))


def debug_words(stream, H):
    """(x, x2) float64 [E*K*2H] for navsim_debug_math fn 17, whose beam is the ELEMENT INDEX i: element i = (e, k, b) carries the
    stream's high word and a low word changed so that low' ^ i * 0x9E3779B9 == low ^ b * 0x9E3779B9 (32-bit), which is all
    gauss_noise reads of the pair -- the value returned is gauss_noise(stream_k, b), bit for bit."""
    n = stream.size * 2 * H
    i = np.arange(n, dtype=np.uint64)
    b = i % np.uint64(2 * H)
    s = np.repeat(stream.reshape(-1), 2 * H)
    mul = np.uint64(0x9E3779B9)
    m32 = np.uint64(noise.M32)
    lo = (s & m32) ^ ((b * mul) & m32) ^ ((i * mul) & m32)
    return lo.astype(np.float64), (s >> np.uint64(32)).astype(np.float64)


def sample(plan, g, p):
    """actions [E,K,H,2] from the plan [E,H,2] and the draws g [E,K,H,2]"""
    E, K, H = g.shape[:3]
    lo, hi, sigma = p["lo"], p["hi"], p["sigma"]
    act = np.zeros((E, K, H, 2))
    eps = None
    for h in range(H):
        eps = g[:, :, 0] if h == 0 else p["beta"] * eps + p["alpha"] * g[:, :, h]
        act[:, :, h] = clamp(plan[:, None, h] + sigma * eps, lo, hi)
    act[:, 0] = clamp(plan, lo, hi)
    if p["stop_sample"] and K >= 2:
        act[:, 1] = clamp(np.zeros(2), lo, hi)
    return act


# ---- rule 6 ---------------------------------------------------------------------------------------------------------------------
def terminal_xy(roll):
    """(x, y) [E,K,2] of pose[e,k,L-1]"""
    L = roll["length"].astype(np.int64)
    E, K = L.shape
    return roll["pose"][np.arange(E)[:, None], np.arange(K)[None, :], np.maximum(L, 1) - 1, :2]


def field_distance(cfg, fields, dist, goal, xy, gp, map_slot=None):
    """D [E,K] float64 and off [E,K] bool: rules 3 - 6 of navsim_goal_path for a robot at xy[e,k] on arena e's field dist[e]
    (fields [M,H,W] float32: what the classes come from)"""
    E, K = xy.shape[:2]
    D, off = np.zeros((E, K)), np.zeros((E, K), bool)
    for e in range(E):
        slot = 0 if cfg.shared_field else (e if map_slot is None else int(map_slot[e]))
        m = gps.classes(cfg, fields[slot], gp)
        for k in range(K):
            d, _, status = gps.query(cfg, m, dist[e], (xy[e, k, 0], xy[e, k, 1], 0.0), goal[e], gp)
            D[e, k], off[e, k] = np.float64(d), status == gps.OFF_FIELD
    return D, off


def cost(roll, p, D=None, off=None):
    """J [E,K] and crash [E,K].  D / off: field_distance's; None: the rollout's own distance."""
    crash = (roll["outcome"] & CRASH) != 0
    if D is None:
        D = roll["distance"].astype(np.float64)
    else:
        D = np.where(off, D + p["off_field_cost"], D)
    J = p["w_goal"] * D - roll["ret"]
    return np.where(crash, J + p["w_crash"], J), crash


# ---- rules 7 and 8 --------------------------------------------------------------------------------------------------------------
def exp_neg(x):
    return ref.math_fn(EXP_NEG, np.ascontiguousarray(x, np.float64).reshape(-1)).reshape(np.shape(x))


def update(actions, J, crash, p):
    """-> dict(plan [E,H,2], w [E,K], jmin, best, cost_best, S, Q, ess, status, action)"""
    E, K, H = actions.shape[:3]
    jmin, best = J[:, 0].copy(), np.zeros(E, np.int32)
    for e in range(E):
        bk = (bool(crash[e, 0]), J[e, 0], 0)
        for k in range(1, K):
            if J[e, k] < jmin[e]:
                jmin[e] = J[e, k]
            if (bool(crash[e, k]), J[e, k], k) < bk:
                bk = (bool(crash[e, k]), J[e, k], k)
        best[e] = bk[2]
    w = exp_neg(-((J - jmin[:, None]) / p["lam"]))
    S, Q, m = np.zeros(E), np.zeros(E), np.zeros((E, H, 2))
    for k in range(K):
        S = S + w[:, k]
        Q = Q + w[:, k] * w[:, k]
        m = m + w[:, k, None, None] * actions[:, k]
    plan = clamp(m / S[:, None, None], p["lo"], p["hi"])
    rows = np.arange(E)
    return dict(plan=plan, w=w, jmin=jmin, best=best, cost_best=J[rows, best], S=S, Q=Q, ess=S * S / Q,
                status=np.where(crash.all(axis=1), ALL_CRASH, OK).astype(np.uint8),
                action=actions[rows, best, 0] if p["select"] else plan[:, 0])


def outputs(u, J, skip=None):
    """navsim_mppi_out and ws->cost as the call leaves them -> dict of arrays with the ABI's dtypes (rule 1 for skipped arenas)"""
    out = dict(action=np.array(u["action"], np.float64), best=u["best"].astype(np.int32), cost_best=np.array(u["cost_best"], np.float64),
               ess=np.array(u["ess"], np.float64), status=u["status"].astype(np.uint8), cost=np.array(J, np.float64))
    if skip is not None:
        for v in out.values():
            v[np.asarray(skip) != 0] = 0
    return out
