"""CPU: the MPPI local planner (include/navsim.h navsim_mppi) -- the NumPy restatement tests/mppi_spec.py against hand-worked cases,
the three warm-start branches, the entry's place in the C ABI, its argument refusals (all of them come back before the device is
touched), the defaults and the keywords on NavGymEnv.  The device against the restatement is tests/test_gpu_mppi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mppi_spec as spec
from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def fake_roll(E, K, H, rng, crash=None):
    """Rollout outputs the specification can read: lengths H, random returns and distances, poses on a line."""
    pose = rng.uniform(1.0, 4.0, (E, K, H, 3))
    return dict(ret=rng.uniform(-0.2, 0.2, (E, K)), distance=rng.uniform(0.5, 5.0, (E, K)), length=np.full((E, K), H, np.int32),
                outcome=(np.zeros((E, K), np.uint8) if crash is None else np.where(crash, 2, 0).astype(np.uint8)), pose=pose)


# ---- the specification against hand-worked cases ------------------------------------------------------------------------------
def test_zero_sigma_and_equal_costs_keep_the_plan_bit_for_bit():
    """sigma = 0 and no stop sample: every sequence IS the plan; with equal costs every weight is exactly 1, S = K = 4 and
    (4 x) / 4 == x in binary floating point: the new plan equals the old one bit for bit, ess = K."""
    rng = np.random.default_rng(1)
    E, K, H = 3, 4, 5
    p = spec.params(n_samples=K, horizon=H, sigma=(0.0, 0.0), stop_sample=0, beta=0.6)
    plan = np.stack([rng.uniform(0.0, 0.5, (E, H)), rng.uniform(-0.64, 0.64, (E, H))], axis=2)
    act = spec.sample(plan, rng.standard_normal((E, K, H, 2)), p)
    for k in range(K):
        assert np.array_equal(bits(act[:, k]), bits(plan))
    roll = fake_roll(E, K, H, rng)
    roll["ret"][:] = roll["ret"][:, :1]; roll["distance"][:] = roll["distance"][:, :1]
    J, crash = spec.cost(roll, p)
    u = spec.update(act, J, crash, p)
    assert (u["w"] == 1.0).all() and (u["S"] == K).all() and (u["ess"] == K).all()
    assert np.array_equal(bits(u["plan"]), bits(plan))
    assert (u["best"] == 0).all() and (u["status"] == spec.OK).all()            # a tie goes to the lowest k
    assert np.array_equal(bits(u["action"]), bits(plan[:, 0]))


def test_tiny_lambda_picks_the_cheapest_sequence():
    """lambda tiny: every weight but the cheapest sequence's underflows to exactly 0 -- plan == actions[jmin], ess == 1."""
    rng = np.random.default_rng(2)
    E, K, H = 4, 7, 3
    p = spec.params(n_samples=K, horizon=H, lam=1e-9, beta=0.5, select=1)
    plan = np.zeros((E, H, 2))
    act = spec.sample(plan, rng.standard_normal((E, K, H, 2)), p)
    assert not act[:, 1].any()                                                   # the stop sample
    assert (act[..., 0] >= 0.0).all() and (act[..., 0] <= 0.5).all() and (np.abs(act[..., 1]) <= 0.64).all()
    J, crash = spec.cost(fake_roll(E, K, H, rng), p)
    u = spec.update(act, J, crash, p)
    kmin = J.argmin(axis=1)
    rows = np.arange(E)
    assert (u["w"][rows, kmin] == 1.0).all() and (np.delete(u["w"], kmin[0], axis=1)[0] == 0.0).all() and (u["w"].sum(axis=1) == 1.0).all()
    assert (u["ess"] == 1.0).all() and (u["best"] == kmin).all()
    assert np.array_equal(bits(u["plan"]), bits(act[rows, kmin]))
    assert np.array_equal(bits(u["action"]), bits(act[rows, kmin, 0])) and np.array_equal(bits(u["cost_best"]), bits(J[rows, kmin]))


def test_crashes_the_best_sequence_and_status_two():
    rng = np.random.default_rng(3)
    E, K, H = 3, 5, 2
    p = spec.params(n_samples=K, horizon=H, w_crash=0.0)                         # without the penalty a crashed sequence may be cheapest
    crash = np.zeros((E, K), bool)
    crash[0] = True                                                              # arena 0: every sequence crashes
    crash[1, :4] = True                                                          # arena 1: only the last one survives
    roll = fake_roll(E, K, H, rng, crash)
    roll["distance"][1, 4] = 50.0                                                # ... and it is the most expensive
    J, cr = spec.cost(roll, p)
    u = spec.update(spec.sample(np.zeros((E, H, 2)), rng.standard_normal((E, K, H, 2)), p), J, cr, p)
    assert list(u["status"]) == [spec.ALL_CRASH, spec.OK, spec.OK]
    assert u["best"][1] == 4 and u["jmin"][1] < J[1, 4]                          # best does not crash; jmin is another sequence
    assert u["best"][0] == J[0].argmin() and u["best"][2] == J[2].argmin()
    p2 = spec.params(n_samples=K, horizon=H, w_crash=7.0)
    J2, _ = spec.cost(roll, p2)
    assert np.array_equal(bits(J2[cr]), bits(J[cr] + 7.0)) and np.array_equal(bits(J2[~cr]), bits(J[~cr]))
    # the goal field's distance replaces the rollout's; off the field it costs off_field_cost more
    D = rng.uniform(0.0, 3.0, (E, K))
    off = np.zeros((E, K), bool); off[2, 1] = True
    J3, _ = spec.cost(roll, p, D, off)
    want = p["w_goal"] * np.where(off, D + p["off_field_cost"], D) - roll["ret"]
    assert np.array_equal(bits(J3), bits(want))
    out = spec.outputs(u, J, skip=[0, 0, 1])
    assert out["status"][2] == 0 and not out["cost"][2].any() and not out["action"][2].any() and out["best"].dtype == np.int32


def test_ar1_chain_and_clamp():
    rng = np.random.default_rng(4)
    E, K, H = 2, 6, 4
    p = spec.params(n_samples=K, horizon=H, beta=0.6, sigma=(0.2, 0.3), stop_sample=0)
    assert p["alpha"] == np.sqrt(1.0 - 0.36) and abs(p["alpha"] - 0.8) < 1e-15
    plan = np.full((E, H, 2), 0.1)
    g = rng.standard_normal((E, K, H, 2))
    act = spec.sample(plan, g, p)
    e, k, c = 1, 3, 1
    eps = g[e, k, 0, c]
    for h in range(H):
        if h:
            eps = p["beta"] * eps + p["alpha"] * g[e, k, h, c]
        want = min(max(0.1 + p["sigma"][c] * eps, p["lo"][c]), p["hi"][c])
        assert act[e, k, h, c] == want
    wide = spec.sample(plan, g, spec.params(n_samples=K, horizon=H, sigma=(5.0, 9.0), stop_sample=0))
    assert (wide[..., 0] == 0.0).any() and (wide[..., 0] == 0.5).any() and (wide[..., 1] == -0.64).any() and (wide[..., 1] == 0.64).any()
    assert wide[..., 0].min() >= 0.0 and wide[..., 0].max() <= 0.5 and np.abs(wide[..., 1]).max() <= 0.64


def test_warm_start_branches():
    p = spec.params(horizon=4, init_action=(0.25, -0.1))
    plan = np.arange(5 * 4 * 2, dtype=np.float64).reshape(5, 4, 2)
    key = np.array([[3, 10], [3, 9], [3, 8], [2, 10], [-1, 0]], np.int64)
    new, nkey, mode = spec.warm_start(plan, key, np.full(5, 3), np.full(5, 10), p, skip=[0, 0, 0, 0, 0])
    assert list(mode) == [0, 1, 2, 2, 2]                      # kept; shifted; a missed step, another episode, never planned: fresh
    assert np.array_equal(new[0], plan[0])
    assert np.array_equal(new[1, :3], plan[1, 1:]) and np.array_equal(new[1, 3], plan[1, 3])
    for e in (2, 3, 4):
        assert (new[e] == np.array([0.25, -0.1])).all()
    assert (nkey == np.array([3, 10])).all()
    kept, kkey, mode = spec.warm_start(plan, key, np.full(5, 3), np.full(5, 10), p, skip=[1, 1, 1, 1, 1])
    assert np.array_equal(kept, plan) and np.array_equal(kkey, key) and (mode == -1).all()
    assert plan[1, 0, 0] == 8.0                               # the inputs are not modified


def test_streams_and_debug_words():
    import scan_noise_f64 as noise
    s = spec.streams(99, 1000, [3, 3, 4], [10, 11, 10], 0, 5)
    assert s.shape == (3, 5) and len(set(s.ravel().tolist())) == 15
    key = (3 << 32) + (10 << 3) + 2
    want = noise.hash4(99 ^ key, 1001 - 1, key, 0x6D707069 + (4 << 32))
    assert spec.streams(99, 1000, [3], [10], 2, 5)[0, 4] == want
    assert not np.array_equal(spec.streams(99, 1000, [3], [10], 1, 5), spec.streams(99, 1000, [3], [10], 0, 5))
    g = spec.draws_model(s, 6)
    assert g.shape == (3, 5, 6, 2) and abs(g.mean()) < 0.3 and 0.7 < g.std() < 1.3
    # the words for the device hook give the same 24-bit fields at element index i as the stream gives at beam b
    lo, hi = spec.debug_words(s, 6)
    i = np.arange(lo.size)
    fa, fb = noise.beam_fields(lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32)), i)
    ga, gb = noise.beam_fields(np.repeat(s.reshape(-1), 12), i % 12)
    assert np.array_equal(fa, ga) and np.array_equal(fb, gb)
    assert np.array_equal(noise.gauss_from_fields(fa, fb).reshape(3, 5, 6, 2), g)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7                  # an entry more, no new version
    assert re.search(r"\bint navsim_mppi\(", header)
    assert "navsim_mppi" in abi.EXPORTS and hasattr(L, "navsim_mppi")
    names = [n for n, _ in abi.NavsimMppiParams._fields_]
    assert struct_fields(header, "navsim_mppi_params") == [("lambda" if n == "lam" else n) for n in names]
    P = abi.NavsimMppiParams
    # six int32 (the last one padding), then sixteen float64
    assert C.sizeof(P) == 24 + 8 * 16 and (P.range.offset, P.sigma.offset, P.beta.offset, P.off_field_cost.offset) == (24, 40, 104, 144)
    assert struct_fields(header, "navsim_mppi_ws") == [n for n, _ in abi.NavsimMppiWs._fields_] == ["plan", "plan_key", "actions", "roll", "cost"]
    assert C.sizeof(abi.NavsimMppiWs) == 14 * C.sizeof(C.c_void_p) and abi.NavsimMppiWs.roll.offset == 3 * C.sizeof(C.c_void_p)
    assert struct_fields(header, "navsim_mppi_out") == [n for n, _ in abi.NavsimMppiOut._fields_] == list(abi.MPPI_OUT)
    assert C.sizeof(abi.NavsimMppiOut) == 5 * C.sizeof(C.c_void_p)
    body = re.search(r"typedef struct navsim_mppi_out \{(.*?)\} navsim_mppi_out;", header, re.S).group(1)
    ctype = {"float64": "double", "uint8": "uint8_t", "int32": "int32_t"}
    for name, (dtype, _) in abi.MPPI_OUT.items():
        assert re.search(r"\b%s\*\s+%s;" % (ctype[dtype], name), body), name
    assert re.search(r"#define NAVSIM_MPPI_OK\s+1\b", header) and re.search(r"#define NAVSIM_MPPI_ALL_CRASH\s+2\b", header)
    assert (abi.MPPI_OK, abi.MPPI_ALL_CRASH) == (spec.OK, spec.ALL_CRASH) == (1, 2)
    text = re.search(r"MPPI local planner.*?int navsim_mppi\(", header, re.S).group(0)
    for phrase in ("0x6D707069", "plan_key[e] == (ep, s - 1)", "nv::exp_neg", "S * S / Q", "stale field", "OFF_FIELD"):
        assert phrase in text, phrase


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, max_peds=4, ped_model=abi.PED_SFM, map_h=16, map_w=16, n_beams=8)
    robot = ("robot_pose", "robot_goal", "prev_action", "prev_pose", "steps", "episode", "field", "scan_threshold", "scan_discomfort")
    peds = ("n_peds", "ped_pose", "ped_vel", "ped_prev_yaw", "ped_dist", "ped_has_legs", "ped_v_pref", "ped_waypoints",
            "ped_n_waypoints", "ped_wp_head")

    def state(skip=()):
        st = abi.NavsimState()
        for k in robot + peds:
            setattr(st, k, None if k in skip else ptr)
        return st

    def workspace(skip=()):
        roll = abi.NavsimRolloutOut(**{k: (None if k in skip else ptr) for k in abi.ROLLOUT_OUT})
        return abi.NavsimMppiWs(roll=roll, **{k: (None if k in skip else ptr) for k in abi.MPPI_WS})

    def outputs(skip=()):
        return abi.NavsimMppiOut(**{k: (None if k in skip else ptr) for k in abi.MPPI_OUT})

    def params(**kw):
        d = dict(n_samples=3, horizon=4, iterations=1, stop_sample=1, select=0, range=1.0, gamma=1.0, sigma=(0.1, 0.2),
                 lo=(0.0, -0.64), hi=(0.5, 0.64), init_action=(0.0, 0.0), beta=0.6, alpha=None, lam=0.05, w_goal=1.0, w_crash=100.0,
                 off_field_cost=10.0)
        d.update(kw)
        if d["alpha"] is None:
            d["alpha"] = float(np.sqrt(1.0 - d["beta"] * d["beta"])) if 0.0 <= d["beta"] < 1.0 else 0.5
        p = abi.NavsimMppiParams()
        for k, v in d.items():
            if k in ("sigma", "lo", "hi", "init_action"):
                getattr(p, k)[:] = list(v)
            else:
                setattr(p, k, v)
        return p

    ref_ = lambda x: None if x is None or x == "null" else C.byref(x)

    def call(c=cfg, s=None, p=None, w=None, o=None, field=None, gp=None, cmd=None):
        s = state() if s is None else s
        p = params() if p is None else p
        w = workspace() if w is None else w
        o = outputs() if o is None else o
        return L.navsim_mppi(ref_(c), ref_(s), ref_(p), ref_(field), ref_(gp), cmd, None, ref_(w), ref_(o), None)

    def changed(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    empty = changed(n_envs=0)
    nan, inf = float("nan"), float("inf")
    assert call(c=empty) == abi.OK                                                # (the arguments below are otherwise acceptable)
    assert call(c=None) == call(c=empty, s="null") == call(c=empty, p="null") == call(c=empty, w="null") == call(c=empty, o="null") == abi.E_ARG
    for k in tuple(abi.MPPI_WS) + tuple(abi.ROLLOUT_OUT):
        assert call(c=empty, w=workspace(skip=(k,))) == abi.E_ARG, k
    for k in abi.MPPI_OUT:
        assert call(c=empty, o=outputs(skip=(k,))) == abi.E_ARG, k
    bad = [dict(n_samples=0), dict(n_samples=257), dict(horizon=0), dict(horizon=33), dict(iterations=0), dict(iterations=9),
           dict(stop_sample=2), dict(stop_sample=-1), dict(select=2), dict(select=-1),
           dict(range=0.0), dict(range=nan), dict(range=cfg.range_max * 1.0001), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan),
           dict(sigma=(-0.1, 0.2)), dict(sigma=(0.1, nan)), dict(sigma=(inf, 0.1)),
           dict(lo=(0.6, -0.64)), dict(lo=(nan, -0.64)), dict(hi=(0.5, inf)), dict(hi=(0.5, nan)),
           dict(init_action=(0.6, 0.0)), dict(init_action=(0.0, -0.7)), dict(init_action=(nan, 0.0)),
           dict(lo=(0.1, -0.64), init_action=(0.2, 0.0)),                        # stop_sample with 0 outside the box
           dict(beta=-0.1), dict(beta=1.0), dict(beta=nan), dict(beta=0.6, alpha=0.8 + 1e-9), dict(beta=0.6, alpha=nan),
           dict(beta=0.0, alpha=0.0),
           dict(lam=0.0), dict(lam=-1.0), dict(lam=nan), dict(lam=inf),
           dict(w_goal=-1.0), dict(w_goal=nan), dict(w_crash=-1.0), dict(w_crash=inf), dict(off_field_cost=-1.0), dict(off_field_cost=nan)]
    for kw in bad:
        assert call(c=empty, p=params(**kw)) == abi.E_ARG, kw
    ok = [dict(n_samples=256, horizon=32, iterations=8), dict(n_samples=1, horizon=1), dict(sigma=(0.0, 0.0)), dict(beta=0.0),
          dict(lo=(0.1, -0.64), init_action=(0.2, 0.0), stop_sample=0), dict(beta=0.6, alpha=0.8), dict(w_goal=0.0, w_crash=0.0, off_field_cost=0.0),
          dict(lo=(0.25, 0.1), hi=(0.25, 0.1), init_action=(0.25, 0.1), stop_sample=0), dict(select=1)]
    for kw in ok:
        assert call(c=empty, p=params(**kw)) == abi.OK, kw
    # the goal field: with its parameters, and with a map that has a navigation grid
    field = abi.NavsimGoalField(dist=ptr, key=None, rebuilds=None)
    gp = abi.NavsimGoalPathParams(hard_clearance=0.3, clearance=0.75, lookahead=2.0, band_cost=3)
    assert call(c=empty, field=field, gp=gp) == abi.OK
    assert call(c=empty, field=field) == abi.E_ARG                                # field without gp
    assert call(c=empty, field=abi.NavsimGoalField(dist=None, key=None, rebuilds=None), gp=gp) == abi.E_ARG
    assert call(c=empty, gp=gp) == abi.OK                                         # gp alone is ignored
    for kw in (dict(hard_clearance=nan), dict(hard_clearance=0.1), dict(lookahead=-1.0), dict(lookahead=inf)):
        g2 = abi.NavsimGoalPathParams(**dict(dict(hard_clearance=0.3, clearance=0.75, lookahead=2.0, band_cost=3), **kw))
        assert call(c=empty, field=field, gp=g2) == abi.E_ARG, kw
    assert call(c=changed(n_envs=0, map_h=4), field=field, gp=gp) == abi.E_ARG
    # the state, and everything navsim_rollout refuses, with its code
    for k in robot + peds:
        assert call(c=empty, s=state(skip=(k,))) == abi.E_ARG, k
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL)) == abi.E_ARG    # no commands: neither the argument nor the state's
    assert call(c=changed(n_envs=0, ped_model=abi.PED_EXTERNAL), cmd=ptr) == abi.OK
    for k, v in (("n_envs", -1), ("n_beams", 0), ("max_peds", 65), ("march_rule", 3), ("time_step", 0.0), ("action_kind", 2), ("ped_model", 3)):
        assert call(c=changed(**dict(dict(n_envs=0), **{k: v}))) == abi.E_ARG, (k, v)
    assert call(c=changed(n_envs=0, field_format=2)) == abi.E_UNSUPPORTED
    assert call(c=changed(n_envs=0, n_beams=13700)) == abi.E_UNSUPPORTED
    assert call(c=changed(n_envs=2 ** 23 + 1), p=params(n_samples=256)) == abi.E_UNSUPPORTED


# ---- defaults and the keywords on NavGymEnv -------------------------------------------------------------------------------------
def test_defaults_and_parameter_struct():
    from nav_gym_amd import lib, robots, sim
    cfg = lib.default_config(n_envs=1)
    d = sim.mppi_defaults(cfg, "keti")
    assert set(d) == set(sim.MPPI_KEYS)
    assert (d["n_samples"], d["horizon"], d["iterations"], d["select"], d["stop_sample"]) == (32, 24, 1, "mean", 1)
    assert d["lo"] == (0.0, -0.64) and d["hi"] == (0.5, 0.64) and d["init_action"] == (0.0, 0.0)
    assert d["range"] == sim.rollout_defaults(cfg)["range"] and d["gamma"] == 1.0
    p = sim.mppi_params(cfg, dict(n_samples=5, beta=0.6, select="best", lam=0.2, sigma=(0.3, 0.1)))
    assert (p.n_samples, p.horizon, p.select, p.lam, list(p.sigma)) == (5, 24, 1, 0.2, [0.3, 0.1])
    assert p.alpha == float(np.sqrt(np.float64(1.0) - np.float64(0.6) * np.float64(0.6)))
    wheels = cfg.copy()
    wheels.action_kind, wheels.wheel_radius, wheels.wheel_track = abi.ACTION_WHEELS, 0.1651, 0.5708
    dw = sim.mppi_defaults(wheels, "husky")
    corners = [robots.wheels_from_twist(v, w, 0.1651, 0.5708) for v in (0.0, 1.0) for w in (-2.0, 2.0)]
    assert dw["lo"] == (float(np.min(corners)),) * 2 and dw["hi"] == (float(np.max(corners)),) * 2 and dw["init_action"] == (0.0, 0.0)
    with pytest.raises(ValueError, match="n_samples, horizon, iterations"):
        sim.mppi_params(cfg, dict(samples=3))
    for kw, text in ((dict(select="median"), "select"), (dict(n_samples=257), "1 .. 256"), (dict(horizon=0), "1 .. 32"),
                     (dict(iterations=9), "1 .. 8"), (dict(beta=1.0), "beta"), (dict(lam=0.0), "lam"), (dict(sigma=(0.1,)), "two values"),
                     (dict(sigma=(-0.1, 0.1)), "sigma"), (dict(init_action=(0.7, 0.0)), "init_action"), (dict(w_crash=-1.0), "w_crash"),
                     (dict(lo=(0.1, -0.64), init_action=(0.2, 0.0)), "stop_sample")):
        with pytest.raises(ValueError, match=text):
            sim.mppi_params(cfg, kw)
    lay = sim.blob_layout(abi.MPPI_OUT, 5)
    assert [(k, d_, shape) for k, d_, _, _, shape in lay[:-1]] == [("action", "float64", (5, 2)), ("best", "int32", (5,)),
                                                                   ("cost_best", "float64", (5,)), ("ess", "float64", (5,)),
                                                                   ("status", "uint8", (5,))]


def test_env_keywords():
    import copy
    import pickle
    import nav_gym_env
    from nav_gym_amd import registry, sim
    from nav_gym_amd.env import NavGymEnv
    assert NavGymEnv._MPPI_KEYS == tuple(k for k in sim.MPPI_KEYS if k not in ("lo", "hi"))
    kw = dict(n_samples=16, horizon=6, iterations=2, sigma=(0.1, 0.3), lam=0.1, beta=0.5, w_goal=2.0, w_crash=50.0, off_field_cost=5.0,
              stop_sample=0, select="best", range=1.5, gamma=0.95, init_action=(0.1, 0.0))
    env = nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", local_planner_params=kw)
    assert env.local_planner == "mppi" and env.local_planner_params == kw
    assert [p.key for p in env._products] == ["planner"] and env._products[0].record == "mppi" and env._products[0].keys == tuple(abi.MPPI_OUT)
    both = nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", goal_path=True)
    assert [p.record for p in both._products] == ["goal_path", "mppi"]           # behind the goal path
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.local_planner == "mppi" and twin.local_planner_params == kw and twin.num_envs == 3
    for call in (env.planner_action, env.planner_plan):
        with pytest.raises(RuntimeError):
            call()                                             # before reset()
    with pytest.raises(ValueError, match="local_planner='dwa'"):                   # parameters without the feature
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner_params=dict(horizon=4))
    with pytest.raises(ValueError, match="n_samples, horizon, iterations"):        # an unknown key names the known ones
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", local_planner_params=dict(n_v=4))
    with pytest.raises(ValueError, match="acc_lin, acc_rot, body_radius"):         # ... and DWA's under 'dwa'
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="dwa", local_planner_params=dict(n_samples=4))
    with pytest.raises(ValueError, match="None or 'dwa'"):
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="cem")
    with pytest.raises(ValueError, match="lo, hi|known"):                          # the box is the action space, not a parameter
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", local_planner_params=dict(lo=(0.0, 0.0)))
    for bad, text in ((dict(select="median"), "select"), (dict(n_samples=0), "1 .. 256"), (dict(beta=1.5), "beta"), (dict(lam=-1.0), "lam")):
        with pytest.raises(ValueError, match=text):                                # refused at construction
            nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", local_planner_params=bad)
    for model, more in (("orca", {}), ("policy", dict(policy_weights="weights.pth"))):
        with pytest.raises(ValueError, match="rollout is not available"):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, local_planner="mppi", pedestrian_model=model, **more)
    for model in ("sfm", "none", "external"):
        assert nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="mppi", pedestrian_model=model).local_planner == "mppi"
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.local_planner is None and plain._products == []
    with pytest.raises(RuntimeError):
        plain.planner_plan()
    dwa = nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="dwa")
    assert [p.record for p in dwa._products] == ["dwa"]
    with pytest.raises(RuntimeError):
        dwa.planner_plan()
    assert "local_planner" not in registry.spec("NavGym-v0")["kwargs"]
