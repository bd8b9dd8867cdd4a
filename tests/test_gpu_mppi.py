"""GPU: the MPPI local planner (include/navsim.h navsim_mppi) against its NumPy restatement tests/mppi_spec.py, bit for bit.
The restatement runs the whole call beside the device -- warm start, then per iteration the samples from the device's own
Gaussian draws (navsim_debug_math fn 17 on the specification's streams), navsim_rollout on those samples through
tests/rollout_call.py, cost, weights and the new plan -- and every array of the workspace and of the outputs is compared: the
samples, the rollout inside (all ten arrays), cost, plan, plan_key, action, best, cost_best, ess, status.  The draws are also
compared with the float64 model of tests/scan_noise_f64.py.  Then: the warm start through NavGymEnv, determinism and shards, and
the planner's behaviour beside the random-shooting controller of tests/test_gpu_rollout.py."""
import numpy as np
import pytest

import lookahead_call as lc
import mppi_call as mc
import mppi_spec as spec
import rollout_call as rc
from gpu_support import eq, gpu, nav_env, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

# the project's own bound on |gauss_noise - float64 model| per draw: G_TOL of tests/test_gpu_scan_noise.py (restated, not imported)
G_TOL = 2e-4
TWIST_BOX = dict(lo=(0.0, -0.64), hi=(0.5, 0.64))


def default_range(g):
    from nav_gym_amd import sim
    return sim.rollout_defaults(g.cfg, float(g.t["scan_discomfort"].max().item()))["range"]


def warm(gpu, g, seed, cmds=False):
    rng = np.random.default_rng(seed)
    for _ in range(3):
        if cmds:
            g.set_ped_cmd(np.stack([rng.uniform(0, 0.6, g.t["ped_cmd"].shape[:2]), rng.uniform(-0.6, 0.6, g.t["ped_cmd"].shape[:2])], axis=2))
        g.step(to_device(gpu, random_actions(rng, g.cfg.n_envs)))


# ---- the four worlds (shaped like the lookahead's: none / sfm / external pedestrians, float32 and packed fields, wheels) ---------
FACE = 80                                                       # x cell of the block's face in world a


def world_a(gpu):
    """No pedestrians, E = 5, 97 beams, a 96 x 120 map with its origin off zero, float32 field.  Arena 0 faces the block's wall
    from 0.62 m; arena 1 stands 0.2 m beside the outer wall (its nav cell is impassable: off the goal field)."""
    E, H, W = 5, 96, 120
    cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=W, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=2, seed=5,
                                 field_format=abi.FIELD_F32, origin_x=-1.0, origin_y=2.0, env_index_base=7)
    gpu.world.lidar_full_circle(cfg, 97)
    g = lc.sim_world(gpu, cfg, lc.room(E, H, W, 3, (FACE, FACE + 4, 20, 76)), 0)
    warm(gpu, g, 1)
    face, y = -1.0 + FACE * 0.05, 2.0 + 48 * 0.05
    lc.place(g, cfg, 0, face - 0.62, y, goal=(-2.0, 0.5))
    lc.place(g, cfg, 1, -1.0 + 40 * 0.05, 2.0 + 3 * 0.05 + 0.2, th=1.0, goal=(1.0, 1.5))
    lc.place(g, cfg, 2, -1.0 + 40 * 0.05, y, goal=(0.4, 0.0))   # the goal within reach of the horizon
    lc.place(g, cfg, 3, -1.0 + 40 * 0.05, y, goal=(1.5, 1.0))
    return g


def world_b(gpu):
    """Social force, 6 slots with 4 present, 128 beams all round, E = 6, packed field, 160-cell outdoor maps."""
    E, S = 6, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=6, ped_model=abi.PED_SFM, n_scan_stack=2, seed=7,
                                 field_format=abi.FIELD_U16T, n_spawn=4)
    gpu.world.lidar_full_circle(cfg, 128)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 7), 4)
    warm(gpu, g, 2)
    return g


def world_c(gpu):
    """NAVSIM_PED_EXTERNAL: the commands come as an argument that differs from the state's."""
    E, S = 4, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=4, ped_model=abi.PED_EXTERNAL, n_scan_stack=1, seed=9,
                                 field_format=abi.FIELD_U16T)
    gpu.world.lidar_full_circle(cfg, 77)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 9), 3)
    warm(gpu, g, 3, cmds=True)
    return g


def world_d(gpu):
    """Wheel speeds as actions, clamped, with a minimum turning radius."""
    E, S = 4, 160
    cfg = gpu.lib.default_config(n_envs=E, map_h=S, map_w=S, max_peds=1, ped_model=abi.PED_NONE, n_scan_stack=1, seed=11,
                                 field_format=abi.FIELD_U16T, action_kind=abi.ACTION_WHEELS, clamp_action=1, min_turning_radius=0.4)
    gpu.world.lidar_full_circle(cfg, 77)
    g = lc.sim_world(gpu, cfg, gpu.world.make_maps(E, S, 11), 0)
    warm(gpu, g, 4)
    return g


def commands(g, seed):
    if g.cfg.ped_model != abi.PED_EXTERNAL:
        return None
    rng = np.random.default_rng(seed)
    shape = tuple(g.t["ped_cmd"].shape[:2])
    return np.stack([rng.uniform(0, 0.6, shape), rng.uniform(-0.6, 0.6, shape)], axis=2)


# ---- the restatement beside the device ---------------------------------------------------------------------------------------------
def device_draws(gpu, stream, H):
    """g [E,K,H,2]: nv::gauss_noise of the specification's streams, read from the device"""
    lo, hi = spec.debug_words(stream, H)
    out = gpu.sim.debug_math(17, to_device(gpu, lo), to_device(gpu, hi))
    return out.cpu().numpy().reshape(stream.shape + (H, 2))


def goal_field_of(gpu, g, params=None):
    """The goal path enabled on g, its fields built for the current state -> dict(dist tensor, gp struct, params dict, fields)"""
    g.enable_goal_path(params)
    g.goal_path()
    gp = g.products["goal_path"].params
    return dict(dist=g.goal_field(), gp=gp, fields=g.host0["field"],
                params=dict(hard_clearance=gp.hard_clearance, clearance=gp.clearance, band_cost=gp.band_cost, lookahead=gp.lookahead))


def spec_call(gpu, g, p, R, ws, gamma=1.0, field=None, ped_cmd=None, skip=None, draws=None):
    """What navsim_mppi must leave in the workspace `ws` (NumPy, as mc.ws_numpy gives it) and in `out`, from the current state.
    draws: per iteration g [E,K,H,2] (None: the device's own).  -> (ws, out) as dicts of NumPy arrays."""
    cfg = g.cfg
    E, K, H = cfg.n_envs, int(p["n_samples"]), int(p["horizon"])
    ep, s = g.t["episode"].cpu().numpy(), g.t["steps"].cpu().numpy()
    sk = np.zeros(E, bool) if skip is None else np.asarray(skip) != 0
    plan, key, _ = spec.warm_start(ws["plan"], ws["plan_key"], ep, s, p, skip=sk)
    goal = g.t["robot_goal"].cpu().numpy()
    act = roll = J = u = None
    for it in range(int(p["iterations"])):
        gd = device_draws(gpu, spec.streams(cfg.seed, cfg.env_index_base, ep, s, it, K), H) if draws is None else draws[it]
        act = spec.sample(plan, gd, p)
        act[sk] = 0.0
        roll = rc.call(gpu, cfg, g.st, act, R, gamma=gamma, ped_cmd=ped_cmd, skip=skip)
        D = off = None
        if field is not None:
            dist = field["dist"].view(gpu.torch.int16).cpu().numpy().view(np.uint16)
            D, off = spec.field_distance(cfg, field["fields"], dist, goal, spec.terminal_xy(roll), field["params"])
        J, crash = spec.cost(roll, p, D, off)
        u = spec.update(act[~sk], J[~sk], crash[~sk], p)
        plan[~sk] = u["plan"]
    full = {}
    for k, v in u.items():                                      # the rows of the arenas that ran, the others 0 (rule 1)
        a = np.zeros((E,) + np.shape(v)[1:], np.asarray(v).dtype)
        a[~sk] = v
        full[k] = a
    out = spec.outputs(full, J, skip=sk)
    cost = out.pop("cost")
    return dict(plan=plan, plan_key=key, actions=act, cost=cost, roll=roll, off=off), out


def same_call(ws_dev, out_dev, ws_want, out_want, what):
    same_bits(ws_dev["actions"], ws_want["actions"], what + " actions")
    for k in rc.KEYS:
        same_bits(ws_dev["roll"][k], ws_want["roll"][k], what + " rollout " + k)
    for k in ("cost", "plan"):
        same_bits(ws_dev[k], ws_want[k], what + " " + k)
    eq(ws_dev["plan_key"], ws_want["plan_key"], what + " plan_key")
    for k in mc.OUT_KEYS:
        same_bits(out_dev[k], out_want[k], what + " " + k)


# ---- (a) samples ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,beta,stop", [(1, 1, 0.0, 0), (2, 6, 0.6, 1), (5, 32, 0.6, 1), (65, 6, 0.0, 0), (256, 32, 0.6, 1), (256, 1, 0.0, 1),
                                           (65, 32, 0.6, 0)])
def test_samples(gpu, K, H, beta, stop):
    g = world_a(gpu)
    cfg, E, R = g.cfg, g.cfg.n_envs, default_range(g)
    assert E == 5
    p = spec.params(n_samples=K, horizon=H, beta=beta, stop_sample=stop, sigma=(0.1, 0.2), init_action=(0.2, 0.1), **TWIST_BOX)
    ws = mc.make_ws(gpu, E, K, H)
    before = mc.ws_numpy(ws)
    mc.call(gpu, cfg, g.st, p, R, ws)
    dev = mc.ws_numpy(ws)
    ep, s = g.t["episode"].cpu().numpy(), g.t["steps"].cpu().numpy()
    plan, key, mode = spec.warm_start(before["plan"], before["plan_key"], ep, s, p)
    assert (mode == 2).all()                                                     # never planned: the fresh plan
    stream = spec.streams(cfg.seed, cfg.env_index_base, ep, s, 0, K)
    want = spec.sample(plan, device_draws(gpu, stream, H), p)
    same_bits(dev["actions"], want, "actions")
    same_bits(dev["actions"][:, 0], spec.clamp(plan, p["lo"], p["hi"]), "sequence 0 is the plan")
    if stop and K >= 2:
        assert not dev["actions"][:, 1].any()
    eq(dev["plan_key"], key, "plan_key")
    # the float64 model of the draw: unclamped entries agree within sigma (1 + beta + beta^2 + ...) G_TOL
    model = spec.sample(plan, spec.draws_model(stream, H), p)
    inside = np.ones(want.shape, bool)
    for c in range(2):
        for a in (want, model):
            inside[..., c] &= (a[..., c] > p["lo"][c]) & (a[..., c] < p["hi"][c])
    geo = sum(float(beta) ** j for j in range(H))
    err = np.abs(want - model) / (p["sigma"] * geo * G_TOL + 1e-12)
    print("K = %d H = %d beta = %g: %d unclamped entries of %d, worst |device - model| / bound = %.3f"
          % (K, H, beta, int(inside.sum()), inside.size, err[inside].max() if inside.any() else 0.0))
    assert inside.any() and (err[inside] <= 1.0).all()
    if K >= 5 and H >= 6:                                                        # distinct sequences, distinct arenas
        flat = dev["actions"][:, 2:].reshape(E * (K - 2), -1)
        assert len(np.unique(flat, axis=0)) == len(flat)


def test_samples_stay_inside_the_box(gpu):
    g = world_a(gpu)
    cfg, E, R, K, H = g.cfg, g.cfg.n_envs, default_range(g), 65, 6
    p = spec.params(n_samples=K, horizon=H, beta=0.6, stop_sample=1, sigma=(3.0, 6.0), init_action=(0.2, 0.1), **TWIST_BOX)   # several box widths
    ws = mc.make_ws(gpu, E, K, H)
    mc.call(gpu, cfg, g.st, p, R, ws)
    a = mc.ws_numpy(ws)["actions"]
    for c in range(2):
        assert a[..., c].min() == p["lo"][c] and a[..., c].max() == p["hi"][c]
        assert (a[:, 2:, :, c] == p["lo"][c]).any() and (a[:, 2:, :, c] == p["hi"][c]).any()


# ---- (b) update and (c) the rollout inside -----------------------------------------------------------------------------------------
CASES = {
    # world, with the goal field, select, iterations, K, H, more parameters
    "a-straight-mean": (world_a, False, 0, 1, 5, 6, {}),
    "a-field-best-3it": (world_a, True, 1, 3, 9, 6, {}),
    "a-wall-all-crash": (world_a, True, 0, 1, 6, 6, dict(stop_sample=0, lo=(0.45, -0.1), hi=(0.5, 0.1), init_action=(0.5, 0.0), sigma=(0.02, 0.05))),
    "a-ties": (world_a, False, 1, 1, 5, 4, dict(sigma=(0.0, 0.0), stop_sample=0, init_action=(0.2, 0.1))),
    "b-sfm-field-mean": (world_b, True, 0, 1, 7, 6, dict(beta=0.6)),
    "c-external-best": (world_c, False, 1, 1, 5, 6, dict(beta=0.6)),
    "d-wheels-field-3it": (world_d, True, 0, 3, 6, 5, dict(lo=(-1.0, -1.0), hi=(5.0, 5.0), sigma=(1.0, 1.0), lam=0.5)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_update_equals_the_specification(gpu, name):
    make, with_field, select, iterations, K, H, more = CASES[name]
    g = make(gpu)
    cfg, E, R = g.cfg, g.cfg.n_envs, default_range(g)
    p = spec.params(**dict(dict(n_samples=K, horizon=H, iterations=iterations, select=select, lam=0.05, **TWIST_BOX), **more))
    field = goal_field_of(gpu, g) if with_field else None
    cmd = commands(g, 8)
    saved = lc.save_state(g)
    ws = mc.make_ws(gpu, E, K, H)
    gamma = 0.9
    for call in range(2):                                                        # a fresh plan, then the kept one (same state)
        before = mc.ws_numpy(ws)
        out = mc.call(gpu, cfg, g.st, p, R, ws, gamma=gamma, field=None if field is None else field["dist"],
                      gp=None if field is None else field["gp"], ped_cmd=cmd)
        want_ws, want_out = spec_call(gpu, g, p, R, before, gamma=gamma, field=field, ped_cmd=cmd)
        same_call(mc.ws_numpy(ws), out, want_ws, want_out, "%s call %d" % (name, call))
    for k, v in lc.save_state(g).items():                                        # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the calls" % k)
    assert (out["status"] >= 1).all() and (out["ess"] >= 1.0).all() and (out["ess"] <= K).all()
    print("%s: status %s best %s ess %s" % (name, out["status"], out["best"], np.round(out["ess"], 2)))
    crash = (want_ws["roll"]["outcome"] & 2) != 0
    rows = np.arange(E)
    assert (~crash[rows, out["best"]] | crash.all(axis=1)).all()                  # best did not crash wherever a sequence did not
    if name == "a-wall-all-crash":                                               # conditions on the test's inputs
        assert out["status"][0] == abi.MPPI_ALL_CRASH and crash[0].all() and (out["status"][2:4] == abi.MPPI_OK).all()
    if name == "a-field-best-3it":                                               # (the stop sequence of arena 1 ends where it stands)
        assert want_ws["off"][1, 1] and not want_ws["off"].all(), "a terminal pose off the goal field, and one on it"
    if name == "a-ties":
        assert (out["best"] == 0).all() and (out["ess"] == K).all()
    if select:
        same_bits(out["action"], want_ws["actions"][rows, out["best"], 0], "action of the best sequence")
    else:
        same_bits(out["action"], want_ws["plan"][:, 0], "action of the new plan")


def test_three_single_iterations_on_a_copied_workspace(gpu):
    """iterations = 1 three times (each call draws iteration 0's noise again, on the plan the call before left) on a copy of the
    workspace, each against the specification; the original workspace takes one call with iterations = 3."""
    g = world_b(gpu)
    cfg, E, R, K, H = g.cfg, g.cfg.n_envs, default_range(g), 6, 5
    p1 = spec.params(n_samples=K, horizon=H, iterations=1, beta=0.6, **TWIST_BOX)
    p3 = spec.params(n_samples=K, horizon=H, iterations=3, beta=0.6, **TWIST_BOX)
    ws = mc.make_ws(gpu, E, K, H)
    twin = mc.copy_ws(ws)
    for i in range(3):
        before = mc.ws_numpy(twin)
        out = mc.call(gpu, cfg, g.st, p1, R, twin)
        want_ws, want_out = spec_call(gpu, g, p1, R, before)
        same_call(mc.ws_numpy(twin), out, want_ws, want_out, "single iteration %d" % i)
    before = mc.ws_numpy(ws)
    out3 = mc.call(gpu, cfg, g.st, p3, R, ws)
    want_ws, want_out = spec_call(gpu, g, p3, R, before)
    same_call(mc.ws_numpy(ws), out3, want_ws, want_out, "three iterations")
    assert not np.array_equal(mc.ws_numpy(ws)["actions"], mc.ws_numpy(twin)["actions"])      # iterations 1 and 2 draw other noise


def test_skip_mask(gpu):
    g = world_a(gpu)
    cfg, E, R, K, H = g.cfg, g.cfg.n_envs, default_range(g), 5, 4
    p = spec.params(n_samples=K, horizon=H, **TWIST_BOX)
    skip = np.array([0, 1, 0, 0, 1], np.uint8)
    ws = mc.make_ws(gpu, E, K, H)
    before = mc.ws_numpy(ws)
    out = mc.call(gpu, cfg, g.st, p, R, ws, skip=skip)
    dev = mc.ws_numpy(ws)
    want_ws, want_out = spec_call(gpu, g, p, R, before, skip=skip)
    same_call(dev, out, want_ws, want_out, "skip")
    on = skip == 1
    same_bits(dev["plan"][on], before["plan"][on], "a skipped arena's plan")     # untouched: still the sentinel
    eq(dev["plan_key"][on], before["plan_key"][on], "a skipped arena's key")
    for k in mc.OUT_KEYS:
        assert not out[k][on].any(), k
    assert not dev["actions"][on].any() and not dev["cost"][on].any()
    rc.zero_rows(dev["roll"], on, "skipped arenas")
    assert (out["status"][~on] == 1).all()


# ---- (e) determinism and shards -------------------------------------------------------------------------------------------------------
def shard(g, lo, hi):
    """(cfg, st) of arenas lo .. hi-1 of g as a world of their own: the same arrays, entered at arena lo, with env_index_base + lo"""
    cfg = g.cfg.copy()
    cfg.n_envs, cfg.env_index_base = hi - lo, g.cfg.env_index_base + lo
    st = abi.NavsimState.from_buffer_copy(g.st)
    for k, (_, shape) in abi.STATE_LAYOUT.items():
        if shape[0] == "E" and k in g.t:
            setattr(st, k, g.t[k].reshape(g.cfg.n_envs, -1)[lo:].data_ptr())       # (the packed field is one flat blob)
    return cfg, st


@pytest.mark.parametrize("make", [world_a, world_b], ids=["a", "b-sfm"])
def test_determinism_and_shards(gpu, make):
    g = make(gpu)
    cfg, E, R, K, H = g.cfg, g.cfg.n_envs, default_range(g), 7, 5
    p = spec.params(n_samples=K, horizon=H, iterations=2, beta=0.6, **TWIST_BOX)
    runs = []
    for _ in range(2):
        ws = mc.make_ws(gpu, E, K, H)
        out = mc.call(gpu, cfg, g.st, p, R, ws)
        runs.append((mc.ws_numpy(ws), out))
    same_call(runs[0][0], runs[0][1], runs[1][0], runs[1][1], "the same state twice")
    cut = E // 2
    for lo, hi in ((0, cut), (cut, E)):
        c2, st2 = shard(g, lo, hi)
        ws = mc.make_ws(gpu, hi - lo, K, H)
        out = mc.call(gpu, c2, st2, p, R, ws)
        part = mc.ws_numpy(ws)
        whole_ws = {k: (v[lo:hi] if k != "roll" else {n: a[lo:hi] for n, a in v.items()}) for k, v in runs[0][0].items()}
        same_call(part, out, whole_ws, {k: v[lo:hi] for k, v in runs[0][1].items()}, "arenas %d .. %d as a world of their own" % (lo, hi - 1))


# ---- (d) the warm start through NavGymEnv ------------------------------------------------------------------------------------------------
def env_world(**kw):
    from nav_gym_amd import env as envmod
    epr = dict(envmod.DEFAULT_KWARGS["env_param_range"], scan_noise_std=([0.0, 0.0], "float"))
    return nav_env(**dict(dict(num_envs=32, num_humans=0, pedestrian_model="none", env_param_range=epr, local_planner="mppi"), **kw))


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_warm_start_through_the_env(gpu, mode):
    """K = 1, sigma = 0: the one sequence is the plan and the update returns it (w = 1, (0 + 1 a) / 1 = a), so the plan changes by
    rule 2 alone and every branch is observed as it happens."""
    import torch
    H = 5
    params = dict(n_samples=1, horizon=H, sigma=(0.0, 0.0), stop_sample=0, init_action=(0.25, 0.1))
    env = env_world(autoreset_mode=mode, local_planner_params=params)
    env.reset()
    sim, E = env.sim, 32
    ws = sim.products["mppi"].extra
    p = spec.params(n_samples=1, horizon=H, sigma=(0.0, 0.0), stop_sample=0, init_action=(0.25, 0.1), **TWIST_BOX)
    state = lambda: (sim.t["episode"].cpu().numpy(), sim.t["steps"].cpu().numpy())
    ep, s = state()
    eq(ws["plan_key"].cpu().numpy(), np.stack([ep, s], axis=1), "plan_key after reset()")
    assert (ws["plan"].cpu().numpy() == np.array([0.25, 0.1])).all() and (env.planner_action()["status"].cpu().numpy() == 1).all()
    assert env.planner_plan() is ws["plan"]
    ramp = np.arange(E * H * 2, dtype=np.float64).reshape(E, H, 2) * 1e-4        # a plan whose every entry differs, inside the box
    ws["plan"].copy_(to_device(gpu, ramp))
    seen = {0: 0, 1: 0, 2: 0, -1: 0}
    drive = np.tile([0.5, 0.0], (E, 1))
    was_pending, fresh_by_step = np.zeros(E, bool), 0
    for t in range(45):
        before, key = ws["plan"].cpu().numpy(), ws["plan_key"].cpu().numpy()
        if t == 20:                                                              # the same state again: kept
            saved = lc.save_state(sim)
            sim.mppi(field=False)
            pending = np.zeros(E, bool)
            for k, v in lc.save_state(sim).items():                              # the state is only read
                assert torch.equal(v, saved[k]), k
        elif t == 30:                                                            # reset(mask): the masked arenas start afresh
            mask = np.zeros(E, bool); mask[::3] = True
            env.reset(mask)
            pending = env.planner_action()["status"].cpu().numpy() == 0          # (next-step mode: arenas still waiting for their reset)
            assert not pending[::3].any()
        else:
            _, _, done, info = env.step(drive)
            pending = done.cpu().numpy() if mode == "next_step" else np.zeros(E, bool)
            eq(info["planner"]["status"].cpu().numpy() != 0, ~pending, "status at step %d" % t)
        ep, s = state()
        plan, nkey, m = spec.warm_start(before, key, ep, s, p, skip=pending)
        same_bits(ws["plan"].cpu().numpy(), plan, "plan at step %d" % t)
        eq(ws["plan_key"].cpu().numpy(), nkey, "plan_key at step %d" % t)
        if t == 20:
            assert (m[~was_pending] == 0).all()
        elif t == 30:
            assert (m[::3] == 2).all()
        else:
            fresh_by_step += int((m == 2).sum())
        was_pending = pending
        for v in m:
            seen[int(v)] += 1
        out = env.planner_action()
        same_bits(out["action"].cpu().numpy()[~pending], plan[~pending, 0], "action at step %d" % t)
        assert not out["action"].cpu().numpy()[pending].any()
    print("%s: kept %d, shifted %d, fresh %d, skipped %d" % (mode, seen[0], seen[1], seen[2], seen[-1]))
    assert seen[0] >= E // 2 and seen[1] > 0 and fresh_by_step > 0, seen         # restarts happened (straight on: arenas crash)
    if mode == "next_step":
        assert seen[-1] > 0, "no arena was pending: nothing was skipped"


def test_env_one_arena_and_goal_field(gpu):
    env = env_world(num_envs=1, goal_path=True, local_planner_params=dict(n_samples=8, horizon=4))
    env.reset()
    _, _, _, info = env.step(np.array([0.1, 0.0]))
    row = info["planner"]
    assert set(row) == set(abi.MPPI_OUT) and row["action"].shape == (2,) and isinstance(row["action"], np.ndarray) and row["status"] == 1
    assert env.planner_plan().shape == (4, 2) and np.array_equal(env.planner_plan()[0], row["action"])
    assert 1.0 <= row["ess"] <= 8.0 and 0 <= row["best"] < 8


# ---- (f) behaviour ---------------------------------------------------------------------------------------------------------------------
def run_env(env, steps, act_of):
    import torch
    E = env.num_envs
    crashed = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    reached = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    env.reset()
    for _ in range(steps):
        _, _, _, info = env.step(act_of(env))
        crashed |= info["is_crash"] != 0
        reached |= info["is_success"] != 0
    return int(crashed.sum().item()), int(reached.sum().item())


def behaviour_env(**kw):
    """shooting_run's world (tests/test_gpu_rollout.py): 64 outdoor arenas, no pedestrians, noise off, no auto-reset"""
    from nav_gym_amd import env as envmod
    epr = dict(envmod.DEFAULT_KWARGS["env_param_range"], scan_noise_std=([0.0, 0.0], "float"))
    return nav_env(**dict(dict(num_envs=64, map_size=200, n_beams=256, seed=23, num_humans=0, pedestrian_model="none", min_goal_dist=3.0,
                               max_goal_dist=8.0, env_param_range=epr, auto_reset=False), **kw))


def shooting(controller, K, H, steps=150, E=64):
    """The random-shooting controller of tests/test_gpu_rollout.py::shooting_run (copied), at K sequences over H steps"""
    import torch
    env = behaviour_env(rollout=K, rollout_params=dict(horizon=H, gamma=1.0))
    rng = np.random.default_rng(17)
    rows = torch.arange(E, device="cuda:0")

    def act_of(env):
        seq = np.stack([np.stack([random_actions(rng, E) for _ in range(H)], axis=1) for _ in range(K)], axis=1)     # [E,K,H,2]
        seq[:, K - 1] = 0.0                                                      # the all-zero sequence is the last one
        seq_t = torch.from_numpy(seq).to("cuda:0")
        pick = torch.zeros(E, dtype=torch.long, device="cuda:0")
        if controller:
            out = env.rollout(seq_t)
            safe = (out["outcome"] & abi.OUTCOME_CRASH) == 0
            pick = torch.where(safe, out["ret"], torch.full_like(out["ret"], -float("inf"))).argmax(dim=1)
        return seq_t[rows, pick, 0].contiguous()
    return run_env(env, steps, act_of)


def mppi_run(select, steps=150, **kw):
    import torch
    env = behaviour_env(goal_path=True, local_planner="mppi", local_planner_params=dict(select=select), **kw)
    bad = []

    def act_of(env):
        out = env.planner_action()
        bad.append(int((out["status"] != abi.MPPI_OK).sum().item()))
        return out["action"].clone()
    return run_env(env, steps, act_of) + (sum(bad),)


def test_behaviour(gpu):
    from nav_gym_amd import lib, sim
    d = sim.mppi_defaults(lib.default_config(n_envs=1))
    K, H = d["n_samples"], d["horizon"]
    plain_crashed, plain_reached = shooting(False, K, H)
    shoot_crashed, shoot_reached = shooting(True, K, H)
    crashed, reached, not_ok = mppi_run("best")
    print("of 64 arenas within 150 steps (K = %d, H = %d): sequence 0's first action -- %d crash, %d reach the goal; random shooting "
          "-- %d crash, %d reach the goal; MPPI select='best' -- %d crash, %d reach the goal"
          % (K, H, plain_crashed, plain_reached, shoot_crashed, shoot_reached, crashed, reached))
    mean = mppi_run("mean")
    peds = mppi_run("best", num_humans=8, pedestrian_model="sfm")
    print("figures, not assertions: MPPI select='mean' -- %d crash, %d reach the goal; select='best' with 8 social-force pedestrians "
          "-- %d crash, %d reach the goal" % (mean[0], mean[1], peds[0], peds[1]))
    assert plain_crashed >= 1, "condition: the same sequences without a controller crash somewhere"
    assert crashed == 0 and not_ok == 0          # the stop sequence exists and standing still cannot crash without pedestrians
    assert reached > shoot_reached
