"""GPU: observed pedestrians (include/navsim.h navsim_ped_observe; NavGymEnv(observe_humans=K)) against the NumPy specification
of tests/ped_observe_spec.py, bit for bit: single calls at the shapes where the lane packing changes, each of the nine
instantiations, the hand-made cases with their known answers, a closed loop beside the oracle under the three reset protocols,
and the gym surface.  Every output is pre-filled with a sentinel: the call writes every element."""
import numpy as np
import pytest

import ped_observe_spec as spec
import ref
from gpu_support import gpu, eq, random_actions, sim_and_oracle, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi
from ped_observe_call import KEYS, STATE, answer, call, device_state, same

pytestmark = pytest.mark.gpu

# ---- a. single calls at the shapes where the lane packing changes ------------------------------------------------------------
@pytest.mark.parametrize("E,N,seed,n_peds", spec.RANDOM_WORLDS, ids=lambda v: str(v) if isinstance(v, int) else "n")
def test_single_call_equals_the_spec(gpu, E, N, seed, n_peds):
    """120 x 120 maps, the packed field, the 270-degree lidar: K in {1, 4, N} x rays in {1, 3}; then the field of view off,
    occlusion off, a skip mask, and no `visible` array."""
    occ, w = spec.random_world(E, N, spec.RANDOM_SIZE, seed, n_peds)
    cfg = spec.random_config(E, N, spec.RANDOM_SIZE, field_format=abi.FIELD_U16T)
    gpu.world.lidar_1081(cfg)
    fields = ref.build_dt(occ)
    st, keep = device_state(gpu, cfg, occ, w)
    seen = 0
    for K in sorted({1, min(4, N), N}):
        for rays in (1, 3):
            p = dict(sensor_range=3.0, max_obs=K, rays=rays)
            want = answer(cfg, fields, w, p)
            same(call(gpu, cfg, st, p), want, "K %d rays %d" % (K, rays))
            seen += int(want["count"].sum())
    K = min(4, N)
    for what, p, kw in (("fov off", dict(fov=0), {}), ("occlusion off", dict(occlusion=0), {}),
                        ("long range", dict(sensor_range=9.0), {}), ("point pedestrians", dict(ped_radius=0.0), {}),
                        ("skip", {}, dict(skip=(np.arange(E) % 2 == 0).astype(np.uint8)))):
        p = dict(dict(sensor_range=3.0, max_obs=K), **p)
        same(call(gpu, cfg, st, p, **kw), answer(cfg, fields, w, p, **kw), what)
    dev = call(gpu, cfg, st, dict(sensor_range=3.0, max_obs=K), visible=False)
    assert (dev["visible"] == 77).all()                                          # NULL: not written
    want = answer(cfg, fields, w, dict(sensor_range=3.0, max_obs=K))
    for k in ("state", "index", "count"):
        eq(dev[k], want[k], "without visible: %s" % k)
    assert N == 1 or seen > 0


# ---- b. each of the nine instantiations --------------------------------------------------------------------------------------
RULES = (abi.MARCH_F64, abi.MARCH_F32, abi.MARCH_F32_FMA)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_field_formats_and_march_rules(gpu, fmt, rule):
    E, N, seed, n_peds = spec.RANDOM_WORLDS[4]
    occ, w = spec.random_world(E, N, spec.RANDOM_SIZE, seed, n_peds)
    cfg = spec.random_config(E, N, spec.RANDOM_SIZE, field_format=fmt, march_rule=rule)
    st, keep = device_state(gpu, cfg, occ, w)
    p = dict(sensor_range=3.0, max_obs=8)
    want = answer(cfg, ref.build_dt(occ), w, p)
    assert want["count"].sum() > 40 and (want["visible"] == 0).sum() > 40
    same(call(gpu, cfg, st, p), want, "format %d rule %d" % (fmt, rule))


@pytest.mark.parametrize("rule", RULES)
def test_packed_field_with_an_overflow_plane(gpu, rule):
    """A 560 x 560 hall: the lines of sight cross cells further than 255 cells from every obstacle, which the packed field
    stores saturated -- their distances come from the float32 overflow plane."""
    occ, w = spec.open_hall()
    cfg = spec.random_config(2, 8, occ.shape[1], field_format=abi.FIELD_U16T, march_rule=rule, shared_field=1)
    fields = ref.build_dt(occ)
    assert fields.max() >= 256.0
    st, keep = device_state(gpu, cfg, occ, w, overflow=True)
    p = dict(sensor_range=30.0, ped_radius=0.1, max_obs=8, fov=0)
    want = answer(cfg, fields, w, p)
    assert want["count"].tolist() == [4, 4] and want["visible"][:, 4:].sum() == 0          # the four in the open; none in the wall
    same(call(gpu, cfg, st, p), want, "overflow plane, rule %d" % rule)


def test_shared_field_and_permuted_map_slots(gpu):
    E, N, seed = 5, 21, 4350
    p = dict(sensor_range=3.0, max_obs=6)
    occ, w = spec.random_world(E, N, spec.RANDOM_SIZE, seed, shared=True)
    cfg = spec.random_config(E, N, spec.RANDOM_SIZE, field_format=abi.FIELD_U16T, shared_field=1)
    st, keep = device_state(gpu, cfg, occ[:1], w)
    want = answer(cfg, ref.build_dt(occ[:1]), w, p)
    assert want["count"].sum() > 10
    same(call(gpu, cfg, st, p), want, "shared field")
    # arena e's map lies in slot perm[e] of the field array
    occ, w = spec.random_world(E, N, spec.RANDOM_SIZE, seed)
    perm = np.array([3, 0, 4, 1, 2])
    stored = np.empty_like(occ); stored[perm] = occ
    cfg = spec.random_config(E, N, spec.RANDOM_SIZE, field_format=abi.FIELD_U16T)
    st, keep = device_state(gpu, cfg, stored, w, map_slot=perm)
    want = answer(cfg, ref.build_dt(stored), w, p, map_slot=perm)
    same(want, answer(cfg, ref.build_dt(occ), w, p), "the specification's own slot table")
    same(call(gpu, cfg, st, p), want, "permuted slots")


# ---- c. the hand-made cases, with their known answers -------------------------------------------------------------------------
def _wall(gpu, peds, fmt, robot_cell_occupied=False, lidar_270=False, skip=None, **params):
    cfg = spec.wall_config(len(peds), lidar_270=lidar_270, field_format=fmt)
    st, keep = device_state(gpu, cfg, spec.wall_map(robot_cell_occupied)[None], spec.wall_case(peds))
    return call(gpu, cfg, st, dict(spec.DEFAULT, **params), skip=skip)


@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_hand_made_cases(gpu, fmt):
    at = spec.at
    o = _wall(gpu, [at(1.5, 0.0)], fmt)                                           # behind the wall
    assert o["visible"].tolist() == [[0]] and o["count"].tolist() == [0] and o["index"].tolist() == [[-1] * 4] and not o["state"].any()
    assert _wall(gpu, [at(1.5, 0.0)], fmt, occlusion=0)["visible"].tolist() == [[1]]
    assert _wall(gpu, [at(1.5, 0.8125)], fmt, rays=3)["visible"].tolist() == [[1]]        # the +radius ray alone is clear
    assert _wall(gpu, [at(1.5, 0.8125)], fmt, rays=1)["visible"].tolist() == [[0]]
    assert _wall(gpu, [at(0.25, 0.0)], fmt)["visible"].tolist() == [[1]]                  # within the radius
    assert _wall(gpu, [at(0.25, 0.0), at(0.5, 0.0)], fmt, robot_cell_occupied=True)["visible"].tolist() == [[1, 0]]
    for peds in ([at(0.0, -0.5), at(0.0, 0.5)], [at(0.0, 0.5), at(0.0, -0.5)]):           # equal distances: the lower index
        o = _wall(gpu, peds, fmt)
        assert o["index"].tolist() == [[0, 1, -1, -1]] and o["state"][0, :2, 4].tolist() == [0.5, 0.5]
        assert o["state"][0, :2, 1].tolist() == [peds[0][1] - spec.ROBOT[1], peds[1][1] - spec.ROBOT[1]]
    assert _wall(gpu, [at(0.5, 0.0)], fmt, ped_radius=0.25, sensor_range=0.25)["visible"].tolist() == [[1]]
    assert _wall(gpu, [at(0.5, 0.0)], fmt, ped_radius=0.25, sensor_range=np.nextafter(0.25, 0.0))["visible"].tolist() == [[0]]
    assert _wall(gpu, [at(-0.5, 0.0)], fmt, lidar_270=True)["visible"].tolist() == [[0]]  # behind a 270-degree lidar
    assert _wall(gpu, [at(-0.5, 0.0)], fmt, lidar_270=True, fov=0)["visible"].tolist() == [[1]]
    peds = [at(0.625, 0.0), at(0.25, 0.125), at(0.5, 0.0)]
    o = _wall(gpu, peds, fmt, max_obs=2)                                          # K below the count
    assert o["count"].tolist() == [3] and o["index"].tolist() == [[1, 2]] and o["visible"].tolist() == [[1, 1, 1]]
    o = _wall(gpu, peds, fmt, max_obs=2, skip=[1])
    assert o["count"].tolist() == [0] and o["index"].tolist() == [[-1, -1]] and not o["state"].any() and not o["visible"].any()


# ---- d. closed loop beside the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ["same_step", "next_step", "reset_mask"])
def test_closed_loop_beside_the_oracle(gpu, protocol):
    """30 steps of 8 arenas with social-force pedestrians through NavSim.step beside the oracle: NavSim.ped_observe after every
    step equals the specification on the ORACLE's state.  next_step: the arenas whose done flag is set are skipped;
    reset_mask: no auto-reset, the finished arenas are restarted after the step and observed again."""
    E, size, N, K = 8, 160, 6, 3
    mode = dict(same_step=abi.AUTORESET_SAME_STEP, next_step=abi.AUTORESET_NEXT_STEP, reset_mask=abi.AUTORESET_NONE)[protocol]
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=1, ped_model=abi.PED_SFM,
                                 auto_reset=mode, n_spawn=8, seed=4343, field_format=abi.FIELD_U16T)
    gpu.world.lidar_1081(cfg)
    occ = gpu.world.make_maps(E, size, 4343)
    g, r, _ = sim_and_oracle(gpu, cfg, occ, 5, final_obs=(mode == abi.AUTORESET_SAME_STEP), min_goal_dist=1.5, max_goal_dist=4.0)
    fields = ref.build_dt(occ)
    p = dict(spec.DEFAULT, sensor_range=4.0, max_obs=K)            # (every key: NavSim's own defaults are the footprints')
    g.enable_ped_observe(p)

    def check(what, skip=None):
        t_skip = None if skip is None else to_device(gpu, skip)
        dev = {k: v.cpu().numpy() for k, v in g.ped_observe(skip=t_skip).items()}
        want = spec.observe(r.cfg, fields, r.a["robot_pose"], r.a["n_peds"], r.a["ped_pose"], r.a["ped_vel"], p, skip=skip)
        same(dev, want, what)
        return want

    check("after the reset")
    rng = np.random.default_rng(5)
    ends = seen = hidden = skipped = 0
    sets = set()
    for t in range(30):
        act = random_actions(rng, E, t)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        done = rout["done"].copy()
        ends += int(done.sum())
        want = check("step %d" % t, skip=done if protocol == "next_step" else None)
        sets.add(g.cur)
        seen += int(want["count"].sum()); hidden += int((want["visible"] == 0).sum())
        if protocol == "next_step":
            skipped += int(done.sum())
            assert (want["count"][done != 0] == 0).all()
        if protocol == "reset_mask" and done.any():
            g.reset_arenas(gpu.torch.from_numpy(done).to(gpu.dev))
            r.restart(done)
            check("after reset(mask) at step %d" % t)
    assert ends > 0, "no episode ended"
    assert seen > 30 and hidden > 30 and sets == {0, 1}
    assert protocol != "next_step" or skipped == ends


# ---- e. the gym surface ------------------------------------------------------------------------------------------------------
def _env(**kw):
    import nav_gym_amd
    from nav_gym_amd import registry
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([4, 4], "int"), obstacle_width=([0.3, 0.5], "float"))
    base = dict(num_envs=6, map_size=100, n_beams=64, seed=3, plan_paths=False, min_goal_dist=2.0, max_goal_dist=4.0,
                indoor_ratio=0.0, num_humans=4, max_episode_steps=6, observe_humans=3, env_param_range=ranges)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


def _direct(gpu, env, skip=None):
    """A direct navsim_ped_observe on the environment's current state, into buffers of its own."""
    sim = env.sim
    return call(gpu, sim.cfg, sim.st, sim.obs_params, skip=skip)


def _from_device_state(env, skip=None):
    """The specification on the environment's state, read back from the device (the maps through their occupancy)."""
    sim = env.sim
    s = sim.numpy_state(*STATE)
    fields = ref.build_dt(np.stack([sim.occupancy(e) for e in range(env.num_envs)]))
    p = sim.obs_params
    return spec.observe(sim.cfg, fields, s["robot_pose"], s["n_peds"], s["ped_pose"], s["ped_vel"],
                        dict(ped_radius=p.ped_radius, sensor_range=p.sensor_range, max_obs=p.max_obs, rays=p.rays,
                             occlusion=p.occlusion, fov=p.fov), skip=skip)


def _host(h):
    return {k: v.cpu().numpy().view(np.uint8) if k == "visible" else v.cpu().numpy() for k, v in h.items()}


def _drive(E):
    a = np.zeros((E, 2))
    a[: E // 2, 0] = 0.5
    return a


@pytest.mark.parametrize("model", ["sfm", "orca", "external"])
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_info_humans(gpu, model, mode):
    """info['humans'] and observed_humans() equal a direct call on the same state and the specification on the state read back;
    dtypes and shapes; the two buffer sets alternate and what a step returned stays intact through the next one; next-step mode
    has empty rows where done is set; reset(mask) refreshes the masked rows."""
    torch = gpu.torch
    env = _env(pedestrian_model=model, autoreset_mode=mode)
    E, K, N = 6, 3, env.cfg.max_peds
    env.reset()
    h = env.observed_humans()
    assert set(h) == set(KEYS)
    assert (h["state"].dtype, h["index"].dtype, h["count"].dtype, h["visible"].dtype) == (torch.float32, torch.int32, torch.int32, torch.bool)
    assert (tuple(h["state"].shape), tuple(h["index"].shape), tuple(h["count"].shape), tuple(h["visible"].shape)) == ((E, K, 5), (E, K), (E,), (E, N))
    same(_host(h), _direct(gpu, env), "after reset()")
    same(_host(h), _from_device_state(env), "after reset(): specification")
    prev, ptrs, ends, empty = None, set(), 0, 0
    for t in range(14):
        kw = dict(human_actions=np.full((E, N, 2), 0.2)) if model == "external" else {}
        _, _, done, info = env.step(_drive(E), **kw)
        h = info["humans"]
        assert h is env.observed_humans()
        ptrs.add(h["state"].data_ptr())
        skip = done.cpu().numpy().astype(np.uint8) if mode == "next_step" else None
        now = _host(h)
        same(now, _direct(gpu, env, skip=skip), "step %d" % t)
        same(now, _from_device_state(env, skip=skip), "step %d: specification" % t)
        if mode == "next_step" and skip.any():
            assert (now["count"][skip != 0] == 0).all() and (now["index"][skip != 0] == -1).all()
            empty += int(skip.sum())
        if prev is not None:                                                     # the pair lifetime
            same(_host(prev[0]), prev[1], "step %d's rows after step %d" % (t - 1, t))
        prev = (h, now)
        ends += int(done.sum())
        assert "humans" not in info.get("final_observation", {})
    assert len(ptrs) == 2 and ends > 0 and (mode != "next_step" or empty == ends)
    mask = np.array([1, 0, 0, 1, 0, 0], bool)
    before = env.sim.numpy_state("robot_pose")["robot_pose"]
    env.reset(mask=mask)
    after = _host(env.observed_humans())
    assert (env.sim.numpy_state("robot_pose")["robot_pose"][mask] != before[mask]).any(axis=1).all()      # they did restart
    same(after, _from_device_state(env, skip=env.sim.out["done"].cpu().numpy() if mode == "next_step" else None), "after reset(mask)")
    env.close()


@pytest.mark.parametrize("pipeline", [0, None])
def test_worlds_that_draw_a_map_per_episode(gpu, pipeline):
    """randomize_maps with navsim_regen behind every step and on the pipelined reset path: the observation is launched behind
    the regenerated (installed) world, so a finished arena's rows belong to its new map."""
    env = _env(num_envs=8, map_size=200, randomize_maps=True, pregen_pipeline=pipeline, use_graphs=False, max_episode_steps=5)
    env.reset()
    ends = 0
    for t in range(12):
        _, _, done, info = env.step(_drive(8))
        same(_host(info["humans"]), _from_device_state(env), "step %d" % t)
        ends += int(done.sum())
    assert env._step_path == ("pipelined" if pipeline is None else "plain") and ends >= 8
    env.close()


def test_single_environment_returns_numpy(gpu):
    env = _env(num_envs=1)
    env.reset()
    for t in range(3):
        _, _, done, info = env.step(np.zeros(2))
        h = info["humans"]
        assert h is env.observed_humans()
        assert isinstance(h["state"], np.ndarray) and h["state"].shape == (3, 5) and h["state"].dtype == np.float32
        assert h["index"].shape == (3,) and h["index"].dtype == np.int32 and isinstance(h["count"], int)
        assert h["visible"].shape == (env.cfg.max_peds,) and h["visible"].dtype == bool
        want = _from_device_state(env)
        eq(h["state"], want["state"][0], "state"); eq(h["index"], want["index"][0], "index")
        assert h["count"] == want["count"][0] and h["visible"].tolist() == (want["visible"][0] != 0).tolist()
    env.close()


def test_feature_off_allocates_and_reports_nothing(gpu):
    env = _env(observe_humans=None)
    env.reset()
    _, _, _, info = env.step(_drive(6))
    assert "humans" not in info and env.sim.products == {}
    env.close()
