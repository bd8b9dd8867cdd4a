"""GPU: scan ground truth (include/navsim.h navsim_scan_labels; NavGymEnv(scan_labels=True)) against the NumPy specification of
tests/scan_labels_spec.py, bit for bit: single calls at the shapes where the lane and interval logic changes, each field format
and march rule with and without the rect records, the overflow plane, shared fields and map slots, the hand-made scenes, a closed
loop beside the oracle under the three reset protocols, scan noise, and the gym surface.  Every output is pre-filled with a
sentinel: the call writes every element."""
import numpy as np
import pytest

import ped_observe_spec
import ref
import scan_labels_spec as spec
from gpu_support import gpu, eq, random_actions, same_bits, sim_and_oracle, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi
from scan_labels_call import KEYS, STATE, STATE_NO_PEDS, call, device_state, same

pytestmark = pytest.mark.gpu


# ---- a. single calls at the shapes where the lane and interval logic changes -------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["270", "360"])
@pytest.mark.parametrize("E,N,B,seed,n_peds", spec.DEVICE_WORLDS, ids=lambda v: str(v) if isinstance(v, int) else "n")
def test_single_call_equals_the_spec(gpu, E, N, B, seed, n_peds, full):
    """160 x 160 rooms, the packed field with and without its rect records: legs rendered and not, a skip mask, no `hits`."""
    seen = np.zeros(4, int)
    for legs in (1, 0):
        cfg, occ, w = spec.device_world(E, N, B, seed, n_peds, full, lidar_legs=legs, field_format=abi.FIELD_U16T)
        fields = ref.build_dt(occ)
        want = spec.answer(cfg, fields, w)
        seen += np.bincount(want["label"].reshape(-1), minlength=4)
        for rects in (True, False):
            st, keep = device_state(gpu, cfg, occ, w, rects=rects)
            same(call(gpu, cfg, st), want, "legs %d rects %d" % (legs, rects))
    skip = (np.arange(E) % 2 == 0).astype(np.uint8)
    same(call(gpu, cfg, st, skip=skip), spec.answer(cfg, fields, w, skip=skip), "skip")
    dev = call(gpu, cfg, st, hits=False)
    assert (dev["hits"] == 777).all()                                            # NULL: not written
    same(dev, want, "without hits", keys=("range", "label", "index"))
    assert seen[spec.WALL] > 0 and seen[spec.BODY] > 0 and (B < 1081 or seen[spec.LEG] > 200)


# ---- b. each field format x march rule ---------------------------------------------------------------------------------------
RULES = (abi.MARCH_F64, abi.MARCH_F32, abi.MARCH_F32_FMA)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_field_formats_and_march_rules(gpu, fmt, rule):
    cfg, occ, w = spec.device_world(*spec.DEVICE_WORLDS[2], False, field_format=fmt, march_rule=rule)
    want = spec.answer(cfg, ref.build_dt(occ), w)
    assert all(np.bincount(want["label"].reshape(-1), minlength=4)[1:] > 200)
    for rects in ((True, False) if fmt == abi.FIELD_U16T else (False,)):
        st, keep = device_state(gpu, cfg, occ, w, rects=rects)
        same(call(gpu, cfg, st), want, "format %d rule %d rects %d" % (fmt, rule, rects))


def _hall():
    occ, w = ped_observe_spec.open_hall()
    E, N = w["ped_pose"].shape[:2]
    w = dict(w, ped_dist=np.random.default_rng(3).uniform(0.0, 2.0, (E, N, 3)), ped_has_legs=(np.arange(E * N).reshape(E, N) % 2).astype(np.uint8))
    return occ, w


@pytest.mark.parametrize("rule", RULES)
def test_packed_field_with_an_overflow_plane(gpu, rule):
    """A 560 x 560 hall: the beams cross cells further than 255 cells from every obstacle, which the packed field stores
    saturated -- their distances come from the float32 overflow plane.  28 m across with range_max = 15 m: walls and beams without a return."""
    occ, w = _hall()
    cfg = spec.config(2, 8, occ.shape[1], lidar=720, field_format=abi.FIELD_U16T, march_rule=rule, shared_field=1, range_max=15.0)
    fields = ref.build_dt(occ)
    assert fields.max() >= 256.0
    want = spec.answer(cfg, fields, w)
    assert all(np.bincount(want["label"].reshape(-1), minlength=4) > 0)
    for rects in (True, False):
        st, keep = device_state(gpu, cfg, occ, w, overflow=True, rects=rects)
        same(call(gpu, cfg, st), want, "overflow plane, rule %d rects %d" % (rule, rects))


def test_shared_field_and_permuted_map_slots(gpu):
    E, N, B, seed, n_peds = spec.DEVICE_WORLDS[2]
    cfg, occ, w = spec.device_world(E, N, B, seed, n_peds, True, field_format=abi.FIELD_U16T)
    perm = np.array([3, 0, 4, 1, 2])
    stored = np.empty_like(occ); stored[perm] = occ
    want = spec.answer(cfg, ref.build_dt(stored), w, map_slot=perm)
    same(want, spec.answer(cfg, ref.build_dt(occ), w), "the specification's own slot table")
    for rects in (True, False):
        st, keep = device_state(gpu, cfg, stored, w, map_slot=perm, rects=rects)
        same(call(gpu, cfg, st), want, "permuted slots, rects %d" % rects)
    cfg.shared_field = 1                                                         # every arena on map 0 (some now stand in a box)
    want = spec.answer(cfg, ref.build_dt(occ[:1]), w)
    st, keep = device_state(gpu, cfg, occ[:1], w, rects=True)
    same(call(gpu, cfg, st), want, "shared field")


# ---- c. the hand-made scenes -------------------------------------------------------------------------------------------------
SCENES = (("body ahead", [spec.ahead(2.0)], 64, {}), ("legs ahead", [spec.ahead(2.0, legs=1)], None, {}),
          ("legs not rendered", [spec.ahead(2.0, legs=1)], None, dict(lidar_legs=0)),
          ("two on one bearing", [spec.ahead(3.0), spec.ahead(1.5)], 64, {}),
          ("behind the wall", [((spec.ROBOT[0] + 4.9625 + 0.5, spec.ROBOT[1], 0.0), 0)], 64, {}),
          ("behind a 270-degree lidar", [spec.ahead(-2.0)], None, {}), ("across the seam", [spec.ahead(-1.5)], 64, {}),
          ("around the lidar", [spec.ahead(0.05, side=0.03, yaw=0.4)], 64, {}),
          ("beyond range_max", [spec.ahead(4.0)], 64, dict(range_max=3.0)), ("single beam", [spec.ahead(-2.0)], 1, {}),
          ("no pedestrian model", [], 64, dict(ped_model=abi.PED_NONE)))


@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_hand_made_scenes(gpu, fmt):
    """The scenes whose answers tests/test_scan_labels.py states, on the device; and three of those answers directly."""
    got = {}
    for name, peds, lidar, kw in SCENES:
        cfg, fields, a, want = spec.hand_scene(peds, lidar=lidar, field_format=fmt, **kw)
        st, keep = device_state(gpu, cfg, spec.room(spec.ROOM)[None], a, rects=fmt == abi.FIELD_U16T)
        got[name] = call(gpu, cfg, st)
        same(got[name], want, name, keys=KEYS if cfg.ped_model != abi.PED_NONE else ("range", "label", "index"))
    o = got["body ahead"]
    assert (o["label"][0, 32], o["index"][0, 32]) == (spec.BODY, 0) and abs(float(o["range"][0, 32]) - 1.78) < 1e-3
    assert got["two on one bearing"]["index"][0, 32] == 1 and got["behind the wall"]["hits"].tolist() == [[0]]
    assert (got["around the lidar"]["label"] == spec.BODY).all() and (got["beyond range_max"]["label"] == spec.NONE).all()
    same(call(gpu, cfg, st, skip=[1]), spec.answer(cfg, fields, a, skip=[1]), "skip", keys=("range", "label", "index"))


# ---- d. closed loop beside the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ["same_step", "next_step", "reset_mask"])
def test_closed_loop_beside_the_oracle(gpu, protocol):
    """30 steps of 8 arenas with social-force pedestrians through NavSim.step beside the oracle: NavSim.scan_labels after every
    step equals the specification on the ORACLE's state, and its `range` equals the newest scan slot of the DEVICE's own
    observation for every arena that is not skipped -- a check that does not pass through the specification.  next_step: the
    arenas whose done flag is set are skipped; reset_mask: no auto-reset, the finished arenas are restarted after the step."""
    E, size, N = 8, 160, 6
    mode = dict(same_step=abi.AUTORESET_SAME_STEP, next_step=abi.AUTORESET_NEXT_STEP, reset_mask=abi.AUTORESET_NONE)[protocol]
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=2, ped_model=abi.PED_SFM,
                                 auto_reset=mode, n_spawn=8, seed=4343, field_format=abi.FIELD_U16T)
    gpu.world.lidar_1081(cfg)
    occ = gpu.world.make_maps(E, size, 4343)
    g, r, _ = sim_and_oracle(gpu, cfg, occ, 5, final_obs=(mode == abi.AUTORESET_SAME_STEP), min_goal_dist=1.5, max_goal_dist=4.0)
    fields = ref.build_dt(occ)
    g.enable_scan_labels()
    seen = np.zeros(4, int)

    def check(what, obs, skip=None):
        t_skip = None if skip is None else to_device(gpu, skip)
        dev = {k: v.cpu().numpy() for k, v in g.scan_labels(skip=t_skip).items()}
        same(dev, spec.answer(r.cfg, fields, r.a, skip=skip), what)
        live = np.ones(E, bool) if skip is None else skip == 0
        same_bits(dev["range"][live], spec.newest_scan(cfg, obs.cpu().numpy())[live], what + ": range against the device's observation")
        seen[:] += np.bincount(dev["label"][live].reshape(-1), minlength=4)

    check("after the reset", g.obs)
    rng = np.random.default_rng(5)
    ends = skipped = 0
    sets = set()
    for t in range(30):
        act = random_actions(rng, E, t)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        done = rout["done"].copy()
        ends += int(done.sum())
        check("step %d" % t, go, skip=done if protocol == "next_step" else None)
        sets.add(g.cur)
        if protocol == "next_step":
            skipped += int(done.sum())
        if protocol == "reset_mask" and done.any():
            g.reset_arenas(gpu.torch.from_numpy(done).to(gpu.dev))
            r.restart(done)
            check("after reset(mask) at step %d" % t, g.obs)
    assert ends > 0, "no episode ended"
    assert all(seen[1:] > 0) and sets == {0, 1}, seen
    assert protocol != "next_step" or skipped == ends


# ---- e. scan noise ---------------------------------------------------------------------------------------------------------------
def test_noise_leaves_the_labels_and_stays_within_eight_sigma(gpu):
    """scan_noise_std = 0.02: where label == 0 the observation beam is range_max bit for bit (those beams never receive noise),
    elsewhere |obs - range| <= 8 std -- a bound: a Box-Muller draw of float32 uniforms cannot exceed sqrt(2 ln 2^24) = 5.8
    standard deviations --, and range, labels and indices equal those of the noise-off run of the same state.  (No auto-reset and a
    robot at rest: what the noisy scan decides -- crash, discomfort -- then moves nothing, and the two runs stay in one state while
    the pedestrians walk.)"""
    E, size, N, std = 8, 160, 6, 0.02
    occ = gpu.world.make_maps(E, size, 4343)
    occ[:4] = 0                                                                  # four open arenas: beams without a return
    got = {}
    for noise in (1, 0):
        cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=1, ped_model=abi.PED_SFM,
                                     auto_reset=abi.AUTORESET_NONE, n_spawn=8, seed=4343, field_format=abi.FIELD_U16T,
                                     add_scan_noise=noise, range_max=3.5)
        gpu.world.lidar_1081(cfg)
        g, r, _ = sim_and_oracle(gpu, cfg, occ, 5, check_reset=False, min_goal_dist=1.5, max_goal_dist=4.0,
                                 noise_std_range=(std, std))
        g.enable_scan_labels()
        obs = g.reset_obs()
        rows = []
        for t in range(3):
            if t:
                obs, _ = g.step(to_device(gpu, np.zeros((E, 2))))
            rows.append(({k: v.cpu().numpy().copy() for k, v in g.scan_labels().items()}, spec.newest_scan(cfg, obs.cpu().numpy()).copy()))
        got[noise] = rows
    rmax = np.float32(3.5)
    moved = n_none = 0
    for (lab, scan), (lab0, scan0) in zip(got[1], got[0]):
        same(lab, lab0, "labels with noise against labels without")
        same_bits(lab0["range"], scan0, "noise off: range against the observation")
        none = lab["label"] == spec.NONE
        same_bits(scan[none], np.full(int(none.sum()), rmax), "beams without a return")
        err = np.abs(scan[~none].astype(np.float64) - lab["range"][~none].astype(np.float64))
        print("max |obs - range| = %.4f = %.2f std over %d beams" % (err.max(), err.max() / std, err.size))
        assert (err <= 8 * std).all()
        moved += int((err > 0).sum()); n_none += int(none.sum())
    assert moved > 1000 and n_none > 1000


# ---- f. the gym surface ------------------------------------------------------------------------------------------------------
def _env(**kw):
    import nav_gym_amd
    from nav_gym_amd import registry
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([4, 4], "int"), obstacle_width=([0.3, 0.5], "float"))
    base = dict(num_envs=6, map_size=100, n_beams=64, seed=3, plan_paths=False, min_goal_dist=2.0, max_goal_dist=4.0,
                indoor_ratio=0.0, num_humans=4, max_episode_steps=6, scan_labels=True, env_param_range=ranges)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


def _keys(env):
    return KEYS if env.cfg.ped_model != abi.PED_NONE else KEYS[:3]


def _from_device_state(env, skip=None):
    """The specification on the environment's state, read back from the device (the maps through their occupancy)."""
    sim = env.sim
    s = sim.numpy_state(*(STATE if sim.cfg.ped_model != abi.PED_NONE else STATE_NO_PEDS))
    fields = ref.build_dt(np.stack([sim.occupancy(e) for e in range(env.num_envs)]))
    return spec.answer(sim.cfg, fields, s, skip=skip)


def _host(h):
    return {k: v.cpu().numpy() for k, v in h.items()}


def _drive(E):
    a = np.zeros((E, 2))
    a[: E // 2, 0] = 0.5
    return a


@pytest.mark.parametrize("model", ["sfm", "orca", "external", "none"])
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_info_scan_labels(gpu, model, mode):
    """info['scan_labels'] and env.scan_labels() equal a direct call on the same state and the specification on the state read
    back; dtypes and shapes; the two buffer sets alternate and what a step returned stays intact through the next one; next-step
    mode has empty rows where done is set; reset(mask) refreshes the masked rows."""
    torch = gpu.torch
    env = _env(pedestrian_model=model, autoreset_mode=mode)
    E, B, N, keys = 6, 64, env.cfg.max_peds, _keys(env)
    env.reset()
    h = env.scan_labels()
    assert tuple(h) == keys and ("hits" in h) == (model != "none")
    assert (h["range"].dtype, h["label"].dtype, h["index"].dtype) == (torch.float32, torch.uint8, torch.int8)
    assert tuple(h["range"].shape) == tuple(h["label"].shape) == tuple(h["index"].shape) == (E, B)
    assert model == "none" or (h["hits"].dtype == torch.int32 and tuple(h["hits"].shape) == (E, N))
    same(_host(h), call(gpu, env.sim.cfg, env.sim.st), "after reset()", keys)
    same(_host(h), _from_device_state(env), "after reset(): specification", keys)
    prev, ptrs, ends, empty, labels = None, set(), 0, 0, set()
    for t in range(14):
        kw = dict(human_actions=np.full((E, N, 2), 0.2)) if model == "external" else {}
        _, _, done, info = env.step(_drive(E), **kw)
        h = info["scan_labels"]
        assert h is env.scan_labels()
        ptrs.add(h["range"].data_ptr())
        skip = done.cpu().numpy().astype(np.uint8) if mode == "next_step" else None
        now = _host(h)
        same(now, call(gpu, env.sim.cfg, env.sim.st, skip=skip), "step %d" % t, keys)
        same(now, _from_device_state(env, skip=skip), "step %d: specification" % t, keys)
        if mode == "next_step" and skip.any():
            assert not now["range"][skip != 0].any() and not now["label"][skip != 0].any() and (now["index"][skip != 0] == -1).all()
            empty += int(skip.sum())
        if prev is not None:                                                     # the pair lifetime
            same(_host(prev[0]), prev[1], "step %d's rows after step %d" % (t - 1, t), keys)
        prev = (h, now)
        ends += int(done.sum())
        labels |= set(np.unique(now["label"]).tolist())
        assert "scan_labels" not in info.get("final_observation", {})
    assert len(ptrs) == 2 and ends > 0 and (mode != "next_step" or empty == ends)
    assert labels <= {0, 1} if model == "none" else spec.WALL in labels
    mask = np.array([1, 0, 0, 1, 0, 0], bool)
    before = env.sim.numpy_state("robot_pose")["robot_pose"]
    env.reset(mask=mask)
    after = _host(env.scan_labels())
    assert (env.sim.numpy_state("robot_pose")["robot_pose"][mask] != before[mask]).any(axis=1).all()      # they did restart
    same(after, _from_device_state(env, skip=env.sim.out["done"].cpu().numpy() if mode == "next_step" else None), "after reset(mask)", keys)
    env.close()


@pytest.mark.parametrize("pipeline", [0, None])
def test_worlds_that_draw_a_map_per_episode(gpu, pipeline):
    """randomize_maps with navsim_regen behind every step and on the pipelined reset path: the labels are launched behind the
    regenerated (installed) world, so a finished arena's rows belong to its new map."""
    env = _env(num_envs=8, map_size=200, randomize_maps=True, pregen_pipeline=pipeline, use_graphs=False, max_episode_steps=5)
    env.reset()
    ends = 0
    for t in range(12):
        _, _, done, info = env.step(_drive(8))
        same(_host(info["scan_labels"]), _from_device_state(env), "step %d" % t)
        ends += int(done.sum())
    assert env._step_path == ("pipelined" if pipeline is None else "plain") and ends >= 8
    env.close()


def test_single_environment_returns_numpy(gpu):
    env = _env(num_envs=1)
    env.reset()
    for t in range(3):
        _, _, done, info = env.step(np.zeros(2))
        h = info["scan_labels"]
        assert h is env.scan_labels()
        want = _from_device_state(env)
        for k, dt, n in (("range", np.float32, 64), ("label", np.uint8, 64), ("index", np.int8, 64), ("hits", np.int32, env.cfg.max_peds)):
            assert isinstance(h[k], np.ndarray) and h[k].shape == (n,) and h[k].dtype == dt, k
            same_bits(h[k], want[k][0], k)
    env.close()


def test_feature_off_allocates_and_reports_nothing(gpu):
    env = _env(scan_labels=False)
    env.reset()
    _, _, _, info = env.step(_drive(6))
    assert "scan_labels" not in info and env.sim.products == {}
    with pytest.raises(RuntimeError):
        env.sim.scan_labels()
    env.close()
