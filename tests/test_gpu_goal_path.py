"""GPU: the goal path (include/navsim.h navsim_goal_path; NavGymEnv(goal_path=True)) against the NumPy specification of
tests/goal_path_spec.py, bit for bit -- dist, distance and subgoal as raw bits, status: single calls on raw states at the grid
sizes where the rebuild's thread-to-cell mapping changes, both field formats, hand-made scenes with known answers, the rebuild /
skip / key rules, a closed loop through NavGymEnv under every reset path, and the refusals.  Every output is pre-filled with a
sentinel: the call writes every element."""
import numpy as np
import pytest

import goal_path_spec as spec
import ref
from goal_path_call import H3, INF, KEYS, GoalField, answer, call, device_state, same
from gpu_support import gpu, eq, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu


# ---- a. single calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
@pytest.mark.parametrize("E,size,seed", spec.RANDOM_WORLDS + ((3, 103, 5303),), ids=lambda v: str(v))
def test_single_call_equals_the_spec(gpu, E, size, seed, fmt):
    """100 x 100 maps -- 20 x 20 nav cells, fewer cells than threads; 500 x 500 -- 100 x 100, ten cells a thread; 103 x 103, no
    multiple of 5 (navsim_build_field takes any size: the last three rows and columns belong to no nav cell).  Then other
    parameters, a skip mask, and a second call that finds every key current."""
    occ, w = spec.random_world(E, size, seed)
    cfg = spec.config(E, size, field_format=fmt)
    fields = ref.build_dt(occ)
    st, keep = device_state(gpu, cfg, occ, w)
    want = answer(cfg, fields, w, {})
    dev = call(gpu, cfg, st, {})
    same(dev, want, "defaults")
    assert dev["field"].count() == E
    assert (dev["field"].key.cpu().numpy()[:, 0] == w["episode"]).all()
    again = call(gpu, cfg, st, {}, field=dev["field"])
    same(again, want, "second call")
    assert again["field"].count() == E
    for what, p in (("narrow", dict(hard_clearance=H3, clearance=H3, band_cost=1, lookahead=0.5)),
                    ("wide band", dict(hard_clearance=0.2, clearance=1.5, band_cost=16, lookahead=6.0))):
        same(call(gpu, cfg, st, p), answer(cfg, fields, w, p), what)
    skip = (np.arange(E) % 2 == 0).astype(np.uint8)
    dev = call(gpu, cfg, st, {}, skip=skip)
    want = answer(cfg, fields, w, {}, skip=skip)
    want["dist"][skip != 0] = 0x7777                                             # neither rebuilt ...
    same(dev, want, "skip")
    assert dev["field"].count() == int((skip == 0).sum()) and (dev["field"].key.cpu().numpy()[skip != 0] == -1).all()


@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
@pytest.mark.parametrize("rows,size", [(85, 330), (330, 85)])
def test_maps_that_are_not_square(gpu, rows, size, fmt):
    """map_h != map_w: 17 x 66 and 66 x 17 nav cells -- the rows and columns the kernel carries along from cell to cell differ, and
    1024 threads step over several rows at once or over a fraction of one.  (xy_to_ij clips x by map_h and y by map_w, env.py:1228
    -1253: on such maps some positions land in a clipped cell -- in the specification as on the device.)"""
    E = 6
    occ, w = spec.random_world(E, max(rows, size), 5309 + rows, n_obstacles=16)
    occ = np.ascontiguousarray(occ[:, :rows, :size])
    w["robot_pose"][:, :2] = np.minimum(w["robot_pose"][:, :2], [size * 0.05 - 0.3, rows * 0.05 - 0.3])
    w["robot_goal"] = np.minimum(w["robot_goal"], [size * 0.05 - 0.3, rows * 0.05 - 0.3])
    cfg = spec.config(E, size, map_h=rows, map_w=size, field_format=fmt)
    assert spec.grid_shape(cfg) == (rows // 5, size // 5)
    st, keep = device_state(gpu, cfg, occ, w)
    want = answer(cfg, ref.build_dt(occ), w, {})
    assert (want["status"] & spec.OK).sum() >= 2 and ((want["dist"] != INF) & (want["dist"] > 0)).sum() > 500
    same(call(gpu, cfg, st, {}), want, "%d x %d cells" % (rows, size))
    p = dict(hard_clearance=H3, clearance=0.5, band_cost=2, lookahead=4.0)
    same(call(gpu, cfg, st, p), answer(cfg, ref.build_dt(occ), w, p), "%d x %d cells, other parameters" % (rows, size))


def test_the_lds_limit(gpu):
    """E = 2 at 1000 x 1000 cells, 200 x 200 nav cells, 122.4 KB of LDS: the reference's map size."""
    E, size = 2, 1000
    occ, w = spec.random_world(E, size, 5304, n_obstacles=60)
    cfg = spec.config(E, size, field_format=abi.FIELD_U16T)
    st, keep = device_state(gpu, cfg, occ, w, overflow=None)
    want = answer(cfg, ref.build_dt(occ), w, {})
    assert (want["status"] != 0).all() and ((want["dist"] != INF) & (want["dist"] > 700)).any()
    same(call(gpu, cfg, st, {}), want, "200 x 200 nav cells")


def test_saturated_packed_field_with_its_overflow_plane(gpu):
    """A 560 x 560 hall: its middle lies further than 255 cells from every wall, which the packed field stores saturated.  With
    clearance = 13 m (260 cells) the class of those cells is decided by the float32 overflow plane."""
    size = 560
    occ = np.ones((1, size, size), np.uint8)
    occ[0, 5:size - 5, 5:size - 5] = 0
    fields = ref.build_dt(occ)
    assert fields.max() >= 270.0
    w = dict(robot_pose=np.array([[3.0, 4.0, 1.0], [14.1, 13.9, -2.0]]), robot_goal=np.array([[25.0, 24.0], [14.0, 14.0]]),
             episode=np.zeros(2, np.int64))
    p = dict(clearance=13.0, lookahead=3.0)
    for fmt in (abi.FIELD_U16T, abi.FIELD_F32):
        cfg = spec.config(2, size, field_format=fmt, shared_field=1)
        st, keep = device_state(gpu, cfg, occ, w, overflow=(fmt == abi.FIELD_U16T))
        want = answer(cfg, fields, w, p, detail=True)
        m = want["classes"][0]
        assert (m == 1).sum() > 20 and (m == 3).sum() > 5000                      # the few clear cells in the middle
        same(call(gpu, cfg, st, p), want, "format %d" % fmt)


def test_permuted_map_slots(gpu):
    E, size, seed = 5, 100, 5305
    occ, w = spec.random_world(E, size, seed)
    perm = np.array([3, 0, 4, 1, 2])
    stored = np.empty_like(occ); stored[perm] = occ                            # arena e's map lies in slot perm[e]
    cfg = spec.config(E, size, field_format=abi.FIELD_U16T)
    st, keep = device_state(gpu, cfg, stored, w, map_slot=perm)
    want = answer(cfg, ref.build_dt(stored), w, {}, map_slot=perm)
    same(want, answer(cfg, ref.build_dt(occ), w, {}), "the specification's own slot table")
    same(call(gpu, cfg, st, {}), want, "permuted slots")


# ---- b. hand-made scenes with known answers ------------------------------------------------------------------------------------
def _scene(gpu, nav, pose, goal, fmt=abi.FIELD_U16T, **params):
    occ = spec.scale5(nav)[None]
    cfg = spec.config(1, occ.shape[1], field_format=fmt)
    w = dict(robot_pose=np.array([pose], np.float64), robot_goal=np.array([goal], np.float64), episode=np.zeros(1, np.int64))
    st, keep = device_state(gpu, cfg, occ, w)
    want = answer(cfg, ref.build_dt(occ), w, params, detail=True)
    dev = call(gpu, cfg, st, params)
    same(dev, want, "scene")
    return dev, want, cfg


@pytest.mark.parametrize("fmt", [abi.FIELD_F32, abi.FIELD_U16T])
def test_spiral_corridor(gpu, fmt):
    """The relaxation has to carry the goal's 0 down ~850 cells of a corridor that turns back on itself: many sweeps, one field."""
    nav = spec.spiral()
    m = spec.classes(spec.config(1, 300), ref.build_dt(spec.scale5(nav))[0], {})
    far = spec.field_from_classes(m, (2, 2))
    far = np.where(far == INF, 0, far)
    jc, ic = np.unravel_index(int(far.argmax()), far.shape)                      # the lane's far end, in the middle
    dev, want, cfg = _scene(gpu, nav, spec.centre(ic, jc) + (0.3,), spec.centre(2, 2), fmt)
    assert dev["status"][0] == spec.OK and dev["dist"][0, jc, ic] == far[jc, ic] > 12000
    assert float(dev["distance"][0]) > 0.9 * far[jc, ic] * cfg.resolution


def test_sealed_room_goal_on_a_wall_and_the_other_scenes(gpu):
    nav = spec.room(24)
    nav[8:16, 8] = nav[8:16, 15] = nav[8, 8:16] = nav[15, 8:16] = True            # a sealed room in the middle
    inside, outside = spec.centre(11, 12), spec.centre(3, 4)
    dev, want, cfg = _scene(gpu, nav, inside + (0.5,), outside)                  # the robot inside, the goal outside
    assert dev["status"][0] == spec.OFF_FIELD and dev["dist"][0, 12, 11] == INF
    d = np.float64(np.hypot(outside[0] - inside[0], outside[1] - inside[1]))
    assert abs(float(dev["distance"][0]) - d) < 1e-6 and abs(float(np.hypot(*dev["subgoal"][0])) - d) < 1e-6
    # the goal IN the room's wall: dist 0 there, and the cell is admissible from both sides -- the one door of the room
    dev, want, cfg = _scene(gpu, nav, outside + (0.5,), spec.centre(8, 10), hard_clearance=H3)
    assert dev["dist"][0, 10, 8] == 0 and dev["status"][0] == spec.OK and dev["dist"][0, 10, 7] == 5 * 3 == dev["dist"][0, 10, 9]
    assert dev["dist"][0, 9, 8] == INF and dev["dist"][0, 11, 8] == INF           # (the wall beside it stays a wall)
    pose = (spec.centre(3, 4)[0] + 0.07, spec.centre(3, 4)[1] - 0.05, 2.0)       # the robot in the goal cell
    dev, want, cfg = _scene(gpu, nav, pose, outside)
    assert dev["status"][0] == spec.OK | spec.REACHED and want["cells"][0] == [(3, 4)]
    assert abs(float(dev["distance"][0]) - float(np.hypot(0.07, 0.05))) < 1e-6
    dev, want, cfg = _scene(gpu, nav, spec.centre(1, 5) + (0.0,), outside, hard_clearance=H3)        # the robot in the band
    assert want["classes"][0][5, 1] == 3 and dev["status"][0] == spec.OK | spec.REACHED and dev["dist"][0, 5, 1] == 7 * 3 + 5 * 3
    far = spec.centre(20, 20)
    dev, want, cfg = _scene(gpu, nav, far + (0.0,), outside, lookahead=0.0)       # look-ahead 0: the robot's own cell centre
    assert dev["status"][0] == spec.OK and np.abs(dev["subgoal"][0]).max() < 1e-6
    assert abs(float(dev["distance"][0]) - dev["dist"][0, 20, 20] * cfg.resolution) < 1e-5
    dev, want, cfg = _scene(gpu, nav, far + (0.0,), outside, lookahead=100.0)     # a look-ahead longer than the path
    assert dev["status"][0] == spec.OK | spec.REACHED and want["cells"][0][-1] == (3, 4) and len(want["cells"][0]) > 17


# ---- c. rebuild, skip and the key ----------------------------------------------------------------------------------------------
def test_rebuild_skip_and_the_key(gpu):
    E, size, seed = 6, 200, 5308
    occ, w = spec.random_world(E, size, seed)
    cfg = spec.config(E, size, field_format=abi.FIELD_U16T)
    fields = ref.build_dt(occ)
    st, keep = device_state(gpu, cfg, occ, w)
    want = answer(cfg, fields, w, {})
    assert want["status"].tolist() == [1, 3, 4, 3, 1, 1]                         # (this seed: arena 0 walks and does not arrive)
    dev = call(gpu, cfg, st, {})
    F = dev["field"]
    same(dev, want, "first call")
    assert F.count() == E
    # nothing changed: nothing is rebuilt -- not even the arena whose stored field the test scribbles on, which proves that
    # the look-up reads the STORED field
    e = int(np.flatnonzero(want["status"] == spec.OK)[0])
    scribbled = want["dist"].copy()
    finite = scribbled[e] != INF
    scribbled[e][finite] = (scribbled[e][finite].astype(np.int64) * 2 + 9).clip(0, INF - 1).astype(np.uint16)
    F.dist.copy_(to_device(gpu, scribbled.view(np.int16)))
    dev = call(gpu, cfg, st, {}, field=F)
    want2 = answer(cfg, fields, w, {}, dist=scribbled)
    same(dev, want2, "scribbled")
    assert F.count() == E and dev["distance"][e] != want["distance"][e]
    # a new goal for arena 1, a new episode number for arena 4: those two alone are rebuilt (the scribble stays)
    w["robot_goal"][1] = w["robot_pose"][3, :2]
    w["episode"][4] += 1
    keep["robot_goal"].copy_(to_device(gpu, w["robot_goal"]))
    keep["episode"].copy_(to_device(gpu, w["episode"]))
    others = [x for x in range(E) if x not in (1, 4, e)]
    fresh = answer(cfg, fields, w, {})
    dev = call(gpu, cfg, st, {}, field=F)
    same(dev, fresh, "goal / episode: rebuilt", arenas=[x for x in (1, 4) if x != e] + others)
    assert F.count() == E + 2
    if e not in (1, 4):
        eq(dev["dist"][e], scribbled[e], "the scribble stays")
    # rebuild[e] forces it
    force = np.zeros(E, np.uint8); force[e] = 1
    dev = call(gpu, cfg, st, {}, field=F, rebuild=force)
    same(dev, fresh, "forced")
    assert F.count() == E + 3
    # a skipped arena is neither rebuilt (although forced, although its key is stale) nor read
    w["episode"][2] += 5
    keep["episode"].copy_(to_device(gpu, w["episode"]))
    skip = np.zeros(E, np.uint8); skip[2] = 1
    dev = call(gpu, cfg, st, {}, field=F, rebuild=np.ones(E, np.uint8), skip=skip)
    assert F.count() == E + 3 + (E - 1) and dev["status"][2] == 0 and dev["distance"][2] == 0 and not dev["subgoal"][2].any()
    assert F.key.cpu().numpy()[2, 0] == w["episode"][2] - 5
    same(dev, fresh, "skip", arenas=[x for x in range(E) if x != 2])
    dev = call(gpu, cfg, st, {}, field=F)                                       # ... and is rebuilt by the next call that reads it
    same(dev, fresh, "after the skip")
    assert F.count() == E + 3 + (E - 1) + 1


# ---- d. closed loop through NavGymEnv ------------------------------------------------------------------------------------------
def _env(**kw):
    import nav_gym_amd
    from nav_gym_amd import registry
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([4, 4], "int"), obstacle_width=([0.3, 0.5], "float"))
    base = dict(num_envs=16, map_size=100, n_beams=64, seed=7, plan_paths=False, min_goal_dist=2.0, max_goal_dist=4.0,
                indoor_ratio=0.0, pedestrian_model="none", max_episode_steps=7, goal_path=True, env_param_range=ranges)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


_FIELD_CACHE = {}


def _from_device_state(env, skip=None):
    """The specification on the environment's state, read back from the device (the maps through their occupancy), fields and
    outputs from scratch (a field is a pure function of the map and the goal cell: computed once per pair)."""
    sim = env.sim
    s = sim.numpy_state("robot_pose", "robot_goal")
    occ = np.stack([sim.occupancy(e) for e in range(env.num_envs)])
    fields = ref.build_dt(occ)
    p = dict(spec.DEFAULT, **(env.goal_path_params or {}))
    E = env.num_envs
    Hc, Wc = spec.grid_shape(sim.cfg)
    out = dict(dist=np.full((E, Hc, Wc), INF, np.uint16), distance=np.zeros(E, np.float32), subgoal=np.zeros((E, 2), np.float32),
               status=np.zeros(E, np.uint8))
    for e in range(E):
        if skip is not None and skip[e]:
            continue
        g = spec.nav_cell(sim.cfg, *s["robot_goal"][e])
        key = (occ[e].tobytes(), g)
        if key not in _FIELD_CACHE:
            m = spec.classes(sim.cfg, fields[e], p)
            _FIELD_CACHE[key] = (m, spec.field_from_classes(m, g))
        m, out["dist"][e] = _FIELD_CACHE[key]
        out["distance"][e], out["subgoal"][e], out["status"][e] = spec.query(sim.cfg, m, out["dist"][e], s["robot_pose"][e],
                                                                             s["robot_goal"][e], p)
    return out


def _host(env, h):
    return dict(distance=h["distance"].cpu().numpy(), subgoal=h["subgoal"].cpu().numpy(), status=h["status"].cpu().numpy(),
                dist=env.goal_field().cpu().numpy().view(np.uint16))


def _check(env, h, what, skip=None):
    dev, want = _host(env, h), _from_device_state(env, skip=skip)
    live = None if skip is None else np.flatnonzero(np.asarray(skip) == 0)      # (a skipped arena's field is not touched)
    same(dev, want, what, arenas=live)
    if skip is not None:
        sk = np.asarray(skip) != 0
        assert not dev["status"][sk].any() and not dev["distance"][sk].any() and not dev["subgoal"][sk].any(), what
    return want


@pytest.mark.parametrize("path", ["same_step", "next_step", "reset_mask", "randomize_staged", "randomize_plain", "randomize_graphed"])
def test_closed_loop_through_the_env(gpu, path):
    """16 arenas, 60 random-action steps, episodes of at most 7 steps: after every step info['goal_path'] and env.goal_field()
    equal the specification on the state read back -- a stale field on any reset path shows up here -- and the rebuild counter
    lies between the restarts and the restarts plus what the resets forced.  The three forms of a world that draws a map per
    episode: staged worlds installed inside the step (the env's default for it; it never uses graphs), navsim_regen behind the
    step as plain launches, and the same as ONE captured graph (the env's default with pregen_pipeline=0) -- the call then
    follows the graph's launch."""
    _FIELD_CACHE.clear()
    kw = dict(same_step={}, next_step=dict(autoreset_mode="next_step"), reset_mask=dict(auto_reset=False),
              randomize_staged=dict(randomize_maps=True), randomize_plain=dict(randomize_maps=True, pregen_pipeline=0, use_graphs=False),
              randomize_graphed=dict(randomize_maps=True, pregen_pipeline=0))[path]
    env = _env(**kw)
    E = env.num_envs
    env.reset()
    _check(env, env.goal_path(), "after reset()")
    assert env.sim.goal_path_rebuilds() == E
    rng = np.random.default_rng(11)
    restarts = masked = skipped = 0
    ptrs, prev = set(), None
    for t in range(60):
        act = np.stack([rng.uniform(0.0, 0.5, E), rng.uniform(-0.64, 0.64, E)], axis=1)
        _, _, done, info = env.step(act)
        h = info["goal_path"]
        assert h is env.goal_path() and set(h) == set(KEYS)
        ptrs.add(h["distance"].data_ptr())
        done = done.cpu().numpy().astype(np.uint8)
        if path == "next_step":
            restarts += int(info["reset_mask"].sum().item())
            skipped += int(done.sum())
            now = _check(env, h, "step %d" % t, skip=done)
        else:
            if path != "reset_mask":
                restarts += int(done.sum())
            now = _check(env, h, "step %d" % t)
        if prev is not None:                                                     # the pair lifetime: last step's rows are intact
            for k in KEYS:
                eq(prev[0][k].cpu().numpy(), prev[1][k], "step %d's %s after step %d" % (t - 1, k, t))
        prev = (h, {k: h[k].cpu().numpy().copy() for k in KEYS})
        if path == "reset_mask" and done.any():
            env.reset(mask=done.astype(bool))
            masked += int(done.sum())
            _check(env, env.goal_path(), "after reset(mask) at step %d" % t)
            prev = None                                                          # (a reset takes a set of buffers like a step does)
    rebuilds = env.sim.goal_path_rebuilds()
    print(path, dict(rebuilds=rebuilds, restarts=restarts, masked=masked, skipped=skipped))
    assert len(ptrs) == 2 and restarts + masked >= 3 * E                         # every arena restarted several times
    assert rebuilds >= restarts and rebuilds <= E * 1 + restarts + masked
    assert path != "next_step" or skipped > 0
    if path.startswith("randomize"):
        assert env._step_path == dict(randomize_staged="pipelined", randomize_plain="plain", randomize_graphed="graphed")[path]
    # a second reset() of every arena, and one through a mask under auto-reset
    env.reset()
    _check(env, env.goal_path(), "after the second reset()")
    mask = np.arange(E) % 3 == 0
    env.reset(mask=mask)
    _check(env, env.goal_path(), "after reset(mask)", skip=env.sim.out["done"].cpu().numpy() if path == "next_step" else None)
    assert env.sim.goal_path_rebuilds() <= rebuilds + E + E                      # (the mask forces its arenas, the keys the rest)
    env.close()


def test_single_environment_returns_numpy(gpu):
    env = _env(num_envs=1)
    env.reset()
    for t in range(3):
        _, _, done, info = env.step(np.array([0.3, 0.1]))
        h = info["goal_path"]
        assert h is env.goal_path()
        assert isinstance(h["distance"], np.float32) and isinstance(h["status"], np.uint8)
        assert isinstance(h["subgoal"], np.ndarray) and h["subgoal"].shape == (2,) and h["subgoal"].dtype == np.float32
        want = _from_device_state(env)
        assert h["distance"].view(np.uint32) == want["distance"][0].view(np.uint32) and h["status"] == want["status"][0]
        eq(h["subgoal"].view(np.uint32), want["subgoal"][0].view(np.uint32), "subgoal")
    env.close()


def test_off_by_default(gpu):
    env = _env(goal_path=False)
    env.reset()
    _, _, _, info = env.step(np.zeros((16, 2)))
    assert "goal_path" not in info and env.sim.products == {}
    with pytest.raises(RuntimeError):
        env.goal_path()
    with pytest.raises(RuntimeError):
        env.sim.goal_path()
    env.close()


# ---- e. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_alone(gpu):
    E, size = 3, 100
    occ, w = spec.random_world(E, size, 5307)
    cfg = spec.config(E, size, field_format=abi.FIELD_U16T)
    st, keep = device_state(gpu, cfg, occ, w)
    F = GoalField(gpu, cfg)

    def refused(rc, c=cfg, s=st, **p):
        dev = call(gpu, c, s, p, field=F, want_rc=rc, n_out=E)
        assert (dev["distance"] == 777.0).all() and (dev["subgoal"] == 777.0).all() and (dev["status"] == 77).all()
        assert (dev["dist"] == 0x7777).all() and F.count() == 0 and (F.key.cpu().numpy() == -1).all()

    nan, inf = float("nan"), float("inf")
    for p in (dict(hard_clearance=nan), dict(clearance=inf), dict(lookahead=nan), dict(hard_clearance=0.15), dict(clearance=0.29),
              dict(band_cost=0), dict(band_cost=17), dict(lookahead=-1.0)):
        refused(abi.E_ARG, **p)
    for k, bad in (("n_envs", -1), ("map_h", 4), ("map_w", 3)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        refused(abi.E_ARG, c=c2)
    for k in ("robot_pose", "robot_goal", "episode", "field"):
        s2 = abi.NavsimState()
        for name, v in keep.items():
            setattr(s2, name, None if name == k else v.data_ptr())
        refused(abi.E_ARG, s=s2)
    shared = cfg.copy(); shared.shared_field = 1
    s2, keep2 = device_state(gpu, cfg, occ, w, map_slot=np.arange(E))
    refused(abi.E_ARG, c=shared, s=s2)
    fmt = cfg.copy(); fmt.field_format = 9
    refused(abi.E_UNSUPPORTED, c=fmt)
    big = cfg.copy(); big.map_h = big.map_w = 1200
    refused(abi.E_UNSUPPORTED, c=big)
    same(call(gpu, cfg, st, {}, field=F), answer(cfg, ref.build_dt(occ), w, {}), "and then the call goes through")
