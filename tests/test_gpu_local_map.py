"""GPU: the egocentric local map (include/navsim.h navsim_local_map; NavGymEnv(observe_local_map=G)) against the NumPy
specification of tests/local_map_spec.py, bit for bit (float32 compared as uint32): single calls at the grid sizes where the
kernel's mapping changes (one cell, the odd scalar path, one wavefront, several strips of 16-byte stores, the maximum), three
cell sizes, both field formats with and without an overflow plane, every way an arena finds its map, maps that are not square off
the origin, the two masks, E = 1 and E = 0, the refusals, and through NavGymEnv under every reset path.  Every output is
pre-filled with a sentinel: the call writes every element."""
import ctypes as C

import numpy as np
import pytest

import dwa_spec
import local_map_spec as spec
import map_geometry_runs as runs
import map_geometry_scenes as mg
import ref
from dwa_call import device_state
from gpu_support import gpu, eq, same_bits, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

F32, U16T = abi.FIELD_F32, abi.FIELD_U16T
SENTINEL = 777.0


def _call(gpu, cfg, st, params, G, visible=None, skip=None, want_rc=0, n_out=None, shift=0):
    """navsim_local_map into a sentinel-filled output of n_out arenas (None: cfg.n_envs) -> NumPy [E,C,G,G].  params: a dict
    (spec.call_params) or an abi.NavsimLocalMapParams (then G only sizes the buffer).  shift: floats by which the output starts
    behind a 16-byte boundary."""
    torch = gpu.torch
    if isinstance(params, dict):
        p = gpu.sim.local_map_params(cfg, {k: v for k, v in params.items() if k in gpu.sim.LOCAL_MAP_KEYS}, G)
        Cn = int(params.get("channels", 4))
    else:
        p, Cn = params, 4
    E = cfg.n_envs if n_out is None else n_out
    n = E * Cn * G * G
    flat = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=gpu.dev)
    out = flat[shift:shift + n]
    t_vis = None if visible is None else to_device(gpu, np.asarray(visible, np.uint8))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_local_map(C.byref(cfg), C.byref(st), C.byref(p), None if visible is None else t_vis.data_ptr(),
                                         None if skip is None else t_skip.data_ptr(), out.data_ptr(), None)
    assert rc == want_rc, rc
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:shift] == SENTINEL).all() and (host[shift + n:] == SENTINEL).all(), "a write outside the output"
    return host[shift:shift + n].reshape(E, Cn, G, G)


def _same(dev, want, what):
    assert dev.dtype == want.dtype == np.float32 and dev.shape == want.shape, (what, dev.dtype, dev.shape, want.dtype, want.shape)
    for ch in range(want.shape[1]):
        same_bits(dev[:, ch], want[:, ch], "%s: channel %d" % (what, ch))


_BASE = {}


def _base():
    """The shared world, its float32 fields and the specification's answers, computed once."""
    if not _BASE:
        occ, w = spec.base_world()
        _BASE.update(occ=occ, w=w, fields=ref.build_dt(occ), want={})
    return _BASE


def _want(cfg, key, params, G, **kw):
    b = _base()
    if key not in b["want"]:
        b["want"][key] = spec.local_map(cfg, b["fields"], b["w"], params, G, **kw)
    return b["want"][key]


# ---- a. single calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_base_world_equals_the_spec(gpu, fmt):
    """E = 5, 100 x 100 maps, six pedestrian slots: G in {1, 7, 16, 64, 128} (and 30, 12: four-cell lanes that do not fill the
    last workgroup), cells of 0.05, 0.1 and 0.33 m, ahead 0 and 1.5 m, 1, 2 and 4 channels; windows partly outside the map."""
    b = _base()
    E, N, size, _ = spec.BASE
    cfg = spec.config(E, size, N, field_format=fmt)
    st, keep = device_state(gpu, cfg, b["occ"], b["w"], overflow=False)
    for G, cell, ahead, ch in spec.CALLS:
        p = spec.call_params(cell, ahead, ch)
        want = _want(cfg, (G, cell, ahead, ch), p, G)
        _same(_call(gpu, cfg, st, p, G), want, "G %d cell %g ahead %g channels %d" % (G, cell, ahead, ch))
    # the one cell outside the map
    p = spec.call_params(0.1, -2.0, 4)
    want = _want(cfg, "outside", p, 1)
    assert want[0, 0, 0, 0] == 0 and (want[1:, 0] != 0).any()
    _same(_call(gpu, cfg, st, p, 1), want, "one cell outside the map")
    # an output that does not start on a 16-byte boundary takes the scalar path at G % 4 == 0 too
    p = spec.call_params(0.1, 0.0, 4)
    for shift in (1, 2, 3, 4):
        _same(_call(gpu, cfg, st, p, 16, shift=shift), _want(cfg, (16, 0.1, 0.0, 4), p, 16), "output shifted by %d floats" % shift)
    # the defaults (cap = 2 m) and a radius of 0: nothing is covered but a centre a pedestrian stands on
    for G, p in ((32, {}), (16, dict(ped_radius=0.0, cap=0.25)), (16, dict(ped_radius=1.0, cap=5.0, cell=0.2))):
        full = dict(spec.DEFAULT, **p)
        _same(_call(gpu, cfg, st, full, G), _want(cfg, ("p", G, tuple(sorted(p.items()))), full, G), "parameters %s" % (p,))


def test_saturated_packed_field_with_its_overflow_plane(gpu):
    """A 560 x 560 hall: its middle lies further than 255 cells from every wall, which the packed field stores saturated -- the
    clearance there comes from the float32 overflow plane.  One shared map, no pedestrians, cap = 20 m."""
    size = 560
    occ = np.ones((1, size, size), np.uint8)
    occ[0, 5:size - 5, 5:size - 5] = 0
    fields = ref.build_dt(occ)
    assert fields.max() >= 270.0
    w = dict(robot_pose=np.array([[14.0, 14.1, 1.0], [3.0, 4.0, -2.0], [13.0, 15.0, 4.0]]), robot_goal=np.zeros((3, 2)),
             prev_action=np.zeros((3, 2)))
    p = dict(cell=0.33, ahead=0.5, cap=20.0, ped_radius=0.3, channels=1)
    for fmt in (U16T, F32):
        cfg = spec.config(3, size, 0, field_format=fmt, shared_field=1)
        st, keep = device_state(gpu, cfg, occ, w, overflow=(fmt == U16T), peds=False)
        for G in (64, 7):
            want = spec.local_map(cfg, fields, w, p, G)
            assert want[0].max() > 255 * 0.05 and (G == 7 or (want[1] == 0).any())
            _same(_call(gpu, cfg, st, p, G), want, "format %d G %d" % (fmt, G))


# ---- b. every way an arena finds its map --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_shared_field_and_permuted_map_slots(gpu, fmt):
    b = _base()
    E, N, size, _ = spec.BASE
    p, G = spec.call_params(0.1, 0.0, 4), 64
    cfg = spec.config(E, size, N, field_format=fmt, shared_field=1)
    st, keep = device_state(gpu, cfg, b["occ"][2:3], b["w"], overflow=False)
    want = spec.local_map(cfg, b["fields"][2:3], b["w"], p, G)
    own = _want(spec.config(E, size, N), (G, 0.1, 0.0, 4), p, G)
    assert (want[2] == own[2]).all() and (want[0, 0] != own[0, 0]).any()
    _same(_call(gpu, cfg, st, p, G), want, "shared field")
    perm = np.array([3, 0, 4, 1, 2])
    stored = np.empty_like(b["occ"]); stored[perm] = b["occ"]                    # arena e's map lies in slot perm[e]
    cfg = spec.config(E, size, N, field_format=fmt)
    st, keep = device_state(gpu, cfg, stored, b["w"], overflow=False, map_slot=perm)
    _same(spec.local_map(cfg, ref.build_dt(stored), b["w"], p, G, map_slot=perm), own, "the specification's own slot table")
    _same(_call(gpu, cfg, st, p, G), own, "permuted slots")


# ---- c. geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,k", [((-7.3, 12.9), 2.0), ((-7.3, 12.9), 0.5), ((-16.0, 32.0), 1.0)])
@pytest.mark.parametrize("H,W", [(85, 330), (330, 85)])
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_maps_that_are_not_square_off_the_origin(gpu, H, W, origin, k, fmt):
    """The worlds of tests/map_geometry_scenes.py with walking pedestrians, robots beyond the leading min(H, W) square in every
    second arena, on grids of 0.1, 0.025 and 0.05 m whose origins are no multiples of them: a cell beyond the leading square
    shows the map that is stored there (the rule bounds column i by map_w and row j by map_h; xy_to_ij's clip does not)."""
    cfg, occ, w = runs.scene(H, W, abi.PED_EXTERNAL, inside=False, seed=9, N=8, E=5, field_format=fmt)
    cfg, w = mg.geometry_twin(cfg, w, origin, k)
    st, keep = device_state(gpu, cfg, occ, w, overflow=None)
    M = min(H, W)
    beyond = 0
    for G, p in ((64, dict(cell=0.1 * k, ahead=0.0, cap=0.8 * k, ped_radius=0.3 * k, channels=4)),
                 (30, dict(cell=0.17 * k, ahead=1.0 * k, cap=2.0 * k, ped_radius=0.3 * k, channels=4))):
        want, info = spec.local_map(cfg, w["field"], w, p, G, detail=True)
        assert info["inside"].any() and not info["inside"].all() and info["covered"].any()
        for e in range(cfg.n_envs):                                             # cells inside the map but beyond the leading square
            wx, wy, _, _ = spec.centres(w["robot_pose"][e], G, p["cell"], p["ahead"])
            far = info["inside"][e] & (((wx - cfg.origin_x) / cfg.resolution >= M) | ((wy - cfg.origin_y) / cfg.resolution >= M))
            beyond += int((far & (want[e, 0] > 0)).sum())
        _same(_call(gpu, cfg, st, p, G), want, "%d x %d origin %s resolution %g G %d" % (H, W, origin, cfg.resolution, G))
    assert beyond > 0, "no free cell beyond the leading square in any window"


@pytest.mark.parametrize("H,W", [(17, 66), (66, 17)])
@pytest.mark.parametrize("fmt", [F32, U16T])
def test_maps_smaller_than_the_window(gpu, H, W, fmt):
    """17 x 66 and 66 x 17 cells (neither side a multiple of the packed field's 8-cell tile): a 2-cell border, one block; every
    window is far larger than the short side."""
    E, N = 3, 3
    occ = np.ones((E, H, W), np.uint8)
    occ[:, 2:H - 2, 2:W - 2] = 0
    occ[1, H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = 1
    long_x = W > H
    at = lambda a, b: (a, b) if long_x else (b, a)                               # (along the long side, across)
    w = dict(robot_pose=np.array([at(0.4, 0.43) + (0.3,), at(1.7, 0.4) + (2.0,), at(3.1, 0.52) + (-1.2,)]),
             robot_goal=np.zeros((E, 2)), prev_action=np.zeros((E, 2)), n_peds=np.array([3, 2, 0], np.int32),
             ped_pose=np.zeros((E, N, 3)), ped_vel=np.full((E, N, 2), 0.25))
    for e in range(E):
        for i in range(N):
            w["ped_pose"][e, i, :2] = at(0.5 + 0.9 * i + 0.2 * e, 0.3 + 0.1 * i)
    cfg = spec.config(E, max(H, W), N, map_h=H, map_w=W, field_format=fmt, origin_x=-1.3, origin_y=0.7)
    for k in ("robot_pose", "ped_pose"):
        w[k][..., 0] += cfg.origin_x; w[k][..., 1] += cfg.origin_y
    st, keep = device_state(gpu, cfg, occ, w, overflow=False)
    fields = ref.build_dt(occ)
    for G, p in ((16, spec.call_params(0.1, 0.0, 4)), (64, spec.call_params(0.05, 0.0, 4)), (7, spec.call_params(0.33, 0.5, 2))):
        want, info = spec.local_map(cfg, fields, w, p, G, detail=True)
        assert info["inside"].any() and not info["inside"].all() and (want[:, 0] > 0).any()
        _same(_call(gpu, cfg, st, p, G), want, "%d x %d G %d" % (H, W, G))


# ---- d. masks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [7, 16, 64])
def test_skip_mask(gpu, G):
    """A skipped arena's block is zero and nothing of the arena is read: a pose that is not a number, a pedestrian count far
    beyond the cap and pedestrians at infinity behind the mask change nothing."""
    b = _base()
    E, N, size, _ = spec.BASE
    cfg = spec.config(E, size, N, field_format=U16T)
    p = spec.call_params(0.1, 0.0, 4)
    skip = np.array([0, 1, 0, 0, 1], np.uint8)
    want = _want(cfg, ("skip", G), p, G, skip=skip)
    assert not want[1].any() and not want[4].any() and want[0].any()
    st, keep = device_state(gpu, cfg, b["occ"], b["w"], overflow=False)
    _same(_call(gpu, cfg, st, p, G, skip=skip), want, "skip")
    bad = {k: np.array(v, copy=True) for k, v in b["w"].items()}
    bad["robot_pose"][1] = np.nan
    bad["robot_pose"][4] = (1e300, -1e300, 1e9)
    bad["n_peds"][[1, 4]] = (1 << 30, -5)
    bad["ped_pose"][1] = np.inf
    bad["ped_vel"][4] = np.nan
    st, keep = device_state(gpu, cfg, b["occ"], bad, overflow=False)
    _same(_call(gpu, cfg, st, p, G, skip=skip), want, "invalid data behind the skip")
    _same(_call(gpu, cfg, st, p, G, skip=np.ones(E, np.uint8)), np.zeros_like(want), "every arena skipped")


def test_visible_mask(gpu):
    b = _base()
    E, N, size, _ = spec.BASE
    cfg = spec.config(E, size, N, field_format=U16T)
    st, keep = device_state(gpu, cfg, b["occ"], b["w"], overflow=False)
    rng = np.random.default_rng(5)
    vis = (rng.random((E, N)) < 0.5).astype(np.uint8)
    vis[spec.TIE_ARENA, :2] = (0, 1)                                            # the tie's loser alone: its velocity shows
    vis[0] = 0
    for G, ch in ((16, 4), (64, 4), (7, 2), (16, 1)):
        p = spec.call_params(0.1, 0.0, ch)
        want = spec.local_map(cfg, b["fields"], b["w"], p, G, visible=vis)
        if ch > 1:
            assert (want != _want(cfg, (G, 0.1, 0.0, ch), p, G)).any()
            assert (want[0, 1] == np.float32(spec.CAP)).all() and not want[0, 2:].any()
        _same(_call(gpu, cfg, st, p, G, visible=vis), want, "visible, G %d channels %d" % (G, ch))
    h = spec.TIE_G // 2
    want = spec.local_map(cfg, b["fields"], b["w"], spec.call_params(0.1, 0.0, 4), 16, visible=vis)
    assert (want[spec.TIE_ARENA, 2, h, h], want[spec.TIE_ARENA, 3, h, h]) == (np.float32(-0.375), np.float32(0.125))
    p = spec.call_params(0.1, 0.0, 4)
    none = _call(gpu, cfg, st, p, 16, visible=np.zeros((E, N), np.uint8))
    _same(none, spec.local_map(cfg, b["fields"], b["w"], p, 16, visible=np.zeros((E, N), np.uint8)), "nobody visible")
    assert (none[:, 1] == np.float32(spec.CAP)).all() and not none[:, 2:].any()
    eq(none[:, 0], _want(cfg, (16, 0.1, 0.0, 4), p, 16)[:, 0], "the wall channel does not depend on the mask")


def test_sixty_four_pedestrians(gpu):
    """max_peds = 64 with counts of 0, 1 and 64: the staging wavefront is full, nearly empty and empty."""
    E, N, size = 3, 64, 200
    occ, w = dwa_spec.random_world(E, N, size, 8104, n_peds=[0, 1, 64])
    cfg = spec.config(E, size, N, field_format=U16T)
    st, keep = device_state(gpu, cfg, occ, w, overflow=False)
    fields = ref.build_dt(occ)
    vis = (np.arange(E * N).reshape(E, N) % 3 != 0).astype(np.uint8)
    for G, p in ((64, spec.call_params(0.15, 0.0, 4, cap=1.0)), (7, spec.call_params(0.33, 0.5, 2)), (128, spec.call_params(0.08, 0.0, 4))):
        want, info = spec.local_map(cfg, fields, w, p, G, detail=True)
        assert info["counted"].tolist() == [0, 1, 64] and (G == 7 or info["covered"][2].sum() > 64)
        _same(_call(gpu, cfg, st, p, G), want, "G %d" % G)
        _same(_call(gpu, cfg, st, p, G, visible=vis), spec.local_map(cfg, fields, w, p, G, visible=vis), "G %d, two thirds visible" % G)


# ---- e. E = 1 and E = 0 ------------------------------------------------------------------------------------------------------------
def test_one_arena_and_none(gpu):
    b = _base()
    _, N, size, _ = spec.BASE
    one = {k: v[3:4] for k, v in b["w"].items()}
    cfg = spec.config(1, size, N, field_format=U16T)
    st, keep = device_state(gpu, cfg, b["occ"][3:4], one, overflow=False)
    for G in (16, 128, 7):
        p = spec.call_params(0.1, 0.0, 4)
        _same(_call(gpu, cfg, st, p, G), spec.local_map(cfg, b["fields"][3:4], one, p, G), "E = 1, G %d" % G)
    empty = cfg.copy(); empty.n_envs = 0
    assert (_call(gpu, empty, st, spec.call_params(0.1, 0.0, 4), 16, n_out=1) == SENTINEL).all()


# ---- f. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_alone(gpu):
    b = _base()
    E, N, size, _ = spec.BASE
    cfg = spec.config(E, size, N, field_format=U16T)
    st, keep = device_state(gpu, cfg, b["occ"], b["w"], overflow=False)
    good = spec.call_params(0.1, 0.0, 4)

    def refused(rc, c=cfg, s=st, **kw):
        p = gpu.sim.local_map_params(cfg, {k: v for k, v in good.items()}, 16)
        for k, v in kw.items():
            setattr(p, k, v)
        assert (_call(gpu, c, s, p, 16, want_rc=rc, n_out=E) == SENTINEL).all(), kw

    nan, inf = float("nan"), float("inf")
    for kw in (dict(cell=nan), dict(cell=0.0), dict(cell=-0.1), dict(cell=inf), dict(cap=0.0), dict(cap=nan), dict(cap=-1.0),
               dict(ahead=inf), dict(ahead=nan), dict(ped_radius=-0.1), dict(ped_radius=nan), dict(channels=3), dict(channels=0),
               dict(channels=8), dict(size=0), dict(size=129), dict(size=-16)):
        refused(abi.E_ARG, **kw)
    for k, bad in (("n_envs", -1), ("map_h", 0), ("map_w", -3), ("max_peds", 65), ("max_peds", 0), ("resolution", 0.0),
                   ("ped_model", abi.PED_NONE)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        refused(abi.E_ARG, c=c2)
    for k in ("robot_pose", "field", "n_peds", "ped_pose", "ped_vel"):
        s2 = abi.NavsimState()
        for name, v in keep.items():
            setattr(s2, name, None if name == k else v.data_ptr())
        refused(abi.E_ARG, s=s2)
    shared = cfg.copy(); shared.shared_field = 1
    s2, keep2 = device_state(gpu, cfg, b["occ"], b["w"], overflow=False, map_slot=np.arange(E))
    refused(abi.E_ARG, c=shared, s=s2)
    fmt = cfg.copy(); fmt.field_format = 9
    refused(abi.E_UNSUPPORTED, c=fmt)
    _same(_call(gpu, cfg, st, good, 16), _want(cfg, (16, 0.1, 0.0, 4), good, 16), "and then the call goes through")


# ---- g. through NavGymEnv -----------------------------------------------------------------------------------------------------------
def _env(**kw):
    import nav_gym_amd
    from nav_gym_amd import registry
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([4, 4], "int"), obstacle_width=([0.3, 0.5], "float"),
                  num_humans=([3, 3], "int"))
    base = dict(num_envs=8, map_size=100, n_beams=64, seed=11, plan_paths=False, min_goal_dist=2.0, max_goal_dist=4.0,
                indoor_ratio=0.0, pedestrian_model="sfm", max_episode_steps=7, observe_local_map=16,
                local_map_params=dict(cap=0.8), env_param_range=ranges)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


def _from_device_state(env, skip=None, visible=None):
    """The specification on the environment's state read back from the device (the maps through their occupancy)."""
    sim = env.sim
    names = ["robot_pose"] + (["n_peds", "ped_pose", "ped_vel"] if sim.cfg.ped_model != abi.PED_NONE else [])
    s = sim.numpy_state(*names)
    occ = np.stack([sim.occupancy(e) for e in range(env.num_envs)])
    p = sim.local_map_params
    params = dict(cell=p.cell, ahead=p.ahead, cap=p.cap, ped_radius=p.ped_radius, channels=p.channels)
    return spec.local_map(sim.cfg, ref.build_dt(occ), s, params, p.size, skip=skip, visible=visible)


def _drive(E, t):
    a = np.zeros((E, 2))
    a[: E // 2, 0] = 0.5
    a[:, 1] = 0.3 if t % 2 else -0.2
    return a


PATHS = dict(same_step={}, next_step=dict(autoreset_mode="next_step"), reset_mask=dict(auto_reset=False),
             staged_worlds=dict(map_size=200, randomize_maps=True, use_graphs=False),
             graphed=dict(map_size=200, randomize_maps=True, pregen_pipeline=0, use_graphs=True),
             visible_only=dict(num_humans=4, observe_humans=4, local_map_params=dict(cap=0.8, visible_only=True, cell=0.2)))


@pytest.mark.parametrize("path", list(PATHS))
def test_through_the_env(gpu, path):
    """8 arenas, 40 steps, G = 16, episodes of at most 7 steps: after every step info['local_map'] equals the specification on
    the state read back; the tensor a step returned is intact after the next step (the two buffer sets alternate)."""
    torch = gpu.torch
    env = _env(**PATHS[path])
    E, G = env.num_envs, 16
    env.reset()
    assert env._step_path == dict(staged_worlds="pipelined", graphed="graphed").get(path, "plain")
    next_step = path == "next_step"

    def visible():
        return env.observed_humans()["visible"].cpu().numpy().astype(np.uint8) if path == "visible_only" else None

    m = env.local_map()
    assert m.dtype == torch.float32 and tuple(m.shape) == (E, 4, G, G) and m.is_contiguous()
    _same(m.cpu().numpy(), _from_device_state(env, visible=visible()), "after reset()")
    ptrs, prev, ends, skipped, refilled, hidden = set(), None, 0, 0, 0, 0
    waiting = np.zeros(E, bool)
    for t in range(40):
        _, _, done, info = env.step(_drive(E, t))
        m = info["local_map"]
        assert m is env.local_map() and "local_map" not in info.get("final_observation", {})
        ptrs.add(m.data_ptr())
        done = done.cpu().numpy().astype(np.uint8)
        now = m.cpu().numpy()
        vis = visible()
        _same(now, _from_device_state(env, skip=done if next_step else None, visible=vis), "step %d" % t)
        if vis is not None:
            n = env.sim.numpy_state("n_peds")["n_peds"]
            hidden += int(sum((vis[e, :n[e]] == 0).sum() for e in range(E)))
        if next_step:
            assert not now[done != 0].any()
            skipped += int(done.sum())
            refilled += int(sum(now[e].any() for e in np.flatnonzero(waiting & (done == 0))))
            assert all(now[e].any() for e in np.flatnonzero(waiting & (done == 0)))
            waiting = done != 0
        if prev is not None:                                                     # the pair lifetime
            same_bits(prev[0].cpu().numpy(), prev[1], "step %d's map after step %d" % (t - 1, t))
        prev = (m, now.copy())
        ends += int(done.sum())
        if path == "reset_mask" and done.any():
            env.reset(mask=done.astype(bool))
            m = env.local_map()
            ptrs.add(m.data_ptr())
            _same(m.cpu().numpy(), _from_device_state(env), "after reset(mask) at step %d" % t)
            prev = None                                                          # (a reset takes a set of buffers like a step does)
    print(path, dict(ends=ends, skipped=skipped, refilled=refilled, hidden=hidden))
    assert len(ptrs) == 2 and ends >= E
    assert not next_step or (skipped > 0 and refilled > 0)
    assert path != "visible_only" or hidden > 0
    env.close()


def test_lifetime_of_a_returned_map(gpu):
    """The tensor step t returned is unchanged after step t + 1 and is the buffer step t + 2 writes."""
    env = _env()
    E = env.num_envs
    env.reset()
    maps, copies = [], []
    for t in range(4):
        _, _, _, info = env.step(_drive(E, t))
        maps.append(info["local_map"])
        copies.append(info["local_map"].cpu().numpy().copy())
        if t >= 1:
            same_bits(maps[t - 1].cpu().numpy(), copies[t - 1], "step %d's map after step %d" % (t - 1, t))
        if t >= 2:
            assert maps[t - 2].data_ptr() == maps[t].data_ptr() and maps[t - 1].data_ptr() != maps[t].data_ptr()
            assert (maps[t - 2].cpu().numpy() != copies[t - 2]).any(), "the robots moved: two steps later the buffer holds a new map"
    env.close()


def test_walls_only_and_single_environment(gpu):
    """A world without pedestrians has the wall channel alone; num_envs == 1 returns a NumPy array [C, G, G]."""
    env = _env(pedestrian_model="none", observe_local_map=12, local_map_params=None)
    env.reset()
    for t in range(3):
        _, _, _, info = env.step(_drive(8, t))
        assert tuple(info["local_map"].shape) == (8, 1, 12, 12)
        _same(info["local_map"].cpu().numpy(), _from_device_state(env), "walls only, step %d" % t)
    env.close()
    env = _env(num_envs=1)
    env.reset()
    for t in range(3):
        _, _, _, info = env.step(np.array([0.4, 0.1]))
        m = info["local_map"]
        assert m is env.local_map() and isinstance(m, np.ndarray) and m.shape == (4, 16, 16) and m.dtype == np.float32
        _same(m[None], _from_device_state(env), "E = 1, step %d" % t)
    env.close()


def test_feature_off_allocates_and_reports_nothing(gpu):
    env = _env(observe_local_map=None, local_map_params=None)
    env.reset()
    _, _, _, info = env.step(_drive(8, 0))
    assert "local_map" not in info and env.sim.products == {}
    with pytest.raises(RuntimeError):
        env.local_map()
    with pytest.raises(RuntimeError):
        env.sim.local_map()
    env.close()
