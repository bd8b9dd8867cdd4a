"""CPU: the local planner (include/navsim.h navsim_dwa) -- the specification of tests/dwa_spec.py on hand-made scenes with known
answers, the entry's place in the C ABI, its argument refusals, the keywords on NavGymEnv, and the population of the random
worlds the device test uses.  The device against that specification is tests/test_gpu_dwa.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dwa_spec as spec
import ref
from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(occ, w, N=0, **params):
    cfg = spec.config(1, occ.shape[0], N)
    p = dict(spec.SMALL, **params)
    o = spec.plan(cfg, ref.build_dt(occ), w, p, detail=True)
    full = dict(spec.DEFAULT, **p)
    return o, cfg, full


# ---- hand-made scenes ----------------------------------------------------------------------------------------------------------
def test_empty_hall_goes_straight_at_full_speed():
    """Goal 3 m straight ahead, w0 = 0, nine turn rates: the middle one is 0 exactly, and the fastest straight candidate wins."""
    w = spec.scene((1.5, 3.0, 0.0), (4.5, 3.0), prev=(0.3, 0.0))
    o, cfg, p = _plan(spec.hall(), w)
    vs, ws = spec.window(cfg, p, 0.3, 0.0)
    assert ws[4] == 0.0 and vs[-1] == 0.5 and vs[0] == pytest.approx(0.1)
    assert o["status"][0] == spec.OK and (o["first_hit"] == 0).all()
    assert o["best"][0] == 4 * 9 + 4 and o["twist"][0].tolist() == [0.5, 0.0] and o["action"][0].tolist() == [0.5, 0.0]
    assert o["clearance"][0] == np.float32(1.0)                                  # the cap: the walls are 1.3 m and more away
    s = o["scores"][0].reshape(5, 9)
    assert (np.diff(s[:, 4]) > 0).all() and (s[4, 4] > np.delete(s[4], 4)).all()


def test_one_stopping_distance_from_a_wall():
    """The robot drives at 0.5 m/s at a wall whose face is 0.9 m ahead: at full speed every turn rate reaches the margin within
    the 1.6 s of the horizon, so the choice is slower."""
    x = 1.5
    face = int(round((x + 0.9) / 0.05))
    w = spec.scene((x, 3.0, 0.0), (5.5, 3.0), prev=(0.5, 0.0))
    o, cfg, p = _plan(spec.hall([(face, spec.HALL, 0, spec.HALL)]), w, acc_lin=2.0)
    hit = o["first_hit"][0].reshape(5, 9)
    vs, _ = spec.window(cfg, p, 0.5, 0.0)
    assert vs[-1] == 0.5 and (hit[4] > 0).all() and (hit[0] == 0).all()
    assert o["status"][0] == spec.OK and o["best"][0] // 9 < 4 and o["twist"][0, 0] < 0.5
    assert hit[o["best"][0] // 9, o["best"][0] % 9] == 0 and np.isneginf(o["scores"][0].reshape(5, 9)[4]).all()


def test_boxed_in_is_blocked_with_the_latest_hit():
    """A dead end 0.6 m ahead and walls 0.45 m to either side, at 0.5 m/s with little braking: every candidate violates the
    margin; the one that does so last is chosen, the lowest index among equals."""
    x, y = 2.0, 3.0
    cx, cy = int(x / 0.05), int(y / 0.05)
    walls = [(cx + 12, spec.HALL, 0, spec.HALL), (0, spec.HALL, cy + 9, spec.HALL), (0, spec.HALL, 0, cy - 9)]
    w = spec.scene((x, y, 0.0), (5.0, 3.0), prev=(0.5, 0.0))
    o, cfg, p = _plan(spec.hall(walls), w, acc_lin=0.5)
    hit = o["first_hit"][0]
    assert o["status"][0] == spec.BLOCKED and (hit > 0).all() and hit.max() > hit.min()
    assert o["best"][0] == int(np.flatnonzero(hit == hit.max())[0]) and np.isneginf(o["scores"][0]).all()
    vs, ws = spec.window(cfg, p, 0.5, 0.0)
    assert o["twist"][0].tolist() == [vs[o["best"][0] // 9], ws[o["best"][0] % 9]]
    assert 0.1 <= o["clearance"][0] <= 0.3 + 1e-6                                # of the steps before the hit


def test_crossing_pedestrian_closes_candidates():
    """A pedestrian walks across the straight line ahead: candidates that are admissible without pedestrians are not with."""
    w = spec.scene((1.5, 3.0, 0.0), (4.5, 3.0), prev=(0.4, 0.0), peds=[(2.6, 2.2)], vels=[(0.0, 0.75)])
    on, cfg, p = _plan(spec.hall(), w, N=1)
    off, _, _ = _plan(spec.hall(), w, N=1, use_peds=0)
    a_on, a_off = on["first_hit"][0] == 0, off["first_hit"][0] == 0
    assert a_off.all() and not a_on.all() and a_on.any() and (on["hit_kind"][0][~a_on] == spec.PED).all()
    assert not a_on[4 * 9 + 4] and off["best"][0] == 4 * 9 + 4 and on["best"][0] != off["best"][0] and on["status"][0] == spec.OK
    none, _, _ = _plan(spec.hall(), w, N=0)                                      # NAVSIM_PED_NONE: ignored whatever use_peds says
    assert (none["first_hit"] == 0).all() and none["best"][0] == off["best"][0]


def test_all_weights_zero_takes_the_lowest_admissible_index():
    w = spec.scene((1.5, 3.0, 0.0), (4.5, 3.0), prev=(0.4, 0.0), peds=[(2.3, 2.45)], vels=[(0.0, 0.0)])
    o, cfg, p = _plan(spec.hall(), w, N=1, w_progress=0.0, w_heading=0.0, w_clearance=0.0, w_speed=0.0)
    adm = o["first_hit"][0] == 0
    assert not adm[0] and adm.any() and (o["scores"][0][adm] == 0.0).all()       # (turning right at any speed meets the pedestrian)
    assert o["best"][0] == int(np.flatnonzero(adm)[0]) > 0 and o["status"][0] == spec.OK


def test_previous_twist_outside_the_limits_collapses_the_window():
    w = spec.scene((1.5, 3.0, 0.0), (4.5, 3.0), prev=(0.9, -2.0))
    o, cfg, p = _plan(spec.hall(), w)
    vs, ws = spec.window(cfg, p, 0.9, -2.0)
    assert (vs == 0.5).all() and (ws == -0.64).all()                             # 0.7 > 0.5 and -1.36 < -0.64: clamp(v0), clamp(w0)
    assert o["twist"][0].tolist() == [0.5, -0.64] and o["best"][0] == 0          # 45 equal candidates: the tie rule
    assert (o["scores"][0] == o["scores"][0][0]).all()
    vs, ws = spec.window(cfg, dict(p, n_v=1, n_w=1), 0.2, 0.1)                   # one candidate: the upper end of the window
    assert vs.tolist() == [0.4] and ws.tolist() == [0.64]


def test_skip_and_subgoal():
    w = spec.scene((1.5, 3.0, 1.0), (4.5, 3.0), prev=(0.3, 0.0))
    cfg = spec.config(1, spec.HALL)
    f = ref.build_dt(spec.hall())
    o = spec.plan(cfg, f, w, spec.SMALL, skip=[1])
    assert all(not o[k].any() for k in spec.KEYS)
    # the goal in the robot's frame as the sub-goal: the same target up to the rotation's rounding
    dx, dy = 3.0, 0.0
    sub = np.array([[np.cos(1.0) * dx + np.sin(1.0) * dy, np.cos(1.0) * dy - np.sin(1.0) * dx]], np.float32)
    a, b = spec.plan(cfg, f, w, spec.SMALL), spec.plan(cfg, f, w, spec.SMALL, subgoal=sub)
    assert a["best"][0] == b["best"][0] and np.abs(a["scores"] - b["scores"]).max() < 1e-6


# ---- the shared random worlds ---------------------------------------------------------------------------------------------------
def test_population_of_the_random_worlds():
    """What the device comparison needs to mean something, on the specification alone."""
    E, N, size, seed = spec.BASE
    occ, w = spec.random_world(E, N, size, seed)
    T = spec.BASE_PARAMS["horizon"]
    pop = spec.population(spec.plan(spec.config(E, size, N), ref.build_dt(occ), w, spec.BASE_PARAMS, detail=True), T)
    print(pop)
    assert pop["blocked"] >= 1 and 4 * pop["partial"] >= E
    assert pop["wall_hits"] > 0 and pop["ped_hits"] > 0 and pop["hits_at_1"] > 0 and pop["hits_at_T"] > 0
    E, N, size, seed = spec.MAXIMA
    occ, w = spec.random_world(E, N, size, seed)
    T = spec.MAXIMA_PARAMS["horizon"]
    pop = spec.population(spec.plan(spec.config(E, size, N), ref.build_dt(occ), w, spec.MAXIMA_PARAMS, detail=True), T)
    print(pop)
    assert pop["partial"] >= 1 and pop["wall_hits"] > 0 and pop["ped_hits"] > 0 and pop["hits_at_T"] > 0


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()         # no structure changed its size
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state() and C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert re.search(r"\bint navsim_dwa\(", header) and "navsim_dwa" in abi.EXPORTS and hasattr(L, "navsim_dwa")
    fields = struct_fields(header, "navsim_dwa_params")
    assert fields == ["acc_lin", "acc_rot", "body_radius", "body_offset", "ped_radius", "margin", "clearance_cap", "w_progress",
                      "w_heading", "w_clearance", "w_speed", "n_discs", "n_v", "n_w", "horizon", "use_peds"]
    assert [n for n, _ in abi.NavsimDwaParams._fields_] == fields
    assert C.sizeof(abi.NavsimDwaParams) == 14 * 8 + 5 * 4 + 4 and abi.NavsimDwaParams.n_discs.offset == 112
    assert struct_fields(header, "navsim_dwa_out") == [n for n, _ in abi.NavsimDwaOut._fields_] == list(abi.DWA_OUT) == list(spec.KEYS)
    for name, value in (("DWA_MAX_DISCS", 4), ("DWA_OK", 1), ("DWA_BLOCKED", 2)):
        assert re.search(r"#define NAVSIM_%s\s+%d\b" % (name, value), header) and getattr(abi, name) == value
    assert (spec.OK, spec.BLOCKED) == (abi.DWA_OK, abi.DWA_BLOCKED)


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib, sim
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, map_h=100, map_w=100, max_peds=4, ped_model=abi.PED_EXTERNAL)
    base = ("robot_pose", "robot_goal", "prev_action", "field")
    peds = ("n_peds", "ped_pose", "ped_vel")

    def state(skip=(), **extra):
        st = abi.NavsimState()
        for k in base + peds + tuple(extra):
            setattr(st, k, None if k in skip else ptr)
        return st

    def outputs(skip=()):
        return abi.NavsimDwaOut(**{k: (None if k in skip else ptr) for k in abi.DWA_OUT})

    def params(**kw):
        p = sim.dwa_params(cfg)
        for k, v in kw.items():
            if k == "body_offset":
                p.body_offset[3] = v
            else:
                setattr(p, k, v)
        return p

    ref_ = lambda x: None if x is None else C.byref(x)
    call = lambda c=cfg, s=state(), p=params(), o=outputs(): L.navsim_dwa(ref_(c), ref_(s), ref_(p), None, None, ref_(o), None)
    assert call(c=None) == call(s=None) == call(p=None) == call(o=None) == abi.E_ARG
    for k in ("twist", "action", "clearance", "best", "status"):
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    for k in base + peds:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
    nan, inf = float("nan"), float("inf")
    for k in ("acc_lin", "acc_rot", "body_radius", "ped_radius", "margin", "clearance_cap"):
        for bad in (nan, inf, -0.01):
            assert call(p=params(**{k: bad})) == abi.E_ARG, (k, bad)
    for k in ("w_progress", "w_heading", "w_clearance", "w_speed", "body_offset"):
        for bad in (nan, inf, -inf):
            assert call(p=params(**{k: bad})) == abi.E_ARG, (k, bad)
    for k, bad in (("n_discs", 0), ("n_discs", 5), ("n_v", 0), ("n_v", 17), ("n_w", 0), ("n_w", 33), ("horizon", 0), ("horizon", 33)):
        assert call(p=params(**{k: bad})) == abi.E_ARG, (k, bad)
    for k, bad in (("n_envs", -1), ("map_h", 0), ("map_w", 0), ("max_peds", 0), ("max_peds", 65), ("action_kind", 2),
                   ("resolution", 0.0), ("time_step", nan)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        assert call(c=c2) == abi.E_ARG, (k, bad)
    wheels = cfg.copy(); wheels.action_kind = abi.ACTION_WHEELS; wheels.wheel_radius = 0.0
    assert call(c=wheels) == abi.E_ARG
    shared = cfg.copy(); shared.shared_field = 1
    assert call(c=shared, s=state(map_slot=1)) == abi.E_ARG
    fmt = cfg.copy(); fmt.field_format = 7
    assert call(c=fmt) == abi.E_UNSUPPORTED
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted, the optional arrays absent, and the
    # pedestrian arrays absent where they are not read
    empty = cfg.copy(); empty.n_envs = 0
    assert call(c=empty, p=params(n_v=16, n_w=32, horizon=32, n_discs=4, margin=0.0), o=outputs(skip=("scores", "first_hit"))) == abi.OK
    assert call(c=empty, p=params(n_v=1, n_w=1, horizon=1, n_discs=1, use_peds=0), s=state(skip=peds)) == abi.OK
    none = empty.copy(); none.ped_model = abi.PED_NONE; none.max_peds = 0
    assert call(c=none, s=state(skip=peds)) == abi.OK


# ---- host wiring ----------------------------------------------------------------------------------------------------------------
def test_parameter_defaults_and_unknown_keys():
    from nav_gym_amd import lib, sim
    cfg = lib.default_config()
    d = sim.dwa_defaults(cfg)
    assert tuple(d) == tuple(sim.DWA_KEYS) == tuple(spec.DEFAULT)
    for k, v in spec.DEFAULT.items():
        assert d[k] == pytest.approx(v), k
    assert (d["margin"], d["ped_radius"], d["clearance_cap"], d["acc_lin"], d["acc_rot"]) == (0.1, 0.3, 1.0, 1.0, 3.2)
    assert (d["n_v"], d["n_w"], d["horizon"]) == (5, 9, 8)
    assert (d["w_progress"], d["w_heading"], d["w_clearance"], d["w_speed"]) == (1.0, 0.2, 0.3, 0.1)
    # the two discs cover the threshold footprint: every corner and edge midpoint lies in one of them
    from nav_gym_amd import robots
    for name in robots.ROBOTS:
        dd = sim.dwa_defaults(cfg, name)
        fp = np.asarray(robots.ROBOTS[name]["threshold_footprint"], np.float64)
        xs = np.linspace(fp[:, 0].min(), fp[:, 0].max(), 27)
        ys = np.linspace(fp[:, 1].min(), fp[:, 1].max(), 27)
        pts = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
        dist = np.min([np.hypot(pts[:, 0] - o, pts[:, 1]) for o in dd["body_offset"]], axis=0)
        assert len(dd["body_offset"]) == 2 and (dist <= dd["body_radius"] + 1e-12).all(), name
    p = sim.dwa_params(cfg, dict(body_offset=(0.0, 0.1, 0.2), n_v=3, horizon=4, use_peds=False, w_speed=2))
    assert (p.n_discs, p.n_v, p.n_w, p.horizon, p.use_peds, p.w_speed) == (3, 3, 9, 4, 0, 2.0)
    assert list(p.body_offset) == [0.0, 0.1, 0.2, 0.0]
    with pytest.raises(ValueError, match="acc_lin, acc_rot, body_radius"):
        sim.dwa_params(cfg, dict(accel=3.0))
    with pytest.raises(ValueError, match="1 .. 4 disc centres"):
        sim.dwa_params(cfg, dict(body_offset=(0.0,) * 5))
    lay = sim.dwa_layout(5, 45)
    assert [(k, d_, shape) for k, d_, _, _, shape in lay[:-1]] == [("twist", "float64", (5, 2)), ("action", "float64", (5, 2)),
                                                                   ("clearance", "float32", (5,)), ("best", "int32", (5,)),
                                                                   ("status", "uint8", (5,))]
    full = sim.dwa_layout(5, 45, scores=True)
    assert [(k, shape) for k, _, _, _, shape in full[5:-1]] == [("scores", (5, 45)), ("first_hit", (5, 45))]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in full) and all(a[3] <= b[2] for a, b in zip(full, full[1:]))


def test_env_keywords():
    import copy
    import pickle
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="dwa", local_planner_params=dict(horizon=4, n_w=5))
    assert env.local_planner == "dwa" and env.local_planner_params == dict(horizon=4, n_w=5)
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.local_planner == "dwa" and twin.local_planner_params == dict(horizon=4, n_w=5) and twin.num_envs == 3
    with pytest.raises(RuntimeError):
        env.planner_action()                               # before reset()
    with pytest.raises(ValueError, match="local_planner='dwa'"):                   # parameters without the feature
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner_params=dict(horizon=4))
    with pytest.raises(ValueError, match="acc_lin, acc_rot, body_radius"):         # an unknown key names the known ones
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="dwa", local_planner_params=dict(steps=4))
    with pytest.raises(ValueError, match="None or 'dwa'"):
        nav_gym_env.make("NavGym-v0", num_envs=3, local_planner="teb")
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.local_planner is None
    with pytest.raises(RuntimeError):
        plain.planner_action()
    assert "local_planner" not in registry.spec("NavGym-v0")["kwargs"] and "local_planner_params" not in registry.spec("NavGym-v0")["kwargs"]
