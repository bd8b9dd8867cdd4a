"""CPU: observed pedestrians (include/navsim.h navsim_ped_observe) -- the entry's place in the C ABI, its argument refusals, the
keywords on NavGymEnv, hand-made cases of the specification (tests/ped_observe_spec.py) with known answers, and the population
of the random worlds the device test uses.  The device against that specification is tests/test_gpu_ped_observe.py."""
import copy
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import ped_observe_spec as spec
import ref
from helpers import struct_fields
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_and_structures_in_header_library_and_exports():
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()         # no structure changed its size
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert re.search(r"\bint navsim_ped_observe\(", header)
    assert "navsim_ped_observe" in abi.EXPORTS and hasattr(L, "navsim_ped_observe")
    fields = struct_fields(header, "navsim_ped_observe_params")
    assert fields == ["ped_radius", "sensor_range", "max_obs", "rays", "occlusion", "fov"]
    assert [n for n, _ in abi.NavsimPedObserveParams._fields_] == fields
    assert C.sizeof(abi.NavsimPedObserveParams) == 2 * 8 + 4 * 4
    fields = struct_fields(header, "navsim_ped_observation")
    assert fields == ["state", "index", "count", "visible"]
    assert [n for n, _ in abi.NavsimPedObservation._fields_] == fields == list(abi.PED_OBSERVATION)
    assert C.sizeof(abi.NavsimPedObservation) == 4 * C.sizeof(C.c_void_p)
    assert abi.MAX_PEDS == 64 and re.search(r"#define NAVSIM_MAX_PEDS\s+64\b", header)


def test_argument_refusals_without_gpu():
    """Every refusal is decided before anything touches the device: they come back on a machine without one."""
    from nav_gym_amd import lib
    L = lib.load()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    cfg = lib.default_config(n_envs=2, max_peds=4, ped_model=abi.PED_SFM, map_h=16, map_w=16)
    st_fields = ("robot_pose", "n_peds", "ped_pose", "ped_vel", "field")

    def state(skip=()):
        st = abi.NavsimState()
        for k in st_fields:
            setattr(st, k, None if k in skip else ptr)
        return st

    def outputs(skip=()):
        o = abi.NavsimPedObservation()
        for k in abi.PED_OBSERVATION:
            setattr(o, k, None if k in skip else ptr)
        return o

    def params(**kw):
        p = abi.NavsimPedObserveParams(ped_radius=0.3, sensor_range=3.0, max_obs=4, rays=3, occlusion=1, fov=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    ref_ = lambda x: None if x is None else C.byref(x)
    call = lambda c=cfg, s=state(), p=params(), o=outputs(): L.navsim_ped_observe(ref_(c), ref_(s), ref_(p), None, ref_(o), None)
    assert call(c=None) == call(s=None) == call(p=None) == call(o=None) == abi.E_ARG
    for k in ("state", "index", "count"):
        assert call(o=outputs(skip=(k,))) == abi.E_ARG, k
    for k in st_fields:
        assert call(s=state(skip=(k,))) == abi.E_ARG, k
    none = cfg.copy(); none.ped_model = abi.PED_NONE
    assert call(c=none) == abi.E_ARG
    for k, bad in (("max_obs", 0), ("max_obs", 65), ("max_obs", -1), ("rays", 0), ("rays", 2), ("rays", 4),
                   ("ped_radius", -0.1), ("ped_radius", float("nan")), ("ped_radius", float("inf")),
                   ("sensor_range", -1.0), ("sensor_range", float("nan")), ("sensor_range", float("inf"))):
        assert call(p=params(**{k: bad})) == abi.E_ARG, (k, bad)
    for k, bad in (("n_envs", -1), ("max_peds", 0), ("max_peds", 65)):
        c2 = cfg.copy(); setattr(c2, k, bad)
        assert call(c=c2) == abi.E_ARG, (k, bad)
    # nothing to do is not an error and launches nothing -- at the bounds of what is accepted
    empty = cfg.copy(); empty.n_envs = 0; empty.max_peds = 64
    assert call(c=empty, p=params(max_obs=64, rays=1, ped_radius=0.0, sensor_range=0.0)) == abi.OK
    assert call(c=empty, o=outputs(skip=("visible",))) == abi.OK                  # (visible may be NULL)


# ---- the keywords on NavGymEnv ----------------------------------------------------------------------------------------------
def test_env_keywords():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, observe_humans=4, observe_params=dict(rays=1, sensor_range=4.0))
    assert env.observe_humans == 4 and env.observe_params == dict(rays=1, sensor_range=4.0)
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.observe_humans == 4 and twin.observe_params == dict(rays=1, sensor_range=4.0) and twin.num_envs == 3
    with pytest.raises(RuntimeError):
        env.observed_humans()                              # before reset()
    assert nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, observe_humans=5, pedestrian_model="orca").observe_humans == 5
    for bad in (0, -1, 6, 2.0, True, "3"):                 # a positive int no larger than the world's pedestrian cap
        with pytest.raises(ValueError):
            nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, observe_humans=bad)
    with pytest.raises(ValueError):                        # no pedestrians to observe
        nav_gym_env.make("NavGym-v0", num_envs=3, observe_humans=1, pedestrian_model="none")
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, observe_humans=1, num_humans=0)
    with pytest.raises(ValueError):                        # parameters without the feature
        nav_gym_env.make("NavGym-v0", num_envs=3, observe_params=dict(rays=1))
    with pytest.raises(ValueError):                        # an unknown key
        nav_gym_env.make("NavGym-v0", num_envs=3, num_humans=5, observe_humans=2, observe_params=dict(beams=3))
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.observe_humans is None
    with pytest.raises(RuntimeError):
        plain.observed_humans()
    assert "observe_humans" not in registry.spec("NavGym-v0")["kwargs"]
    assert "observe_params" not in registry.spec("NavGym-v0")["kwargs"]


def test_parameter_defaults_and_unknown_keys():
    from nav_gym_amd import lib, sim
    cfg = lib.default_config(max_peds=7)
    p = sim.ped_observe_params(cfg)
    assert p.ped_radius == sim.ped_orca_params(cfg).ped_radius and p.sensor_range == cfg.range_max
    assert (p.max_obs, p.rays, p.occlusion, p.fov) == (7, 3, 1, 1)
    p = sim.ped_observe_params(cfg, dict(max_obs=3, rays=1, occlusion=False, fov=0, ped_radius=0.25, sensor_range=2.0))
    assert (p.ped_radius, p.sensor_range, p.max_obs, p.rays, p.occlusion, p.fov) == (0.25, 2.0, 3, 1, 0, 0)
    with pytest.raises(ValueError):
        sim.ped_observe_params(cfg, dict(range=3.0))
    # the four arrays of one set inside their blob: in the structure's order, 16-byte aligned, disjoint
    lay = sim.ped_observation_layout(5, 3, 7)
    assert [(k, d, shape) for k, d, _, _, shape in lay[:-1]] == [
        ("state", "float32", (5, 3, 5)), ("index", "int32", (5, 3)), ("count", "int32", (5,)), ("visible", "uint8", (5, 7))]
    assert [hi - lo for _, _, lo, hi, _ in lay[:-1]] == [300, 60, 20, 35]
    assert all(lo % 16 == 0 for _, _, lo, _, _ in lay) and all(a[3] <= b[2] for a, b in zip(lay, lay[1:])) and lay[-1][3] >= lay[-2][3]


# ---- hand-made cases of the specification: a 60 x 60 map with one wall 0.8 m ahead of the robot --------------------------------
def _run(peds, robot_cell_occupied=False, lidar_270=False, skip=None, vel=None, **params):
    cfg = spec.wall_config(len(peds), lidar_270=lidar_270)
    w = spec.wall_case(peds, vel=vel)
    return spec.observe(cfg, ref.build_dt(spec.wall_map(robot_cell_occupied)), w["robot_pose"], w["n_peds"], w["ped_pose"],
                        w["ped_vel"], params, skip=skip, detail=True)


def test_spec_behind_the_wall():
    o = _run([spec.at(1.5, 0.0)])                          # 0.7 m behind the wall: all three lines of sight end in it
    assert o["visible"].tolist() == [[0]] and o["count"].tolist() == [0] and not o["clear"].any()
    assert o["index"].tolist() == [[-1] * 4] and not o["state"].any()
    o = _run([spec.at(1.5, 0.0)], occlusion=0)             # without occlusion everything in range and view is seen
    assert o["visible"].tolist() == [[1]] and o["index"][0, 0] == 0 and not o["needs_march"].any()


def test_spec_side_ray():
    """The centre and the -radius silhouette point lie behind the wall's end, the +radius point looks past it."""
    p = spec.at(1.5, 0.8125)
    o = _run([p], rays=3)
    assert o["clear"][0, 0].tolist() == [False, True, False] and o["visible"].tolist() == [[1]]
    o = _run([p], rays=1)
    assert o["visible"].tolist() == [[0]] and o["count"].tolist() == [0]


def test_spec_within_the_radius_needs_no_cast():
    o = _run([spec.at(0.25, 0.0)])
    assert o["visible"].tolist() == [[1]] and not o["needs_march"].any()
    o = _run([spec.at(0.25, 0.0), spec.at(0.5, 0.0)], robot_cell_occupied=True)      # every cast ends in the robot's own cell
    assert o["visible"].tolist() == [[1, 0]] and o["needs_march"].tolist() == [[False, True]]


def test_spec_equal_distances_go_by_index():
    for peds in ([spec.at(0.0, -0.5), spec.at(0.0, 0.5)], [spec.at(0.0, 0.5), spec.at(0.0, -0.5)]):
        o = _run(peds, vel=[(0.25, 0.0), (0.0, 0.5)])
        assert o["d"][0, 0] == o["d"][0, 1] == 0.5
        assert o["index"].tolist() == [[0, 1, -1, -1]] and o["count"].tolist() == [2]
        assert o["state"][0, 0].tolist() == [0.0, peds[0][1] - spec.ROBOT[1], 0.25, 0.0, 0.5]
        assert o["state"][0, 1].tolist() == [0.0, peds[1][1] - spec.ROBOT[1], 0.0, 0.5, 0.5]


def test_spec_range_boundary_is_inside():
    assert _run([spec.at(0.5, 0.0)], ped_radius=0.25, sensor_range=0.25)["visible"].tolist() == [[1]]       # d - r == range
    assert _run([spec.at(0.5, 0.0)], ped_radius=0.25, sensor_range=np.nextafter(0.25, 0.0))["visible"].tolist() == [[0]]


def test_spec_field_of_view():
    behind = [spec.at(-0.5, 0.0)]                          # bearing pi: outside the 270-degree lidar
    assert _run(behind, lidar_270=True)["visible"].tolist() == [[0]]
    assert _run(behind, lidar_270=True, fov=0)["visible"].tolist() == [[1]]
    assert _run([spec.at(0.0, 0.5)], lidar_270=True)["visible"].tolist() == [[1]]


def test_spec_cap_and_skip():
    peds = [spec.at(0.625, 0.0), spec.at(0.25, 0.125), spec.at(0.5, 0.0)]
    o = _run(peds, max_obs=2)
    assert o["count"].tolist() == [3] and o["index"].tolist() == [[1, 2]] and o["visible"].tolist() == [[1, 1, 1]]
    assert o["state"][0, :, 4].tolist() == [float(np.float32(np.sqrt(0.25 ** 2 + 0.125 ** 2))), 0.5]
    o = _run(peds, max_obs=2, skip=[1])
    assert o["count"].tolist() == [0] and o["index"].tolist() == [[-1, -1]] and not o["state"].any() and not o["visible"].any()


def test_spec_rotates_into_the_robot_frame():
    cfg = spec.wall_config(1)
    w = spec.wall_case([spec.at(0.0, 0.5)], vel=[(0.0, 0.25)], robot=spec.ROBOT[:2] + (np.pi / 2,))
    o = spec.observe(cfg, ref.build_dt(spec.wall_map()), w["robot_pose"], w["n_peds"], w["ped_pose"], w["ped_vel"], {})
    x, y, vx, vy, d = o["state"][0, 0].tolist()            # straight ahead of a robot that looks along +y, walking away from it
    assert abs(x - 0.5) < 1e-7 and abs(y) < 1e-7 and abs(vx - 0.25) < 1e-7 and abs(vy) < 1e-7 and d == 0.5


# ---- the random worlds of the device test hold every kind of pedestrian ---------------------------------------------------------
def test_population_of_the_random_worlds():
    """A condition on the test's own inputs, not a measurement: enough pedestrians of every kind for the device comparison to
    mean something (sensor_range = 3 m on 6 m maps, K = 4)."""
    total = dict(seen=0, occluded=0, side_only=0, out_of_range=0, max_count=0)
    for E, N, seed, n_peds in spec.RANDOM_WORLDS:
        occ, w = spec.random_world(E, N, spec.RANDOM_SIZE, seed, n_peds)
        pop = spec.population(spec.random_config(E, N, spec.RANDOM_SIZE), ref.build_dt(occ), w, dict(sensor_range=3.0, max_obs=4))
        print((E, N), pop)
        for k, v in pop.items():
            total[k] = max(total[k], v) if k == "max_count" else total[k] + v
    assert total["seen"] >= 40 and total["occluded"] >= 15 and total["side_only"] >= 4 and total["out_of_range"] >= 10
    assert total["max_count"] > 4                          # an arena sees more than K: the cap is exercised
