"""CPU: ORCA pedestrians of NavGym-v0 (include/navsim.h navsim_ped_orca) -- the entry's place in the C ABI, its argument
refusals, the keyword on NavGymEnv, and the specification itself (tests/ped_orca_spec.py: a composition of the oracle's
functions) run closed-loop on the oracle alone.  The device against that specification is tests/test_gpu_ped_orca.py."""
import copy
import ctypes as C
import math
import pickle

import numpy as np
import pytest

import ped_orca_spec as spec
import ref
from helpers import keti_thresholds
from nav_gym_amd import abi, world

CLOSE = 0.6 - 1e-4                  # the margin test_crowd_orca_properties uses for discs of 0.3 m


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_stays_7_with_one_new_export():
    from nav_gym_amd import lib
    L = lib.load()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert abi.NavsimConfig._fields_[-1][0] == "max_episode_steps" and abi.NavsimStepIO._fields_[-1][0] == "truncated"
    assert "navsim_ped_orca" in abi.EXPORTS and hasattr(L, "navsim_ped_orca")

    class Orca(C.Structure):        # include/navsim.h's field lists, written out again
        _fields_ = [("time_step", C.c_float), ("neighbor_dist", C.c_float), ("time_horizon", C.c_float),
                    ("time_horizon_obst", C.c_float), ("max_neighbors", C.c_int32)]

    class PedOrca(C.Structure):
        _fields_ = [("orca", Orca), ("ped_radius", C.c_double), ("robot_radius", C.c_double), ("safety_space", C.c_double),
                    ("robot_visible", C.c_int32)]
    assert C.sizeof(abi.NavsimPedOrcaParams) == C.sizeof(PedOrca) == 56
    assert [(n, getattr(abi.NavsimPedOrcaParams, n).offset) for n, _ in abi.NavsimPedOrcaParams._fields_] == \
        [("orca", 0), ("ped_radius", 24), ("robot_radius", 32), ("safety_space", 40), ("robot_visible", 48)]


def test_argument_refusals_without_gpu():
    from nav_gym_amd import lib, sim
    L = lib.load()
    cfg = lib.default_config(n_envs=2, max_peds=5, ped_model=abi.PED_EXTERNAL)
    st = abi.NavsimState()
    one = (C.c_double * 64)()
    ptr = C.addressof(one)
    for name in ("n_peds", "ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head",
                 "robot_pose", "prev_action"):
        setattr(st, name, ptr)
    call = lambda c, p, out=ptr: L.navsim_ped_orca(C.byref(c), C.byref(st), None if p is None else C.byref(p), out, None)
    good = sim.ped_orca_params(cfg)
    assert call(cfg, good, None) == abi.E_ARG                                    # no ped_cmd
    assert call(cfg, None) == abi.E_ARG                                          # no parameters
    for model in (abi.PED_NONE, abi.PED_SFM):
        c2 = cfg.copy(); c2.ped_model = model
        assert call(c2, good) == abi.E_ARG, model
    c2 = cfg.copy(); c2.max_peds = abi.ORCA_MAX_AGENTS                           # 64 pedestrians + the robot
    assert call(c2, good) == abi.E_ARG
    for key, bad in (("ped_radius", 0.0), ("ped_radius", -0.3), ("robot_radius", 0.0), ("time_step", 0.0), ("time_step", -0.2),
                     ("time_horizon", 0.0), ("time_horizon", -5.0), ("max_neighbors", -1)):
        assert call(cfg, sim.ped_orca_params(cfg, {key: bad})) == abi.E_ARG, (key, bad)
    with pytest.raises(ValueError):
        sim.ped_orca_params(cfg, {"neighbour_dist": 3.0})
    # the defaults: orca.py:62-65, the simulator's time step, discs around the footprints of robots.py
    assert (good.orca.neighbor_dist, good.orca.time_horizon, good.orca.time_horizon_obst, good.orca.max_neighbors) == (10, 5, 5, 10)
    assert good.orca.time_step == np.float32(cfg.time_step) and good.safety_space == 0.0 and good.robot_visible == 1
    assert good.ped_radius == math.hypot(0.22, 0.19) and abs(good.ped_radius - 0.291) < 1e-3
    assert good.robot_radius == math.hypot(0.70, 0.4)


# ---- the keyword on NavGymEnv -----------------------------------------------------------------------------------------------
def test_env_keyword():
    import nav_gym_env
    from nav_gym_amd import registry
    env = nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", randomize_maps=True,
                           orca_params=dict(max_neighbors=4, safety_space=0.05))
    assert env.pedestrian_model == "orca" and env.cfg.ped_model == abi.PED_EXTERNAL
    assert env.pregen_pipeline == 0 and env.orca_params == dict(max_neighbors=4, safety_space=0.05)
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.pedestrian_model == "orca" and twin.cfg.ped_model == abi.PED_EXTERNAL and twin.num_envs == 3
        assert twin.orca_params == dict(max_neighbors=4, safety_space=0.05) and twin.pregen_pipeline == 0
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", randomize_maps=True, pregen_pipeline=4)
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, pedestrian_model="orca", orca_params=dict(max_neighbours=4))
    kwargs = registry.spec("NavGym-v0")["kwargs"]
    assert "orca_params" not in kwargs and kwargs.get("pedestrian_model", "sfm") != "orca"
    assert nav_gym_env.make("NavGym-v0", num_envs=3).orca_params is None


# ---- the specification, closed loop on the oracle ----------------------------------------------------------------------------
def _scene(starts, goals, v_pref, headings):
    """One obstacle-free 240 x 240 arena, the robot parked at (1.5, 1.5), pedestrians with one waypoint each: their goal."""
    n = len(starts)
    cfg = ref.default_config(n_envs=1, map_h=240, map_w=240, max_peds=n, ped_model=abi.PED_EXTERNAL,
                             auto_reset=abi.AUTORESET_NONE, n_spawn=0, n_beams=64, time_step=0.2)
    world.lidar_full_circle(cfg, 64)
    occ = world.make_maps(1, 240, 7, n_obstacles=0)
    P = cfg.max_waypoints
    wp = np.zeros((1, n, P, 2)); wp[0, :, 0] = goals
    pose = np.zeros((1, n, 3)); pose[0, :, :2] = starts; pose[0, :, 2] = headings
    rp = np.array([[1.5, 1.5, 0.0]])
    thr, dthr = keti_thresholds(cfg)
    r = ref.RefSim(cfg, dict(
        field=ref.build_dt(occ), scan_noise_std=np.zeros(1, np.float32),
        scan_threshold=thr, scan_discomfort=dthr,
        robot_pose=rp, robot_goal=np.array([[10.5, 10.5]]), prev_action=np.zeros((1, 2)), prev_pose=np.zeros((1, 3)),
        n_hist=np.zeros(1, np.int32), episode=np.zeros(1, np.int64), steps=np.zeros(1, np.int64),
        n_peds=np.full(1, n, np.int32), ped_pose=pose, ped_vel=np.zeros((1, n, 2)), ped_prev_yaw=np.zeros((1, n)),
        ped_dist=np.zeros((1, n, 3)), ped_v_pref=np.full((1, n), v_pref), ped_has_legs=np.ones((1, n), np.uint8),
        ped_waypoints=wp, ped_n_waypoints=np.ones((1, n), np.int32), ped_cmd=np.zeros((1, n, 2))))
    r.reset_obs()
    return cfg, r


def _min_pair_dist(xy):
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    return d[np.triu_indices(len(xy), 1)].min()


def _roll(cfg, r, p, steps):
    closest = np.inf
    for _ in range(steps):
        cmd, head, _ = spec.ped_orca(cfg, r.a, p)
        r.a["ped_wp_head"][...] = head
        r.set_ped_cmd(cmd)
        r.step(np.zeros((1, 2)))
        assert not r.out["done"].any()                              # the parked robot is never in the way
        closest = min(closest, _min_pair_dist(r.a["ped_pose"][0, :, :2]))
    return closest


@pytest.mark.parametrize("v_pref", [0.6, 1.0])
def test_head_on_pair_passes_and_arrives(v_pref):
    starts = np.array([[3.0, 6.0], [9.0, 6.001]])
    goals = starts[::-1].copy()
    cfg, r = _scene(starts, goals, v_pref, [0.0, math.pi])
    closest = _roll(cfg, r, spec.params(cfg, ped_radius=0.3), 150)
    miss = np.sqrt(((r.a["ped_pose"][0, :, :2] - goals) ** 2).sum(1)).max()
    print("head-on v_pref %.1f: closest approach %.4f, farthest from its goal %.3g" % (v_pref, closest, miss))
    assert closest >= CLOSE
    assert miss < 0.05


def test_circle_crossing_keeps_its_distance():
    ang = np.arange(8) * (2 * math.pi / 8)
    starts = np.stack([6.0 + 4.0 * np.cos(ang), 6.0 + 4.0 * np.sin(ang)], axis=1)
    goals = np.stack([6.0 - 4.0 * np.cos(ang), 6.0 - 4.0 * np.sin(ang)], axis=1)
    cfg, r = _scene(starts, goals, 0.6, ang + math.pi)
    closest = _roll(cfg, r, spec.params(cfg, ped_radius=0.3), 200)
    print("circle of 8: closest approach %.4f" % closest)
    assert closest >= CLOSE                                          # (arriving is not required: the symmetric case stalls, as in rvo2)


def _random_world():
    import torch
    E, size, N = 24, 240, 8
    cfg = ref.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=2, ped_model=abi.PED_EXTERNAL,
                             auto_reset=abi.AUTORESET_SAME_STEP, n_spawn=8, seed=4343, time_step=0.2)
    world.lidar_1081(cfg)
    occ = world.make_maps(E, size, 4343)
    a = world.make_world(cfg, occ, n_peds=6, device="cpu", field=torch.from_numpy(ref.build_dt(occ)), min_goal_dist=1.5,
                         max_goal_dist=4.0, v_pref_range=(0.3, 0.6))
    host = {k: v.numpy() for k, v in a.items()}
    host["scan_threshold"], host["scan_discomfort"] = keti_thresholds(cfg)
    return cfg, host


def _random_rollout(cfg, host, alone):
    r = ref.RefSim(cfg, {k: v.copy() for k, v in host.items()})
    r.reset_obs()
    p = spec.params(cfg, ped_radius=0.3)                             # discs of 0.3 m: CLOSE is their margin
    rng = np.random.default_rng(5)
    E = cfg.n_envs
    live = bound = close = 0
    iu = np.triu_indices(6, 1)
    for _ in range(80):
        cmd, head, binds = spec.ped_orca(cfg, r.a, p, alone=alone)
        r.a["ped_wp_head"][...] = head
        r.set_ped_cmd(cmd)
        live += int(r.a["n_peds"].sum()); bound += int(binds.sum())
        r.step(np.stack([rng.uniform(0.0, 0.5, E), rng.uniform(-0.64, 0.64, E)], axis=1))
        xy = r.a["ped_pose"][:, :6, :2]
        d = np.sqrt(((xy[:, :, None] - xy[:, None]) ** 2).sum(-1))
        close += int((d[:, iu[0], iu[1]] < CLOSE).sum())
    return live, bound, close


def test_random_world_constraints_bind_and_separate():
    cfg, host = _random_world()
    live, bound, close = _random_rollout(cfg, host, alone=False)
    _, bound_alone, close_alone = _random_rollout(cfg, host, alone=True)
    print("random world: constraints bind in %d of %d queries; pair-steps closer than %.4f: %d with ORCA, %d with every "
          "pedestrian alone" % (bound, live, CLOSE, close, close_alone))
    assert live == 24 * 6 * 80 and bound_alone == 0
    assert 4 * bound >= live
    assert close_alone > 0 and 10 * close <= close_alone             # relative: spawns may overlap, the robot does not reciprocate
