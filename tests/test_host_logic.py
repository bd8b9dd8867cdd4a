"""CPU: host-side logic -- C ABI surface, struct layouts, registry / env wrapper, world generation,
sharding (world_size 2 over gloo).  No GPU compute."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref
from nav_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """include/navsim.h <-> libnavsim_hip.so <-> abi.EXPORTS agree (the .so loads without a GPU)."""
    from nav_gym_amd import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "navsim.h")).read()
    declared = set(re.findall(r"\b(navsim_[a-z0-9_]+)\s*\(", header))
    declared -= {"navsim_config", "navsim_state", "navsim_step_io"}
    assert declared == set(abi.EXPORTS), (declared ^ set(abi.EXPORTS))
    for name in abi.EXPORTS:
        assert hasattr(L, name), name
    assert L.navsim_abi_version() == abi.ABI_VERSION
    assert L.navsim_sizeof_config() == C.sizeof(abi.NavsimConfig)
    assert L.navsim_sizeof_state() == C.sizeof(abi.NavsimState)
    assert L.navsim_sizeof_step_io() == C.sizeof(abi.NavsimStepIO)
    assert L.navsim_error_string(-1) == b"invalid argument"
    assert L.navsim_step_kernel_name() == b"navsim_step_kernel"


def test_default_config_matches_oracle_and_reference():
    from nav_gym_amd import lib
    a, b = lib.default_config(), ref.default_config()
    assert bytes(a) == bytes(b)                       # HIP library and oracle agree field by field
    assert (a.n_beams, a.time_step, a.range_max, a.axle_offset) == (512, 0.2, 25.0, 0.14474)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before any launch (error codes, never exceptions across the ABI)."""
    from nav_gym_amd import lib
    L = lib.load()
    cfg = lib.default_config()
    st, io = abi.NavsimState(), abi.NavsimStepIO()
    assert L.navsim_step(C.byref(cfg), C.byref(st), C.byref(io), None) == abi.E_ARG
    assert L.navsim_step(None, None, None, None) == abi.E_ARG
    cfg.max_peds = 1000
    assert L.navsim_reset_obs(C.byref(cfg), C.byref(st), C.byref(io), None, None) == abi.E_UNSUPPORTED
    assert L.navsim_field_bytes(2, 500, 500, abi.FIELD_U16T) == 2 * 63 * 63 * 64 * 2
    assert L.navsim_field_bytes(2, 500, 500, abi.FIELD_F32) == 2 * 500 * 500 * 4
    assert L.navsim_build_dt_workspace_bytes(3, 10, 20) == 3 * 10 * 20 * 2


def test_graft_entry_library_check():
    """__graft_entry__.build()'s post-build check (ABI version and export list) passes on the in-tree library."""
    import __graft_entry__ as entry
    entry.check_library()


def test_argument_validation_of_round2_entry_points():
    """navsim_build_rects, the CrowdSim entry points and the new config fields reject bad arguments with error
    codes before any launch (checked here without a GPU)."""
    from nav_gym_amd import lib
    L = lib.load()
    assert L.navsim_rect_table_bytes(2, 500, 500) == 2 * 63 * 63 * 16
    assert L.navsim_build_rects(None, 1, 8, 8, None, abi.FIELD_U16T, None, None, None, 0, None) == abi.E_ARG
    one = C.c_char_p(b"x" * 64)
    assert L.navsim_build_rects(one, 1, 2000, 2000, one, abi.FIELD_U16T, None, one, one, 1 << 30, None) == abi.E_UNSUPPORTED
    mp = abi.NavsimCrowdMapParams(angular_min=-3.14, angular_max=3.14, angular_max_range=6.0, angular_dim=0, normalize=1,
                                  map_size_m=14.0, map_resolution=0.1, submap_size_m=6.0)
    assert L.navsim_crowd_angular_map(C.byref(mp), 1, 0, 4, one, None, None, one, None) == abi.E_ARG      # angular_dim 0
    mp.angular_dim = 72
    assert L.navsim_crowd_angular_map(C.byref(mp), 1, 1, 99, one, one, None, one, None) == abi.E_ARG      # too many vertices
    mp.submap_size_m = 1000.0
    assert L.navsim_crowd_local_map(C.byref(mp), 1, 140, one, one, 1, one, None) == abi.E_UNSUPPORTED     # window beyond LDS
    op = abi.NavsimOrcaParams(time_step=0.25, neighbor_dist=10, time_horizon=5, time_horizon_obst=5, max_neighbors=10)
    assert L.navsim_crowd_orca(C.byref(op), 1, abi.ORCA_MAX_AGENTS + 1, one, None, one, 0, 4, None, None, None, None, one,
                               None, None) == abi.E_ARG
    assert L.navsim_crowd_orca(C.byref(op), 1, 4, one, None, one, 40, 4, one, None, None, None, one, None, None) == abi.E_ARG
    assert L.navsim_crowd_orca(C.byref(op), 0, 4, one, None, one, 0, 4, None, None, None, None, one, None, None) == 0
    assert L.navsim_crowd_agent_step(None, None, None, 3, 0.25, None) == abi.E_ARG
    # config fields that replaced the environment knobs are validated by navsim_step
    cfg = lib.default_config()
    assert (cfg.march_rule, cfg.step_block, cfg.ped_split) == (abi.MARCH_F32, 0, 0)
    assert (cfg.max_waypoints, cfg.action_kind, cfg.clamp_action) == (64, abi.ACTION_TWIST, 0)
    st, io = abi.NavsimState(), abi.NavsimStepIO()
    for name in ("field", "scan_threshold", "scan_discomfort", "robot_pose", "robot_goal", "prev_action", "prev_pose",
                 "n_hist", "episode", "steps"):
        setattr(st, name, C.cast(one, C.c_void_p))
    for name in ("action", "obs", "reward", "done", "is_success", "is_crash", "distance"):
        setattr(io, name, C.cast(one, C.c_void_p))
    for field, bad in (("step_block", 100), ("ped_split", 3), ("march_rule", 3), ("action_kind", 2)):
        c2 = cfg.copy(); setattr(c2, field, bad)
        assert L.navsim_step(C.byref(c2), C.byref(st), C.byref(io), None) == abi.E_ARG, field
    c2 = cfg.copy(); c2.field_format = abi.FIELD_F32; st.rect_table = C.cast(one, C.c_void_p)
    assert L.navsim_step(C.byref(c2), C.byref(st), C.byref(io), None) == abi.E_UNSUPPORTED       # rect records need the packed field
    c2 = cfg.copy(); c2.n_beams = 20000; c2.ped_model = abi.PED_SFM; c2.max_peds = 64; st.rect_table = None
    assert L.navsim_step(C.byref(c2), C.byref(st), C.byref(io), None) in (abi.E_ARG, abi.E_UNSUPPORTED)   # LDS beyond a CU
    # round 5: navsim_step_install and the pipelined swap / stage refuse what they cannot do, before any launch
    ptr = C.cast(one, C.c_void_p)
    c2 = cfg.copy(); c2.n_envs = 4; c2.regen_cap = 4; c2.auto_reset = 1; c2.n_spawn = 2; c2.regen_min_steps = 0
    assert L.navsim_step_install(C.byref(c2), C.byref(st), C.byref(io), None, ptr, ptr, ptr, None, None) == abi.E_ARG      # no staged state
    assert L.navsim_step_install(C.byref(c2), C.byref(st), C.byref(io), C.byref(st), ptr, ptr, ptr, None, None) == abi.E_ARG   # no rule, no fallback, no done_steps
    c2.regen_min_steps = -1
    assert L.navsim_step(C.byref(c2), C.byref(st), C.byref(io), None) == abi.E_ARG
    c2.regen_min_steps = 8; st.done_steps = ptr; st.spawn_pose = ptr; st.spawn_goal = ptr
    c2.regen_cap = 2                                                       # a cap below n_envs: every arena decides alone
    assert L.navsim_step_install(C.byref(c2), C.byref(st), C.byref(io), C.byref(st), ptr, ptr, ptr, None, None) == abi.E_UNSUPPORTED
    odd = C.c_void_p(ptr.value + 1)                                        # mark[] is consumed in 32-bit words
    assert L.navsim_step_install(C.byref(c2), C.byref(st), C.byref(io), C.byref(st), ptr, odd, ptr, None, None) == abi.E_ARG
    assert L.navsim_regen_swap(C.byref(c2), C.byref(st), C.byref(st), C.byref(io), ptr, ptr, odd, None, None) == abi.E_ARG
    c0 = c2.copy(); c0.n_envs = 0; c0.regen_cap = 1; c0.field_format = abi.FIELD_U16T    # an empty shard: nothing to launch
    assert L.navsim_step_install(C.byref(c0), C.byref(st), C.byref(io), C.byref(st), ptr, ptr, ptr, ptr, None) == 0
    assert L.navsim_step_install_replan(C.byref(c0), C.byref(st), C.byref(io), C.byref(st), ptr, ptr, ptr, ptr, 8, None) == 0
    assert L.navsim_regen_helper(None) == 0
    st.map_slot = ptr; c2.shared_field = 1
    assert L.navsim_step(C.byref(c2), C.byref(st), C.byref(io), None) == abi.E_ARG              # one shared map has no slots


def test_workspace_size_queries():
    """The four workspace queries over a grid of configurations (they run without a device): every size is positive,
    navsim_regen_workspace_bytes never shrinks with regen_cap or n_envs and grows from cap 1 to cap 2 (NavSim's staging
    passes probe the per-arena cost by that difference), navsim_replan_workspace_bytes never shrinks with max_queries,
    and null or invalid arguments give 0."""
    from nav_gym_amd import lib
    L = lib.load()
    caps, envs = (1, 2, 3, 4, 5, 64), (1, 40, 4096)
    for fmt in (abi.FIELD_F32, abi.FIELD_U16T):
        for side in (100, 260, 520, 528, 1000):
            for plan in (0, 1):
                for peds in (0, 6, 64):
                    cfg = lib.default_config(map_h=side, map_w=side, field_format=fmt, regen_plan=plan, max_peds=peds,
                                             n_spawn=8, ped_model=abi.PED_SFM if peds else abi.PED_NONE)
                    regen = {}
                    for E in envs:
                        for cap in caps:
                            cfg.n_envs, cfg.regen_cap = E, cap
                            regen[E, cap] = L.navsim_regen_workspace_bytes(C.byref(cfg))
                            assert regen[E, cap] > 0, (fmt, side, plan, peds, E, cap)
                        assert all(regen[E, a] <= regen[E, b] for a, b in zip(caps, caps[1:])), (fmt, side, plan, peds, E)
                        assert regen[E, 2] - regen[E, 1] >= 1
                        assert L.navsim_ped_policy_workspace_bytes(C.byref(cfg)) > 0
                        replan = [L.navsim_replan_workspace_bytes(C.byref(cfg), q) for q in (0, 1, 5, 64, 4096)]
                        assert replan[0] > 0 and all(a <= b for a, b in zip(replan, replan[1:])), (E, replan)
                    for cap in caps:
                        assert all(regen[a, cap] <= regen[b, cap] for a, b in zip(envs, envs[1:])), (fmt, side, plan, peds, cap)
            for m in (1, 3, 64):
                assert L.navsim_build_rects_workspace_bytes(m, side, side) > 0
    cfg = lib.default_config()
    assert L.navsim_regen_workspace_bytes(None) == 0 and L.navsim_ped_policy_workspace_bytes(None) == 0
    assert L.navsim_replan_workspace_bytes(None, 4) == 0 and L.navsim_replan_workspace_bytes(C.byref(cfg), -1) == 0
    cfg.regen_cap = 0
    assert L.navsim_regen_workspace_bytes(C.byref(cfg)) == 0
    for bad in ((0, 100, 100), (3, 0, 100), (3, 100, -1)):
        assert L.navsim_build_rects_workspace_bytes(*bad) == 0


def test_registry_and_env_surface(golden_dir):
    import nav_gym_env
    from nav_gym_amd import registry
    u = np.load(os.path.join(golden_dir, "golden_units.npz"))
    spec = registry.spec("NavGym-v0")
    kw = spec["kwargs"]
    # the registered kwargs equal the reference's (captured by make_golden.py)
    ref_kw = dict(zip(u["kwargs_keys"].tolist(), u["kwargs_vals"].tolist()))
    assert set(ref_kw) | {"env_param_range"} == set(kw)
    for k, v in ref_kw.items():
        assert str(kw[k]) == v, k
    ref_ep = dict(zip(u["env_param_keys"].tolist(), u["env_param_vals"].tolist()))
    assert {k: str(v) for k, v in kw["env_param_range"].items()} == ref_ep
    env = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert env.observation_space.spaces["observation"].shape == (512 + 7,)
    assert env.action_space.low.tolist() == [0.0, pytest.approx(-0.64)] and env.action_space.high.tolist() == [0.5, pytest.approx(0.64)]
    assert env.cfg.n_beams == 512 and env.cfg.angle_min == -3.141592
    for m in ("reset", "step", "compute_reward", "compute_rewards", "compute_terminals", "compute_done",
              "compute_info", "_override_reward_factor", "render"):
        assert callable(getattr(env, m))
    env._override_reward_factor(reward_scale=3.0)
    assert env.cfg.reward_scale == 3.0
    with pytest.raises(NotImplementedError):
        nav_gym_env.make("NavGym-v0", robot_type="turtlebot")
    import torch
    if not torch.cuda.is_available():                 # the product path has no CPU fallback
        from nav_gym_amd.lib import NavsimError
        with pytest.raises(NavsimError):
            env.reset()


def test_env_pickles_like_an_ezpickle_and_looks_like_a_gym_env():
    """env.py:30, 56-78: the reference is `gym.Env, utils.EzPickle` -- a pickle of it carries the constructor's arguments
    and unpickling builds a fresh environment from them (rlkit-style snapshots pickle the env).  Same here, including
    the build's own keyword arguments; and what wrappers read of a gym.Env is there whether or not gym is installed."""
    import copy
    import pickle
    import nav_gym_env
    env = nav_gym_env.make("NavGym-v0", num_envs=5, n_beams=1081, map_size=300, num_humans=3, seed=11, reward_scale=7.0,
                           num_scan_stack=2, plan_paths=False, action_kind="wheels", robot_type="husky")
    for other in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert type(other) is type(env) and other is not env and other.sim is None
        assert other._ctor_kwargs == env._ctor_kwargs
        assert bytes(other.cfg) == bytes(env.cfg)                  # the whole navsim_config, derived from the same arguments
        assert other.observation_space.spaces["observation"].shape == (2 * 1081 + 7,)
        assert np.array_equal(other.action_space.low, env.action_space.low)
    assert env.unwrapped is env and env.reward_range[0] == -float("inf") and env.reward_range[1] == float("inf")
    assert hasattr(env, "spec") and hasattr(env, "metadata") and callable(env.seed) and callable(env.close)
    from nav_gym_amd import registry
    if registry.HAVE_GYM:
        import gym
        assert isinstance(env, gym.Env)


def test_env_fallbacks_are_announced_once():
    """Round-4 verdict: plan_paths silently fell back to False above 1000 cells per side and field_format to FIELD_F32
    above 1024.  Both are RuntimeWarnings now, once per process."""
    import warnings
    import nav_gym_env
    from nav_gym_amd import abi
    from nav_gym_amd.env import NavGymEnv
    NavGymEnv._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        env = nav_gym_env.make("NavGym-v0", num_envs=2, map_size=1100)
        assert env.plan_paths is False and env.cfg.field_format == abi.FIELD_F32
        texts = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
        assert any("plan_paths" in t for t in texts) and any("field_format" in t for t in texts), texts
        n = len(texts)
        nav_gym_env.make("NavGym-v0", num_envs=2, map_size=1100)                 # the second time: silent
        assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == n
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        nav_gym_env.make("NavGym-v0", num_envs=2, map_size=500)                  # nothing falls back: nothing is said
        nav_gym_env.make("NavGym-v0", num_envs=2, map_size=1100, plan_paths=False, field_format=abi.FIELD_F32)
        assert not [x for x in w if issubclass(x.category, RuntimeWarning)]


def test_env_refuses_a_lidar_wider_than_one_turn_with_pedestrians():
    """include/navsim.h angle_last: the step returns NAVSIM_E_UNSUPPORTED for angle_last - angle_min > 2 pi in a world with
    pedestrians, so the constructor says so.  Exactly 2 pi, a reversed lidar, and any width without pedestrians are taken."""
    import nav_gym_env
    from nav_gym_amd import abi
    mk = lambda **kw: nav_gym_env.make("NavGym-v0", num_envs=2, map_size=200, **kw)
    for lidar in ((-3.5, 3.5, 90), (-3.2, 6.2, 90), (0.0, float(np.nextafter(2 * np.pi, 7.0)), 8)):
        for model in ("sfm", "external", "orca"):
            with pytest.raises(ValueError, match="2\\*pi"):
                mk(lidar=lidar, pedestrian_model=model)
        for kw in (dict(pedestrian_model="none"), dict(num_humans=0)):
            env = mk(lidar=lidar, **kw)
            assert env.cfg.ped_model == abi.PED_NONE and (env.cfg.angle_min, env.cfg.angle_last, env.cfg.n_beams) == lidar
    for lidar in ((-np.pi, np.pi, 90), (0.0, 2 * np.pi, 8), (1.0, -1.0, 33), (-0.75 * np.pi, 0.75 * np.pi, 1081)):
        env = mk(lidar=lidar)
        assert env.cfg.ped_model == abi.PED_SFM and (env.cfg.angle_min, env.cfg.angle_last) == lidar[:2]


def test_env_picks_the_pipelined_reset_path_where_it_pays():
    """NavGymEnv(pregen_pipeline=None), worlds with a new map per episode: 8 where the reset is heavy -- corridor maps with planned
    starts, the reference's own kind --, 4 otherwise, 0 where the pipeline is not available; an explicit value wins.  With
    regen_min_steps = 0 (default) the pipeline changes no result, so the choice is one of speed only."""
    import pickle
    import nav_gym_env
    from nav_gym_amd import abi
    mk = lambda **kw: nav_gym_env.make("NavGym-v0", **kw)
    e = mk(num_envs=8, map_size="reference", randomize_maps=True)
    assert e.pregen_pipeline == 4 and e.regen_min_steps == 0 and e.cfg.regen_min_steps == 0
    assert e.cfg.regen_cap == 8 and e.cfg.defer_reset_scan == 0 and e.use_graphs is False       # every arena decides alone
    assert pickle.loads(pickle.dumps(e)).pregen_pipeline == 4
    assert mk(num_envs=8, map_size="reference", randomize_maps=True, pregen_pipeline=0).pregen_pipeline == 0
    g = mk(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0, use_graphs=True)       # graph replay asked for: the other form
    assert g.pregen_pipeline == 0 and g.use_graphs is True
    assert mk(num_envs=8, map_size="reference", randomize_maps=True, pregen_pipeline=2, regen_min_steps=8).cfg.regen_min_steps == 8
    assert mk(num_envs=8, map_size="reference").pregen_pipeline == 0                              # maps stay: nothing to stage
    assert mk(num_envs=1, map_size="reference", randomize_maps=True).pregen_pipeline == 0         # one arena: reset() is the user's
    assert mk(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0).pregen_pipeline == 4   # outdoor maps: a lighter reset
    assert mk(num_envs=8, map_size=500, randomize_maps=True, plan_paths=False).pregen_pipeline == 4
    assert mk(num_envs=8, map_size=1100, randomize_maps=True).pregen_pipeline == 0                # float32 field: no pipeline
    assert mk(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0, pregen_pipeline=2).pregen_pipeline == 2


def test_env_reset_path_chosen_after_the_fact_equals_the_explicit_one():
    """NavGymEnv._choose_reset_path(0) -- what reset() calls when the staged copy of the world does not fit -- leaves the
    environment as pregen_pipeline=0 makes it, except for cfg.regen_cap: the fallback takes min(num_envs, 64), the constructor
    leaves the library's 64.  The expected tuples (pregen_pipeline, cfg.defer_reset_scan, cfg.regen_cap, use_graphs) of the
    explicit form were recorded from the constructor before the choice had a method of its own."""
    import nav_gym_env
    grid = [(dict(num_envs=8, map_size="reference", randomize_maps=True), (0, 1, 64, False)),
            (dict(num_envs=8, map_size="reference", randomize_maps=True, pregen_pipeline=0), (0, 1, 64, False)),
            (dict(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0, use_graphs=True), (0, 1, 64, True)),
            (dict(num_envs=8, map_size="reference", randomize_maps=True, pregen_pipeline=2, regen_min_steps=8), (0, 1, 64, False)),
            (dict(num_envs=8, map_size="reference"), (0, 0, 64, False)),
            (dict(num_envs=1, map_size="reference", randomize_maps=True), (0, 0, 64, False)),
            (dict(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0), (0, 1, 64, True)),
            (dict(num_envs=8, map_size=500, randomize_maps=True, plan_paths=False), (0, 1, 64, True)),
            (dict(num_envs=8, map_size=1100, randomize_maps=True), (0, 1, 64, True)),
            (dict(num_envs=8, map_size=500, randomize_maps=True, indoor_ratio=0.0, pregen_pipeline=2), (0, 1, 64, True))]
    for kw, want in grid:
        a = nav_gym_env.make("NavGym-v0", **kw)
        a._choose_reset_path(0)
        b = nav_gym_env.make("NavGym-v0", **dict(kw, pregen_pipeline=0))
        assert (b.pregen_pipeline, b.cfg.defer_reset_scan, b.cfg.regen_cap, b.use_graphs) == want, kw
        assert (a.pregen_pipeline, a.cfg.defer_reset_scan, a.use_graphs) == (want[0], want[1], want[3]), kw
        assert a.cfg.regen_cap == min(kw["num_envs"], 64), kw          # THE difference between the two
        a.cfg.regen_cap = b.cfg.regen_cap
        assert bytes(a.cfg) == bytes(b.cfg), kw


def test_host_classes_declare_their_state():
    """NavSim and NavGymEnv assign their attributes in __init__: no method asks getattr(self, "name", ...) or
    hasattr(self, "name") for one that may not exist yet (a computed name, getattr(self, "reward_" + k), is another thing)."""
    import ast
    import nav_gym_amd
    for name in ("sim.py", "env.py"):
        tree = ast.parse(open(os.path.join(os.path.dirname(nav_gym_amd.__file__), name)).read())
        bad = [n.lineno for n in ast.walk(tree)
               if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ("getattr", "hasattr")
               and len(n.args) >= 2 and isinstance(n.args[0], ast.Name) and n.args[0].id == "self"
               and isinstance(n.args[1], ast.Constant) and isinstance(n.args[1].value, str)]
        assert not bad, "%s: getattr / hasattr of self with a literal name at lines %s" % (name, bad)
        if name == "sim.py":                              # ... and the reset path's plan is declared with the rest, as None
            init = [f for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "NavSim"
                    for f in c.body if isinstance(f, ast.FunctionDef) and f.name == "__init__"][0]
            declared = [n for n in ast.walk(init) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant)
                        and n.value.value is None and any(isinstance(t, ast.Attribute) and t.attr == "pg_plan" and
                                                          isinstance(t.value, ast.Name) and t.value.id == "self" for t in n.targets)]
            assert len(declared) == 1


def _plan_cfg(E=512, mode=abi.AUTORESET_SAME_STEP, regen_cap=None, regen_min_steps=0, regen_plan=0, regen_indoor_ratio=0.0):
    """The six fields sim.pregen_plan reads, in a navsim_config made without the library."""
    cfg = abi.NavsimConfig()
    cfg.n_envs, cfg.auto_reset, cfg.regen_cap, cfg.regen_min_steps = E, mode, E if regen_cap is None else regen_cap, regen_min_steps
    cfg.regen_plan, cfg.regen_indoor_ratio = regen_plan, regen_indoor_ratio
    return cfg


def _plan(cfg, costmap=False, **kw):
    from nav_gym_amd import sim
    return sim.pregen_plan(cfg, cfg.auto_reset == abi.AUTORESET_NEXT_STEP, costmap, **kw)


# The reset path's mode, row by row: (configuration, costmap, enable_pregen's keywords) -> the whole record, written out by hand
# from the code of NavSim.enable_pregen before pregen_plan existed.  Rows a, b, c, d, f, g and the override rows' base cases were
# then held against what that enable_pregen left on the device (profiles/r21_pregen_plan/: worlds t_abc, t_d, t_fg); row e
# (4096 arenas) rests on reading its arithmetic: 2 P max(8, E // 64) = 512 and max(8, E // 128) = 32.
_NEXT, _REFDEF = dict(mode=abi.AUTORESET_NEXT_STEP), dict(regen_plan=1, regen_indoor_ratio=0.5)
_INSTALL = dict(pipeline=4, install=True)
_A = dict(period=4, install=True, shared_maps=True, fallback=True, heavy=False, helper=False, lanes=1, stage_cap=64, side_priority=0,
          lone=False, beside=False, poll=False, late_cap=8, late_defer_scan=False)
_D = dict(_A, heavy=True, helper=True, lanes=2, stage_cap=128, poll=True)
_F = dict(period=3, install=False, shared_maps=False, fallback=False, heavy=False, helper=False, lanes=1, stage_cap=48, side_priority=0,
          lone=False, beside=False, poll=False, late_cap=0, late_defer_scan=False)
PLAN_ROWS = {
    "a": (dict(), False, _INSTALL, _A),
    "b": (_NEXT, False, _INSTALL, dict(_A, lone=True)),
    "c": (_NEXT, False, dict(_INSTALL, late_beside=True), dict(_A, beside=True, late_defer_scan=True)),
    "d": (dict(_REFDEF, E=1024), True, _INSTALL, _D),
    "e": (dict(_REFDEF, E=4096), True, _INSTALL, dict(_D, stage_cap=512, late_cap=32)),
    "f": (dict(E=48, regen_cap=8, regen_min_steps=12), False, dict(pipeline=3), _F),
    "g": (dict(E=48, regen_cap=8), False, dict(), dict(_F, period=0, stage_cap=8, side_priority=-1)),
    "g, a cap above n_envs": (dict(E=6, regen_cap=64), False, dict(), dict(_F, period=0, stage_cap=64, side_priority=-1)),
    # explicit arguments against the defaults
    "d, fallback_poll=False": (dict(_REFDEF, E=1024), True, dict(_INSTALL, fallback_poll=False), dict(_D, poll=False)),
    "a, fallback_poll=True": (dict(), False, dict(_INSTALL, fallback_poll=True), dict(_A, poll=True)),
    "b, fallback_poll=True": (_NEXT, False, dict(_INSTALL, fallback_poll=True), dict(_A, lone=True)),        # next-step: never polled
    "d, stage_lanes=1": (dict(_REFDEF, E=1024), True, dict(_INSTALL, stage_lanes=1), dict(_D, lanes=1)),
    "a, stage_lanes=2": (dict(), False, dict(_INSTALL, stage_lanes=2), dict(_A, lanes=2)),
    "a, stage_cap=3": (dict(), False, dict(_INSTALL, stage_cap=3), dict(_A, stage_cap=3)),
    "f, stage_cap=3": (dict(E=48, regen_cap=8, regen_min_steps=12), False, dict(pipeline=3, stage_cap=3), dict(_F, stage_cap=3)),
    "a, stage_cap above n_envs": (dict(), False, dict(_INSTALL, stage_cap=4000), dict(_A, stage_cap=512)),
    "a, fallback_cap=4": (dict(), False, dict(_INSTALL, fallback_cap=4), dict(_A, late_cap=4)),
    "a, fallback_cap above n_envs": (dict(E=6), False, dict(_INSTALL, fallback_cap=40), dict(_A, stage_cap=6, late_cap=6)),
    "a, map_slots=False": (dict(), False, dict(_INSTALL, map_slots=False), dict(_A, shared_maps=False)),
    "a under the rule": (dict(regen_min_steps=16), False, _INSTALL, dict(_A, fallback=False, late_cap=0)),
    "a under the rule, fallback=True": (dict(regen_min_steps=16), False, dict(_INSTALL, fallback=True), _A),
    "b under the rule": (dict(_NEXT, regen_min_steps=16), False, _INSTALL, dict(_A, fallback=False, late_cap=0)),
    "c under the rule": (dict(_NEXT, regen_min_steps=16), False, dict(_INSTALL, late_beside=True), dict(_A, fallback=False, late_cap=0)),
    "c, same-step": (dict(), False, dict(_INSTALL, late_beside=True), _A),
    # next-step, what keeps an arena from regenerating itself: a costmap, planned starts, corridor maps
    "b with a costmap": (_NEXT, True, _INSTALL, _A),
    "b with planned starts": (dict(_NEXT, regen_plan=1), True, _INSTALL, dict(_A, heavy=True, lanes=2)),
    "b with corridor maps": (dict(_NEXT, regen_indoor_ratio=0.5), False, _INSTALL, dict(_A, heavy=True, lanes=2)),
    "d, next-step": (dict(_REFDEF, E=1024, **_NEXT), True, _INSTALL, dict(_D, poll=False)),
    # 1280 arenas: both caps beyond their floor of 8; one period: a pass of 2 x 8 arenas
    "a, 1280 arenas": (dict(E=1280), False, _INSTALL, dict(_A, stage_cap=160, late_cap=10)),
    "a, pipeline=1": (dict(E=6), False, dict(pipeline=1, install=True), dict(_A, period=1, stage_cap=6, late_cap=6)),
    # AS IT IS, known and not right: `lone` does not look at regen_min_steps -- with 0 < regen_min_steps < 4 P the
    # library runs rule-only.  The fix turns this row's lone into False.
    "b, 0 < regen_min_steps < 4 P": (dict(_NEXT, regen_min_steps=8), False, _INSTALL, dict(_A, lone=True)),
}


@pytest.mark.parametrize("row", sorted(PLAN_ROWS))
def test_pregen_plan_rows(row):
    from nav_gym_amd import sim
    cfg_kw, costmap, call, want = PLAN_ROWS[row]
    plan = _plan(_plan_cfg(**cfg_kw), costmap, **call)
    assert plan == sim.PregenPlan(**want) and [type(v) for v in plan] == [type(want[k]) for k in plan._fields], plan


_RULE = ("enable_pregen(pipeline=%d) needs cfg.regen_min_steps >= %d (it is %d): an arena must not want its next world before the "
         "pass that stages it was waited for -- or fallback=True (install=True)")
_REFUSALS = {
    "auto_reset": "enable_pregen needs cfg.auto_reset = 1 (the step advances episode[e] when an arena finishes)",
    "fallback": "enable_pregen(fallback=True) is a feature of install=True",
    "install": "enable_pregen(install=True) needs pipeline >= 1 and cfg.regen_cap >= n_envs (every finished arena decides alone "
               "inside the step: there is no cap in index order)",
    "lanes": "enable_pregen(stage_lanes=%r): 1, or 2 with install=True and pipeline > 0"}


@pytest.mark.parametrize("cfg_kw,call,text", [
    (dict(mode=abi.AUTORESET_NONE), dict(), _REFUSALS["auto_reset"]),
    (dict(mode=abi.AUTORESET_NONE), dict(fallback=True, pipeline=-1, stage_lanes=3), _REFUSALS["auto_reset"]),         # the first wins
    (dict(), dict(fallback=True), _REFUSALS["fallback"]),
    (dict(), dict(fallback=True, pipeline=4), _REFUSALS["fallback"]),
    (dict(), dict(fallback=True, pipeline=-1, stage_lanes=3), _REFUSALS["fallback"]),
    (dict(), dict(pipeline=-1), _RULE % (-1, -4, 0)),
    (dict(regen_min_steps=7), dict(pipeline=-2, install=True, fallback=True), _RULE % (-2, -8, 7)),
    (dict(), dict(pipeline=4), _RULE % (4, 16, 0)),
    (dict(regen_min_steps=15), dict(pipeline=4.9), _RULE % (4, 16, 15)),
    (dict(regen_cap=8), dict(pipeline=4, install=True, fallback=False, stage_lanes=3), _RULE % (4, 16, 0)),
    (dict(), dict(install=True), _REFUSALS["install"]),
    (dict(), dict(install=True, fallback=True, stage_lanes=2), _REFUSALS["install"]),
    (dict(regen_cap=511), dict(pipeline=4, install=True), _REFUSALS["install"]),
    (dict(regen_cap=511, regen_min_steps=16), dict(pipeline=4, install=True, stage_lanes=3), _REFUSALS["install"]),
    (dict(), dict(pipeline=4, install=True, stage_lanes=3), _REFUSALS["lanes"] % 3),
    (dict(), dict(pipeline=4, install=True, stage_lanes=-1), _REFUSALS["lanes"] % -1),
    (dict(), dict(stage_lanes=2), _REFUSALS["lanes"] % 2),
    (dict(regen_min_steps=16), dict(pipeline=4, stage_lanes=2), _REFUSALS["lanes"] % 2)])
def test_pregen_plan_refusals(cfg_kw, call, text):
    """The five refusals of enable_pregen, word for word as before pregen_plan existed; of two that hold at once the earlier."""
    with pytest.raises(ValueError) as e:
        _plan(_plan_cfg(**cfg_kw), **call)
    assert str(e.value) == text


def test_pregen_plan_invariants_over_the_grid():
    """Every keyword argument at every boolean / None choice, 6 / 600 / 1280 arenas, pipeline 0 / 1 / 4, both restart modes
    (15 552 points); the configuration's other fields drawn per point.  A point is refused or its plan holds together."""
    import itertools
    import random
    rng = random.Random(0)
    n_plans = 0
    for E, P, nxt, install, slots, beside, scap, fb, fcap, poll, lanes in itertools.product(
            (6, 600, 1280), (0, 1, 4), (False, True), (False, True), (False, True), (False, True), (None, 3), (None, False, True),
            (None, 4), (None, False, True), (None, 1, 2)):
        costmap, plan_, indoor = rng.random() < 0.5, rng.randrange(2), rng.choice((0.0, 0.5))
        cfg = _plan_cfg(E, abi.AUTORESET_NEXT_STEP if nxt else abi.AUTORESET_SAME_STEP, rng.choice((E, E, 8, 64)),
                        rng.choice((0, 4 * P)), plan_, indoor)
        try:
            p = _plan(cfg, costmap, pipeline=P, install=install, stage_cap=scap, map_slots=slots, fallback=fb, fallback_cap=fcap,
                      late_beside=beside, fallback_poll=poll, stage_lanes=lanes)
        except ValueError:
            continue
        n_plans += 1
        heavy = bool(plan_) or indoor > 0
        assert p.heavy == heavy and p.period == P and p.install == install
        assert not p.lone or (p.fallback and nxt and not heavy and not costmap)
        assert not p.beside or (p.fallback and nxt)
        assert not (p.lone and p.beside)
        assert not p.poll or (p.fallback and not nxt)
        assert p.lanes in (1, 2) and (p.lanes == 1 or (install and P > 0))
        assert 1 <= p.stage_cap <= max(E, cfg.regen_cap)
        assert p.late_cap <= E and (p.late_cap > 0) == p.fallback
        assert not p.fallback or install
        assert p.late_defer_scan == p.beside and p.shared_maps == (install and slots) and p.helper == (bool(plan_) and indoor > 0)
    assert n_plans > 3000, n_plans


def test_world_generation_is_shard_invariant():
    import torch
    from nav_gym_amd import lib, world
    cfg = lib.default_config(n_envs=6, map_h=120, map_w=120, max_peds=4, n_spawn=4, ped_model=abi.PED_SFM, seed=9)
    occ = world.make_maps(6, 120, 9)
    assert occ.shape == (6, 120, 120) and set(np.unique(occ)) == {0, 1}
    assert (occ[:, :5] == 1).all() and (occ[:, :, -5:] == 1).all()          # 5-cell border wall
    field = torch.from_numpy(ref.build_dt(occ))
    a = world.make_world(cfg, occ, n_peds=3, device="cpu", field=field, min_goal_dist=2, max_goal_dist=5, robot_clearance=0.6)
    cells = (a["spawn_pose"][:, :, :2] / 0.05).long()
    for e in range(6):                                 # spawns sit on free cells with clearance
        assert (field[e][cells[e, :, 1], cells[e, :, 0]] >= 0.6 / 0.05).all()
    cfg2 = cfg.copy(); cfg2.n_envs = 2; cfg2.env_index_base = 4
    occ2 = world.make_maps(2, 120, 9, env_index_base=4)
    assert np.array_equal(occ2, occ[4:])
    b = world.make_world(cfg2, occ2, n_peds=3, device="cpu", field=field[4:], min_goal_dist=2, max_goal_dist=5, robot_clearance=0.6)
    for k in b:
        if k != "n_peds":
            assert torch.equal(b[k], a[k][4:]), k
    ind = world.indoor_map(np.random.default_rng(1), 200, 3, 100)
    assert ind.shape == (200, 200) and 0.05 < (ind == 0).mean() < 0.9


def test_shard_range():
    from nav_gym_amd.sharding import shard_range
    for n, w in ((4096, 8), (16384, 8), (10, 3), (5, 8)):
        spans = [shard_range(n, r, w) for r in range(w)]
        assert sum(c for _, c in spans) == n
        assert all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(w - 1))


_WORKER = r"""
import os, sys
sys.path[:0] = [%(root)r + "/nav-gym_amd", %(root)r + "/oracle", %(root)r + "/tests"]
import numpy as np, torch, torch.distributed as dist
import ref
from helpers import keti_thresholds
from nav_gym_amd import abi, lib, world
from nav_gym_amd.sharding import shard_range, gather_rows
rank, ws = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=ws)
E_total, size = 5, 100            # ragged: 3 + 2 arenas
def run(start, count):
    cfg = lib.default_config(n_envs=count, map_h=size, map_w=size, max_peds=3, n_spawn=4, ped_model=abi.PED_SFM,
                             auto_reset=1, seed=21, env_index_base=start)
    world.lidar_full_circle(cfg, 64)
    occ = world.make_maps(count, size, 21, env_index_base=start)
    f = ref.build_dt(occ)
    a = world.make_world(cfg, occ, n_peds=2, device="cpu", field=torch.from_numpy(f), min_goal_dist=1.5, max_goal_dist=4, robot_clearance=0.6)
    host = {k: v.numpy() for k, v in a.items()}
    host["scan_threshold"], host["scan_discomfort"] = keti_thresholds(cfg)
    sim = ref.RefSim(cfg, host); sim.reset_obs()
    rng = np.random.default_rng(3)
    acts = np.stack([rng.uniform(0, 0.5, (12, E_total)), rng.uniform(-0.6, 0.6, (12, E_total))], axis=2)
    for t in range(12):
        obs, out = sim.step(acts[t, start:start + count])
    return obs.copy(), out["reward"].copy(), out["done"].copy()
start, count = shard_range(E_total, rank, ws)
obs, rew, done = run(start, count)
g_obs = gather_rows(torch.from_numpy(obs)); g_rew = gather_rows(torch.from_numpy(rew)); g_done = gather_rows(torch.from_numpy(done))
if rank == 0:
    f_obs, f_rew, f_done = run(0, E_total)
    assert np.array_equal(g_obs.numpy(), f_obs), "sharded obs differ from the single-shard run"
    assert np.array_equal(g_rew.numpy(), f_rew) and np.array_equal(g_done.numpy(), f_done)
    print("SHARD_OK", g_obs.shape)
dist.barrier(); dist.destroy_process_group()
"""


def test_two_rank_sharding_over_gloo(tmp_path):
    """N > 1 path on CPU: two ranks step their arena blocks (oracle as the stepper), gather rows over
    gloo; the result must equal the single-shard run bit for bit (global-index keyed worlds)."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    port = 29500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "SHARD_OK" in outs[0]


_GATHER8 = r"""
import os, sys
sys.path[:0] = [%(root)r + "/nav-gym_amd"]
import torch, torch.distributed as dist
from nav_gym_amd.sharding import shard_range, RowGather
rank, ws = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=ws)
ok = True
for total, D in ((16384, 3), (4096, 5), (4099, 2)):        # c4's and c5's totals over 8 ranks (2048 / 512 rows each), and a ragged one
    start, count = shard_range(total, rank, ws)
    rows = (torch.arange(start, start + count, dtype=torch.float32)[:, None] * 8.0 + torch.arange(D, dtype=torch.float32)[None, :])
    g = RowGather(total, (D,), torch.float32, "cpu", rank, ws)
    assert g.equal == (total %% ws == 0) and g.count == count
    for rep in range(2):                                   # the resident buffers serve every call
        out = g.run(rows + rep)
        want = torch.arange(total, dtype=torch.float32)[:, None] * 8.0 + torch.arange(D, dtype=torch.float32)[None, :] + rep
        ok = ok and torch.equal(out, want)
if rank == 0:
    print("GATHER8_OK" if ok else "GATHER8_BAD")
dist.barrier(); dist.destroy_process_group()
"""


def test_row_gather_delivers_eight_shards_in_global_arena_order(tmp_path):
    """sharding.RowGather with EIGHT gloo ranks at the shard sizes of BASELINE's 8-GPU configs (c4: 16 384 arenas = 8 x 2048,
    c5: 4 096 = 8 x 512) and a ragged total: what every rank receives is the shards' rows concatenated in rank order =
    global arena order -- the layout tests/test_gpu_autoreset.py::test_eight_shards_equal_one_world_at_the_configured_totals
    compares against one world holding all arenas."""
    script = tmp_path / "gather8.py"
    script.write_text(_GATHER8 % {"root": ROOT})
    port = 31500 + (os.getpid() % 2000)
    procs = []
    for r in range(8):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="8", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "GATHER8_OK" in outs[0], outs[0]


def _bench(args, **env):
    e = dict(os.environ, OMP_NUM_THREADS="1", **env)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=240)


def test_bench_gpus_flag_spawns_ranks():
    """`python bench.py --gpus 2` with no launcher around it spawns two ranks itself (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_*), they rendezvous (gloo here, RCCL on the GPU box), the max over ranks is taken and
    rank 0's line says n_gpus = 2.  --dry-run: control flow only, no GPU work (there is no GPU here)."""
    import json
    r = _bench(["--gpus", "2", "--dry-run", "--steps", "7"], NAVSIM_BENCH_BACKEND="gloo")
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == 2 and out["steps"] == 7 and out["dry_run"] is True
    assert out["max_rank_time"] == 2.0                    # rank 1 reports 2.0, rank 0 1.0: MAX over ranks


def test_bench_launcher_propagates_a_failed_rank():
    r = _bench(["--gpus", "2", "--dry-run"], NAVSIM_BENCH_BACKEND="gloo", NAVSIM_BENCH_FAIL_RANK="1")
    assert r.returncode != 0 and "rank 1 exit 3" in r.stderr


def test_bench_rejects_mismatched_world_size():
    e = dict(os.environ, WORLD_SIZE="2", RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_bench_takes_world_size_from_the_launcher():
    """`torchrun --nproc-per-node 2 bench.py` without --gpus: the launcher's WORLD_SIZE is the rank count."""
    import json
    port = str(29600 + (os.getpid() % 2000))
    procs = []
    for r in range(2):
        e = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                 NAVSIM_BENCH_BACKEND="gloo", OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run"], env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=240) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    out = json.loads([ln for ln in outs[0][0].splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2


def test_bench_strong_scaling_splits_the_configured_totals():
    """--scaling strong shards the workload's TOTAL (c2: 4096, c4: 16384, c5: 4096) by sharding.shard_range; weak
    keeps the per-GPU count.  Two gloo ranks; the gathered rows (one per arena, holding its global index) must arrive
    in global arena order."""
    import json
    for wl, total in (("c2", 4096), ("c4", 16384), ("c5", 4096)):
        r = _bench(["--gpus", "2", "--dry-run", "--scaling", "strong", "--workload", wl], NAVSIM_BENCH_BACKEND="gloo")
        assert r.returncode == 0, r.stderr
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert out["scaling"] == "strong" and out["envs_total"] == total
        assert out["shards"] == [[0, total // 2], [total // 2, total // 2]] and out["gather_in_global_order"] is True
    r = _bench(["--gpus", "2", "--dry-run", "--workload", "c4", "--scaling", "weak"], NAVSIM_BENCH_BACKEND="gloo")
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["scaling"] == "weak" and out["shards"] == [[0, 2048], [2048, 2048]] and out["envs_total"] == 4096


def test_bench_default_with_several_gpus_reports_both_curves():
    """Round-3 verdict: BASELINE.json's metric reads "4096 envs ..., 1/2/4/8 MI355X" -- a FIXED total.  With N > 1 a --full
    invocation therefore measures both curves: `value` (and value_strong) on the strong split of the 4096 arenas, value_weak
    on 4096 arenas PER GPU, each with its own envs_total.  (Dry run: the keys and the shards; values are null.)"""
    import json
    r = _bench(["--gpus", "2", "--dry-run", "--full"], NAVSIM_BENCH_BACKEND="gloo")
    assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["scaling"] == "strong" and out["envs_total"] == 4096 and out["shards"] == [[0, 2048], [2048, 2048]]
    assert "value_strong" in out and "value_weak" in out
    assert out["weak"]["scaling"] == "weak" and out["weak"]["envs_total"] == 8192 and out["weak"]["envs_per_gpu"] == 4096
    assert out["weak"]["shards"] == [[0, 4096], [4096, 4096]]
    # one GPU: the two coincide, the line says "weak" like the contract's example
    r = _bench(["--gpus", "1", "--dry-run"])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["scaling"] == "weak" and out["envs_total"] == 4096 and "value_weak" in out and "weak" not in out


def test_bench_strong_scaling_ragged_split():
    """A total that does not divide: the first total % world ranks own one more arena, every arena is owned exactly
    once, and the padded all_gather of ragged shards still returns the rows in global order."""
    import json
    r = _bench(["--gpus", "3", "--dry-run", "--scaling", "strong", "--total-envs", "4099"], NAVSIM_BENCH_BACKEND="gloo")
    assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["shards"] == [[0, 1367], [1367, 1366], [2733, 1366]] and out["envs_total"] == 4099
    assert out["gather_in_global_order"] is True


def test_bench_without_gpu_fails_loudly():
    """The product path has no CPU fallback: bench.py refuses to run without a MI355X."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    r = _bench(["--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_husky_skid_steer_command():
    """Husky as a skid-steer base (husky.urdf.xacro:61-67: track 0.5708 m, wheel radius 0.1651 m): wheel speeds <->
    the (v, omega) the step integrates; equal speeds drive straight, opposite speeds turn on the spot."""
    from nav_gym_amd import robots
    tw = robots.husky_twist_from_wheels(np.array([3.0, 2.0, -1.0]), np.array([3.0, 4.0, 1.0]))
    assert np.allclose(tw[0], [3.0 * 0.1651, 0.0]) and tw[2, 0] == 0.0 and tw[2, 1] > 0
    assert np.allclose(tw[1], [0.1651 * 3.0, 0.1651 * 2.0 / 0.5708])
    wl, wr = robots.husky_wheels_from_twist(tw[:, 0], tw[:, 1])
    assert np.allclose(wl, [3.0, 2.0, -1.0]) and np.allclose(wr, [3.0, 4.0, 1.0])


def test_export_transform_matches_reference_utils():
    """export._transform restates utils.transform_xys (ros_env.py:100-135 uses it for the three footprint
    polygons); golden: the reference's own output for a translation (3.25, -1.5) and yaw 0.7."""
    from nav_gym_amd import export
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_units.npz"))
    got = export._transform(d["tf_xys_in"], 3.25, -1.5, 0.7)
    assert np.abs(got - d["tf_xys_out"][:, :2]).max() < 1e-12
    q = export._quaternion_from_yaw(0.7)
    assert abs(q[2] - np.sin(0.35)) < 1e-15 and abs(q[3] - np.cos(0.35)) < 1e-15 and q[0] == 0.0 and q[1] == 0.0


class _FakeSim(object):
    def __init__(self, t, obs):
        self.t, self.obs = t, obs


def _fake_env(n_peds=3):
    """An env-shaped namespace over CPU tensors: what export.py / render() read, without a GPU."""
    import types
    import torch
    from nav_gym_amd import lib, robots
    H = 60
    cfg = lib.default_config(n_envs=2, map_h=H, map_w=H, max_peds=4, n_beams=64, ped_model=abi.PED_SFM)
    field = torch.ones((2, H, H), dtype=torch.float32)
    field[:, :3] = 0; field[:, -3:] = 0; field[:, :, :3] = 0; field[:, :, -3:] = 0
    field[1, 20:30, 40:50] = 0
    t = {"field": field,
         "robot_pose": torch.tensor([[1.0, 1.0, 0.0], [1.5, 1.0, 0.7]], dtype=torch.float64),
         "robot_goal": torch.tensor([[2.0, 2.0], [2.5, 0.5]], dtype=torch.float64),
         "n_peds": torch.tensor([0, n_peds], dtype=torch.int32),
         "ped_pose": torch.rand((2, 4, 3), dtype=torch.float64) * 2 + 0.3,
         "ped_vel": torch.rand((2, 4, 2), dtype=torch.float64),
         "ped_waypoints": torch.rand((2, 4, cfg.max_waypoints, 2), dtype=torch.float64) * 2 + 0.3}
    obs = torch.full((2, 64 + 7), 25.0, dtype=torch.float32)
    obs[1, :32] = 0.8                                       # half of the beams return at 0.8 m
    obs[1, -1] = 0.7
    env = types.SimpleNamespace(cfg=cfg, sim=_FakeSim(t, obs), robot_type="keti", map_size=H)
    return env


def test_export_fields_follow_ros_env():
    """export.reset_map_fields / strict_update_fields against the field list of the reference's RosEnv
    (ros_env.py:65-185; nav_gym/srv/ResetMap.srv:1-6, StrictUpdate.srv:1-9): the same request fields, the same
    attributes filled, the reference's width <- height swap (ros_env.py:72-73), the latest scan of the stack."""
    from nav_gym_amd import export, robots
    env = _fake_env()
    m = export.reset_map_fields(env, arena=1)
    assert set(m) == {"data", "resolution", "width", "height", "origin_position", "origin_orientation"}
    assert m["data"].dtype == np.int8 and set(np.unique(m["data"])) == {0, 100} and m["data"][25, 45] == 100
    assert m["origin_orientation"] == (0.0, 0.0, 0.0, 1.0) and m["resolution"] == 0.05
    u = export.strict_update_fields(env, arena=1)
    assert set(u) == {"humans", "pose", "footprint", "threshold_footprint", "discomfort_threshold_footprint", "scan"}
    assert set(u["pose"]) == {"frame_id", "position", "orientation"} and u["pose"]["frame_id"] == "map"   # ros_env.py:94-103
    assert set(u["scan"]) == {"frame_id", "angle_min", "angle_max", "angle_increment", "range_max", "ranges"}  # :139-151
    assert u["scan"]["frame_id"] == "laser_link" and len(u["scan"]["ranges"]) == 64
    assert len(u["humans"]) == 3 and set(u["humans"][0]) == {"track_id", "detection_id", "position", "orientation", "linear"}
    for key in ("footprint", "threshold_footprint", "discomfort_threshold_footprint"):      # ros_env.py:105-137
        exp = export._transform(robots.KETI[key], 1.5, 1.0, 0.7)
        assert np.allclose(u[key], exp) and u[key].shape == (4, 2)
    assert export.strict_update_fields(env, arena=0)["humans"] == []


def test_render_arena_picture():
    """render() (env.py:833-1050) as a NumPy rasteriser: 800 x 800 x 3 float32 BGR in [0, 1]; obstacles black, free
    space white, the goal a blue 1 m square, lidar returns below range_max green discs (none for beams at
    range_max), drawn in the reference's flipped (world) orientation."""
    from nav_gym_amd import render as rd, robots
    H = 100
    data = np.zeros((H, H), np.int8)
    data[:5] = 100; data[-5:] = 100; data[:, :5] = 100; data[:, -5:] = 100
    mi = {"data": data, "origin": (0.0, 0.0), "resolution": 0.05, "width": H, "height": H}
    robot = dict(px=2.0, py=1.5, theta=0.3, gx=3.5, gy=3.5, footprint=robots.KETI["footprint"],
                 threshold_footprint=robots.KETI["threshold_footprint"],
                 discomfort_threshold_footprint=robots.KETI["discomfort_threshold_footprint"])
    humans = [dict(px=1.0, py=3.0, theta=1.0, gx=1.2, gy=4.0, footprint=robots.HUMAN["footprint"])]
    scan = np.full(64, 25.0, np.float32); scan[:16] = 1.0
    lidar = dict(angle_min=-np.pi, angle_last=np.pi - 2 * np.pi / 64, range_max=np.float32(25.0))
    img = rd.render_arena(mi, robot, humans, scan, 0.3, lidar)
    assert img.shape == (800, 800, 3) and img.dtype == np.float32 and img.min() >= 0.0 and img.max() <= 1.0
    px = lambda x, y: img[799 - int(y / 0.05 * 8) - 4, int(x / 0.05 * 8) + 4]          # world (x, y) -> pixel (flipped rows)
    assert tuple(px(0.1, 0.1)) == (0.0, 0.0, 0.0) and tuple(px(0.6, 4.4)) == (1.0, 1.0, 1.0)
    assert tuple(px(3.5, 3.5)) == (0.0, 0.0, 1.0)                                       # goal: BGR (0, 0, 1)
    assert tuple(px(1.2, 4.0)) == (1.0, 1.0, 0.0)                                       # pedestrian's local goal
    green = (img[..., 0] == 0) & (img[..., 1] == 1) & (img[..., 2] == 0)
    assert green.sum() > 16 * 20
    none = rd.render_arena(mi, robot, [], np.full(64, 25.0, np.float32), 0.3, lidar)
    assert not ((none[..., 0] == 0) & (none[..., 1] == 1) & (none[..., 2] == 0)).any()
    # xy_to_ij of the renderer is the reference's batch_xy_to_ij (golden vectors)
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_units.npz"))
    mi500 = {"origin": (0.0, 0.0), "resolution": 0.05, "width": 500, "height": 500}
    assert np.array_equal(rd.xy_to_ij(d["xy_500"], mi500), d["ij_500"])


def test_crowd_sim_reset_reproduces_the_reference_cases():
    """CrowdSim.reset (crowd_sim.py:626-722) on the host: the 24 numbered 'test' (square crossing) and 'val' (circle crossing)
    cases recorded from the reference's own method (tests/golden/make_golden.py crowd_reset, the reference's own config
    file) -- robot, humans with their per-episode attributes and robot_visible flags, obstacle outlines, the occupancy map
    and the static obstacles as pedestrians -- are reproduced bit for bit by crowd_reset_scenario."""
    import os
    from nav_gym_amd import crowd
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_crowd_reset.npz"))
    n = int(d["n"])
    assert n == 24
    humans, obstacles = set(), set()
    for k in range(n):
        sc = crowd.crowd_reset_scenario(crowd.CROWD_DEFAULTS, str(d["phase"][k]), int(d["case"][k]))
        shape = tuple(d["map_shape_%d" % k])
        m = np.unpackbits(d["map_%d" % k])[: shape[0] * shape[1]].reshape(shape)
        for key, got in (("robot", sc["robot"]), ("humans", sc["humans"]), ("verts", sc["verts"]), ("static", sc["static"])):
            exp = d["%s_%d" % (key, k)]
            assert got.shape == exp.shape and np.array_equal(got, exp), (k, key)
        assert np.array_equal(sc["free_map"], m), k
        assert sc["circle_radius"] == float(d["circle_radius_%d" % k])
        humans.add(len(sc["humans"])); obstacles.add(len(sc["verts"]))
    assert len(humans) >= 4 and len(obstacles) >= 8            # ragged counts, as the reference draws them
    a = crowd.crowd_reset_scenario(crowd.CROWD_DEFAULTS, "train", 0, seed=5)
    b = crowd.crowd_reset_scenario(crowd.CROWD_DEFAULTS, "train", 0, seed=6)
    assert not np.array_equal(a["robot"], b["robot"])


def test_crowd_sim_is_registered_like_the_reference():
    """`import crowd_sim` registers 'CrowdSim-v0' (crowd_sim/__init__.py:3-6); construction touches neither the GPU nor the
    library; configuration entries are the reference's config names."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "nav-gym_amd"))
    import crowd_sim
    from nav_gym_amd import registry
    assert registry.spec("CrowdSim-v0")["entry_point"] == "nav_gym_amd.crowd:CrowdSimEnv"
    env = crowd_sim.make("CrowdSim-v0", num_envs=3, human_num=7, time_step=0.25)
    assert isinstance(env, crowd_sim.CrowdSimEnv) and env.cfg["human_num"] == 7 and env.cfg["time_limit"] == 35
    assert env.case_size["test"] == 500 and env.case_size["val"] == 50
    with pytest.raises(TypeError):
        crowd_sim.make("CrowdSim-v0", no_such_entry=1)
    with pytest.raises(RuntimeError):
        env.step(None)


def test_render_debug_text_follows_the_reference_formats():
    """render()'s debug text (env.py:182-217): the two multi-line strings in the reference's formats, the six reward terms of
    compute_rewards (env.py:513-573) for one observation -- their sum equals the oracle's reward for that observation --
    and the overlay: red glyph pixels on the twelve baselines y = 50 + 50 i from x = 50 (env.py:1035-1046)."""
    from nav_gym_amd import render as rd
    txt = rd.obs_text(7, [1.0, 2.0], [1.234, -0.005], [0.3, -0.1], 1.5, [10.0, 11.0])
    assert txt == "t: 7\nprev_pose: (1.00 2.00)\npose: (1.23 -0.01)\nvel: (0.30 -0.10)\nyaw: 1.50\ngoal: (10.00 11.00)"
    B = 64
    rng = np.random.default_rng(0)
    thr = np.full(B, 0.6, np.float32); dthr = np.full(B, 0.9, np.float32)
    factors = dict(reward_scale=15.0, reward_success_factor=1, reward_crash_factor=1, reward_progress_factor=0.001,
                   reward_forward_factor=0.0, reward_rotation_factor=0.005, reward_discomfort_factor=0.01)
    cfg = ref.default_config(n_beams=B, n_scan_stack=1)
    seen = set()
    for case in range(40):
        scan = rng.uniform(1.0, 20.0, B).astype(np.float32)
        if case % 3 == 1:
            scan[5] = 0.7                                  # discomfort
        if case % 5 == 2:
            scan[9] = 0.3                                  # crash
        prev = rng.uniform(-5, 5, 2); pose = prev + rng.uniform(-0.1, 0.1, 2)
        vel = np.array([rng.uniform(0, 0.5), rng.uniform(-0.6, 0.6)])
        goal = pose + (rng.uniform(-0.2, 0.2, 2) if case % 7 == 3 else rng.uniform(3, 6, 2))
        t = rd.reward_terms(scan, prev, pose, vel, goal, thr, dthr, factors, 0.5)
        obs = np.concatenate([scan.astype(np.float64), prev, pose, vel, [0.2]])
        out = ref.reward_done(cfg, obs[None], goal[None], thr, dthr)
        assert abs(sum(t.values()) - float(out["reward"][0])) < 1e-9, (case, t)
        seen |= {k for k, v in t.items() if v != 0.0}
    assert {"reward_success", "reward_crash", "reward_progress", "reward_rotation", "reward_discomfort"} <= seen
    rt = rd.reward_text(t).split("\n")
    assert len(rt) == 6 and rt[2] == "reward_progress: {:.5f}".format(t["reward_progress"])
    img = np.ones((800, 800, 3), np.float32)
    rd.overlay_text(img, txt, rd.reward_text(t))
    red = (img == np.array([0, 0, 1], np.float32)).all(axis=2)
    for i in range(12):
        assert red[50 + 50 * i - 14: 50 + 50 * i, 50:400].any(), i
        assert not red[50 + 50 * i + 1: 50 + 50 * i + 30, :].any(), i
    assert not red[:, :50].any()
