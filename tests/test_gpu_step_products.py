"""GPU: what the four launches behind the step -- info['humans'], ['goal_path'], ['planner'], ['local_map'] -- promise in common
through NavGymEnv, with all four on at once so that the planner reads the goal path's sub-goal and the local map the observer's
`visible`: (a) what step t returned is unchanged after step t + 1 (the two buffer sets); (b) step t + 2 hands out the very
objects of step t (views are made once per buffer parity); (c) after reset(mask) and after a state_dict / load_state_dict round
trip every getter returns what a direct NavSim call on that state returns, bit for bit; (d) num_envs == 1 returns NumPy values
of the documented dtypes.  What each product computes is held to its specification by its own test module."""
import numpy as np
import pytest

from gpu_support import gpu, same_bits  # noqa: F401  (gpu: the module's fixture)

pytestmark = pytest.mark.gpu

KEYS = ("humans", "goal_path", "planner", "local_map")
# (auto-reset mode, arenas, local map size): both modes at three arenas and at one, a map size that is no multiple of 4 in each
WORLDS = (("same_step", 3, 8), ("next_step", 3, 7), ("same_step", 1, 7), ("next_step", 1, 8))
STEPS, SAVE_AT = 6, 2


def _env(mode, E, G):
    import nav_gym_amd
    from nav_gym_amd import registry
    ranges = dict(nav_gym_amd.DEFAULT_KWARGS["env_param_range"], obstacle_number=([4, 4], "int"), obstacle_width=([0.3, 0.5], "float"),
                  num_humans=([3, 3], "int"))
    return registry.make("NavGym-v0", num_envs=E, map_size=100, n_beams=64, seed=5, plan_paths=False, min_goal_dist=2.0,
                         max_goal_dist=4.0, indoor_ratio=0.0, pedestrian_model="sfm", max_episode_steps=3, env_param_range=ranges,
                         auto_reset=True, autoreset_mode=mode, observe_humans=2, goal_path=True, local_planner="dwa",
                         local_planner_params=dict(n_v=2, n_w=3, horizon=2), observe_local_map=G,
                         local_map_params=dict(visible_only=True))


def _host(v):
    """A product's value as NumPy copies: {name: array} of a dict, else one array under 'map'."""
    items = v.items() if isinstance(v, dict) else [("map", v)]
    return {k: x.cpu().numpy().copy() if hasattr(x, "is_cuda") else np.array(x) for k, x in items}


def _same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        same_bits(a[k], b[k], "%s: %s" % (what, k))


def _getters(env):
    """The four getters that return what info holds (goal_field(), which has no info key, rides with the goal path in (c))."""
    return dict(humans=env.observed_humans(), goal_path=env.goal_path(), planner=env.planner_action(), local_map=env.local_map())


def _direct(gpu, env, rebuild):
    """The four NavSim calls on the environment's current state, in the order of their dependencies, as the environment's
    protocol makes them: next-step auto-reset skips the arenas whose `done` is set.  The rows of arena 0 for num_envs == 1."""
    sim = env.sim
    skip = sim.out["done"] if env.auto_reset and env.autoreset_mode == "next_step" else None
    humans = sim.ped_observe(skip=skip)
    goal = sim.goal_path(rebuild=rebuild, skip=skip)
    planner = sim.dwa(subgoal=goal["subgoal"], skip=skip)
    local = sim.local_map(skip=skip, visible=humans["visible"])
    gpu.torch.cuda.synchronize()
    out = dict(humans=_host(humans), goal_path=_host(goal), planner={k: v for k, v in _host(planner).items() if k in env._PLANNER_KEYS},
               local_map=_host(local))
    out["humans"]["visible"] = out["humans"]["visible"].astype(bool)
    if env.num_envs == 1:
        out = {key: {k: v[0] for k, v in d.items()} for key, d in out.items()}
        out["humans"]["count"] = np.array(int(out["humans"]["count"]))          # (documented as an int)
    out["goal_path"]["field"] = _host(sim.goal_field())["map"]                  # (the device's fields, whatever num_envs is)
    return out


def _getters_bits(env):
    got = {k: _host(v) for k, v in _getters(env).items()}
    got["goal_path"]["field"] = _host(env.goal_field())["map"]
    return got


_RUNS = {}


def _run(gpu, world):
    """One environment driven once for all four products: per step the objects info held, their bits then and their bits one
    step later; after reset(mask) and after load_state_dict the getters' bits and those of the direct calls."""
    if world in _RUNS:
        return _RUNS[world]
    torch = gpu.torch
    mode, E, G = world
    env = _env(mode, E, G)
    env.reset()
    act = np.zeros((E, 2))
    act[:, 0], act[: (E + 1) // 2, 1] = 0.4, 0.2
    objs, then, later, sd = [], [], [], None
    for t in range(STEPS):
        _, _, _, info = env.step(act[0] if E == 1 else act)
        torch.cuda.synchronize()
        if t:
            later.append({k: _host(objs[-1][k]) for k in KEYS})
        objs.append({k: info[k] for k in KEYS})
        then.append({k: _host(info[k]) for k in KEYS})
        assert all(info[k] is v for k, v in _getters(env).items())
        if t == SAVE_AT:
            sd = env.state_dict()
    every = torch.ones(E, dtype=torch.uint8, device=gpu.dev)
    stages = {}
    mask = np.arange(E) % 2 == 0
    env.reset(mask=mask)
    got = _getters_bits(env)
    stages["reset(mask)"] = (got, _direct(gpu, env, torch.from_numpy(mask.astype(np.uint8)).to(gpu.dev)))
    env.load_state_dict(sd)
    got = _getters_bits(env)
    stages["load_state_dict"] = (got, _direct(gpu, env, every))
    env.close()
    _RUNS[world] = dict(objs=objs, then=then, later=later, stages=stages)
    return _RUNS[world]


# (d) the documented dtypes of num_envs == 1: (type, dtype, shape) per name; K = 2 rows, N pedestrians, G cells a side
def _documented(N, G):
    return dict(humans=dict(state=(np.ndarray, np.float32, (2, 5)), index=(np.ndarray, np.int32, (2,)), count=(int, None, ()),
                            visible=(np.ndarray, np.bool_, (N,))),
                goal_path=dict(distance=(np.float32, np.float32, ()), subgoal=(np.ndarray, np.float32, (2,)), status=(np.uint8, np.uint8, ())),
                planner=dict(action=(np.ndarray, np.float64, (2,)), twist=(np.ndarray, np.float64, (2,)),
                             clearance=(np.float32, np.float32, ()), best=(np.int32, np.int32, ()), status=(np.uint8, np.uint8, ())),
                local_map=dict(map=(np.ndarray, np.float32, (4, G, G))))


@pytest.mark.parametrize("key", KEYS)
def test_what_the_products_promise_in_common(gpu, key):
    for world in WORLDS:
        mode, E, G = world
        r = _run(gpu, world)
        what = "%s, %s, E = %d, G = %d" % (key, mode, E, G)
        changed = 0
        for t in range(STEPS - 1):                                                # (a) intact through the next step
            _same_bits(r["then"][t][key], r["later"][t][key], "%s: step %d's value after step %d" % (what, t, t + 1))
            changed += any(r["then"][t][key][k].tobytes() != r["then"][t + 1][key][k].tobytes() for k in r["then"][t][key])
        # (three arenas hand out views of the device's buffers: there the comparison must have had something to show; the NumPy
        #  values of one arena are host copies of their own)
        assert changed or E == 1, "%s: no step changed the value, the comparison above shows nothing" % what
        if E > 1:                                                                 # (b) one set of views per buffer parity
            for t in range(STEPS - 2):
                a, b, c = r["objs"][t][key], r["objs"][t + 1][key], r["objs"][t + 2][key]
                assert a is c and a is not b, "%s: steps %d, %d, %d" % (what, t, t + 1, t + 2)
                if isinstance(a, dict):
                    assert all(a[k] is c[k] for k in a)
        for stage, (got, direct) in r["stages"].items():                          # (c) the getters after the two other run sites
            _same_bits(got[key], direct[key], "%s: getter after %s against the direct call" % (what, stage))
        if E == 1:                                                                # (d) NumPy values of the documented dtypes
            N = r["then"][0]["humans"]["visible"].shape[0]
            v = r["objs"][0][key]
            for k, (kind, dtype, shape) in _documented(N, G)[key].items():
                x = v[k] if isinstance(v, dict) else v
                assert isinstance(x, kind) and np.shape(x) == shape and (dtype is None or x.dtype == dtype), (what, k, type(x))
            assert (set(v) if isinstance(v, dict) else {"map"}) == set(_documented(N, G)[key])
