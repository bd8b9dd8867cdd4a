"""GPU: navsim_ped_orca_walls (include/navsim.h) -- ORCA pedestrians that avoid the arena's listed rectangles, one kernel --
against its specification (tests/ped_orca_walls_spec.py: the selection in numpy float32 + the CPU oracle's navsim_crowd_orca
with one polygon set per query) bit for bit over every lane layout, on worlds whose rect_index rows the device built or
generated itself; max_rects = 0 against navsim_ped_orca; a permuted map_slot; the gym surface; and the float64 swept-clearance
check of tests/orca_f64.py on the device's velocities."""
import functools

import numpy as np
import pytest

import ped_orca_spec as spec
import ped_orca_walls_scenes as ws
import ped_orca_walls_spec as wspec
from nav_gym_amd import abi
from gpu_support import gpu, action_rows, eq, fresh_sim, limit_world, to_device  # noqa: F401  (gpu: the module's fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
STATE = ("ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head", "n_peds", "robot_pose",
         "prev_action")


def _device_world(gpu, E, N, occ):
    """field, then build_rects, then build_rect_index (world.make_world) on the device; the pedestrians come from the scenes"""
    cfg = gpu.lib.default_config(n_envs=E, map_h=ws.SIZE, map_w=ws.SIZE, max_peds=N, n_scan_stack=1, ped_model=abi.PED_EXTERNAL,
                                 auto_reset=abi.AUTORESET_NONE, n_spawn=8, seed=4343, field_format=abi.FIELD_U16T, time_step=0.2)
    gpu.world.lidar_full_circle(cfg, 64)
    arrays, _ = limit_world(gpu, cfg, occ, n_peds=N, v_pref_range=(0.3, 0.6), robot_clearance=0.6)
    assert "rect_index" in arrays and (cfg.resolution, cfg.origin_x, cfg.origin_y) == (ws.RES, 0.0, 0.0)
    g = fresh_sim(gpu, cfg, arrays)
    return cfg, g, wspec.decode_rows(g.t["rect_index"].cpu().numpy())


def _load(gpu, g, a):
    for k in STATE:
        g.t[k].copy_(to_device(gpu, np.ascontiguousarray(a[k])).to(g.t[k].dtype).reshape(g.t[k].shape))
    g.t["ped_cmd"].fill_(SENTINEL)


def _call(gpu, g, cfg, a, p, rects, K, what):
    """one call on the device and in the specification, from the same state -> (the device's ped_cmd, the census)"""
    a = dict(a, ped_cmd=np.full(a["ped_cmd"].shape, SENTINEL))
    _load(gpu, g, a)
    dropped = gpu.torch.full((cfg.n_envs, cfg.max_peds), -1, dtype=gpu.torch.int32, device=gpu.dev)
    got = g.ped_orca_walls({k: p[k] for k in spec.KEYS}, K, dropped).cpu().numpy()
    want_cmd, want_head, want_dropped, census = wspec.ped_orca_walls(cfg, a, p, rects, K)
    live = np.arange(cfg.max_peds)[None, :] < np.clip(a["n_peds"], 0, cfg.max_peds)[:, None]
    assert (want_cmd[~live] == SENTINEL).all() and not (want_cmd[live] == SENTINEL).any()
    eq(got, want_cmd, "ped_cmd (%s)" % what)                         # live rows, and dead rows still holding the sentinel
    eq(g.t["ped_wp_head"].cpu().numpy(), want_head, "ped_wp_head (%s)" % what)
    eq(dropped.cpu().numpy(), np.where(live, want_dropped, -1), "dropped (%s)" % what)
    return got, census


@functools.lru_cache(maxsize=None)
def _answers(gpu, shape):
    E, N, cs = ws.calls(shape)
    cfg, g, rects = _device_world(gpu, E, N, ws.occupancy(E))
    # what the builder listed: never a free cell, and on this map the ring and every box
    occ, drawn = ws.occupancy(1)[0], np.zeros((ws.SIZE, ws.SIZE), np.uint8)
    for x0, y0, x1, y1 in (r for r in rects[0] if r.any()):
        drawn[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = 1
    print("%s: %d rectangles listed: %s" % (shape, int(rects[0].any(1).sum()), [tuple(int(v) for v in r) for r in rects[0] if r.any()]))
    assert not (drawn & ~occ & 1).any() and np.array_equal(drawn, occ)
    out = []
    for c, (s, K, kw) in enumerate(cs):
        p = spec.params(cfg, **kw)
        got, census = _call(gpu, g, cfg, ws.state(s, cfg), p, rects, K, "%s call %d: max_rects %d %s" % (shape, c, K, kw))
        out.append((cfg, p, got, census))
    return out


@pytest.mark.parametrize("shape", list(ws.SHAPES))
def test_single_calls_vs_specification(gpu, shape):
    """ped_cmd, ped_wp_head and dropped equal the specification bit for bit: max_rects 1, 3, 8, 32; time_horizon_obst 0.5, 2,
    5; the robot visible or not; max_neighbors 0 (ped_orca_walls_scenes.VARIANTS)"""
    assert len(_answers(gpu, shape)) == len(ws.VARIANTS)


def test_census_of_the_calls(gpu):
    ws.census_of([(shape, item[3]) for shape in ws.SHAPES for item in _answers(gpu, shape)], 10, "device calls")


def test_swept_clearance_of_the_device_velocities(gpu):
    """The scenes and the bound of tests/test_ped_orca_walls.py::test_swept_clearance, on the velocities the kernel returned."""
    def answer(shape, c):
        cfg, p, got, census = _answers(gpu, shape)[c]
        return got, census, cfg, p
    ws.swept_check(answer, "device")


def test_no_rectangles_is_navsim_ped_orca(gpu):
    E, N, cs = ws.calls("7x8")
    cfg, g, _ = _device_world(gpu, E, N, ws.occupancy(E))
    a, p = ws.state(cs[0][0], cfg), spec.params(cfg)
    _load(gpu, g, a)
    want = g.ped_orca({k: p[k] for k in spec.KEYS}).clone()
    want_head = g.t["ped_wp_head"].clone()
    _load(gpu, g, a)
    dropped = gpu.torch.full((E, N), -1, dtype=gpu.torch.int32, device=gpu.dev)
    got = g.ped_orca_walls({k: p[k] for k in spec.KEYS}, 0, dropped)
    assert gpu.torch.equal(got, want) and gpu.torch.equal(g.t["ped_wp_head"], want_head)
    live = np.arange(N)[None, :] < a["n_peds"][:, None]
    eq(dropped.cpu().numpy(), np.where(live, 0, -1), "dropped at max_rects 0")
    assert (want.cpu().numpy()[live] != SENTINEL).all()


def test_permuted_map_slot(gpu):
    """Arenas on different maps; a state whose map_slot is a permutation answers with the permuted rows."""
    E, N = 6, 8
    occ = gpu.world.make_maps(E, ws.SIZE, 977, n_obstacles=6)
    cfg, g, rects = _device_world(gpu, E, N, occ)
    assert len({rects[e].tobytes() for e in range(E)}) == E
    s = ws.arenas(E, N, 8900)
    a, p = ws.state(s, cfg), spec.params(cfg, time_horizon_obst=2.0)
    straight, _ = _call(gpu, g, cfg, a, p, rects, 8, "own slots")
    perm = np.array([3, 0, 5, 1, 2, 4], np.int32)
    slots = to_device(gpu, perm)
    g.st.map_slot = slots.data_ptr()
    try:
        permuted, _ = _call(gpu, g, cfg, a, p, rects[perm], 8, "permuted slots")
    finally:
        g.st.map_slot = None
    assert not np.array_equal(straight, permuted)


def _spec_state(sim):
    return sim.numpy_state("ped_cmd", "ped_wp_head", "ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints",
                           "n_peds", "robot_pose", "prev_action")


def test_regenerated_world(gpu):
    """A world navsim_regen drew (outdoor maps): its rect_index rows were written by the generator, not by the builder."""
    from nav_gym_amd import registry
    env = registry.make("NavGym-v0", num_envs=6, map_size=200, n_beams=256, seed=23, plan_paths=False, min_goal_dist=2.0,
                        max_goal_dist=6.0, indoor_ratio=0.0, num_humans=8, randomize_maps=True, pregen_pipeline=0,
                        pedestrian_model="orca", orca_params=dict(max_obst_rects=8, time_horizon_obst=2.0))
    env.reset()
    sim = env.sim
    assert "map_slot" not in sim.t
    rects = wspec.decode_rows(sim.t["rect_index"].cpu().numpy())
    assert all(int(r.any(1).sum()) >= 4 for r in rects), [int(r.any(1).sum()) for r in rects]      # the ring at least
    for act in action_rows(3, 6):                                          # pedestrians and robots in motion
        env.step(act)
    rects = wspec.decode_rows(sim.t["rect_index"].cpu().numpy())
    a = _spec_state(sim)
    binds = 0
    for K, tho in ((8, 2.0), (3, 5.0)):
        p = spec.params(sim.cfg, time_horizon_obst=tho)
        want_cmd, want_head, want_dropped, census = wspec.ped_orca_walls(sim.cfg, a, p, rects, K)
        dropped = gpu.torch.zeros((6, sim.cfg.max_peds), dtype=gpu.torch.int32, device=gpu.dev)
        sim.t["ped_wp_head"].copy_(to_device(gpu, a["ped_wp_head"]))
        got = sim.ped_orca_walls({k: p[k] for k in spec.KEYS}, K, dropped).cpu().numpy()
        eq(got, want_cmd, "ped_cmd on the regenerated world, max_rects %d" % K)
        eq(sim.t["ped_wp_head"].cpu().numpy(), want_head, "ped_wp_head on the regenerated world")
        eq(dropped.cpu().numpy(), want_dropped, "dropped on the regenerated world")
        binds += census["walls bind"]
    assert binds > 0
    env.close()


def test_through_the_env(gpu):
    """NavGymEnv(pedestrian_model='orca', orca_params=dict(max_obst_rects=8, ...)): 50 steps equal the host composition of
    NavSim.ped_orca_walls and a step, and no pedestrian centre stands on an occupied cell."""
    from nav_gym_amd import registry
    kw = dict(num_envs=4, seed=31)
    a = registry.make("NavGym-v0", pedestrian_model="orca", orca_params=dict(max_obst_rects=8, time_horizon_obst=2.0), **kw)
    b = registry.make("NavGym-v0", pedestrian_model="external", **kw)
    assert gpu.torch.equal(a.reset()["observation"], b.reset()["observation"])
    occ = [a.sim.occupancy(e) for e in range(4)]
    cfg = a.sim.cfg
    assert int(a.sim.t["n_peds"].sum()) > 0
    for t, act in enumerate(action_rows(50, 4)):
        cmd = b.sim.ped_orca_walls(dict(time_horizon_obst=2.0), 8).clone()
        xa, xb = a.step(act), b.step(act, human_actions=cmd)
        assert gpu.torch.equal(xa[0]["observation"], xb[0]["observation"]), t
        assert gpu.torch.equal(xa[1], xb[1]) and gpu.torch.equal(xa[2], xb[2]), t
        st = a.sim.numpy_state("ped_pose", "n_peds")
        for e in range(4):
            xy = st["ped_pose"][e, :int(st["n_peds"][e]), :2]
            i = np.floor((xy[:, 0] - cfg.origin_x) / cfg.resolution).astype(int)
            j = np.floor((xy[:, 1] - cfg.origin_y) / cfg.resolution).astype(int)
            assert not occ[e][j, i].any(), (t, e, xy[occ[e][j, i] != 0])
    assert gpu.torch.equal(a.sim.t["ped_pose"], b.sim.t["ped_pose"])
    a.close(); b.close()
