"""navsim_step_sorted: the longest-first sort on a FRONT workgroup of the step's own launch (kernels_step.hpp
navsim_step_kernel, launch_order_sort) instead of a kernel of its own between two steps.

The order is a scheduling hint, so two things are checked: that the front workgroup writes what navsim_launch_order
would (a permutation, descending up to one histogram bucket, an outlier that does not flatten the rest) at every block
size -- its loops stride by the step's own block size and its scan owns 1024 / BLOCK buckets per thread -- and that a
rollout which sorts inside its launches equals one that never sorts, bit for bit.  The sweep's worlds carry pedestrian
slots (20, two of them alive) and 65 beams: with 100 x 100 maps that is the smallest world whose dynamic LDS (index row
2.4 KB + the pedestrian scratch and pair table 6.3 KB) holds the sort's 4.2 KB at EVERY block size; the variants without
pedestrians are covered by the rollouts (shape B: the plain 256-thread kernel with parked rays) and by the refusal."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import gpu, device_world, eq, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

SIZE = 100                  # cells per side of the sweep's maps
OUTLIER = 2_000_000_000


@pytest.fixture(scope="module")
def base_maps(gpu):
    return gpu.world.make_maps(8, SIZE, 41)                     # closed outdoor maps; larger worlds repeat them


@pytest.fixture(scope="module")
def sweep_worlds(gpu, base_maps):
    """One world per arena count, shared by the block sizes (every NavSim copies what it changes)."""
    worlds = {}
    for E in (1, 63, 257, 2500):
        cfg = gpu.lib.default_config(n_envs=E, map_h=SIZE, map_w=SIZE, max_peds=20, ped_model=abi.PED_SFM, n_spawn=4,
                                     auto_reset=1, n_scan_stack=1, seed=41, field_format=abi.FIELD_U16T)
        gpu.world.lidar_full_circle(cfg, 65)
        occ = np.ascontiguousarray(np.tile(base_maps, ((E + 7) // 8, 1, 1))[:E])
        arrays = device_world(gpu, cfg, occ, 2, min_goal_dist=3.0, max_goal_dist=8.0)
        assert "rect_index" in arrays and cfg.closed_maps == 1
        worlds[E] = (cfg, arrays)
    return worlds


def _copy_cfg(cfg, **kw):
    c = cfg.copy()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _step_sorted(gpu, g, cost, order):
    """One navsim_step_sorted launch of NavSim g with the caller's buffers; the return code."""
    g._flip()
    rc = g.lib.navsim_step_sorted(C.byref(g.cfg), C.byref(g.st), C.byref(g.io), cost.data_ptr() if cost is not None else None,
                                  order.data_ptr() if order is not None else None, None)
    if rc == 0:
        g.cur = 1 - g.cur
    gpu.torch.cuda.synchronize()
    return rc


def _check_order(o, c, E, outlier_at=None):
    assert np.array_equal(np.sort(o), np.arange(E)), "not a permutation"
    c = c.astype(np.int64)
    width = min(int(c.max()), 4 * int(c.mean()) + 1) // 1023 + 2
    s = c[o]
    if outlier_at is not None:
        assert outlier_at in o[:50], "the outlier is not among the first 50"
        s = s[s < OUTLIER]
    print("E %d: widest ascent %d, bucket width %d" % (E, int(np.diff(s).max()) if len(s) > 1 else 0, width))
    assert (np.diff(s) <= width).all(), "not descending up to one bucket"


@pytest.mark.parametrize("E", [1, 63, 257, 2500])
@pytest.mark.parametrize("step_block", [64, 256, 512, 1024])
def test_front_workgroup_sorts(gpu, sweep_worlds, step_block, E):
    torch = gpu.torch
    cfg, arrays = sweep_worlds[E]
    g = gpu.sim.NavSim(_copy_cfg(cfg, step_block=step_block), arrays, launch_order=True)
    g.reset_obs()
    gen = torch.Generator(device=gpu.dev); gen.manual_seed(1000 * step_block + E)
    cost = torch.randint(0, 50000, (E,), dtype=torch.int32, device=gpu.dev, generator=gen)
    order = torch.full((E,), -7, dtype=torch.int32, device=gpu.dev)
    assert _step_sorted(gpu, g, cost, order) == 0
    _check_order(order.cpu().numpy(), cost.cpu().numpy(), E)
    assert (g.t["arena_cost"] > 0).all(), "the arenas behind the front workgroup did not all step"
    at = 17 % E
    cost[at] = OUTLIER                                           # one held-up workgroup must not flatten the rest
    order.fill_(-7)
    assert _step_sorted(gpu, g, cost, order) == 0
    _check_order(order.cpu().numpy(), cost.cpu().numpy(), E, outlier_at=at)
    assert np.array_equal(g.t["steps"].cpu().numpy() + g.t["episode"].cpu().numpy() > 0, np.ones(E, bool)), "an arena was skipped"


def _plain_world(gpu, base_maps, E, rect_table, beams, **cfg_kw):
    cfg = gpu.lib.default_config(n_envs=E, map_h=SIZE, map_w=SIZE, max_peds=1, ped_model=abi.PED_NONE, n_spawn=4, auto_reset=1,
                                 n_scan_stack=1, seed=41, field_format=abi.FIELD_U16T, **cfg_kw)
    if beams == 1081:
        gpu.world.lidar_1081(cfg)
    else:
        gpu.world.lidar_full_circle(cfg, beams)
    return cfg, device_world(gpu, cfg, base_maps[:E], 0, rect_table=rect_table, min_goal_dist=3.0, max_goal_dist=8.0)


def _snapshot(g):
    s = g.numpy_state()
    s["obs0"], s["obs1"] = g.obs_buf[0].cpu().numpy(), g.obs_buf[1].cpu().numpy()
    for k, v in g.out_buf[0].items():
        s["out0_" + k] = v.cpu().numpy()
    for k, v in g.out_buf[1].items():
        s["out1_" + k] = v.cpu().numpy()
    return s


def test_unsupported_without_room_for_the_sort(gpu, base_maps):
    """No rect records, no pedestrians, 64 threads per arena: the step has no dynamic LDS at all.  NAVSIM_E_UNSUPPORTED, and
    nothing is launched."""
    cfg, arrays = _plain_world(gpu, base_maps, 8, rect_table=False, beams=65, step_block=64)
    assert "rect_index" not in arrays
    g = gpu.sim.NavSim(cfg, arrays, launch_order=True)
    g.reset_obs()
    cost = gpu.torch.arange(8, dtype=gpu.torch.int32, device=gpu.dev)
    order = gpu.torch.full((8,), -7, dtype=gpu.torch.int32, device=gpu.dev)
    before = _snapshot(g)
    assert _step_sorted(gpu, g, cost, order) == abi.E_UNSUPPORTED
    assert (order.cpu().numpy() == -7).all()
    after = _snapshot(g)
    for k in before:
        eq(before[k], after[k], k)
    # ... and NavSim then sorts with the separate kernel, for good
    g.lpt_period = 1
    g.t["launch_order"].copy_(gpu.torch.arange(7, -1, -1, dtype=gpu.torch.int32, device=gpu.dev))
    for _ in range(3):
        g.step(gpu.torch.zeros((8, 2), dtype=gpu.torch.float64, device=gpu.dev))
    assert g.sorts_in_launch == 0 and g.sort_in_launch is False
    assert np.array_equal(np.sort(g.t["launch_order"].cpu().numpy()), np.arange(8))


def test_refusals_launch_nothing(gpu, base_maps):
    """NULL and aliased pointers: an error before any launch -- state, outputs and sort_order stay what they were."""
    cfg, arrays = _plain_world(gpu, base_maps, 8, rect_table=None, beams=1081, step_block=256)     # (parked rays: 4.3 KB of dynamic LDS)
    g = gpu.sim.NavSim(cfg, arrays, launch_order=True)
    g.reset_obs()
    torch = gpu.torch
    cost = torch.arange(8, dtype=torch.int32, device=gpu.dev)
    order = torch.full((8,), -7, dtype=torch.int32, device=gpu.dev)
    before = _snapshot(g)
    for what, c_, o_ in (("sort_cost NULL", None, order), ("sort_order NULL", cost, None),
                         ("sort_cost == st.arena_cost", g.t["arena_cost"], order),
                         ("sort_order == st.launch_order", cost, g.t["launch_order"])):
        rc = _step_sorted(gpu, g, c_, o_)
        assert rc == abi.E_ARG, (what, rc)
        assert (order.cpu().numpy() == -7).all(), what
        after = _snapshot(g)
        for k in before:
            eq(before[k], after[k], "%s: %s" % (what, k))
    assert _step_sorted(gpu, g, cost, order) == 0                # the same call with proper buffers is accepted
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(8))


@pytest.fixture(scope="module")
def rollout_worlds(gpu):
    """Shape A: E = 64, 240 x 240 maps, 1081 beams, 5 SFM pedestrians.  Shape B: E = 64, no pedestrians, 256 threads per arena
    (parked rays).  Each with the rollout that never sorts, computed once."""
    torch = gpu.torch
    E, size = 64, 240
    occ = gpu.world.make_maps(E, size, 5)
    worlds = {}
    for shape, kw, n_peds in (("A", dict(max_peds=6, ped_model=abi.PED_SFM), 5),
                              ("B", dict(max_peds=1, ped_model=abi.PED_NONE, step_block=256), 0)):
        cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, n_spawn=8, auto_reset=1, seed=5, field_format=abi.FIELD_U16T, **kw)
        gpu.world.lidar_1081(cfg)
        arrays = device_world(gpu, cfg, occ, n_peds)
        gen = torch.Generator(device=gpu.dev); gen.manual_seed(2)
        acts = torch.rand((10, E, 2), generator=gen, device=gpu.dev, dtype=torch.float64)
        acts[..., 0] *= 0.5; acts[..., 1] = acts[..., 1] * 1.28 - 0.64
        plain = gpu.sim.NavSim(cfg, arrays, launch_order=False)
        assert "launch_order" not in plain.t
        trace = [(plain.reset_obs().cpu().numpy(), {})]
        for t in range(10):
            o, out = plain.step(acts[t])
            trace.append((o.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}))
        worlds[shape] = (cfg, arrays, acts, trace, plain.numpy_state())
    return worlds


def _rollout_against(gpu, world, in_launch):
    cfg, arrays, acts, trace, state = world
    E = cfg.n_envs
    rev = np.arange(E - 1, -1, -1)
    lpt = gpu.sim.NavSim(cfg, arrays, launch_order=True)         # (a 64-arena launch is one generation: off by default)
    lpt.lpt_period = 3
    if not in_launch:
        lpt.sort_in_launch = False                               # as if the library had no navsim_step_sorted
    lpt.t["launch_order"].copy_(to_device(gpu, rev.astype(np.int32)))
    eq(lpt.reset_obs().cpu().numpy(), trace[0][0], "reset obs")
    for t in range(10):
        o, out = lpt.step(acts[t])
        eq(o.cpu().numpy(), trace[t + 1][0], "obs of step %d" % t)
        for k, v in trace[t + 1][1].items():
            eq(out[k].cpu().numpy(), v, "%s of step %d" % (k, t))
    s = lpt.numpy_state()
    for k in state:
        eq(s[k], state[k], "state %s" % k)
    order = lpt.t["launch_order"].cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(E)) and not np.array_equal(order, rev)      # re-sorted by now
    assert (lpt.t["arena_cost"] > 0).all()
    assert lpt.st.launch_order == lpt.t["launch_order"].data_ptr() and lpt.st.arena_cost == lpt.t["arena_cost"].data_ptr()
    return lpt


@pytest.mark.parametrize("shape", ["A", "B"])
def test_sorting_launches_are_result_neutral(gpu, rollout_worlds, shape):
    """Ten steps with lpt_period = 3 from a reversed order, the sorts inside the step launches (before steps 2-6 and 9),
    against launch_order=False: observations, outputs and state bit-equal."""
    lpt = _rollout_against(gpu, rollout_worlds[shape], in_launch=True)
    assert lpt.sorts_in_launch == 6 and lpt.sort_in_launch is True


@pytest.mark.parametrize("shape", ["A", "B"])
def test_fallback_to_the_separate_sort(gpu, rollout_worlds, shape):
    """The same rollout with the export made unavailable on the NavSim object: navsim_launch_order ahead of navsim_step."""
    lpt = _rollout_against(gpu, rollout_worlds[shape], in_launch=False)
    assert lpt.sorts_in_launch == 0
