"""GPU: every entry point that carves a caller's workspace, given EXACTLY the bytes its size query returns, writes nowhere
else, and its results do not depend on how much more it is given.

The pattern, per workspace: one uint8 tensor of 1 MiB of guard + the queried bytes + 1 MiB of guard, the guards filled with
0xA5, the middle view handed to the call -- a sub-buffer carved too far back lands in a guard and is seen (never outside
the allocation).  A twin run of the same world uses the whole, 2 MiB larger tensor as its workspace; every output and
every state array of the two runs must be equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import gpu, device_sim, rect_pairs, regen_layout, seeded_action  # noqa: F401  (gpu: the module's fixture)
from helpers import policy_weights
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 1 << 20


def _guarded(gpu, nbytes):
    """(whole tensor, the view of exactly nbytes between the guards)"""
    buf = gpu.torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=gpu.torch.uint8, device=gpu.dev)
    buf[GUARD:GUARD + nbytes] = 0
    return buf, buf[GUARD:GUARD + nbytes]


def _roomy(gpu, nbytes):
    return gpu.torch.zeros(nbytes + 2 * GUARD, dtype=gpu.torch.uint8, device=gpu.dev)


def _guards_intact(gpu, buf, nbytes, what):
    gpu.torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()), "%s: wrote below its workspace" % what
    assert bool((buf[GUARD + nbytes:] == 0xA5).all()), "%s: wrote beyond the %d bytes its query returns" % (what, nbytes)


def _same_arrays(gpu, ta, tb, cfg, what):
    """two dicts of state arrays, bit for bit (scheduling hints and the workspaces apart; waypoint slots beyond a route's
    length keep whatever the buffer held; the record index compared by what it says)"""
    bits = lambda t: t.contiguous().reshape(-1).view(gpu.torch.uint8)
    assert set(ta) == set(tb)
    for k in ta:
        if k in ("arena_cost", "launch_order") or "_ws" in k:
            continue
        x, y = ta[k], tb[k]
        if k == "rect_index":
            assert np.array_equal(rect_pairs(x, cfg.map_h, cfg.map_w), rect_pairs(y, cfg.map_h, cfg.map_w)), "%s: state %s" % (what, k)
            continue
        if k == "ped_waypoints":
            live = gpu.torch.arange(cfg.max_waypoints, device=gpu.dev)[None, None, :] < ta["ped_n_waypoints"][..., None].long()
            x, y = x[live], y[live]
        assert gpu.torch.equal(bits(x), bits(y)), "%s: state %s" % (what, k)


def _same(gpu, a, b, what):
    """obs, outputs and every state array of the two simulators"""
    gpu.torch.cuda.synchronize()
    bits = lambda t: t.contiguous().reshape(-1).view(gpu.torch.uint8)
    assert gpu.torch.equal(bits(a.obs), bits(b.obs)), "%s: obs" % what
    for k in a.out:
        assert gpu.torch.equal(bits(a.out[k]), bits(b.out[k])), "%s: %s" % (what, k)
    _same_arrays(gpu, a.t, b.t, a.cfg, what)


@pytest.mark.parametrize("layout", ["packed-corridors-planned", "float32-smallest", "packed-overflow-plane"])
def test_regen_stays_inside_the_queried_workspace(gpu, layout):
    """navsim_regen: one step, every done flag set by hand (more arenas than regen_cap: the cap applies), regen()."""
    cfg, occ, n_peds, wkw = regen_layout(gpu, layout)
    nbytes = gpu.lib.load().navsim_regen_workspace_bytes(C.byref(cfg))
    buf, view = _guarded(gpu, nbytes)
    sims = []
    for ws in (view, _roomy(gpu, nbytes)):
        g = device_sim(gpu, cfg, occ, n_peds, **wkw)
        if layout == "packed-overflow-plane":
            assert "field_overflow" in g.t
        if layout == "packed-corridors-planned":
            assert "rect_table" in g.t and "costmap" in g.t
        g.t["regen_ws"] = ws
        g.step(seeded_action(gpu, cfg.n_envs, 1))
        g.out["done"].fill_(1)
        goals = g.t["spawn_goal"].clone()
        g.regen()
        gpu.torch.cuda.synchronize()
        assert int((g.t["spawn_goal"] != goals).flatten(1).any(1).sum()) == cfg.regen_cap    # regen_cap arenas got a new world
        g.step(seeded_action(gpu, cfg.n_envs, 2))
        sims.append(g)
    _guards_intact(gpu, buf, nbytes, "navsim_regen (%s)" % layout)
    _same(gpu, sims[0], sims[1], "navsim_regen (%s)" % layout)


def test_regen_stage_stays_inside_the_queried_workspace(gpu):
    """navsim_regen_stage_part through enable_pregen(): the pass takes count / list from the layout of ITS workspace."""
    cfg, occ, n_peds, wkw = regen_layout(gpu, "packed-corridors-planned")
    sims, bufs = [], []
    for guarded in (True, False):
        g = device_sim(gpu, cfg, occ, n_peds, **wkw)
        g.enable_pregen()
        nbytes = gpu.lib.load().navsim_regen_workspace_bytes(C.byref(g.stage_cfg))
        assert g.stage_ws.numel() == nbytes
        buf, view = _guarded(gpu, nbytes)
        ws = view if guarded else _roomy(gpu, nbytes)
        g.stage_ws = ws
        for ln in g.stage_lane:
            ln["ws"] = ws
        for k in (1, 2):                                # the second swap installs what the guarded pass staged
            g.step(seeded_action(gpu, cfg.n_envs, k))
            g.out["done"].fill_(1)
            g.regen()
            g.pregen_sync()
        g.step(seeded_action(gpu, cfg.n_envs, 3))
        sims.append(g); bufs.append((buf, nbytes))
    _guards_intact(gpu, bufs[0][0], bufs[0][1], "navsim_regen_stage_part")
    _same(gpu, sims[0], sims[1], "navsim_regen_stage_part")
    _same_arrays(gpu, sims[0].stage_t, sims[1].stage_t, cfg, "the worlds staged last")


@pytest.mark.parametrize("flags", [True, False])
def test_replan_stays_inside_the_queried_workspace(gpu, flags):
    """navsim_replan, 8 arenas x 6 pedestrians on planned routes, at most 5 queries per call: with the step's flags
    (st.ped_due), and without -- the pass that fills `due` inside the workspace."""
    E, size, N, Q = 8, 260, 6, 5
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=abi.PED_SFM, n_spawn=6, auto_reset=1,
                                 seed=23, field_format=abi.FIELD_U16T, ped_min_goal_dist=3.0, obstacle_number=6)
    gpu.world.lidar_full_circle(cfg, 180)
    occ = gpu.world.make_maps(E, size, 23, n_obstacles=6)
    nbytes = gpu.lib.load().navsim_replan_workspace_bytes(C.byref(cfg), Q)
    buf, view = _guarded(gpu, nbytes)
    sims, replanned = [], 0
    for ws in (view, _roomy(gpu, nbytes)):
        g = device_sim(gpu, cfg, occ, N, plan_paths=True, v_pref_range=(0.5, 0.6))
        g.t["replan_ws_%d" % Q] = ws
        for t in range(150):
            g.step(seeded_action(gpu, E, t))
            before = g.t["ped_n_waypoints"].clone(), g.t["ped_wp_head"].clone()
            g.replan(Q, flags=flags)
            replanned += int(((g.t["ped_n_waypoints"] != before[0]) | (g.t["ped_wp_head"] != before[1])).sum())
        sims.append(g)
    assert replanned > 0, "no pedestrian was ever re-planned"
    _guards_intact(gpu, buf, nbytes, "navsim_replan")
    _same(gpu, sims[0], sims[1], "navsim_replan")


@pytest.mark.parametrize("fused", [False, True])
def test_ped_policy_stays_inside_the_queried_workspace(gpu, fused):
    """navsim_ped_policy / navsim_ped_scan_policy, 2 arenas x 3 pedestrians with 512 beams, stand-in weights."""
    E, size, N = 2, 200, 3
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, ped_model=abi.PED_EXTERNAL, n_spawn=4,
                                 auto_reset=1, seed=7, field_format=abi.FIELD_U16T, ped_n_beams=512)
    gpu.world.lidar_full_circle(cfg, 180)
    occ = gpu.world.make_maps(E, size, 7)
    nbytes = gpu.lib.load().navsim_ped_policy_workspace_bytes(C.byref(cfg))
    buf, view = _guarded(gpu, nbytes)
    sims = []
    for ws in (view, _roomy(gpu, nbytes)):
        g = device_sim(gpu, cfg, occ, N)
        g.set_policy(policy_weights(3))
        g.t["policy_ws"] = ws
        scans = gpu.torch.zeros((E, N, 512), dtype=gpu.torch.float32, device=gpu.dev)
        for t in range(3):
            g.ped_policy(fused=fused, scans_out=scans if fused else None)
            g.step(seeded_action(gpu, E, t))
        g.t["scans_seen"] = scans if fused else g.ped_scans()
        sims.append(g)
    assert float(sims[0].t["ped_cmd"].abs().sum()) > 0.0
    _guards_intact(gpu, buf, nbytes, "navsim_ped_scan_policy" if fused else "navsim_ped_policy")
    _same(gpu, sims[0], sims[1], "navsim_ped_scan_policy" if fused else "navsim_ped_policy")


def test_build_rects_chunks_inside_the_queried_workspace(gpu):
    """navsim_build_rects, 3 maps of 100 x 100 on exactly navsim_build_rects_workspace_bytes(3, 100, 100): the call takes as
    many maps per pass as that holds; the table equals the one sim.build_rects builds on its own, larger scratch."""
    from nav_gym_amd.sim import _ptr, _stream
    E, size = 3, 100
    L = gpu.lib.load()
    occ = gpu.torch.from_numpy(gpu.world.make_maps(E, size, 5)).to(gpu.dev).contiguous()
    packed, f32, _ = gpu.sim.build_field(occ, abi.FIELD_U16T)
    expect = gpu.sim.build_rects(occ, packed, abi.FIELD_U16T, f32)
    nbytes = L.navsim_build_rects_workspace_bytes(E, size, size)
    buf, view = _guarded(gpu, nbytes)
    table = gpu.torch.zeros_like(expect)
    gpu.lib.check(L.navsim_build_rects(_ptr(occ), E, size, size, _ptr(packed), abi.FIELD_U16T, _ptr(f32), _ptr(table), _ptr(view),
                                       nbytes, _stream()), "navsim_build_rects")
    _guards_intact(gpu, buf, nbytes, "navsim_build_rects")
    assert gpu.torch.equal(table, expect)
    # one map's worth less than a single map needs: refused, nothing launched
    assert L.navsim_build_rects(_ptr(occ), E, size, size, _ptr(packed), abi.FIELD_U16T, _ptr(f32), _ptr(table), _ptr(view),
                                9 * size * size - 1, _stream()) == abi.E_ARG
