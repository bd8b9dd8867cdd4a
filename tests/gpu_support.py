"""What the GPU tests share: the `gpu` fixture, host <-> device copies, the two comparisons (by value, by bits), the same
world in NavSim and in the oracle, the rollouts' random actions, and raw navsim_state structs for the calls that take one.
A plain module (tests/ is on sys.path): test files import from here, never from each other."""
import numpy as np
import pytest

import ref
from helpers import footprints
from nav_gym_amd import abi

TOL = 1e-5   # north_star tolerance on ranges / pose (the tests assert equality, which is stricter)

NOT_STATE = ("field", "field_overflow", "rect_table", "rect_index")      # device-only forms of the map: the oracle reads its own field


@pytest.fixture(scope="module")
def gpu():
    import torch
    from nav_gym_amd import lib, sim, world
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    lib.load()
    return type("G", (), dict(torch=torch, lib=lib, sim=sim, world=world, dev=torch.device("cuda:0")))


def to_device(gpu, a, dtype=None):
    t = gpu.torch.from_numpy(np.ascontiguousarray(a)).to(gpu.dev)
    return t if dtype is None else t.to(dtype)


def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- comparisons (pinned by tests/test_support.py) ---------------------------------------------------------------------------
def eq(a, b, what):
    """Equal by VALUE (np.array_equal): NaN differs from NaN, -0.0 equals 0.0.  same_bits is the comparison of raw bits."""
    a = np.asarray(a); b = np.asarray(b)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        diff = np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))
        at = tuple(bad[0])
        raise AssertionError("%s: %d mismatches, max |diff| %.3e (north_star tol %g), first at %s: %r != %r"
                             % (what, len(bad), diff, TOL, bad[0], a[at], b[at]))


def same_bits(a, b, what):
    """Equal dtype, shape and BITS (through the unsigned view of the item size): -0.0 differs from 0.0, a NaN equals itself."""
    a = np.asarray(a); b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s %s against %s %s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    u = np.dtype("u%d" % a.dtype.itemsize)
    eq(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u), what)


def state_equal(g, r, what, skip=(), live_waypoints_only=False):
    """Every state array the oracle holds against NavSim's, by value.  live_waypoints_only: ped_waypoints up to ped_n_waypoints
    (after a re-plan the slots beyond a route's length keep whatever the buffer held before).  Returns NavSim's arrays as read."""
    gs = g.numpy_state()
    for k, v in r.a.items():
        if k not in gs or k in NOT_STATE or k in skip:
            continue
        if k == "ped_waypoints" and live_waypoints_only:
            live = np.arange(v.shape[2])[None, None, :] < r.a["ped_n_waypoints"][..., None]
            eq(gs[k][live], v[live], "state %s %s" % (k, what))
        else:
            eq(gs[k], v, "state %s %s" % (k, what))
    return gs


# ---- the same world on the device and in the oracle --------------------------------------------------------------------------
def keti_thresholds(gpu, cfg):
    """(scan_threshold, scan_discomfort) of the Keti footprints on the device; helpers.keti_thresholds is the host twin."""
    return tuple(gpu.sim.scan_threshold(cfg, to_device(gpu, fp)) for fp in footprints())


def device_world(gpu, cfg, occ, n_peds, thr=None, dthr=None, robot="keti", **world_kw):
    """world.make_world on the device plus the thresholds of the robot's footprints (thr / dthr: float32 [B] arrays in their place)."""
    arrays = gpu.world.make_world(cfg, occ, n_peds=n_peds, device=gpu.dev, **world_kw)
    for key, fp, given in zip(("scan_threshold", "scan_discomfort"), footprints(robot), (thr, dthr)):
        arrays[key] = gpu.sim.scan_threshold(cfg, to_device(gpu, fp)) if given is None else to_device(gpu, given)
    return arrays


def host_arrays(arrays, occ):
    """The oracle's copy of a device world: every array but the device-only forms of the map, and its own float32 field."""
    host = {k: v.cpu().numpy() for k, v in arrays.items() if k not in NOT_STATE}
    host["field"] = ref.build_dt(occ)
    return host


def sim_and_oracle(gpu, cfg, occ, n_peds, final_obs=False, check_reset=True, **world_kw):
    """The same world in NavSim and in RefSim -> (g, r, host); the first observations are compared unless check_reset is False
    (then neither side has scanned yet)."""
    arrays = device_world(gpu, cfg, occ, n_peds, **world_kw)
    host = host_arrays(arrays, occ)
    g = gpu.sim.NavSim(cfg, arrays, final_obs=final_obs)
    r = ref.RefSim(cfg, host)
    if check_reset:
        eq(g.reset_obs().cpu().numpy(), r.reset_obs(), "reset obs")
    return g, r, host


def random_actions(rng, E, t=None):
    """One row of actions per arena; at every seventh step t a burst of straight driving, which provokes crashes (t None: none)."""
    act = np.stack([rng.uniform(0.0, 0.5, E), rng.uniform(-0.64, 0.64, E)], axis=1)
    if t is not None and t % 7 == 3:
        act[:, 0] = 0.5; act[:, 1] = 0.0
    return act


def rollout_pair(gpu, cfg, occ, n_peds, steps, seed, policy=None, **world_kw):
    """Runs the same world through the HIP step and the oracle; yields (t, obs, outputs, oracle obs, oracle outputs, g, r) per
    step.  policy: HumanPolicy weights -> pedestrians are driven by navsim_ped_policy on both sides."""
    g, r, _ = sim_and_oracle(gpu, cfg, occ, n_peds, **world_kw)
    rng = np.random.default_rng(seed)
    E = cfg.n_envs
    for t in range(steps):
        act = random_actions(rng, E, t)
        if policy is not None:
            if t == 0:
                g.set_policy(policy)
            g.ped_policy(); r.ped_policy(policy)
        elif cfg.ped_model == abi.PED_EXTERNAL:
            cmd = np.stack([rng.uniform(0, 0.6, (E, cfg.max_peds)), rng.uniform(-0.6, 0.6, (E, cfg.max_peds))], axis=2)
            g.set_ped_cmd(cmd); r.set_ped_cmd(cmd)
        go, gout = g.step(to_device(gpu, act))
        ro, rout = r.step(act)
        yield t, go.cpu().numpy(), to_numpy(gout), ro, rout, g, r


def device_sim(gpu, cfg, occ, n_peds, **world_kw):
    """A NavSim alone, first observation taken, on a copy of cfg (make_world notes in it whether the maps are closed)."""
    cfg = cfg.copy()
    g = gpu.sim.NavSim(cfg, device_world(gpu, cfg, occ, n_peds, **world_kw))
    g.reset_obs()
    return g


def seeded_action(gpu, E, seed):
    return to_device(gpu, random_actions(np.random.default_rng(seed), E))


def regen_layout(gpu, layout):
    """(cfg, occ, pedestrians, make_world keywords) of the three navsim_regen layouts"""
    kw = dict(auto_reset=1, n_spawn=6, seed=31, min_goal_dist=3.0, max_goal_dist=8.0, spawn_clearance=0.9,
              ped_min_robot_dist=2.0, ped_min_goal_dist=4.0)
    if layout == "packed-corridors-planned":            # distance transform, rect builder, the fork, both planner stages
        E, size = 12, 260
        cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=6, ped_model=abi.PED_SFM, regen_cap=3,
                                     field_format=abi.FIELD_U16T, regen_plan=1, regen_indoor_ratio=0.5, **kw)
        occ, n_peds, wkw = gpu.world.make_maps(E, size, 31), 5, dict(plan_paths=True)
    elif layout == "float32-smallest":
        E, size = 12, 200
        cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=1, ped_model=abi.PED_NONE, regen_cap=3,
                                     field_format=abi.FIELD_F32, regen_plan=0, regen_indoor_ratio=0.0, **kw)
        occ, n_peds, wkw = gpu.world.make_maps(E, size, 31), 0, {}
    else:                                               # "packed-overflow-plane": its scratch exists above 520 cells per side only
        E, size = 4, 528
        cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=1, ped_model=abi.PED_NONE, regen_cap=2,
                                     field_format=abi.FIELD_U16T, regen_plan=0, regen_indoor_ratio=0.0, **kw)
        occ = np.zeros((E, size, size), np.uint8)       # 259 free cells from the border wall to the centre: the field saturates
        occ[:, :5] = 1; occ[:, -5:] = 1; occ[:, :, :5] = 1; occ[:, :, -5:] = 1
        occ[:, 40:60, 40:60] = 1
        n_peds, wkw = 0, {}
    gpu.world.lidar_full_circle(cfg, 180)
    return cfg, occ, n_peds, wkw


# ---- one world under several simulators: the 48-arena world of the time-limit and ORCA tests, and NavGym-v0 beside it ----------
def limit_config(gpu, mode, ped_model=abi.PED_NONE, S=2, fmt=abi.FIELD_U16T, T=0, E=48, size=240, N=8, **kw):
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=S, ped_model=ped_model,
                                 auto_reset=mode, n_spawn=8, seed=4343, field_format=fmt, **kw)
    gpu.world.lidar_1081(cfg)
    cfg.max_episode_steps = T
    return cfg


def limit_world(gpu, cfg, occ=None, n_peds=6, **world_kw):
    """-> (device arrays, host arrays) to build several simulators from: fresh_sim clones the former, fresh_oracle copies the
    latter.  The host copy carries done_steps (also under NAVSIM_AUTORESET_NONE: restart_state records it)."""
    if occ is None:
        occ = gpu.world.make_maps(cfg.n_envs, cfg.map_h, 4343)
    arrays = device_world(gpu, cfg, occ, n_peds, **dict(dict(min_goal_dist=1.5, max_goal_dist=4.0), **world_kw))
    host = host_arrays(arrays, occ)
    host["done_steps"] = np.zeros(cfg.n_envs, np.int32)
    return arrays, host


def fresh_sim(gpu, cfg, arrays, final_obs=False):
    g = gpu.sim.NavSim(cfg, {k: v.clone() for k, v in arrays.items()}, final_obs=final_obs)
    g.reset_obs()
    return g


def fresh_oracle(cfg, host, mode=None):
    c = cfg.copy()
    if mode is not None:
        c.auto_reset = mode
    r = ref.RefSim(c, {k: v.copy() for k, v in host.items()})
    r.reset_obs()
    return r


def nav_env(**kw):
    from nav_gym_amd import registry
    base = dict(num_envs=48, map_size=200, n_beams=256, seed=23, plan_paths=False, min_goal_dist=2.0, max_goal_dist=6.0,
                indoor_ratio=0.0, num_humans=3)
    base.update(kw)
    return registry.make("NavGym-v0", **base)


def action_rows(K, E, seed=2):
    rng = np.random.default_rng(seed)
    return [random_actions(rng, E) for _ in range(K)]


def env_rollout(env, acts):
    """reset() and one step per row of acts -> [first observation, dict(obs, rew, done, trunc[, final][, reset]) per step]"""
    import torch
    obs = env.reset()
    rec = [obs["observation"].clone()]
    for act in acts:
        o, rew, done, info = env.step(act)
        item = dict(obs=o["observation"].clone(), rew=rew.clone(), done=done.clone())
        item["trunc"] = info["TimeLimit.truncated"].clone() if "TimeLimit.truncated" in info else torch.zeros_like(done)
        if "final_observation" in info:
            item["final"] = info["final_observation"]["observation"].clone()
        if "reset_mask" in info:
            item["reset"] = info["reset_mask"].clone()
        rec.append(item)
    torch.cuda.synchronize()
    return rec


# ---- the small worlds of the navsim_ped_orca tests ------------------------------------------------------------------------------
ORCA_SENTINEL = -7.25          # ped_cmd before a call: dead rows must still hold it afterwards


def small_orca_config(gpu, E, N, size=240, mode=abi.AUTORESET_SAME_STEP):
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=1, ped_model=abi.PED_EXTERNAL,
                                 auto_reset=mode, n_spawn=8, seed=4343, field_format=abi.FIELD_U16T)
    gpu.world.lidar_full_circle(cfg, 64)
    return cfg


def orca_pair(gpu, cfg, n_peds, moving=True, hand_made=None, **world_kw):
    """The same world on the device and in the oracle; moving: pedestrians and robots already have velocities."""
    occ = gpu.world.make_maps(cfg.n_envs, cfg.map_h, 4343)
    arrays, host = limit_world(gpu, cfg, occ, n_peds=n_peds, v_pref_range=(0.3, 0.6), **world_kw)
    if hand_made is not None:
        hand_made(host)
        for k in ("ped_waypoints", "ped_n_waypoints"):
            arrays[k] = to_device(gpu, host[k])
    g, r = fresh_sim(gpu, cfg, arrays), fresh_oracle(cfg, host)
    if moving:                                                       # (after the first observation, which clears prev_action)
        rng = np.random.default_rng(11)
        vel = rng.uniform(-0.5, 0.5, host["ped_vel"].shape)
        prev = random_actions(rng, cfg.n_envs)
        g.t["ped_vel"].copy_(to_device(gpu, vel)); r.a["ped_vel"][...] = vel
        g.t["prev_action"].copy_(to_device(gpu, prev)); r.a["prev_action"][...] = prev
    return g, r


# ---- raw states for the calls that take a navsim_state ------------------------------------------------------------------------
def device_field(gpu, cfg, occ_t, overflow=False):
    """The field of occ in cfg.field_format -> {"field": ..., ["field_overflow": ...]}.  overflow True / False: the packed field
    must / must not saturate somewhere; None: as it comes."""
    if cfg.field_format == abi.FIELD_F32:
        return {"field": gpu.sim.build_dt(occ_t)}
    field, plane, nsat = gpu.sim.build_field(occ_t, abi.FIELD_U16T)
    assert overflow is None or (nsat > 0) == overflow, nsat
    return {"field": field, "field_overflow": plane} if nsat > 0 else {"field": field}


def device_state(gpu, cfg, occ, w, keys, overflow=False, map_slot=None):
    """navsim_state over device copies of the arrays `keys` ({name: dtype}) of the world `w` and the field of `occ` [M,H,W] in
    cfg.field_format (overflow: see device_field).  -> (st, keepalive)"""
    keep = {k: to_device(gpu, np.ascontiguousarray(w[k], dtype=dt)) for k, dt in keys.items()}
    keep.update(device_field(gpu, cfg, to_device(gpu, occ), overflow))
    if map_slot is not None:
        keep["map_slot"] = to_device(gpu, np.asarray(map_slot, np.int32))
    st = abi.NavsimState()
    for k, v in keep.items():
        setattr(st, k, v.data_ptr())
    return st, keep


def device_map_arrays(gpu, cfg, occ, world, rects):
    """The world's arrays with the field, and if `rects` the record table and index rows, the device builds from occ, in
    world.make_world's order (field, records, index rows, closed_maps).  Sets cfg.closed_maps."""
    occ_t = to_device(gpu, occ)
    a = {k: v for k, v in world.items() if k != "field"}
    packed, f32, nsat = gpu.sim.build_field(occ_t, cfg.field_format)
    a["field"] = packed
    assert nsat == 0
    if rects and cfg.field_format != abi.FIELD_F32:
        a["rect_table"] = gpu.sim.build_rects(occ_t, packed, cfg.field_format, f32)
        a["rect_index"], _ = gpu.sim.build_rect_index(a["rect_table"], occ.shape[1], occ.shape[2])
        cfg.closed_maps = int(bool((gpu.sim.maps_closed(occ_t) == 1).all().item()))
    return a


# ---- the record table and its index, decoded on the host -----------------------------------------------------------------------
def decode_rect_table(table, H, W):
    """Host evaluation of navsim_build_rects records: -> (d2 int64 [E,H,W], valid bool [E,H,W])."""
    E = table.shape[0]
    tpr = (W + 7) // 8
    rec = table.view(np.uint32).reshape(E, -1, 4)
    yy, xx = np.mgrid[0:H, 0:W]
    tile = (yy // 8) * tpr + (xx // 8)
    r = rec[:, tile]                                            # [E,H,W,4]
    def sx(w): return (w & 0xFFFF).astype(np.int16).astype(np.int64)
    def sy(w): return (w >> 16).astype(np.int16).astype(np.int64)
    def dist2(lo, hi):
        ddx = np.maximum(0, np.maximum(sx(lo) - xx, xx - sx(hi)))
        ddy = np.maximum(0, np.maximum(sy(lo) - yy, yy - sy(hi)))
        return ddx * ddx + ddy * ddy
    d2 = np.minimum(dist2(r[..., 0], r[..., 1]), dist2(r[..., 2], r[..., 3]))
    valid = (r[..., 0] & 0xFFFF) != 0x7FFF
    return d2, valid


def decode_rect_index(rows, H, W):
    """Host evaluation of the index form (navsim_build_rect_index): rows uint8 [E, R] -> the 16-byte records it stands for
    (uint32 [E, T, 4]) and which tiles carry an index."""
    E = rows.shape[0]
    T_ = ((H + 7) // 8) * ((W + 7) // 8)
    lst = rows[:, :2048].copy().view(np.uint32).reshape(E, 256, 2)
    pair = rows[:, 2048:2048 + 2 * T_].copy().view(np.uint16).reshape(E, T_)
    has = pair != 0xFFFF
    ia, ib = (pair & 0xFF).astype(np.int64), (pair >> 8).astype(np.int64)
    rec = np.zeros((E, T_, 4), np.uint32)
    ar = np.arange(E)[:, None]
    rec[..., 0:2] = lst[ar, ia]; rec[..., 2:4] = lst[ar, ib]
    return rec, has


def rect_pairs(rows, H, W):
    """navsim_state.rect_index decoded: the two rectangles every tile names (-1: none).  Which list index a rectangle gets
    depends on the order its workgroup's threads insert it (kernels_rect.hpp rect_index_kernel); what a tile names does not."""
    rows = rows.cpu().numpy()
    T = ((H + 7) // 8) * ((W + 7) // 8)
    lst = np.ascontiguousarray(rows[:, :256 * 8]).view(np.int64)                     # [E, 256]
    pair = np.ascontiguousarray(rows[:, 256 * 8:256 * 8 + 2 * T]).view(np.uint16)    # [E, T]: A | B << 8
    both = np.stack([np.take_along_axis(lst, (pair & 0xFF).astype(np.int64), 1),
                     np.take_along_axis(lst, (pair >> 8).astype(np.int64), 1)], axis=2)
    both[pair == 0xFFFF] = -1
    return both
