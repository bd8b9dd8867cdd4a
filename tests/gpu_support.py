"""What the GPU tests share: the `gpu` fixture, host <-> device copies, the two comparisons (by value, by bits), the same
world in NavSim and in the oracle, the rollouts' random actions, raw navsim_state structs for the calls that take one, and the
worlds and the expected step of the scan-noise tests (NoisyStep: oracle for the clean scans, tests/scan_noise_f64.py for the draws).
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


# ---- scan noise: the worlds of tests/test_scan_noise.py and tests/test_gpu_scan_noise.py, and what a noisy step must return ------
NOISE_E, NOISE_STEPS = 24, 30
NOISE_CAP = 0.01               # share of a case's arena-steps whose crash the model may leave undecided (within TOL of a threshold)
NOISE_CASES = {                # (the table of the tests' module docstrings: both finish paths, every key)
    "none-fan77-f32": dict(mode=abi.AUTORESET_NONE, S=1, B=77, fan=True, ped_model=abi.PED_NONE, N=1, n_peds=0, step_block=64,
                           fmt=abi.FIELD_F32, size=160, seed=515, base=0, T=0),
    "same-circle200-sfm": dict(mode=abi.AUTORESET_SAME_STEP, S=3, B=200, fan=False, ped_model=abi.PED_SFM, N=6, n_peds=5, step_block=256,
                               fmt=abi.FIELD_U16T, size=200, seed=2 ** 40 + 99, base=1000, T=0),
    "next-fan1081-external": dict(mode=abi.AUTORESET_NEXT_STEP, S=2, B=1081, fan=True, ped_model=abi.PED_EXTERNAL, N=4, n_peds=4,
                                  step_block=0, fmt=abi.FIELD_U16T, size=180, seed=616, base=0, T=0),
    "same-fan77-limit7": dict(mode=abi.AUTORESET_SAME_STEP, S=2, B=77, fan=True, ped_model=abi.PED_NONE, N=1, n_peds=0, step_block=256,
                              fmt=abi.FIELD_U16T, size=160, seed=717, base=0, T=7),
}


def noise_world(default_config, name):
    """-> (cfg, occ, host): a case of NOISE_CASES as host arrays (NumPy; the field is the oracle's), the same on a machine with and
    without a GPU.  Lidar range 3 m on 8-10 m maps: a good share of the beams ends at range_max.  Arena 0 has no noise, the
    others a std in (0, 0.05], unsorted.  Starts 0.5 m clear of the walls and goals 1.5-4 m away: robots crash, arrive and come
    close to walls within 30 steps; every other goal lies 0.8 m ahead of its start."""
    from nav_gym_amd import world
    c = NOISE_CASES[name]
    E, N, size, K = NOISE_E, c["N"], c["size"], 8
    cfg = default_config(n_envs=E, map_h=size, map_w=size, max_peds=N, n_scan_stack=c["S"], ped_model=c["ped_model"], auto_reset=c["mode"],
                         n_spawn=K, seed=c["seed"], field_format=c["fmt"], step_block=c["step_block"], add_scan_noise=1, range_max=3.0,
                         env_index_base=c["base"], lidar_legs=1)
    cfg.max_episode_steps = c["T"]
    if c["fan"]:
        world.lidar_1081(cfg); cfg.n_beams = c["B"]
    else:
        world.lidar_full_circle(cfg, c["B"])
    small = int(c["seed"] % 1000)
    occ = world.make_maps(E, size, small)
    field = ref.build_dt(occ)
    res = cfg.resolution
    rng = np.random.default_rng(small)

    def centres(cells):
        return np.stack([(cells % size + 0.5) * res + cfg.origin_x, (cells // size + 0.5) * res + cfg.origin_y], axis=-1)
    h = dict(field=field, spawn_pose=np.zeros((E, K, 3)), spawn_goal=np.zeros((E, K, 2)))
    for e in range(E):
        free = np.flatnonzero(field[e].ravel() >= 0.5 / res)
        xy = centres(free)
        for k in range(K):
            s = xy[rng.integers(len(xy))]
            d = np.hypot(*(xy - s).T)
            ok = np.flatnonzero((d > 1.5) & (d < 4.0))
            th = rng.uniform(0.0, 2.0 * np.pi)
            h["spawn_pose"][e, k] = (s[0], s[1], th)
            h["spawn_goal"][e, k] = xy[ok[rng.integers(len(ok))]] if len(ok) else xy[np.argmax(d)]
            if k % 2 == 0:                                          # every other goal 0.8 m ahead of its start: reached in a few steps
                h["spawn_goal"][e, k] = (s[0] + 0.8 * np.cos(th), s[1] + 0.8 * np.sin(th))
    h["robot_pose"], h["robot_goal"] = h["spawn_pose"][:, 0].copy(), h["spawn_goal"][:, 0].copy()
    h["prev_action"], h["prev_pose"] = np.zeros((E, 2)), np.zeros((E, 3))
    h["n_hist"], h["episode"], h["steps"] = np.zeros(E, np.int32), np.zeros(E, np.int64), np.zeros(E, np.int64)
    h["done_steps"] = np.zeros(E, np.int32)
    std = (0.05 * (1.0 - rng.random(E))).astype(np.float32)
    std[0] = 0.0
    h["scan_noise_std"] = std
    h["scan_threshold"], h["scan_discomfort"] = (ref.scan_threshold(cfg, fp) for fp in footprints())
    if c["ped_model"] != abi.PED_NONE:
        P = cfg.max_waypoints
        h["n_peds"] = np.full(E, c["n_peds"], np.int32)
        h["ped_pose"], h["ped_goal"] = np.zeros((E, N, 3)), np.zeros((E, N, 2))
        for e in range(E):
            xy = centres(np.flatnonzero(field[e].ravel() >= 0.5 / res))
            near = xy[np.hypot(*(xy - h["robot_pose"][e, :2]).T) < 3.0]      # in the lidar's range of the first start
            for i in range(N):
                p = near[rng.integers(len(near))]
                h["ped_pose"][e, i] = (p[0], p[1], rng.uniform(0.0, 2.0 * np.pi))
                h["ped_goal"][e, i] = xy[rng.integers(len(xy))]
        h["ped_vel"], h["ped_prev_yaw"], h["ped_dist"] = np.zeros((E, N, 2)), np.zeros((E, N)), np.zeros((E, N, 3))
        h["ped_v_pref"] = rng.uniform(0.3, 0.6, (E, N))
        h["ped_has_legs"] = (rng.random((E, N)) < 0.5).astype(np.uint8)
        h["ped_waypoints"] = np.zeros((E, N, P, 2)); h["ped_waypoints"][:, :, 0] = h["ped_goal"]
        h["ped_n_waypoints"], h["ped_wp_head"] = np.ones((E, N), np.int32), np.zeros((E, N), np.int32)
        h["ped_cmd"] = np.zeros((E, N, 2))
    return cfg, occ, h


def noise_inputs(cfg, rng, t):
    """(action [E,2], ped_cmd [E,N,2] or None) of step t: random_actions with its crash bursts, commands for PED_EXTERNAL"""
    act = random_actions(rng, cfg.n_envs, t)
    cmd = None
    if cfg.ped_model == abi.PED_EXTERNAL:
        cmd = np.stack([rng.uniform(0, 0.6, (cfg.n_envs, cfg.max_peds)), rng.uniform(-0.6, 0.6, (cfg.n_envs, cfg.max_peds))], axis=2)
    return act, cmd


class NoisyStep(object):
    """What one step of a world with scan noise must return, from the state before it: the oracle supplies every CLEAN scan and
    every noise-free output, tests/scan_noise_f64.py every draw, and the model's noisy first scan alone decides the branch.

    Two oracles without noise, restart or time limit, stepped from the same snapshot.  `free` has thresholds 0: it never
    crashes, so its newest scan slot is the clean first scan at the integrated pose (C1) and its state and outputs are those of
    a step without a crash.  `crashed` has thresholds +inf: it always crashes, so its newest slot is the clean re-scan at its
    prev_pose with the pedestrians where the step left them -- the crash re-scan (C2) from the snapshot's prev_pose (the pose the
    step reverts to: robot_pose with its yaw wrapped, which rounds to another float32 heading above pi), and with prev_pose set
    to a start pose the first scan of an arena that restarts inside the step (C3; the step keeps the leg phases
    there, which a reset_obs would clear).  Arenas that a call RESETS (NEXT_STEP's reset_mask) take `free`'s reset_obs."""
    SKIP = NOT_STATE + ("scan_threshold", "scan_discomfort", "counters")

    def __init__(self, cfg, host):
        import scan_noise_f64 as model
        self.model = model
        self.cfg = cfg
        c = cfg.copy()
        c.auto_reset, c.add_scan_noise, c.max_episode_steps = abi.AUTORESET_NONE, 0, 0
        B = cfg.n_beams
        self.thr, self.dthr = host["scan_threshold"].astype(np.float32), host["scan_discomfort"].astype(np.float32)
        self.free = ref.RefSim(c, dict(host, scan_threshold=np.zeros(B, np.float32), scan_discomfort=np.zeros(B, np.float32)))
        self.crashed = ref.RefSim(c, dict(host, scan_threshold=np.full(B, np.inf, np.float32), scan_discomfort=np.full(B, np.inf, np.float32)))
        self.keys = [k for k in self.free.a if k not in self.SKIP]

    def _load(self, r, state, obs):
        for k in self.keys:
            if k in state:
                r.a[k][...] = state[k]
        r.obs[r.cur][...] = obs

    def _snap(self, r):
        return {k: r.a[k].copy() for k in self.keys}

    def stream(self, e, key):
        return self.model.noise_stream(int(self.cfg.seed), int(self.cfg.env_index_base) + e, key)

    def noisy(self, clean, e, std, key):
        return self.model.noisy(clean, std, self.stream(e, key), np.float32(self.cfg.range_max))

    def first_obs(self, state, obs):
        """The first observation of every arena from `state` (reset_obs): -> (scan float64 [E,S,B], clean float32 [E,B], tail)"""
        cfg = self.cfg
        E, S, B = cfg.n_envs, cfg.n_scan_stack, cfg.n_beams
        self._load(self.free, state, obs)
        row = self.free.reset_obs().copy()
        clean = row[:, (S - 1) * B:S * B]
        scan = np.stack([self.noisy(clean[e], e, state["scan_noise_std"][e], self.model.first_obs_key(state["episode"][e]))
                         for e in range(E)])
        return np.repeat(scan[:, None, :], S, axis=1), clean, row[:, S * B:], self._snap(self.free)

    def reward(self, x, e, crash, row32):
        """reward_scalar's sum in float64, in its order; the discomfort term from the float32 row the step returned"""
        c = self.cfg
        dist, prev_dist, vel = x["distance_f64"][e], x["prev_distance"][e], x["vel"][e]
        success = dist < c.distance_threshold
        disc, rmin = False, 0.0
        if not crash:
            disc = bool((row32 < self.dthr).any())
            den = ((self.dthr - self.thr) + np.float32(1e-6)).astype(np.float64)
            rmin = float(np.min((row32.astype(np.float64) - self.thr.astype(np.float64)) / den))
        r_success = 1.0 * c.reward_success_factor * c.reward_scale if success else 0.0
        r_crash = -1.0 * c.reward_crash_factor * c.reward_scale if crash else 0.0
        r_progress = (prev_dist - dist) * c.reward_progress_factor * c.reward_scale
        r_forward = vel[0] * c.reward_forward_factor * c.reward_scale
        r_rotation = -1.0 * (vel[1] * vel[1]) * c.reward_rotation_factor * c.reward_scale
        r_discomfort = -(1.0 - rmin) * c.reward_discomfort_factor * c.reward_scale if disc else 0.0
        return r_success + r_crash + r_progress + r_forward + r_rotation + r_discomfort

    def expect(self, state, obs, act, pending=None):
        """state: every state array before the step; obs [E,D]: the observation before it; pending: NEXT_STEP's reset mask.
        -> dict: per arena crash / undecided / success / trunc / done / restarted / fresh (the row is a first observation);
        view_scan [E,S,B] float64 + view_tail: the ended or continuing episode's row (obs, or final_obs of a restarted arena);
        obs_scan / obs_tail: the row of `obs`; exact [E,S,B]: entries that must match bit for bit; state: the state after it."""
        cfg, m = self.cfg, self.model
        E, S, B, T = cfg.n_envs, cfg.n_scan_stack, cfg.n_beams, cfg.max_episode_steps
        mode = cfg.auto_reset
        pending = np.zeros(E, bool) if pending is None else np.asarray(pending) != 0
        std = state["scan_noise_std"]
        new = slice((S - 1) * B, S * B)
        self._load(self.free, state, obs)
        oa = self.free.step(act)[0].copy()
        outa, sa = {k: v.copy() for k, v in self.free.out.items()}, self._snap(self.free)
        self._load(self.crashed, state, obs)
        ok = self.crashed.step(act)[0].copy()
        outk, sk = {k: v.copy() for k, v in self.crashed.out.items()}, self._snap(self.crashed)
        x = dict(crash=np.zeros(E, bool), undecided=np.zeros(E, bool), margin=np.zeros(E), crossed=np.zeros(E, bool))
        row = np.zeros((E, B)); clean = np.zeros((E, B), np.float32)
        steps_now = state["steps"] + 1
        for e in np.flatnonzero(~pending):
            key = m.step_key(state["episode"][e], steps_now[e])
            m1 = self.noisy(oa[e, new], e, std[e], key)
            x["margin"][e] = np.min(m1 - self.thr.astype(np.float64))
            x["crash"][e] = x["margin"][e] < 0.0
            x["undecided"][e] = abs(x["margin"][e]) <= TOL
            c1 = oa[e, new]
            x["crossed"][e] = bool(((m1 > cfg.range_max) | ((m1 < self.thr) != (c1 < self.thr)) | ((m1 < self.dthr) != (c1 < self.dthr))).any())
            if x["crash"][e]:
                clean[e] = ok[e, new]; row[e] = self.noisy(ok[e, new], e, std[e], key + 1)
            else:
                clean[e] = c1; row[e] = m1
        crash = x["crash"]
        x["success"] = (outa["is_success"] != 0) & ~pending
        done = (x["success"] | crash) & ~pending
        x["trunc"] = (~done & (steps_now >= T) & ~pending) if T > 0 else np.zeros(E, bool)
        x["done"] = done | x["trunc"]
        restart = x["done"] & (mode != abi.AUTORESET_NONE) & (cfg.n_spawn > 0)
        x["restarted"] = restart & (mode == abi.AUTORESET_SAME_STEP)
        x["fresh"] = x["restarted"] | pending
        x["pending"] = pending
        # the noise-free parts: reward inputs (pose: the integrated one, also after a crash), distance, goals, tails, state
        goal, p = state["robot_goal"], sa["robot_pose"]
        dx, dy = goal[:, 0] - p[:, 0], goal[:, 1] - p[:, 1]
        x["distance_f64"] = np.sqrt(dx * dx + dy * dy)
        px, py = goal[:, 0] - state["prev_pose"][:, 0], goal[:, 1] - state["prev_pose"][:, 1]
        x["prev_distance"] = np.sqrt(px * px + py * py)
        x["vel"] = state["prev_action"]
        x["out"] = {k: np.where(crash.reshape((E,) + (1,) * (outa[k].ndim - 1)), outk[k], outa[k])
                    for k in ("distance", "is_success", "achieved_goal", "desired_goal")}
        x["view_goals"] = np.concatenate([x["out"]["achieved_goal"], x["out"]["desired_goal"]], axis=1)
        n_hist = state["n_hist"]
        x["old"] = (S - 1 - np.arange(S)[None, :] <= n_hist[:, None]) & (np.arange(S)[None, :] < S - 1)      # [E,S]: slot j is history
        prev = obs[:, :S * B].reshape(E, S, B)
        shifted = np.concatenate([prev[:, 1:], prev[:, -1:]], axis=1).astype(np.float64)
        x["view_scan"] = np.where(x["old"][:, :, None], shifted, row[:, None, :])
        x["view_clean"] = clean
        x["view_tail"] = np.where(crash[:, None], ok[:, S * B:], oa[:, S * B:])
        post = {k: np.where(crash.reshape((E,) + (1,) * (sa[k].ndim - 1)), sk[k], sa[k]) for k in self.keys}
        x["obs_scan"], x["obs_tail"], x["obs_clean"] = x["view_scan"].copy(), x["view_tail"].copy(), clean.copy()
        if restart.any():                                           # the next start / goal pair, the next episode number
            self._load(self.free, post, obs)
            mask = np.ascontiguousarray(restart, dtype=np.uint8)
            L = ref.lib()
            L.navsim_restart_cpu.argtypes = [ref.C.POINTER(abi.NavsimConfig), ref.C.POINTER(abi.NavsimState), ref.C.c_void_p]
            assert L.navsim_restart_cpu(ref.C.byref(self.free.cfg), ref.C.byref(self.free.st), mask.ctypes.data_as(ref.C.c_void_p)) == 0
            post = self._snap(self.free)
        if x["restarted"].any():
            # the first observation of the new episode, scanned inside the step: tail, goals and robot state as reset_obs gives
            # them, the pedestrians' leg phases as the step left them, the clean scan from `crashed` standing on the start pose
            who = x["restarted"]
            self.free.reset_obs(np.ascontiguousarray(who, dtype=np.uint8))
            fresh_row, fresh_state = self.free.obs[self.free.cur].copy(), self._snap(self.free)
            for k in self.keys:
                if k not in ("ped_dist", "ped_prev_yaw"):
                    post[k][who] = fresh_state[k][who]
            for k in ("achieved_goal", "desired_goal"):
                x["out"][k] = np.where(who[:, None], self.free.out[k], x["out"][k])
            start = dict(state)
            start["prev_pose"] = np.where(who[:, None], post["robot_pose"], state["prev_pose"])
            self._load(self.crashed, start, obs)
            c3 = self.crashed.step(act)[0][:, new].copy()
            for e in np.flatnonzero(who):
                x["obs_scan"][e] = self.noisy(c3[e], e, std[e], m.first_obs_key(post["episode"][e]))[None, :]
                x["obs_clean"][e] = c3[e]
                x["obs_tail"][e] = fresh_row[e, S * B:]
        if pending.any():                                           # NEXT_STEP: this call resets them
            scan, cl, tail, st1 = self.first_obs(state, obs)
            for k in self.keys:
                post[k][pending] = st1[k][pending]
            x["obs_scan"][pending], x["obs_clean"][pending], x["obs_tail"][pending] = scan[pending], cl[pending], tail[pending]
            for k in ("achieved_goal", "desired_goal"):
                x["out"][k] = np.where(pending[:, None], self.free.out[k], x["out"][k])
            for k in ("distance", "is_success"):
                x["out"][k] = np.where(pending, 0, x["out"][k])
            if "ped_due" in post:
                post["ped_due"][pending] = 0
        x["state"] = post
        return x


def noise_emulation(cfg, host, steps=NOISE_STEPS, seed=5):
    """The case's rollout with NoisyStep in the device's place (every row rounded to float32 as the device stores it): yields
    (t, x, clean beams that count) per step.  What the CPU test measures a case's coverage and tie rate on."""
    E, S, B = cfg.n_envs, cfg.n_scan_stack, cfg.n_beams
    ns = NoisyStep(cfg, host)
    state = {k: np.array(v) for k, v in host.items() if k not in NoisyStep.SKIP}
    if "ped_waypoints" in state:
        state["ped_due"] = np.zeros(E, np.int64)
    scan, clean, tail, state1 = ns.first_obs(state, np.zeros((E, S * B + abi.OBS_TAIL), np.float32))
    state.update(state1)
    obs = np.concatenate([scan.reshape(E, S * B).astype(np.float32), tail], axis=1)
    rng = np.random.default_rng(seed)
    done = np.zeros(E, bool)
    for t in range(steps):
        act, cmd = noise_inputs(cfg, rng, t)
        if cmd is not None:
            state["ped_cmd"] = cmd
        pending = done if cfg.auto_reset == abi.AUTORESET_NEXT_STEP else None
        x = ns.expect(state, obs, act, pending)
        x["inputs"] = (act, cmd)
        x["reward_of"] = lambda e, crash, row32, x=x: ns.reward(x, e, crash, row32)
        yield t, x
        state.update(x["state"])
        obs = np.concatenate([x["obs_scan"].reshape(E, S * B).astype(np.float32), x["obs_tail"]], axis=1)
        done = x["done"]


def noise_coverage(n, x, range_max):
    """adds one step's counts to n: what a case has to meet (crashes with a re-scan, restarts or resets, truncations, the share of
    beams at range_max, noisy values that crossed a bound their clean value had not) and its undecided arena-steps"""
    live = ~x["pending"]
    n["arena_steps"] = n.get("arena_steps", 0) + int(live.sum())
    n["undecided"] = n.get("undecided", 0) + int((x["undecided"] & live).sum())
    n["crashes"] = n.get("crashes", 0) + int((x["crash"] & live).sum())
    n["successes"] = n.get("successes", 0) + int(x["success"].sum())
    n["restarts"] = n.get("restarts", 0) + int(x["restarted"].sum()) + int(x["pending"].sum())
    n["truncations"] = n.get("truncations", 0) + int(x["trunc"].sum())
    n["crossed"] = n.get("crossed", 0) + int((x["crossed"] & live).sum())
    n["beams"] = n.get("beams", 0) + int(x["view_clean"][live].size)
    n["at_range_max"] = n.get("at_range_max", 0) + int((x["view_clean"][live] == np.float32(range_max)).sum())
    return n


def noise_coverage_met(n, cfg):
    """the case met what it is for (asserted on the model's run here and on the device's)"""
    assert n["undecided"] <= NOISE_CAP * n["arena_steps"], n
    assert n["crashes"] >= 3, n
    if cfg.auto_reset != abi.AUTORESET_NONE:
        assert n["restarts"] >= 3, n
        assert n["successes"] >= 1, n
    if cfg.max_episode_steps > 0:
        assert n["truncations"] >= 1, n
    assert 0.05 * n["beams"] <= n["at_range_max"] <= 0.95 * n["beams"], n
    assert n["crossed"] >= 1, n
