"""Device-resident state of E arenas and the calls into the C ABI (include/navsim.h).

torch is plumbing here: it owns the HBM buffers and the HIP stream; every computation of the hot
path happens in libnavsim_hip.so.
"""
import collections
import ctypes as C
import numbers
import os

import numpy as np

from . import abi
from .lib import check, load, require_gpu

_TORCH_DTYPE = None


def _dtype(name):
    global _TORCH_DTYPE
    import torch
    if _TORCH_DTYPE is None:
        _TORCH_DTYPE = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32,
                        "int64": torch.int64, "uint8": torch.uint8, "int8": torch.int8}
    return _TORCH_DTYPE[name]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- thin functional wrappers over the mirror primitives (used by tests and by NavSim) ----------
def build_rect_index(table, H, W):
    """navsim_build_rect_index: the index form of a record table (int32 CUDA [E, T, 4] from build_rects) -> (uint8 [E, R] rows,
    int32 [E] distinct rectangles per map).  What the fused step stages in LDS (navsim_state.rect_index)."""
    torch = require_gpu()
    L = load()
    E = table.shape[0]
    rows = torch.empty((E, L.navsim_rect_index_bytes(1, H, W)), dtype=torch.uint8, device=table.device)
    n_rects = torch.zeros(E, dtype=torch.int32, device=table.device)
    check(L.navsim_build_rect_index(_ptr(table), E, H, W, _ptr(rows), _ptr(n_rects), _stream()), "navsim_build_rect_index")
    return rows, n_rects


def maps_closed(occ):
    """navsim_maps_closed: occ uint8 CUDA [E,H,W] -> int32 [E], 1 where the map's outer ring of 3 cells is fully occupied.
    cfg.closed_maps may be set when every map of a world is closed (the LDS form of the march has no bounds test)."""
    torch = require_gpu()
    occ = occ.to(torch.uint8).contiguous()
    E, H, W = occ.shape
    closed = torch.zeros(E, dtype=torch.int32, device=occ.device)
    check(load().navsim_maps_closed(_ptr(occ), E, H, W, _ptr(closed), _stream()), "navsim_maps_closed")
    return closed


def build_dt(occ):
    """occ: uint8 CUDA tensor [E,H,W] (nonzero = occupied) -> float32 distance field [E,H,W]."""
    torch = require_gpu()
    L = load()
    occ = occ.contiguous()
    E, H, W = occ.shape
    field = torch.empty((E, H, W), dtype=torch.float32, device=occ.device)
    per_map = L.navsim_build_dt_workspace_bytes(1, H, W)
    chunk = max(1, min(E, (512 << 20) // max(per_map, 1)))       # <= 512 MiB of scratch
    ws = torch.empty(per_map * chunk, dtype=torch.uint8, device=occ.device)
    check(L.navsim_build_dt(_ptr(occ), E, H, W, _ptr(field), _ptr(ws), ws.numel(), _stream()), "navsim_build_dt")
    return field


def build_field(occ, fmt=abi.FIELD_U16T, keep_overflow=None):
    """occ: uint8 CUDA tensor [E,H,W] -> (field, overflow, n_saturated).

    fmt FIELD_F32: field is the float32 [E,H,W] distance field, overflow None.
    fmt FIELD_U16T: field is the packed uint16 tile blob the fused step streams; the float32 plane is
    computed alongside (the reset path samples spawn cells from it) and returned as `overflow`;
    it is only REQUIRED by the step when n_saturated > 0."""
    torch = require_gpu()
    L = load()
    occ = occ.contiguous()
    E, H, W = occ.shape
    if fmt == abi.FIELD_F32:
        return build_dt(occ), None, 0
    nbytes = L.navsim_field_bytes(E, H, W, fmt)
    field = torch.empty(nbytes // 2, dtype=torch.int16, device=occ.device)     # opaque blob
    overflow = torch.empty((E, H, W), dtype=torch.float32, device=occ.device)
    nsat = torch.zeros(1, dtype=torch.int32, device=occ.device)
    per_map = L.navsim_build_dt_workspace_bytes(1, H, W)
    chunk = max(1, min(E, (512 << 20) // max(per_map, 1)))
    ws = torch.empty(per_map * chunk, dtype=torch.uint8, device=occ.device)
    check(L.navsim_build_field(_ptr(occ), E, H, W, fmt, _ptr(field), _ptr(overflow), _ptr(nsat), _ptr(ws),
                               ws.numel(), _stream()), "navsim_build_field")
    return field, overflow, int(nsat.item())          # reset path: a sync is fine here


def build_rects(occ, field, fmt, overflow=None):
    """navsim_build_rects: occ uint8 CUDA [E,H,W] + the distance field built from it (build_field's `field`, and
    its float32 plane when cells are saturated) -> int32 [E, T, 4] two-rectangle records of the 8x8 tiles."""
    torch = require_gpu()
    L = load()
    occ = occ.contiguous()
    E, H, W = occ.shape
    T = ((H + 7) // 8) * ((W + 7) // 8)
    table = torch.empty((E, T, 4), dtype=torch.int32, device=occ.device)
    per = L.navsim_build_rects_workspace_bytes(1, H, W) + 256
    chunk = max(1, min(E, (1 << 30) // per))                      # <= 1 GiB of scratch
    ws = torch.empty(per * chunk, dtype=torch.uint8, device=occ.device)
    check(L.navsim_build_rects(_ptr(occ), E, H, W, _ptr(field), int(fmt), _ptr(overflow), _ptr(table), _ptr(ws),
                               ws.numel(), _stream()), "navsim_build_rects")
    return table


def cast_static(field, queries, max_range, march_rule=abi.MARCH_F32):
    torch = require_gpu()
    E, H, W = field.shape
    q = queries.contiguous()
    out = torch.empty(q.shape[:2], dtype=torch.float32, device=field.device)
    check(load().navsim_cast_static(_ptr(field), E, H, W, _ptr(q), q.shape[1], float(max_range), int(march_rule),
                                    _ptr(out), _stream()), "navsim_cast_static")
    return out


def render_polys(ranges, angles, verts, n_verts, origin):
    require_gpu()
    E, B = ranges.shape
    check(load().navsim_render_polys(_ptr(ranges), _ptr(angles), E, B, _ptr(verts), _ptr(n_verts),
                                     verts.shape[1], _ptr(origin), _stream()), "navsim_render_polys")
    return ranges


def render_legs(ranges, angles, agents, n_agents, origin):
    require_gpu()
    E, B = ranges.shape
    check(load().navsim_render_legs(_ptr(ranges), _ptr(angles), E, B, _ptr(agents), _ptr(n_agents),
                                    agents.shape[1], _ptr(origin), _stream()), "navsim_render_legs")
    return ranges


def integrate(pose, cmd, time_step, axle_offset, vel_out=None):
    require_gpu()
    check(load().navsim_integrate(_ptr(pose), _ptr(cmd), _ptr(vel_out), pose.shape[0], float(time_step),
                                  float(axle_offset), _stream()), "navsim_integrate")
    return pose


def scan_threshold(cfg, footprint):
    torch = require_gpu()
    fp = footprint.contiguous()
    out = torch.empty(cfg.n_beams, dtype=torch.float32, device=fp.device)
    check(load().navsim_scan_threshold(C.byref(cfg), _ptr(fp), fp.shape[0], _ptr(out), _stream()),
          "navsim_scan_threshold")
    return out


def reward_done(cfg, obs, goals, thr, dthr):
    torch = require_gpu()
    obs = obs.contiguous()
    is64 = obs.dtype == torch.float64
    goals = goals.to(obs.dtype).contiguous()
    n = obs.shape[0]
    dev = obs.device
    out = dict(reward=torch.empty(n, dtype=torch.float64, device=dev),
               done=torch.empty(n, dtype=torch.uint8, device=dev),
               is_success=torch.empty(n, dtype=torch.float32, device=dev),
               is_crash=torch.empty(n, dtype=torch.float32, device=dev),
               distance=torch.empty(n, dtype=torch.float64, device=dev))
    check(load().navsim_reward_done(C.byref(cfg), _ptr(obs), _ptr(goals), int(is64), n, _ptr(thr), _ptr(dthr),
                                    _ptr(out["reward"]), _ptr(out["done"]), _ptr(out["is_success"]),
                                    _ptr(out["is_crash"]), _ptr(out["distance"]), _stream()), "navsim_reward_done")
    return out


def costmap(occ):
    """occ uint8 CUDA [n,H,W] -> uint8 [n,H/5,W/5] (env.py:312-332)."""
    torch = require_gpu()
    occ = occ.contiguous()
    n, H, W = occ.shape
    out = torch.zeros((n, H // 5, W // 5), dtype=torch.uint8, device=occ.device)
    check(load().navsim_costmap(_ptr(occ), n, H, W, _ptr(out), _stream()), "navsim_costmap")
    return out


def plan(cost, start, goal, interval, max_wp=8, res_c=0.25, origin=(0.0, 0.0), map_index=None):
    """Shortest 4-connected paths + waypoints for n queries (env.py:343-354, 1261-1277)."""
    torch = require_gpu()
    L = load()
    cost = cost.contiguous()
    _, Hc, Wc = cost.shape
    start = start.to(torch.float64).contiguous().reshape(-1, 2)
    n = start.shape[0]
    goal = goal.to(torch.float64).contiguous().reshape(n, 2)
    dev = cost.device
    mi = None if map_index is None else map_index.to(device=dev, dtype=torch.int32).contiguous()
    wp = torch.zeros((n, max_wp, 2), dtype=torch.float64, device=dev)
    n_wp = torch.zeros(n, dtype=torch.int32, device=dev)
    cells = torch.zeros(n, dtype=torch.int32, device=dev)
    plen = torch.zeros(n, dtype=torch.float64, device=dev)
    check(L.navsim_plan(_ptr(cost), _ptr(mi), n, Hc, Wc, float(res_c), float(origin[0]), float(origin[1]), _ptr(start),
                        _ptr(goal), float(interval), max_wp, _ptr(wp), _ptr(n_wp), _ptr(cells), _ptr(plen), _stream()),
          "navsim_plan")
    return wp, n_wp, cells, plen


def crowd_check(params, free_map, robot, agents, global_time, n_agents=None):
    """navsim_crowd_check: CrowdSim.step's collision / goal / reward block (crowd_sim.py:808-949) for E envs.
    params: dict with the fields of navsim_crowd_params; tensors on the GPU.  -> reward, done, info, min_dist."""
    torch = require_gpu()
    L = load()
    p = abi.NavsimCrowdParams(**{k: float(v) for k, v in params.items()})
    free_map = free_map.to(torch.uint8).contiguous()
    E, G = free_map.shape[0], free_map.shape[1]
    dev = free_map.device
    robot = robot.to(torch.float64).contiguous().reshape(E, 10)
    agents = agents.to(torch.float64).contiguous().reshape(E, -1, 5)
    A = agents.shape[1]
    gt = global_time.to(torch.float64).contiguous().reshape(E)
    na = None if n_agents is None else n_agents.to(device=dev, dtype=torch.int32).contiguous()
    reward = torch.zeros(E, dtype=torch.float64, device=dev); done = torch.zeros(E, dtype=torch.uint8, device=dev)
    info = torch.zeros(E, dtype=torch.int32, device=dev); md = torch.zeros(E, dtype=torch.float64, device=dev)
    check(L.navsim_crowd_check(C.byref(p), E, A, G, _ptr(free_map), _ptr(robot), _ptr(agents), _ptr(na), _ptr(gt),
                               _ptr(reward), _ptr(done), _ptr(info), _ptr(md), _stream()), "navsim_crowd_check")
    return reward, done, info, md


def _crowd_map_params(params):
    p = abi.NavsimCrowdMapParams()
    for k, v in params.items():
        setattr(p, k, int(v) if k in ("angular_dim", "normalize") else float(v))
    return p


def crowd_angular_map(params, robot, verts, n_obst=None):
    """navsim_crowd_angular_map: CrowdSim.get_local_map_angular (crowd_sim.py:1055-1102) for E envs.
    robot [E,4] px, py, theta, radius; verts [E,O,V,2]; -> float64 [E, angular_dim]."""
    torch = require_gpu()
    p = _crowd_map_params(params)
    robot = robot.to(torch.float64).contiguous()
    E = robot.shape[0]
    verts = verts.to(torch.float64).contiguous()
    O, V = (verts.shape[1], verts.shape[2]) if verts.numel() else (0, 4)
    no = None if n_obst is None else n_obst.to(device=robot.device, dtype=torch.int32).contiguous()
    out = torch.empty((E, p.angular_dim), dtype=torch.float64, device=robot.device)
    check(load().navsim_crowd_angular_map(C.byref(p), E, O, V, _ptr(robot), _ptr(verts) if O else None, _ptr(no), _ptr(out),
                                          _stream()), "navsim_crowd_angular_map")
    return out


def crowd_local_map(params, free_map, robot, rotate=True):
    """navsim_crowd_local_map: CrowdSim.get_local_map (crowd_sim.py:1104-1186) for E envs -> uint8 [E,S,S]."""
    torch = require_gpu()
    p = _crowd_map_params(params)
    free_map = free_map.to(torch.uint8).contiguous()
    E, G = free_map.shape[0], free_map.shape[1]
    robot = robot.to(torch.float64).contiguous()
    S = int(round(p.submap_size_m / p.map_resolution))
    out = torch.empty((E, S, S), dtype=torch.uint8, device=free_map.device)
    check(load().navsim_crowd_local_map(C.byref(p), E, G, _ptr(free_map), _ptr(robot), int(bool(rotate)), _ptr(out),
                                        _stream()), "navsim_crowd_local_map")
    return out


def _overridden(d, params, noun, keys):
    """The dict of defaults `d` with the overrides `params` (a dict or None) applied; a key that `d` does not have raises
    ValueError naming the `noun` and the `keys` a caller may give."""
    for k, v in (params or {}).items():
        if k not in d:
            raise ValueError("unknown %s parameter %r (known: %s)" % (noun, k, ", ".join(keys)))
        d[k] = v
    return d


def _set_fields(p, d, keys, flags=()):
    """d[k] into the ctypes struct p for every k of keys, as the field's type asks: an int (0 / 1 for the flags) or a float."""
    kinds = dict(p._fields_)
    for k in keys:
        setattr(p, k, int(bool(d[k])) if k in flags else int(d[k]) if kinds[k] is C.c_int32 else float(d[k]))
    return p


def blob_layout(table, E, sym=None, omit=()):
    """Where the arrays of an output table lie in one byte blob.  table: {name: (dtype, trailing shape behind E)} as abi states
    them, a str in a shape being an extent that `sym` resolves; names in `omit` are left out.  Returns [(name, dtype, first byte,
    end byte, shape), ...] in the table's order, each start rounded up to 16 bytes, and a last entry (None, None, start, end, None)
    whose end byte is the blob's size: at least 16."""
    out, at = [], 0
    for k, (d, shape) in table.items():
        if k in omit:
            continue
        full = (E,) + tuple(sym[s] if isinstance(s, str) else s for s in shape)
        n = int(np.prod(full)) * np.dtype(d).itemsize
        out.append((k, d, at, at + n, full))
        at = (at + n + 15) // 16 * 16
    out.append((None, None, at, max(at, 16), None))
    return out


ORCA_KEYS = ("time_step", "neighbor_dist", "time_horizon", "time_horizon_obst", "max_neighbors")
PED_ORCA_KEYS = ORCA_KEYS + ("ped_radius", "robot_radius", "safety_space", "robot_visible", "max_obst_rects")


def ped_orca_defaults(cfg, robot_type="keti"):
    """The parameters of navsim_ped_orca as a dict: orca.py:62-65's neighbourhood, the simulator's time step, discs around
    the footprints of robots.py (the pedestrian's ~ 0.291 m), no safety space, the robot visible.  max_obst_rects is not a
    field of the struct: it is navsim_ped_orca_walls's max_rects (0: static obstacles are not ORCA obstacles)."""
    from . import robots
    return dict(time_step=cfg.time_step, neighbor_dist=10.0, time_horizon=5.0, time_horizon_obst=5.0, max_neighbors=10,
                ped_radius=robots.footprint_radius(robots.HUMAN["footprint"]),
                robot_radius=robots.footprint_radius(robots.ROBOTS[robot_type]["footprint"]),
                safety_space=0.0, robot_visible=1, max_obst_rects=0)


def ped_orca_params(cfg, params=None, robot_type="keti"):
    """abi.NavsimPedOrcaParams of ped_orca_defaults(cfg) overridden by the dict `params`; an unknown key raises ValueError."""
    d = _overridden(ped_orca_defaults(cfg, robot_type), params, "ORCA", PED_ORCA_KEYS)
    p = abi.NavsimPedOrcaParams()
    _set_fields(p.orca, d, ORCA_KEYS)
    return _set_fields(p, d, ("ped_radius", "robot_radius", "safety_space", "robot_visible"), flags=("robot_visible",))


PED_OBSERVE_KEYS = ("ped_radius", "sensor_range", "max_obs", "rays", "occlusion", "fov")


def ped_observe_defaults(cfg, robot_type="keti"):
    """The parameters of navsim_ped_observe as a dict: the pedestrian disc ped_orca_defaults uses, the lidar's range and field
    of view, three lines of sight per pedestrian, a row for every pedestrian the arena can hold."""
    return dict(ped_radius=ped_orca_defaults(cfg, robot_type)["ped_radius"], sensor_range=cfg.range_max, max_obs=cfg.max_peds,
                rays=3, occlusion=1, fov=1)


def ped_observe_params(cfg, params=None, robot_type="keti"):
    """abi.NavsimPedObserveParams of ped_observe_defaults(cfg) overridden by the dict `params`; an unknown key raises ValueError."""
    d = _overridden(ped_observe_defaults(cfg, robot_type), params, "observation", PED_OBSERVE_KEYS)
    return _set_fields(abi.NavsimPedObserveParams(), d, PED_OBSERVE_KEYS, flags=("occlusion", "fov"))


GOAL_PATH_KEYS = ("hard_clearance", "clearance", "band_cost", "lookahead")


def goal_path_defaults(cfg):
    """The parameters of navsim_goal_path as a dict: cells closer than 0.3 m to a wall are impassable (never below the three
    map cells the rule requires), cells closer than 0.75 m cost three times their length, the sub-goal lies 2 m down the field."""
    return dict(hard_clearance=max(0.3, 3.0 * cfg.resolution), clearance=max(0.75, 3.0 * cfg.resolution), band_cost=3, lookahead=2.0)


def goal_path_params(cfg, params=None):
    """abi.NavsimGoalPathParams of goal_path_defaults(cfg) overridden by the dict `params`; an unknown key raises ValueError."""
    d = _overridden(goal_path_defaults(cfg), params, "goal-path", GOAL_PATH_KEYS)
    return _set_fields(abi.NavsimGoalPathParams(), d, GOAL_PATH_KEYS)


def goal_path_layout(E):
    """Where navsim_goal_path_out's arrays lie in one byte blob: [(name, dtype, first byte, end byte, shape), ...] in
    abi.GOAL_PATH_OUT's order, each start rounded up to 16 bytes, and a last entry whose end byte is the blob's size."""
    return blob_layout(abi.GOAL_PATH_OUT, E)


DWA_KEYS = ("acc_lin", "acc_rot", "body_radius", "body_offset", "ped_radius", "margin", "clearance_cap", "w_progress", "w_heading",
            "w_clearance", "w_speed", "n_v", "n_w", "horizon", "use_peds")


def dwa_defaults(cfg, robot_type="keti"):
    """The parameters of navsim_dwa as a dict: two discs that cover the robot's threshold footprint (robots.py) -- at the centres
    of the two halves of its x extent, radius the half-diagonal of a half --, a 0.1 m margin, 0.3 m pedestrian discs, clearance
    counted up to 1 m, 1.0 m/s^2 and 3.2 rad/s^2, 5 x 9 candidates rolled out over 8 steps, weights 1 / 0.2 / 0.3 / 0.1 for
    progress, heading, clearance and speed.  body_offset is a sequence of 1 .. 4 disc centres (n_discs is its length)."""
    from . import robots
    fp = np.asarray(robots.ROBOTS[robot_type]["threshold_footprint"], np.float64)
    x_lo, x_hi, half_y = float(fp[:, 0].min()), float(fp[:, 0].max()), float(np.abs(fp[:, 1]).max())
    quarter = (x_hi - x_lo) / 4.0
    return dict(acc_lin=1.0, acc_rot=3.2, body_radius=float(np.hypot(quarter, half_y)), body_offset=(x_lo + quarter, x_hi - quarter),
                ped_radius=0.3, margin=0.1, clearance_cap=1.0, w_progress=1.0, w_heading=0.2, w_clearance=0.3, w_speed=0.1,
                n_v=5, n_w=9, horizon=8, use_peds=1)


def dwa_params(cfg, params=None, robot_type="keti"):
    """abi.NavsimDwaParams of dwa_defaults(cfg) overridden by the dict `params`; an unknown key raises ValueError."""
    d = _overridden(dwa_defaults(cfg, robot_type), params, "planner", DWA_KEYS)
    offs = [float(x) for x in np.atleast_1d(np.asarray(d["body_offset"], np.float64))]
    if not 1 <= len(offs) <= abi.DWA_MAX_DISCS:
        raise ValueError("body_offset holds 1 .. %d disc centres, not %d" % (abi.DWA_MAX_DISCS, len(offs)))
    p = _set_fields(abi.NavsimDwaParams(), d, [k for k in DWA_KEYS if k != "body_offset"], flags=("use_peds",))
    p.body_offset[:len(offs)], p.n_discs = offs, len(offs)
    return p


def dwa_layout(E, C_, scores=False):
    """Where navsim_dwa_out's arrays lie in one byte blob: [(name, dtype, first byte, end byte, shape), ...] in abi.DWA_OUT's
    order (the two per-candidate arrays only with scores=True), each start rounded up to 16 bytes, and a last entry whose end
    byte is the blob's size."""
    return blob_layout(abi.DWA_OUT, E, {"C": C_}, omit=() if scores else [k for k, (_, shape) in abi.DWA_OUT.items() if "C" in shape])


LOCAL_MAP_KEYS = ("cell", "ahead", "cap", "ped_radius", "channels")


def local_map_defaults(cfg):
    """The parameters of navsim_local_map as a dict (the grid's size apart, which is asked for): 0.1 m cells around the pose
    origin, clearances counted up to 2 m, 0.3 m pedestrian discs; four channels -- walls, pedestrian clearance, the covering
    pedestrian's velocity -- in a world with a pedestrian model, the wall channel alone in one without."""
    return dict(cell=0.1, ahead=0.0, cap=2.0, ped_radius=0.3, channels=1 if cfg.ped_model == abi.PED_NONE else 4)


def local_map_params(cfg, params=None, size=None):
    """abi.NavsimLocalMapParams of local_map_defaults(cfg) overridden by the dict `params`, with `size` cells a side; an unknown
    key raises ValueError."""
    d = _overridden(local_map_defaults(cfg), params, "local map", LOCAL_MAP_KEYS)
    p = _set_fields(abi.NavsimLocalMapParams(), d, LOCAL_MAP_KEYS)
    p.size = 0 if size is None else int(size)
    return p


LOOKAHEAD_KEYS = ("range",)


def lookahead_range_min(discomfort_max):
    """The least cap R that navsim_lookahead's rule 5 allows for thresholds up to discomfort_max: 0.1 m above them."""
    return float(discomfort_max) + 0.1


LOOKAHEAD_OBS_KEYS = ("noise", "rows")
LOOKAHEAD_OBS_NOISE = {"off": abi.LOOKOBS_NOISE_OFF, "step": abi.LOOKOBS_NOISE_STEP}
LOOKAHEAD_OBS_ROWS = ("full", "scan")


def lookahead_obs_defaults():
    """The parameters of navsim_lookahead_obs as a dict: noise 'step' (the scan noise the step itself would draw; 'off': none)
    and rows 'full' (the whole observation row of every candidate; 'scan': its newest scan slot and its tail only)."""
    return dict(noise="step", rows="full")


def lookahead_obs_choice(d):
    """(abi.LOOKOBS_NOISE_* constant, 'full' | 'scan') of a parameter dict; anything else raises ValueError."""
    if not (isinstance(d["noise"], str) and d["noise"] in LOOKAHEAD_OBS_NOISE):
        raise ValueError("lookahead_obs noise must be 'step' or 'off', not %r" % (d["noise"],))
    if not (isinstance(d["rows"], str) and d["rows"] in LOOKAHEAD_OBS_ROWS):
        raise ValueError("lookahead_obs rows must be 'full' or 'scan', not %r" % (d["rows"],))
    return LOOKAHEAD_OBS_NOISE[d["noise"]], d["rows"]


def lookahead_defaults(cfg, discomfort_max=0.0):
    """The parameters of navsim_lookahead as a dict: range, the candidates' scan cap R -- the smallest multiple of 0.25 m that
    lies 0.1 m above the largest discomfort threshold (discomfort_max, metres; NavSim.enable_lookahead reads it from the state),
    never above the lidar's range."""
    return dict(range=min(float(cfg.range_max), float(np.ceil(lookahead_range_min(discomfort_max) / 0.25)) * 0.25))


ROLLOUT_KEYS = ("range", "gamma")


def rollout_defaults(cfg, discomfort_max=0.0):
    """The parameters of navsim_rollout as a dict: range, the scans' cap R with the lookahead's default and lower bound
    (lookahead_defaults, lookahead_range_min), and gamma, the discount of `ret` (1.0: the plain sum of rewards).  The sequence
    count K and the horizon H are arguments of NavSim.enable_rollout."""
    return dict(range=lookahead_defaults(cfg, discomfort_max)["range"], gamma=1.0)


ROLLOUT_OBS_KEYS = ("gamma", "noise", "rows")
ROLLOUT_OBS_ROWS = ("last", "all")


def rollout_obs_defaults():
    """The parameters of navsim_rollout_obs as a dict: gamma, the discount of `ret` (1.0: the plain sum of rewards); noise 'step'
    (the scan noise each future step itself would draw; 'off': none); rows 'last' (the observation row of every sequence's last
    evaluated step; 'all': the rows of all H steps as well).  The sequence count K and the horizon H are arguments of
    NavSim.enable_rollout_obs."""
    return dict(gamma=1.0, noise="step", rows="last")


def rollout_obs_choice(d):
    """(gamma, abi.LOOKOBS_NOISE_* constant, 'last' | 'all') of a parameter dict; anything else raises ValueError."""
    gamma = d["gamma"]
    if isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not 0.0 <= gamma <= 1.0:
        raise ValueError("rollout_obs gamma must lie in [0, 1], not %r" % (gamma,))
    if not (isinstance(d["noise"], str) and d["noise"] in LOOKAHEAD_OBS_NOISE):
        raise ValueError("rollout_obs noise must be 'step' or 'off', not %r" % (d["noise"],))
    if not (isinstance(d["rows"], str) and d["rows"] in ROLLOUT_OBS_ROWS):
        raise ValueError("rollout_obs rows must be 'last' or 'all', not %r" % (d["rows"],))
    return float(gamma), LOOKAHEAD_OBS_NOISE[d["noise"]], d["rows"]


PED_FORECAST_KEYS = ("robot", "model")
PED_FORECAST_ROBOT = {"hold": abi.FORECAST_HOLD, "stop": abi.FORECAST_STOP, "actions": abi.FORECAST_ACTIONS}
PED_FORECAST_MODEL = {"true": abi.FORECAST_TRUE, "const_vel": abi.FORECAST_CONST_VEL}


def ped_forecast_defaults(cfg):
    """The parameters of navsim_ped_forecast as a dict: robot -- what the robot is assumed to do over the horizon: 'hold' (the
    state's prev_action, repeated), 'stop' (the zero twist) or 'actions' (the caller's [E,H,2]) -- and model: 'true' (the
    configured pedestrian model: the social force, or external commands held) or 'const_vel'.  The horizon H is an argument of
    NavSim.enable_ped_forecast."""
    return dict(robot="hold", model="true")


MPPI_KEYS = ("n_samples", "horizon", "iterations", "sigma", "lam", "beta", "w_goal", "w_crash", "off_field_cost", "stop_sample",
             "select", "range", "gamma", "init_action", "lo", "hi")
MPPI_SELECT = {"mean": 0, "best": 1, 0: 0, 1: 1}


def mppi_defaults(cfg, robot_type="keti", discomfort_max=0.0):
    """The parameters of navsim_mppi as a dict.  The action box lo / hi: the robot's linvel_range / rotvel_range (robots.py), or
    under ACTION_WHEELS the least and the greatest wheel speed over the corners of that box, as NavGymEnv builds its
    action_space.  K = 32 sequences over H = 24 steps, one iteration; sigma half of the box per component, the noise strongly
    correlated over the horizon (beta = 0.9: a sequence is a manoeuvre, not a jitter); the plan starts at the action nearest to
    0; sequence 1 stands still (stop_sample); the cost is w_goal = 3 per metre of goal distance at the horizon's end minus the
    rollout's return, + w_crash = 100 for a crash, + off_field_cost = 10 m for an end pose off the goal field; temperature
    lam = 0.05; select 'mean' (the new plan's first action; 'best': the best sequence's).  range / gamma: rollout_defaults'.
    Tuning, not correctness, from the behaviour run of profiles/r24_mppi/summary.txt (64 outdoor arenas, 150 steps, goal_path on,
    select='best'): the robot turns at 0.64 rad/s at most, so a horizon of 8 steps (1.6 s) sees no progress behind a turn and
    stands still -- 13 of 64 arenas reach their goal; H = 16 with beta = 0.9 and the wider sigma: 33; w_goal = 3: 44; H = 24: 58.
    No setting crashed without pedestrians."""
    from . import robots
    spec = robots.ROBOTS[robot_type]
    (v0, v1), (w0, w1) = spec["linvel_range"], spec["rotvel_range"]
    if cfg.action_kind == abi.ACTION_WHEELS:
        corners = [robots.wheels_from_twist(v, w, cfg.wheel_radius, cfg.wheel_track) for v in (v0, v1) for w in (w0, w1)]
        lo = (float(np.min(corners)),) * 2
        hi = (float(np.max(corners)),) * 2
    else:
        lo, hi = (float(v0), float(w0)), (float(v1), float(w1))
    d = dict(n_samples=32, horizon=24, iterations=1, sigma=tuple(0.5 * (h - l) for l, h in zip(lo, hi)), lam=0.05, beta=0.9,
             w_goal=3.0, w_crash=100.0, off_field_cost=10.0, stop_sample=1, select="mean",
             init_action=tuple(min(max(0.0, l), h) for l, h in zip(lo, hi)), lo=lo, hi=hi)
    d.update(rollout_defaults(cfg, discomfort_max))
    return d


def mppi_params(cfg, params=None, robot_type="keti", discomfort_max=0.0):
    """abi.NavsimMppiParams of mppi_defaults(cfg, robot_type) overridden by the dict `params`; an unknown key or a value
    navsim_mppi would refuse raises ValueError.  alpha = sqrt(1 - beta * beta) is computed here, in float64."""
    d = _overridden(mppi_defaults(cfg, robot_type, discomfort_max), params, "planner", MPPI_KEYS)
    if d["select"] not in MPPI_SELECT:
        raise ValueError("select must be 'mean' or 'best', not %r" % (d["select"],))
    p = abi.NavsimMppiParams()
    p.n_samples, p.horizon, p.iterations = int(d["n_samples"]), int(d["horizon"]), int(d["iterations"])
    p.stop_sample, p.select = int(bool(d["stop_sample"])), MPPI_SELECT[d["select"]]
    p.range, p.gamma = float(d["range"]), float(d["gamma"])
    for k in ("sigma", "lo", "hi", "init_action"):
        v = np.asarray(d[k], np.float64).reshape(-1)
        if v.shape != (2,):
            raise ValueError("%s holds two values (one per action component), not %r" % (k, d[k]))
        getattr(p, k)[:] = [float(v[0]), float(v[1])]
    p.beta, p.lam = float(d["beta"]), float(d["lam"])
    p.w_goal, p.w_crash, p.off_field_cost = float(d["w_goal"]), float(d["w_crash"]), float(d["off_field_cost"])
    if not 1 <= p.n_samples <= abi.ROLLOUT_MAX_K:
        raise ValueError("the planner samples 1 .. %d sequences per arena, not %r" % (abi.ROLLOUT_MAX_K, d["n_samples"]))
    if not 1 <= p.horizon <= abi.ROLLOUT_MAX_H:
        raise ValueError("the planner looks 1 .. %d steps ahead, not %r" % (abi.ROLLOUT_MAX_H, d["horizon"]))
    if not 1 <= p.iterations <= abi.MPPI_MAX_ITERATIONS:
        raise ValueError("the planner runs 1 .. %d iterations, not %r" % (abi.MPPI_MAX_ITERATIONS, d["iterations"]))
    if not 0.0 <= p.beta < 1.0:
        raise ValueError("beta must lie in [0, 1), not %r" % (d["beta"],))
    if not (p.lam > 0.0 and np.isfinite(p.lam)):
        raise ValueError("lam must be positive, not %r" % (d["lam"],))
    for i in range(2):
        if not (np.isfinite(p.sigma[i]) and p.sigma[i] >= 0.0):
            raise ValueError("sigma must not be negative, not %r" % (d["sigma"],))
        if not (np.isfinite(p.lo[i]) and np.isfinite(p.hi[i]) and p.lo[i] <= p.init_action[i] <= p.hi[i]):
            raise ValueError("init_action must lie inside the action box [%r, %r], not %r" % (d["lo"], d["hi"], d["init_action"]))
        if p.stop_sample and not p.lo[i] <= 0.0 <= p.hi[i]:
            raise ValueError("stop_sample needs the action 0 inside the box [%r, %r]" % (d["lo"], d["hi"]))
    for k in ("w_goal", "w_crash", "off_field_cost"):
        if not (np.isfinite(getattr(p, k)) and getattr(p, k) >= 0.0):
            raise ValueError("%s must not be negative, not %r" % (k, d[k]))
    p.alpha = float(np.sqrt(np.float64(1.0) - np.float64(p.beta) * np.float64(p.beta)))
    return p


def ped_observation_layout(E, K, N):
    """Where navsim_ped_observation's arrays lie in one byte blob: [(name, dtype, first byte, end byte, shape), ...] in
    abi.PED_OBSERVATION's order, each start rounded up to 16 bytes, and a last entry whose end byte is the blob's size."""
    return blob_layout(abi.PED_OBSERVATION, E, {"K": K, "N": N})


def crowd_orca(params, agents, pref_vel, verts=None, n_agents=None, n_obst=None, obst_set=None, theta=None):
    """navsim_crowd_orca: ORCA.predict (orca.py:85-135) for Q pedestrians: agents [Q,A,6] (agent 0 = the pedestrian),
    pref_vel [Q,2], verts [S,O,V,2] CCW polygons -> (new velocity [Q,2], ActionRot (v, r) [Q,2]), float64 tensors."""
    torch = require_gpu()
    p = abi.NavsimOrcaParams(**{k: (int(v) if k == "max_neighbors" else float(v)) for k, v in params.items()})
    agents = agents.to(torch.float64).contiguous()
    Q, A = agents.shape[0], agents.shape[1]
    dev = agents.device
    pref_vel = pref_vel.to(device=dev, dtype=torch.float64).contiguous().reshape(Q, 2)
    if verts is None or verts.numel() == 0:
        verts, O, V = None, 0, 4
    else:
        verts = verts.to(device=dev, dtype=torch.float64).contiguous()
        O, V = verts.shape[1], verts.shape[2]
    i32 = lambda a: None if a is None else a.to(device=dev, dtype=torch.int32).contiguous()
    na, no, os_ = i32(n_agents), i32(n_obst), i32(obst_set)
    th = None if theta is None else theta.to(device=dev, dtype=torch.float64).contiguous()
    vel = torch.empty((Q, 2), dtype=torch.float64, device=dev)
    act = torch.empty((Q, 2), dtype=torch.float64, device=dev)
    check(load().navsim_crowd_orca(C.byref(p), Q, A, _ptr(agents), _ptr(na), _ptr(pref_vel), O, V, _ptr(verts), _ptr(no),
                                   _ptr(os_), _ptr(th), _ptr(vel), _ptr(act), _stream()), "navsim_crowd_orca")
    return vel, act


def crowd_agent_step(pose, action, time_step):
    """navsim_crowd_agent_step: Agent.step with an ActionRot (agent.py:108-141) -> (pose [n,3], vel [n,2])."""
    torch = require_gpu()
    pose = pose.to(torch.float64).contiguous().clone()
    action = action.to(device=pose.device, dtype=torch.float64).contiguous()
    vel = torch.empty((pose.shape[0], 2), dtype=torch.float64, device=pose.device)
    check(load().navsim_crowd_agent_step(_ptr(pose), _ptr(action), _ptr(vel), pose.shape[0], float(time_step), _stream()),
          "navsim_crowd_agent_step")
    return pose, vel


def debug_kernarg_layout():
    """navsim_debug_kernarg_layout: the step kernels' views of their arguments (references into the kernarg segment) against the
    by-value copies, in one probe launch.  Raises when they differ."""
    require_gpu()
    check(load().navsim_debug_kernarg_layout(_stream()), "navsim_debug_kernarg_layout")


def debug_xy_to_ij(cfg, xy, as_f32):
    """Device batch_xy_to_ij (env.py:1228-1253): xy float64 CUDA [n,2] -> int32 [n,2] (i, j)."""
    torch = require_gpu()
    xy = xy.to(torch.float64).contiguous()
    out = torch.empty((xy.shape[0], 2), dtype=torch.int32, device=xy.device)
    check(load().navsim_debug_xy_to_ij(C.byref(cfg), _ptr(xy), int(bool(as_f32)), _ptr(out), xy.shape[0], _stream()),
          "navsim_debug_xy_to_ij")
    return out


def debug_spawn_decisions(cfg, cost, kind, start, goal, robot=None):
    """navsim_debug_spawn_decisions: the spawn loops' acceptance rules on supplied candidates (tests only).
    cost uint8 CUDA [Hc,Wc]; kind int32 [n]; start / goal / robot float64 [n,2] -> int32 codes [n]."""
    torch = require_gpu()
    dev = cost.device
    cost = cost.to(torch.uint8).contiguous()
    Hc, Wc = cost.shape
    kind = torch.as_tensor(kind).to(device=dev, dtype=torch.int32).contiguous()
    n = kind.shape[0]
    f64 = lambda a: None if a is None else torch.as_tensor(a).to(device=dev, dtype=torch.float64).contiguous().reshape(n, 2)
    start, goal, robot = f64(start), f64(goal), f64(robot)
    ws = torch.zeros((n, cfg.max_waypoints, 2), dtype=torch.float64, device=dev)
    code = torch.full((n,), -1, dtype=torch.int32, device=dev)
    L = load()
    L.navsim_debug_spawn_decisions.argtypes = [C.POINTER(abi.NavsimConfig), C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
    check(L.navsim_debug_spawn_decisions(C.byref(cfg), _ptr(cost), Hc, Wc, n, _ptr(kind), _ptr(start), _ptr(goal),
                                         _ptr(robot), _ptr(ws), _ptr(code), _stream()), "navsim_debug_spawn_decisions")
    return code


def debug_math(fn, x, x2=None):
    torch = require_gpu()
    out = torch.empty_like(x)
    check(load().navsim_debug_math(fn, _ptr(x), _ptr(x2), _ptr(out), x.numel(), _stream()), "navsim_debug_math")
    return out


def concurrent_stream(device, priority=0, tries=8, beside=None):
    """A stream whose kernels really run BESIDE those of the current stream.  HIP spreads a process's streams over a handful of
    hardware queues (four by default) in creation order; two streams that land on the same queue take turns, whatever the
    events between them say -- a process that has created a few streams before (torch hands its pool out round-robin) got a
    staging stream on the main stream's queue one time in four, and the pipelined reset path then ran at 1.6 M env-steps/s
    instead of 2.4 M (profiles/_diag/bench_bisect.py).  So: try a few candidates, time two ~50 us spin kernels queued on the two
    streams at once, and keep the first candidate on which they overlap (else the best seen)."""
    import torch
    if not hasattr(torch.cuda, "_sleep"):                       # (no spin kernel to time with: any stream)
        return torch.cuda.Stream(device=device, priority=priority)
    others = list(beside) if beside else [torch.cuda.current_stream(device)]     # beside: the streams it must not share a queue with
    best, best_ratio = None, None
    spin = 100_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(tries):
        cand = torch.cuda.Stream(device=device, priority=priority)
        with torch.cuda.stream(cand):                           # one spin alone: what "beside" is measured against (twice: warm-up)
            for rep in range(2):
                torch.cuda.synchronize(device)
                e0.record(cand); torch.cuda._sleep(spin); e1.record(cand)
                torch.cuda.synchronize(device)
        alone = e0.elapsed_time(e1)
        worst = 0.0
        for other in others:
            for rep in range(2):
                torch.cuda.synchronize(device)
                e0.record(other)
                cand.wait_event(e0)
                with torch.cuda.stream(cand):
                    torch.cuda._sleep(spin)
                with torch.cuda.stream(other):
                    torch.cuda._sleep(spin)
                other.wait_stream(cand)
                e1.record(other)
                torch.cuda.synchronize(device)
            worst = max(worst, e0.elapsed_time(e1) / max(alone, 1e-6))
        if best_ratio is None or worst < best_ratio:
            best, best_ratio = cand, worst
        if worst < 1.5:
            return cand
    return best


# ---- the reset path's mode: what NavSim.enable_pregen decides before it allocates anything (no torch, no library, no device) ----
PregenPlan = collections.namedtuple("PregenPlan", (
    "period",           # P: a staging pass every P steps (0: one between every two steps)
    "install",          # step() is navsim_step_install: a finished arena's own workgroup installs its staged world
    "shared_maps",      # live and staged state share the per-map arrays through slot tables
    "fallback",         # navsim_regen for the arenas that finish before their world is staged (flags the step writes: NavSim.late)
    "heavy",            # corridor maps OR planned starts: navsim_regen is the long chain of launches
    "helper",           # corridor maps AND planned starts: navsim_regen forks, a helper stream for the fork
    # side streams the passes alternate between.  KNOWN, NOT FIXED HERE: with 2 lanes a pass's part is
    # pg_passes % 2, and pregen_sync / pregen_join reset pg_k but not pg_passes
    "lanes",
    "stage_cap",        # arenas one pass stages
    "side_priority",    # of lane 0's side stream
    # NEXT_STEP, worlds of outdoor maps without planning or costmap: NO fallback call at all -- an arena that finds nothing staged
    # regenerates its own world inside the step's launch, in place of the step it does not take (include/navsim.h
    # navsim_step_install with late = NULL; kernels_regen_dev.hpp regen_lone).  The library refuses (fewer than 256 threads per
    # arena): _launch falls back to the flags + navsim_regen form.  KNOWN, NOT FIXED HERE: regen_min_steps
    # is not consulted -- with 0 < regen_min_steps < 4 P the library runs rule-only and a late arena keeps its old map
    "lone",
    # NEXT_STEP (round 6): an arena learns when its episode ENDS whether the next world is staged; if not, the caller's
    # navsim_regen generates it BESIDE the next step's launch, on a stream of its own (include/navsim.h
    # navsim_step_install_next) -- nothing of the reset path is left on the steps' critical path, and no rule is needed
    # MEASURED AND NOT THE DEFAULT (late_beside=True asks for it): c5, 512 arenas, no rule: 5.4 M env-steps/s against 6.9 M
    # with the fallback's (mostly empty) launches behind the step on the same stream -- the two cross-stream waits per step
    # cost more than the three launches they take off the critical path (profiles/r06_c5/README.md; the same finding as
    # round 5's two-stream re-plan).  KNOWN, NOT FIXED HERE: in both next-step forms, this and `lone`,
    # reset_arenas(mask) restarts an arena whose latest done flag is set a second time (the step has restarted it already)
    "beside",
    "poll",             # same-step: regen() reads "any late flag set?" back before it launches the fallback
    "late_cap",         # arenas one fallback call serves (0: no fallback)
    "late_defer_scan"))  # the fallback's configuration gets defer_reset_scan = 1 (the beside form)


def late_cap_for(E, asked=None):
    """Arenas one navsim_regen call of a fallback (the per-step one, reset_arenas' own) serves where nobody asks for a number."""
    # (every launch of the fallback is sized by its cap whether anybody is late or not: with 16 slots the planner's
    #  four launches alone dispatched 2 x 960 empty 1024-thread workgroups per step, 0.25 ms of a 0.38 ms step of the
    #  reference's configuration, profiles/r05_refdef/timeline_pipeline8_no_rule_cap16.txt.  Late arenas are one in
    #  ~100 steps of that loop; more of them than the cap in ONE step would restart in place, counted as regen_unserved.)
    return int(min(E, asked if asked else max(8, E // 128)))


def pregen_plan(cfg, next_step, has_costmap, pipeline=0, install=False, stage_cap=None, map_slots=True, fallback=None,
                fallback_cap=None, late_beside=False, fallback_poll=None, stage_lanes=None):
    """NavSim.enable_pregen's keyword arguments (described there), the world's configuration, its restart mode (NavSim.next_step)
    and whether it has a costmap -> PregenPlan, or enable_pregen's ValueError."""
    if not cfg.auto_reset:
        raise ValueError("enable_pregen needs cfg.auto_reset = 1 (the step advances episode[e] when an arena finishes)")
    E, P, install = cfg.n_envs, int(pipeline), bool(install)
    fallback = bool(install and P > 0 and cfg.regen_min_steps < 4 * P if fallback is None else fallback)
    if fallback and not install:
        raise ValueError("enable_pregen(fallback=True) is a feature of install=True")
    if P < 0 or (P > 0 and cfg.regen_min_steps < 4 * P and not fallback):
        raise ValueError("enable_pregen(pipeline=%d) needs cfg.regen_min_steps >= %d (it is %d): an arena must not want its "
                         "next world before the pass that stages it was waited for -- or fallback=True (install=True)"
                         % (P, 4 * P, cfg.regen_min_steps))
    if install and (not P or cfg.regen_cap < E):
        raise ValueError("enable_pregen(install=True) needs pipeline >= 1 and cfg.regen_cap >= n_envs (every finished arena "
                         "decides alone inside the step: there is no cap in index order)")
    heavy = bool(cfg.regen_plan) or cfg.regen_indoor_ratio > 0.0
    lanes = int(stage_lanes) if stage_lanes else (2 if (install and P and heavy) else 1)
    if lanes not in (1, 2) or (lanes == 2 and not (install and P)):
        raise ValueError("enable_pregen(stage_lanes=%r): 1, or 2 with install=True and pipeline > 0" % (stage_lanes,))
    # a pipelined pass serves what the swaps of P steps marked: P caps' worth of arenas (twice that: what a pass leaves
    # waits for the next one and would be late)
    cap = cfg.regen_cap
    if P:
        # (install: every launch of a pass is sized by the cap, not by what it serves -- 512 slots for the ~35 arenas a pass
        #  of the reference's configuration stages made its planner launches dispatch 30 000 empty workgroups, 367 us each)
        per_step = max(8, E // 64) if install else cfg.regen_cap
        cap = int(min(E, stage_cap if stage_cap else 2 * P * per_step))
    beside = bool(fallback and next_step and late_beside)
    return PregenPlan(
        period=P, install=install, shared_maps=bool(install and map_slots), fallback=fallback, heavy=heavy,
        helper=bool(cfg.regen_plan and cfg.regen_indoor_ratio > 0.0), lanes=lanes, stage_cap=cap, side_priority=0 if P else -1,
        lone=bool(fallback and next_step and not late_beside and not heavy and not has_costmap), beside=beside,
        poll=bool(fallback and (heavy if fallback_poll is None else fallback_poll) and not next_step),
        late_cap=late_cap_for(E, fallback_cap) if fallback else 0, late_defer_scan=beside)


class _StepProduct(object):
    """What one enable_* call of NavSim makes for a launch behind the step (observed pedestrians, goal path, local planner, local
    map): the parameters, two sets of outputs -- they flip with NavSim.cur, so what a call returned stays intact through the next
    step like everything else a step returns -- and the arguments of the call, built here once: every buffer behind them is
    allocated once and only ever written in place.
    params: the rule's ctypes struct (None: a rule without parameters).  layout: blob_layout()'s list; each set is ONE allocation (blob[i]) with the arrays carved
    out of it (buf[i]: {name: tensor}), so that a caller who wants them on the host copies once (host()).
    cfg, st, par: byrefs of the simulator's config and state and of params.  out[i]: the call's output argument for set i -- the
    byref of an out_type filled with buf[i]'s pointers (struct[i]) or, without an out_type, the pointer of the blob itself (a
    layout of one array).  extra: further device state of the product ({name: tensor}) that the call takes through one more
    struct, extra_struct, whose byref is extra_ref."""

    def __init__(self, sim, params, layout, out_type=None, extra=None, extra_struct=None):
        import torch
        self.params, self.layout = params, layout
        self.blob = [torch.zeros(layout[-1][3], dtype=torch.uint8, device=sim.device) for _ in range(2)]
        self.buf = [{k: blob[lo:hi].view(_dtype(d)).view(shape) for k, d, lo, hi, shape in layout[:-1]} for blob in self.blob]
        self.cfg, self.st, self.par = C.byref(sim.cfg), C.byref(sim.st), None if params is None else C.byref(params)
        self.struct = [out_type(**{k: v.data_ptr() for k, v in buf.items()}) if out_type else None for buf in self.buf]
        self.out = [C.byref(s) if out_type else C.c_void_p(blob.data_ptr()) for s, blob in zip(self.struct, self.blob)]
        self.extra, self.extra_struct = extra or {}, extra_struct
        self.extra_ref = None if extra_struct is None else C.byref(extra_struct)

    def host(self, cur):
        """Set cur's arrays as NumPy arrays, from ONE device -> host copy."""
        blob = self.blob[cur].cpu().numpy()
        return {k: blob[lo:hi].view(d).reshape(shape) for k, d, lo, hi, shape in self.layout[:-1]}


class NavSim(object):
    """E arenas resident on one GPU.  `arrays` maps navsim_state field names to numpy arrays or
    torch tensors (host or device); missing optional fields stay NULL."""

    def __init__(self, cfg, arrays, device="cuda:0", launch_order=None, final_obs=False):
        """launch_order: None = longest-first launch order when a launch runs several generations of
        workgroups, True / False = force it on / off (a scheduling hint: results never depend on it).
        final_obs: keep the terminal observation of arenas that restart inside the step that ends their episode
        (cfg.auto_reset = AUTORESET_SAME_STEP; include/navsim.h navsim_step_io.final_obs) -> self.final.
        cfg.auto_reset = AUTORESET_NEXT_STEP: step() hands the done flags of the previous step to the launch as its reset mask
        (the arenas that finished are reset by the next step; regen() then serves those arenas)."""
        torch = require_gpu()
        self.lib = load()
        self.cfg = cfg.copy()
        self.device = torch.device(device)
        # everything the enable_* calls and the lazily made streams set, at its "not enabled" value
        # staging (enable_pregen): pregen_plan()'s record of the mode, the staged state, what a pass serves, the lanes (lane 0 = want /
        # stage_io / stage_ws / side)
        self.pregen = self.pg_install = False
        self.pg_period = self.pg_k = self.pg_passes = self.stage_cap = 0
        self.pg_open, self.pg_swapped, self.pg_staged, self.stage_lane = [], [], [], []
        self.stage_t, self.stage_st, self.stage_cfg, self.stage_obs, self.stage_io, self.stage_ws = {}, None, None, None, None, None
        self.pg_plan = self.want = self.mark = self.ready = self.side = self.ev_swapped = self.ev_staged = None
        # fallback: the arenas that finished before their world was staged (flags the step writes, navsim_regen for them)
        self.late, self.late_cfg, self.late_ws, self.late_cap = None, None, None, 0
        self.late_poll = self.lone = False
        # reset_arenas with staged worlds: the flags navsim_reset_install writes; its fallback's workspace and cap
        # where enable_pregen made none (rule-only worlds)
        self.rs_late, self.rs_ws, self.rs_cap = None, None, 0
        # next-step "beside" form: the fallback on a stream of its own beside the next step's launch
        self.late2 = self.urgent = self.ev_stepped = self.ev_urgent = None
        # overlap and graphs: the re-plan inside or beside the step, the captured steps
        self.pg_replan_cap, self.pg_replan_in_step = 0, True
        self._side = self._regen_helper = self._action_ref = None
        self._graphs, self._graph_args, self._graph_cfg = {}, None, None
        # policy and orca
        self.policy_t, self.policy_w, self._scan_stream, self._orca_default = {}, None, None, None
        # episode statistics (enable_episode_stats): the accumulators, the totals, the two sets of published rows (they flip with
        # self.cur like out_buf) and, per parity, the arguments of navsim_episode_stats_update
        self.ep_acc, self.ep_totals, self.ep_buf, self._ep_args = None, None, None, {}
        # the other launches behind the step: 'ped_observe', 'goal_path', 'dwa', 'local_map', 'scan_labels' -> the _StepProduct its enable_* call
        # made (parameters, two sets of outputs, the call's arguments; the goal path's field, keys and rebuild counter as its extra)
        self.products = {}
        self.t = {}
        self.st = abi.NavsimState()
        for name, (dtype, shape) in abi.STATE_LAYOUT.items():
            a = arrays.get(name)
            if a is None:
                setattr(self.st, name, None)
                continue
            if name == "field" and self.cfg.field_format != abi.FIELD_F32:
                t = a.to(self.device).contiguous()              # packed blob, kept as is
                want = self.lib.navsim_field_bytes(self.cfg.n_envs, self.cfg.map_h, self.cfg.map_w,
                                                   self.cfg.field_format)
                if t.numel() * t.element_size() != want:
                    raise ValueError("field blob has %d bytes, expected %d" % (t.numel() * t.element_size(), want))
                self.t[name] = t
                setattr(self.st, name, t.data_ptr())
                continue
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(np.ascontiguousarray(a))
            t = a.to(device=self.device, dtype=_dtype(dtype)).contiguous()
            if t.data_ptr() == a.data_ptr():
                t = t.clone()
            want = abi.resolve_shape(shape, self.cfg)
            if tuple(t.shape) != want:
                raise ValueError("%s: shape %s, expected %s" % (name, tuple(t.shape), want))
            self.t[name] = t
            setattr(self.st, name, t.data_ptr())
        if self.cfg.closed_maps and "rect_index" in self.t:
            # cfg.closed_maps is an assertion about THIS world that the LDS form of the march relies on without a bounds
            # test (include/navsim.h): verify it once, against the distance fields as they stand (round-4 advisor)
            n_open = torch.zeros(1, dtype=torch.int32, device=self.device)
            check(self.lib.navsim_world_closed(C.byref(self.cfg), C.byref(self.st), _ptr(n_open), _stream()), "navsim_world_closed")
            if int(n_open.item()):
                raise ValueError("cfg.closed_maps = 1, but %d arenas have a map without a closed ring of 3 occupied cells "
                                 "(navsim_maps_closed / navsim_world_closed): clear closed_maps or close the maps" % int(n_open.item()))
        self.due = None
        if "ped_waypoints" in self.t:
            # ABI 5: the index of every pedestrian's current waypoint (a route starts at its first one), and the two buffers
            # of "waits for navsim_replan" flags the step writes / navsim_step_part reads.  The flags of the LATEST step
            # live in due[self.cur] -- they flip with the observation buffers (_flip)
            if "ped_wp_head" not in self.t:
                self.t["ped_wp_head"] = torch.zeros((self.cfg.n_envs, self.cfg.max_peds), dtype=torch.int32, device=self.device)
                self.st.ped_wp_head = self.t["ped_wp_head"].data_ptr()
            self.due = [torch.zeros(self.cfg.n_envs, dtype=torch.int64, device=self.device) for _ in range(2)]
            self.st.ped_due = self.due[0].data_ptr()
            self.st.ped_due_prev = self.due[1].data_ptr()
        if "done_steps" not in self.t and self.cfg.auto_reset:  # length of every arena's last episode (cfg.regen_min_steps)
            self.t["done_steps"] = torch.zeros(self.cfg.n_envs, dtype=torch.int32, device=self.device)
            self.st.done_steps = self.t["done_steps"].data_ptr()
        if "counters" not in self.t:                            # what the library's caps left unserved (include/navsim.h)
            self.t["counters"] = torch.zeros(abi.N_COUNTERS, dtype=torch.int64, device=self.device)
            self.st.counters = self.t["counters"].data_ptr()
        if "beam_table" not in self.t:                          # accelerator table, built on device
            tab = torch.empty((self.cfg.n_beams, 2), dtype=torch.float64, device=self.device)
            check(self.lib.navsim_beam_table(C.byref(self.cfg), _ptr(tab), _stream()), "navsim_beam_table")
            self.t["beam_table"] = tab
            self.st.beam_table = tab.data_ptr()
        # longest-first launch order (navsim_launch_order): the step measures every arena's workgroup, every
        # few steps the arenas are re-sorted so that the slow ones start first (lpt_period = 0 disables).  8 measured
        # against 4 / 16 / 32 / 64 in profiles/r03_lpt/: the costs drift slowly, the sort is 13 us.  With the sort inside the step's
        # launch (profiles/r12_lpt/) periods 1 and 2 win 1.7 % on c2 and 2.9 % on c3 and nothing measurable on c4: 8 stays
        self.lpt_period = 8
        self._steps_launched = 0
        # only when a launch runs several generations of workgroups: with one generation everything starts
        # at once and the order is irrelevant (threads per arena as dispatch_step picks them)
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count or 256
        block = self.cfg.step_block or (                    # step_plan.hpp pick_step_block (the ABI has no query for it)
            64 if self.cfg.n_beams <= 64 else (256 if self.cfg.n_envs >= 12 * n_cu or self.cfg.n_beams <= 256 else
                                               (512 if self.cfg.n_envs > 2 * n_cu or self.cfg.n_beams <= 512 else 1024)))
        generations = self.cfg.n_envs * (block // 64) / float(32 * n_cu)
        if (launch_order is True or (launch_order is None and generations > 1.25)) and "arena_cost" not in self.t:
            self.t["arena_cost"] = torch.zeros(self.cfg.n_envs, dtype=torch.int32, device=self.device)
            self.t["launch_order"] = torch.arange(self.cfg.n_envs, dtype=torch.int32, device=self.device)
            self.st.arena_cost = self.t["arena_cost"].data_ptr()
            self.st.launch_order = self.t["launch_order"].data_ptr()
        # The sort runs INSIDE a step's launch where it can (navsim_step_sorted: a front workgroup beside the arenas'), on the
        # costs of the step before, into the order of the steps that follow: a second buffer of each, alternated in _launch.
        # t["arena_cost"] / t["launch_order"] always name the pair st points at.  _reorder() only marks the sort as due.
        self._sort_pending = False
        self._sort_spare = None                     # (cost, order): the buffers st does not point at, made on first use
        self.sort_in_launch = hasattr(self.lib, "navsim_step_sorted")   # False: the library has no such export, or it refused
        self.sorts_in_launch = 0                    # sorts that ran inside a step's launch
        E = self.cfg.n_envs
        D = self.cfg.n_scan_stack * self.cfg.n_beams + abi.OBS_TAIL
        self.obs_buf = [torch.zeros((E, D), dtype=torch.float32, device=self.device) for _ in range(2)]
        self.cur = 0
        # what step() returns beside the observation (reward, done, info, the two goal arrays): two sets, flipped with the
        # observation buffers, so that the arrays a step returned stay intact through the NEXT step (round-4 advisor: the
        # env handed out views of single buffers that the next step overwrote -- `obs = next_obs`, `dones.append(done)`)
        self.out_buf = [{k: torch.zeros(abi.resolve_shape(s, self.cfg), dtype=_dtype(d), device=self.device)
                         for k, (d, s) in abi.IO_LAYOUT.items() if k not in ("obs", "obs_prev", "action")} for _ in range(2)]
        # ABI 7: with a time limit (cfg.max_episode_steps > 0 when the simulator is made) the step also returns `truncated`,
        # flipped with the other outputs; without one io.truncated stays NULL and the outputs keep their ABI-6 keys
        if self.cfg.max_episode_steps > 0:
            for b in self.out_buf:
                b.update({k: torch.zeros(abi.resolve_shape(s, self.cfg), dtype=_dtype(d), device=self.device)
                          for k, (d, s) in abi.LIMIT_LAYOUT.items()})
        self.action = torch.zeros((E, 2), dtype=torch.float64, device=self.device)
        self.io = abi.NavsimStepIO()
        self.io.action = self.action.data_ptr()
        for k, v in self.out_buf[0].items():
            setattr(self.io, k, v.data_ptr())
        # ABI 6: terminal observations (same-step restarts), kept in pairs like everything a step returns
        self.final_buf = None
        if final_obs:
            self.final_buf = [{k: torch.zeros(abi.resolve_shape(s, self.cfg), dtype=_dtype(d), device=self.device)
                               for k, (d, s) in abi.FINAL_LAYOUT.items()} for _ in range(2)]
        self.next_step = self.cfg.auto_reset == abi.AUTORESET_NEXT_STEP

    @property
    def obs(self):
        return self.obs_buf[self.cur]

    @property
    def out(self):
        """reward / done / is_success / is_crash / distance / achieved_goal / desired_goal of the latest step; with a time limit
        (cfg.max_episode_steps > 0 when the simulator was made) also truncated: the arenas whose episode the limit cut."""
        return self.out_buf[self.cur]

    @property
    def final(self):
        """final_obs / final_goals of the latest step: rows of the arenas whose done flag that step set (others: stale)."""
        return None if self.final_buf is None else self.final_buf[self.cur]

    @property
    def reset_flags(self):
        """AUTORESET_NEXT_STEP: the arenas the latest step RESET (= the done flags of the step before it)."""
        return self.out_buf[1 - self.cur]["done"]

    def _flip(self):
        self.io.obs_prev = self.obs_buf[self.cur].data_ptr()
        self.io.obs = self.obs_buf[1 - self.cur].data_ptr()
        # NEXT_STEP: whoever finished in the latest step (its done flags, out_buf[cur]) is reset by the launch that follows
        self.io.reset_mask = self.out_buf[self.cur]["done"].data_ptr() if self.next_step else None
        if self.final_buf is not None:
            for k, v in self.final_buf[1 - self.cur].items():
                setattr(self.io, k, v.data_ptr())
        for k, v in self.out_buf[1 - self.cur].items():
            setattr(self.io, k, v.data_ptr())
        if self.due is not None:                    # the launch reads the latest flags and writes the other buffer
            self.st.ped_due_prev = self.due[self.cur].data_ptr()
            self.st.ped_due = self.due[1 - self.cur].data_ptr()

    def _latest_flags(self):
        """st.ped_due -> the flags the latest step wrote (due[self.cur]): what navsim_replan / navsim_regen read and clear.
        (True after every step by construction; enable_graphs captures both parities from one state.)"""
        if self.due is not None:
            self.st.ped_due = self.due[self.cur].data_ptr()
            self.st.ped_due_prev = self.due[1 - self.cur].data_ptr()

    def reset_obs(self, mask=None):
        """First observation of an episode (reference reset(), env.py:808-831) for masked envs."""
        # a reset-only launch writes the goal arrays of the arenas it resets and nothing else: the other set starts as a copy
        for k, v in self.out_buf[1 - self.cur].items():
            v.copy_(self.out_buf[self.cur][k])
        m = None
        if mask is not None:
            import torch
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
        # an arena that is reset is not finished: its done flag (NEXT_STEP: the next launch's reset mask) is cleared, and with
        # it the time limit's truncated flag
        for k in [k for k in ("done", "truncated") if k in self.out_buf[0]]:
            if m is None:
                self.out_buf[1 - self.cur][k].zero_()
            else:
                self.out_buf[1 - self.cur][k].mul_(m == 0)
        self._flip()
        check(self.lib.navsim_reset_obs(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), _ptr(m), _stream()),
              "navsim_reset_obs")
        self.clear_episode_stats(m)
        if self.due is not None:                    # a reset-only launch advances nobody: the latest flags stay the latest
            self.due[1 - self.cur].copy_(self.due[self.cur])
        self.cur = 1 - self.cur
        return self.obs

    def _reorder(self):
        # re-sort before steps 2..5 (short runs profit from the very first measured costs), then every lpt_period-th
        self._steps_launched += 1
        n = self._steps_launched
        # (nothing is launched here: the plain step sorts inside its own launch, every other launcher calls _flush_sort first)
        if "launch_order" in self.t and self.lpt_period > 0 and (2 <= n <= 5 or n % self.lpt_period == 0):
            self._sort_pending = True

    def _flush_sort(self):
        """A sort that is due, as a kernel of its own ahead of the launch that follows (navsim_launch_order): the launchers whose
        kernels have no front workgroup for it, and libraries without navsim_step_sorted."""
        if self._sort_pending:
            self._sort_pending = False
            check(self.lib.navsim_launch_order(_ptr(self.t["arena_cost"]), _ptr(self.t["launch_order"]), self.cfg.n_envs,
                                               _stream()), "navsim_launch_order")

    def _launch_sorted(self):
        """navsim_step_sorted: the step writes the other cost buffer while the front workgroup sorts the costs of the step before
        into the other order buffer, which the launches that follow take (stream order makes it visible to them).
        False = not launched (NAVSIM_E_UNSUPPORTED): the caller takes the separate kernel, from now on."""
        import torch
        if self._sort_spare is None:
            self._sort_spare = (torch.zeros_like(self.t["arena_cost"]), self.t["launch_order"].clone())
        cost_next, order_next = self._sort_spare
        cost, order = self.t["arena_cost"], self.t["launch_order"]
        self.st.arena_cost = cost_next.data_ptr()
        rc = self.lib.navsim_step_sorted(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), _ptr(cost), _ptr(order_next), _stream())
        if rc == abi.E_UNSUPPORTED:
            self.st.arena_cost = cost.data_ptr()
            self.sort_in_launch = False
            return False
        if rc:
            self.st.arena_cost = cost.data_ptr()
            check(rc, "navsim_step_sorted")
        self.t["arena_cost"], self.t["launch_order"] = cost_next, order_next
        self.st.launch_order = order_next.data_ptr()
        self._sort_spare = (cost, order)
        self._sort_pending = False
        self.sorts_in_launch += 1
        return True

    def _set_action(self, action):
        """io.action -> the caller's tensor where it is resident in the step's own format (stream-ordered: no copy), else the
        simulator's buffer with a copy of it."""
        import torch
        if (isinstance(action, torch.Tensor) and action.is_cuda and action.dtype == torch.float64 and action.is_contiguous()
                and action.device == self.device and action.numel() == self.action.numel()):
            self.io.action = action.data_ptr()
            self._action_ref = action
        else:
            self.action.copy_(self._as(action, self.action))
            self.io.action = self.action.data_ptr()

    def step(self, action=None):
        """One fused launch: NavGymEnv.step for all E arenas.  `action` [E,2] (v, omega)."""
        if action is not None:
            self._set_action(action)
        self._reorder()
        self._flip()
        self._launch()
        self.cur = 1 - self.cur
        return self.obs, self.out

    def _launch(self):
        """The step's launch on the current stream: navsim_step, or navsim_step_install behind the staging pass it may rest on."""
        if not self.pg_install and self._sort_pending and self.sort_in_launch and self._launch_sorted():
            return
        self._flush_sort()
        if not self.pg_install:
            rc = self.lib.navsim_step(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), _stream())
            if rc:
                check(rc, "navsim_step")
            return
        import torch                                            # enable_pregen(pipeline=P, install=True)
        main = torch.cuda.current_stream()
        P, k = self.pg_period, self.pg_k
        if k % P == 0 and k >= 2 * P:
            main.wait_event(self.pg_staged[(k // P - 2) % 3])   # the pass queued two periods ago; the later two may still run
        # what every navsim_step_install* call starts with; behind it: the late flags, the re-plan cap, the stream
        head = (C.byref(self.cfg), C.byref(self.st), C.byref(self.io), C.byref(self.stage_st), _ptr(self.stage_obs), _ptr(self.mark),
                _ptr(self.ready))
        stream = C.c_void_p(main.cuda_stream)
        if self.late2 is not None:
            return self._launch_next_step(main, head, stream)
        # pg_replan_cap > 0 (worlds with planned pedestrian routes): navsim_replan of the previous step's flags inside this launch
        # where the search fits the arena's workgroup (navsim_step_install_replan); else the caller re-plans behind the step
        late = None if self.lone else self.late
        if self.pg_replan_cap > 0 and self.pg_replan_in_step:
            rc = self.lib.navsim_step_install_replan(*head, _ptr(late), int(self.pg_replan_cap), stream)
            if rc == 0:
                return
            if rc != abi.E_UNSUPPORTED:
                check(rc, "navsim_step_install_replan")
            self.pg_replan_in_step = False
        rc = self.lib.navsim_step_install(*head, _ptr(late), stream)
        if rc == abi.E_UNSUPPORTED and late is None and self.late is not None:
            self.lone = False                                   # (fewer than 256 threads per arena: flags + navsim_regen behind the step)
            rc = self.lib.navsim_step_install(*head, _ptr(self.late), stream)
        check(rc, "navsim_step_install")

    def _launch_next_step(self, main, head, stream):
        """NEXT_STEP with staged worlds: the step's launch (arenas that finished in the previous call install their staged worlds
        at its front) and, on the `urgent` stream at the same time, navsim_regen for the arenas that call flagged as late."""
        prev, nxt = self.late2[self.cur], self.late2[1 - self.cur]      # (self.cur: the buffers of the PREVIOUS call)
        cap = int(self.pg_replan_cap) if self.pg_replan_in_step else 0
        rc = self.lib.navsim_step_install_next(*head, _ptr(nxt), _ptr(prev), cap if cap > 0 else -1, stream)
        if rc == abi.E_UNSUPPORTED and cap > 0:                 # the search does not fit the arena's workgroup: re-plan behind the step
            self.pg_replan_in_step = False
            rc = self.lib.navsim_step_install_next(*head, _ptr(nxt), _ptr(prev), -1, stream)
        check(rc, "navsim_step_install_next")
        # beside it: the new worlds of the arenas the previous call found unstaged (mostly nobody: launches that find nothing to do)
        urgent = self.urgent
        urgent.wait_event(self.ev_stepped)                      # the previous call (its flags, its state) -- NOT this launch
        self._late_cfg_now().defer_reset_scan = 1
        # (self.io: this call's buffers -- _flip() ran: its obs stays; no fork: the helper stream belongs to the staging passes)
        self._call_regen(self.late_cfg, self.late_ws, urgent, "navsim_regen (arenas whose world was not staged, beside the step)",
                         current_obs=False, latest_flags=False, fork=False, done=prev, reset_mask=None)
        self.ev_urgent.record(urgent)
        main.wait_event(self.ev_urgent)                         # whatever follows this step on the caller's stream sees both
        self.ev_stepped.record(main)

    # arrays navsim_regen writes: the staged state of enable_pregen() owns a copy of each
    STAGED = ("field", "field_overflow", "rect_table", "rect_index", "costmap", "scan_noise_std", "robot_pose", "robot_goal", "prev_action",
              "prev_pose", "n_hist", "steps", "episode", "n_peds", "ped_pose", "ped_vel", "ped_prev_yaw", "ped_dist",
              "ped_v_pref", "ped_has_legs", "ped_waypoints", "ped_n_waypoints", "ped_wp_head", "ped_goal", "spawn_pose", "spawn_goal")

    MAPS = ("field", "field_overflow", "rect_table", "rect_index", "costmap")      # the per-map arrays (navsim_state.map_slot)

    def enable_pregen(self, scratch_bytes=4 << 30, pipeline=0, install=False, stage_cap=None, map_slots=True, fallback=None,
                      fallback_cap=None, late_beside=False, fallback_poll=None, stage_lanes=None):
        """navsim_regen off the step's critical path (include/navsim.h navsim_regen_swap): the world every arena will
        get at the end of its CURRENT episode -- a function of (seed, global arena, episode number) only -- is generated
        ahead of time into a second, staged state by the ordinary navsim_regen on a side stream; regen() then only
        installs the staged worlds of the finished arenas (one copy kernel on the caller's stream) and queues the next
        staging pass.  Same state, same observations as navsim_regen, bit for bit.  Needs cfg.auto_reset = 1.

        pipeline = P > 0 (round 5): a staging pass every P steps, and the steps wait only for the pass queued two periods
        earlier -- a pass has P .. 2 P steps of wall time to finish beside the step kernels instead of having to fit between
        two steps.  That needs the simulation's own guarantee that an arena does not want its next world sooner:
        cfg.regen_min_steps >= 4 P (shorter episodes restart in place, in navsim_regen and the oracle alike), which makes
        the outcome independent of timing; counters()['regen_late'] stays 0.

        install=True (with pipeline): no swap kernel either -- step() is navsim_step_install, in which a finished arena's own
        workgroup copies its staged world in place of the restart's second scan; regen() only queues the passes.  Every
        arena decides alone, so cfg.regen_cap must be >= n_envs (no cap in index order); `stage_cap` bounds what ONE pass
        stages (default: what 2 P steps finish at one arena in 64 per step) -- arenas beyond it wait for the next pass.
        fallback (with install; default: on when cfg.regen_min_steps < 4 P): no rule is needed -- an arena that finishes before
        its world is staged is regenerated on the spot by the ordinary navsim_regen (regen() launches it after every step, with
        the flags the step wrote: launches that find nothing to do when nobody was late, `fallback_cap` arenas at most -- more late arenas than that in
        ONE step restart on their old map like navsim_regen's own cap, counters()['regen_unserved']).  The
        rollout then equals step + navsim_regen whatever the passes' timing, also with cfg.regen_min_steps = 0: the reference's
        "a new map at every reset()" unchanged.
        fallback_poll (with fallback; round 6): the fallback's navsim_regen is launched only when the step flagged somebody -- regen()
        reads "any flag set?" back from the device (one byte, a host wait for the step's launch) instead of enqueueing the
        call's launches blind.  Default: on where that call is the long chain of worlds with corridor maps or planned starts
        (~18 launches, ~160 us of mostly empty launches behind every ~80 us step of the reference's configuration:
        profiles/r05_refdef/timeline_pipeline8_no_rule_cap16.txt), off where it is three short launches (c5) and under graph
        capture.  Same rollout either way.
        stage_lanes (with install and pipeline; round 6): 2 = the staging passes alternate between two side streams, each with its own
        share of the arenas (navsim_regen_stage_part: groups of four by mark word), workspace and helper stream, so that two
        passes run at the same time -- a pass for corridor maps with planned starts is a chain of ~25 latency-bound launches
        (the planner's four wait for their longest search each) that leaves the chip idle, and the passes' rate is what bounds the
        reference's configuration once the fallback's blind launches are gone.  Default: 2 for those worlds, else 1.
        map_slots (with install): the live and the staged state share the per-map arrays (t['field'], ... then hold 2 E slots)
        and each has a slot table (navsim_state.map_slot); an install exchanges two table entries instead of copying the
        map -- numpy_state() resolves the table, code that indexes t['field'] by arena must go through t['map_slot']."""
        import torch
        # the whole decision first (it raises what this call refuses): a refused call leaves the simulator as it was
        plan = pregen_plan(self.cfg, self.next_step, "costmap" in self.t, pipeline, install, stage_cap, map_slots, fallback,
                           fallback_cap, late_beside, fallback_poll, stage_lanes)
        self.pg_plan = plan
        E, P = self.cfg.n_envs, plan.period
        self.pg_period, self.pg_k = P, 0
        self.ready = torch.zeros(2 * E, dtype=torch.int64, device=self.device) if P else None
        # (the per-map arrays of a slot-table world are allocated ONCE at twice the size below instead of cloned and then concatenated:
        #  fresh device memory is what the first reset() of a large world waits for -- 50 GB at 4096 arenas of 1000 x 1000 cells)
        self.stage_t = {k: self.t[k].clone() for k in self.STAGED if k in self.t and not (plan.shared_maps and k in self.MAPS)}
        self.stage_t["episode"] = self.t["episode"] + 1
        self.stage_st = abi.NavsimState()
        C.memmove(C.byref(self.stage_st), C.byref(self.st), C.sizeof(self.st))
        for k, v in self.stage_t.items():
            setattr(self.stage_st, k, v.data_ptr())
        if plan.shared_maps:
            for k in self.MAPS:
                if k in self.t:
                    live = self.t[k]
                    n = live.shape[0]
                    both = torch.empty((2 * n,) + tuple(live.shape[1:]), dtype=live.dtype, device=live.device)
                    both[:n].copy_(live); both[n:].copy_(live)          # (the staged half: any valid world; _stage_all() redraws it)
                    del live
                    self.t[k] = self.stage_t[k] = both
                    setattr(self.st, k, both.data_ptr()); setattr(self.stage_st, k, both.data_ptr())
            self.t["map_slot"] = torch.arange(E, dtype=torch.int32, device=self.device)
            self.stage_t["map_slot"] = torch.arange(E, 2 * E, dtype=torch.int32, device=self.device)
            self.st.map_slot = self.t["map_slot"].data_ptr()
            self.stage_st.map_slot = self.stage_t["map_slot"].data_ptr()
        self.stage_st.arena_cost = None
        self.stage_st.launch_order = None
        self.stage_st.counters = None          # staging ahead serves nobody yet: navsim_regen_swap counts the installs
        self.stage_st.ped_due = None           # the live arenas' flags: navsim_regen_swap clears them at the install
        self.stage_st.ped_due_prev = None
        self.stage_obs = torch.zeros_like(self.obs_buf[0])
        self.want = torch.ones(E, dtype=torch.uint8, device=self.device)
        self.mark = torch.zeros((E + 3) // 4 * 4, dtype=torch.uint8, device=self.device)   # consumed in 32-bit words
        self.stage_io = abi.NavsimStepIO()
        self.stage_io.obs = self.stage_obs.data_ptr()
        self.stage_io.done = self.want.data_ptr()
        self._stage_all(scratch_bytes)
        self.stage_cap = plan.stage_cap
        self.stage_cfg = self.cfg.copy()
        self.stage_cfg.regen_cap = self.stage_cap
        nbytes = self.lib.navsim_regen_workspace_bytes(C.byref(self.stage_cfg))
        self.stage_ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        # a high-priority stream: its few small kernels go first whenever wave slots free up.  (Measured and dropped:
        # CU-masked streams -- hipExtStreamCreateWithCUMask, 8 / 16 / 32 CUs for the staging passes and the rest for the
        # steps -- did not make the passes overlap a step kernel that fills the chip: c5 3.0 M env-steps/s either way.
        # Pipelined passes: the stream's priority, either way round, changes nothing -- c5 62.8 us per step.)
        # (Its priority: high for the pass that must fit between two steps; ordinary for pipelined passes, which have 2 P steps
        # of slack -- and a process that has used a high-priority stream replays hipGraphs ~10 us per kernel slower from then
        # on: a reference-default environment built afterwards ran at 0.59 M env-steps/s instead of 0.87 M,
        # profiles/_diag/after_pregen.py.)
        self.side = concurrent_stream(self.device, priority=plan.side_priority)
        # navsim_regen's helper stream (the distance transform of new corridor maps beside the searches): beside the steps AND
        # beside the passes -- three streams, three hardware queues
        if plan.helper:
            self._regen_helper = concurrent_stream(self.device, beside=[torch.cuda.current_stream(self.device), self.side])
            check(self.lib.navsim_regen_helper(C.c_void_p(self._regen_helper.cuda_stream)), "navsim_regen_helper")
        # lane 0 = the objects above; lane 1: its own want[], io, workspace, stream and helper stream
        self.stage_lane = [dict(want=self.want, io=self.stage_io, ws=self.stage_ws, side=self.side,
                                helper=self._regen_helper)]
        if plan.lanes == 2:
            want2 = torch.zeros(E, dtype=torch.uint8, device=self.device)
            io2 = abi.NavsimStepIO()
            C.memmove(C.byref(io2), C.byref(self.stage_io), C.sizeof(io2))
            io2.done = want2.data_ptr()
            side2 = concurrent_stream(self.device, beside=[torch.cuda.current_stream(self.device), self.side], priority=0)
            helper2 = None
            if self._regen_helper is not None:
                helper2 = concurrent_stream(self.device, beside=[torch.cuda.current_stream(self.device), self.side, side2])
            self.stage_lane.append(dict(want=want2, io=io2, ws=torch.zeros(nbytes, dtype=torch.uint8, device=self.device), side=side2,
                                        helper=helper2))
        self.pg_passes = 0
        self.ev_swapped, self.ev_staged = torch.cuda.Event(), torch.cuda.Event()
        self.ev_staged.record(torch.cuda.current_stream())
        self.pg_swapped = [torch.cuda.Event() for _ in range(3)]      # pass j uses slot j % 3; step j P waits for pass j - 2
        self.pg_staged = [torch.cuda.Event() for _ in range(3)]
        self.pregen = True
        self.pg_install = plan.install
        self.pg_replan_cap, self.pg_replan_in_step = 0, True       # (set pg_replan_cap to re-plan inside the step's launch, _launch)
        # the fallback: flags the step writes, and a navsim_regen of its own size for the arenas they name
        self.late = torch.zeros(E, dtype=torch.uint8, device=self.device) if plan.fallback else None
        self.lone = plan.lone
        self.late2 = None
        if plan.beside:
            self.late2 = [torch.zeros(E, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.urgent = concurrent_stream(self.device, beside=[torch.cuda.current_stream(self.device), self.side])
            self.ev_stepped, self.ev_urgent = torch.cuda.Event(), torch.cuda.Event()
            self.ev_stepped.record(torch.cuda.current_stream())
        self.late_poll = plan.poll
        if plan.fallback:
            self.late_cfg = self.cfg.copy()
            self.late_cap = plan.late_cap
            self.late_cfg.regen_cap = self.late_cap
            if plan.late_defer_scan:
                self.late_cfg.defer_reset_scan = 1          # (the launch skips a flagged arena altogether: its row is navsim_regen's,
                                                            #  also when the arena lies beyond this call's cap and restarts in place)
            self.late_ws = torch.zeros(self.lib.navsim_regen_workspace_bytes(C.byref(self.late_cfg)), dtype=torch.uint8, device=self.device)

    def restage_all(self, scratch_bytes=4 << 30, slots_from_live=False):
        """After regenerate_all() on a world with enable_pregen(): every staged world is stale (reset() drew new worlds and,
        the second time, new episode numbers) -- stage the world behind each arena's current one again.
        slots_from_live: the live slot table was replaced (load_state_dict) -- the staged one is its complement."""
        import torch
        for ln in self.stage_lane:
            ln["side"].synchronize()
        torch.cuda.current_stream().synchronize()
        for ln in self.stage_lane[1:]:
            ln["want"].zero_()
        if slots_from_live and "map_slot" in self.t:
            free = torch.ones(2 * self.cfg.n_envs, dtype=torch.bool, device=self.device)
            free[self.t["map_slot"].long()] = False
            self.stage_t["map_slot"].copy_(torch.nonzero(free).flatten().to(torch.int32))
        self.stage_t["episode"].copy_(self.t["episode"] + 1)
        self.want.fill_(1)
        self.mark.zero_()
        if self.late2 is not None:
            self.urgent.synchronize()
            for b in self.late2:
                b.zero_()
            self.ev_stepped.record(torch.cuda.current_stream())
        self.pg_k, self.pg_open = 0, []
        self._stage_all(scratch_bytes)
        self.ev_staged.record(torch.cuda.current_stream())

    def _stage_all(self, scratch_bytes):
        """The (first) staging of every arena, in chunks of as many arenas as the scratch allows (reset path)."""
        import torch
        E = self.cfg.n_envs
        cfg = self.cfg.copy()
        ws = self._regen_chunk(cfg, scratch_bytes)
        for _ in range((E + cfg.regen_cap - 1) // cfg.regen_cap):
            check(self.lib.navsim_regen_stage(C.byref(cfg), C.byref(self.stage_st), C.byref(self.stage_io), _ptr(self.want),
                                              _ptr(self.mark), _ptr(self.ready), _ptr(ws), ws.numel(), _stream()),
                  "navsim_regen_stage (first staging)")
        torch.cuda.current_stream().synchronize()
        assert int(self.want.sum().item()) == 0

    def _regen_pregen(self):
        import torch
        main = torch.cuda.current_stream()
        P, k = self.pg_period, self.pg_k
        self.pg_k += 1
        j = k // P if P else 0
        if self.pg_install:                              # step() has installed; only the passes are left
            need = self.late is not None and self.late2 is None and not self.lone
            if need and self.late_poll and not torch.cuda.is_current_stream_capturing():
                # (the host waits for the step's launch here; what it saves is the fallback's blind launches behind EVERY step)
                need = bool(self.late.any().item())
            if need:   # ... and whoever finished before its world was staged (rare): now
                # this call does not fork: navsim_regen's helper stream belongs to the staging passes, whose distance transforms the
                # fallback's (mostly empty) fork / join would queue behind -- the pass back on the step's critical path
                # (round-5 advisor).  A helper equal to the call's own stream means "no fork" (include/navsim.h).
                self._call_regen(self._late_cfg_now(), self.late_ws, main, "navsim_regen (arenas whose world was not staged)",
                                 fork=False, done=self.late)
            if k % P == 0:
                self._latest_flags()
                self._queue_pass(main, self.pg_swapped[j % 3], self.pg_staged[j % 3])
            return self.obs
        if not P:
            main.wait_event(self.ev_staged)             # the staging pass that served the arenas of the last swap
        elif k % P == 0 and j >= 2:
            main.wait_event(self.pg_staged[(j - 2) % 3])    # the pass queued two periods ago; the later two may still run
        self._latest_flags()
        io = self._io_copy(obs=self.obs)
        check(self.lib.navsim_regen_swap(C.byref(self.cfg), C.byref(self.st), C.byref(self.stage_st), C.byref(io),
                                         _ptr(self.stage_obs), _ptr(self.want), _ptr(self.mark), _ptr(self.ready),
                                         C.c_void_p(main.cuda_stream)),
              "navsim_regen_swap")
        if P and k % P != 0:
            return self.obs                             # the next pass takes these arenas' marks with it
        swapped, staged = (self.pg_swapped[j % 3], self.pg_staged[j % 3]) if P else (self.ev_swapped, self.ev_staged)
        self._queue_pass(main, swapped, staged)
        return self.obs

    def pregen_sync(self):
        """Pipelined pre-generation: wait (host) for every staging pass queued so far and start the period count anew -- the
        next 2 P steps then rest on no earlier pass.  Call it before capturing steps into a hipGraph: a captured wait must
        not refer to an event recorded outside the capture."""
        import torch
        for ln in self.stage_lane:
            ln["side"].synchronize()
        torch.cuda.current_stream().synchronize()
        self.pg_k = 0
        self.pg_open = []

    def pregen_join(self):
        """Pipelined pre-generation: the current stream waits for the staging passes still open (the last two periods') --
        the join a hipGraph capture needs before it ends; a replay then starts like pregen_sync() left things."""
        import torch
        main = torch.cuda.current_stream()
        for ev in self.pg_open:
            main.wait_event(ev)
        self.pg_k = 0
        self.pg_open = []

    def _queue_pass(self, main, swapped, staged):
        """A staging pass on the side stream, behind everything `main` holds now."""
        if self.pg_period:
            self.pg_open = (self.pg_open + [staged])[-2:]
        n = len(self.stage_lane)
        part = self.pg_passes % n
        ln = self.stage_lane[part]
        self.pg_passes += 1
        side = ln["side"]
        swapped.record(main)
        side.wait_event(swapped)
        C.memmove(C.byref(self.stage_cfg), C.byref(self.cfg), C.sizeof(self.cfg))     # the configuration as it stands NOW
        self.stage_cfg.regen_cap = self.stage_cap
        ws = ln["ws"]
        if n > 1 and ln["helper"] is not None:                 # this lane's passes fork their distance transforms to their own helper
            self.lib.navsim_regen_helper(C.c_void_p(ln["helper"].cuda_stream))
        check(self.lib.navsim_regen_stage_part(C.byref(self.stage_cfg), C.byref(self.stage_st), C.byref(ln["io"]), _ptr(ln["want"]),
                                               _ptr(self.mark), _ptr(self.ready), _ptr(ws), ws.numel(), part, n,
                                               C.c_void_p(side.cuda_stream)),
              "navsim_regen_stage_part")
        if n > 1 and ln["helper"] is not None and self._regen_helper is not None:
            self.lib.navsim_regen_helper(C.c_void_p(self._regen_helper.cuda_stream))
        staged.record(side)

    def close(self):
        """Waits for what this simulator has in flight on streams of its own (staging passes, the overlapped re-plan): their
        kernels write into arrays that are about to be released."""
        extra = [ln[k] for ln in self.stage_lane[1:] for k in ("side", "helper")]
        for st in [self.side, self._side, self._scan_stream, self._regen_helper, self.urgent] + extra:
            if st is not None:
                try:
                    st.synchronize()
                except Exception:
                    pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _choose_regen_helper(self):
        """navsim_regen's helper stream for worlds whose reset forks (include/navsim.h navsim_regen_helper): one that really runs
        beside the current stream, chosen once (before any hipGraph capture of the call)."""
        if self._regen_helper is None and self.cfg.regen_plan and self.cfg.regen_indoor_ratio > 0.0:
            self._regen_helper = concurrent_stream(self.device)
            check(self.lib.navsim_regen_helper(C.c_void_p(self._regen_helper.cuda_stream)), "navsim_regen_helper")

    def _io_copy(self, **fields):
        """self.io by value, with `fields` (name = tensor or None) on top."""
        io = abi.NavsimStepIO()
        C.memmove(C.byref(io), C.byref(self.io), C.sizeof(io))
        for k, v in fields.items():
            setattr(io, k, None if v is None else v.data_ptr())
        return io

    def _regen_ws(self):
        """navsim_regen's workspace for self.cfg, made on first use."""
        if "regen_ws" not in self.t:
            import torch
            nbytes = self.lib.navsim_regen_workspace_bytes(C.byref(self.cfg))
            self.t["regen_ws"] = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return self.t["regen_ws"]

    def _replan_ws(self, cap):
        """navsim_replan's workspace for `cap` queries, made on first use."""
        key = "replan_ws_%d" % cap
        if key not in self.t:
            import torch
            nbytes = self.lib.navsim_replan_workspace_bytes(C.byref(self.cfg), cap)
            self.t[key] = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return self.t[key]

    def _regen_chunk(self, cfg, scratch_bytes):
        """cfg.regen_cap = as many arenas as `scratch_bytes` of navsim_regen workspace serve (what one more arena costs: the
        difference of two size queries) -> that workspace."""
        import torch
        cfg.regen_cap = 1
        per = self.lib.navsim_regen_workspace_bytes(C.byref(cfg))
        cfg.regen_cap = 2
        per = max(self.lib.navsim_regen_workspace_bytes(C.byref(cfg)) - per, 1)
        cfg.regen_cap = int(max(1, min(self.cfg.n_envs, scratch_bytes // per)))
        return torch.empty(self.lib.navsim_regen_workspace_bytes(C.byref(cfg)), dtype=torch.uint8, device=self.device)

    def _late_cfg_now(self):
        """late_cfg = the configuration as it stands NOW, with the fallback's own cap."""
        C.memmove(C.byref(self.late_cfg), C.byref(self.cfg), C.sizeof(self.cfg))
        self.late_cfg.regen_cap = self.late_cap
        return self.late_cfg

    def _call_regen(self, cfg, ws, stream, what, current_obs=True, latest_flags=True, fork=True, **fields):
        """navsim_regen on `stream` (None: the current one) with a copy of self.io: obs -> the current buffer (current_obs) and
        `fields` on top (done = the flags of the arenas to serve).  latest_flags: st.ped_due -> the flags of the latest step.
        fork=False: the call's own stream is handed to the library as helper stream for its duration (include/navsim.h: no fork)."""
        if current_obs:
            fields["obs"] = self.obs
        io = self._io_copy(**fields)
        if latest_flags:
            self._latest_flags()
        stream = _stream() if stream is None else C.c_void_p(stream.cuda_stream)
        helper = None if fork else self._regen_helper
        if helper is not None:
            self.lib.navsim_regen_helper(stream)
        check(self.lib.navsim_regen(C.byref(cfg), C.byref(self.st), C.byref(io), _ptr(ws), ws.numel(), stream), what)
        if helper is not None:
            self.lib.navsim_regen_helper(C.c_void_p(helper.cuda_stream))

    def regen(self):
        """navsim_regen right after step(): finished arenas get a new map, tables, pedestrians, first obs."""
        if self.pregen:
            return self._regen_pregen()
        self._choose_regen_helper()
        # NEXT_STEP: the arenas the latest step RESET, i.e. those that finished the step before
        self._call_regen(self.cfg, self._regen_ws(), None, "navsim_regen", **({"done": self.reset_flags} if self.next_step else {}))
        return self.obs

    def reset_arenas(self, mask, new_world=False, scratch_bytes=1 << 30):
        """reset() of the arenas of `mask` (uint8 / bool [E]) alone (env.py:730-831 is per environment): navsim_restart -- the
        next start / goal pair of the arena's table, the next episode number -- then their first observations
        (navsim_reset_obs) on the same map, or with new_world=True a new world each (navsim_regen in chunks of cfg.regen_cap
        arenas; worlds that draw a map per episode).  The other arenas keep their state and their rows.
        With enable_pregen(pipeline=P, install=True): new_world=True only, as ONE launch (navsim_reset_install) -- a masked arena
        starts episode[e] + 1, which is the episode its staged world was generated for, and installs it; an arena whose staged
        world is not complete is regenerated on the spot by navsim_regen (chunks of the fallback's cap).  Same state and rows as
        without staged worlds, whatever the passes' timing.  The staging passes keep their cadence (regen() queues them): a mask
        of more arenas than one pass stages (stage_cap) is restaged over several passes, and the arenas among them that finish
        before that go through the fallback (counters()['regen_late']).  With the rule alone (cfg.regen_min_steps >= 4 P, no
        fallback) an episode that starts at a reset is not covered by the rule's guarantee: an arena that finishes it before the
        pass that restages it restarts in place, counted in regen_late."""
        import torch
        if self.pregen:
            return self._reset_arenas_staged(mask, new_world)
        m = torch.as_tensor(mask).to(device=self.device).ne(0).to(torch.uint8).contiguous()
        check(self.lib.navsim_restart(C.byref(self.cfg), C.byref(self.st), _ptr(m), _stream()), "navsim_restart")
        self.reset_obs(m)
        if self.due is not None:                        # nobody of a reset arena waits for navsim_replan
            self.due[self.cur].mul_(m == 0)
        if new_world:
            self._choose_regen_helper()
            cfg = self.cfg.copy()
            cfg.regen_min_steps = 0
            ws = self._regen_ws()
            idx = torch.nonzero(m).flatten()
            chunk = torch.zeros_like(m)
            for a in range(0, int(idx.numel()), int(self.cfg.regen_cap)):
                chunk.zero_()
                chunk[idx[a:a + int(self.cfg.regen_cap)]] = 1
                self._call_regen(cfg, ws, None, "navsim_regen (reset of some arenas)", done=chunk)
            torch.cuda.current_stream().synchronize()  # `chunk` is released on return
        return self.obs

    def _reset_arenas_staged(self, mask, new_world):
        """reset_arenas on a simulator with staged worlds: reset_obs(mask)'s bookkeeping around navsim_reset_install, then
        navsim_regen for the arenas the launch flagged as late."""
        import torch
        if not self.pg_install or self.late2 is not None:
            raise ValueError("reset_arenas with enable_pregen needs install=True and not late_beside=True (the swap form's staged "
                             "worlds follow the episodes' own order; the beside form keeps two flag buffers)")
        if not new_world:
            raise ValueError("reset_arenas(new_world=False) is not available with enable_pregen: the staged worlds are new worlds")
        E = self.cfg.n_envs
        m = torch.as_tensor(mask).to(device=self.device).ne(0).to(torch.uint8).contiguous()
        keep = m == 0
        if self.rs_late is None:
            self.rs_late = torch.zeros(E, dtype=torch.uint8, device=self.device)
        # what reset_obs(mask) does around its launch: the other set of outputs starts as a copy, a reset arena is not finished
        for k, v in self.out_buf[1 - self.cur].items():
            v.copy_(self.out_buf[self.cur][k])
        for k in [k for k in ("done", "truncated") if k in self.out_buf[0]]:
            self.out_buf[1 - self.cur][k].mul_(keep)
        if self.late is not None:                       # ... and no longer waits for the step's fallback
            self.late.mul_(keep)
        self._flip()
        main = torch.cuda.current_stream()
        check(self.lib.navsim_reset_install(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), C.byref(self.stage_st),
                                            _ptr(self.stage_obs), _ptr(self.mark), _ptr(self.ready), _ptr(m), _ptr(self.rs_late),
                                            C.c_void_p(main.cuda_stream)), "navsim_reset_install")
        if self.due is not None:                        # nobody was advanced; nobody of a reset arena waits for navsim_replan
            self.due[1 - self.cur].copy_(self.due[self.cur])
            self.due[1 - self.cur].mul_(keep)
        self.cur = 1 - self.cur
        self.clear_episode_stats(m)
        idx = torch.nonzero(self.rs_late).flatten()     # (a host wait for the launch: a reset is not the per-step path)
        if int(idx.numel()):
            if self.late_ws is not None:                # the step's fallback: its workspace serves, on the same stream
                ws, cap = self.late_ws, self.late_cap
            else:
                if self.rs_ws is None:
                    self.rs_cap = late_cap_for(E)
                    cfg = self.cfg.copy()
                    cfg.regen_cap = self.rs_cap
                    self.rs_ws = torch.zeros(self.lib.navsim_regen_workspace_bytes(C.byref(cfg)), dtype=torch.uint8, device=self.device)
                ws, cap = self.rs_ws, self.rs_cap
            cfg = self.cfg.copy()                       # the configuration as it stands now, with the fallback's cap
            cfg.regen_cap = cap
            cfg.regen_min_steps = 0                     # a reset asks for a new world whatever the abandoned episode's length
            chunk = torch.zeros_like(m)
            for a in range(0, int(idx.numel()), cap):   # at most `cap` flags per call: nobody restarts in place
                chunk.zero_()
                chunk[idx[a:a + cap]] = 1
                # (no fork: navsim_regen's helper stream belongs to the staging passes, as for the per-step fallback)
                self._call_regen(cfg, ws, main, "navsim_regen (reset of arenas whose world was not staged)", fork=False, done=chunk)
            main.synchronize()                          # `chunk` is released on return
        return self.obs

    def regenerate_all(self, new_episode=False, scratch_bytes=4 << 30):
        """reset() of EVERY arena on the device (env.py:730-831 for the whole batch): navsim_regen with all arenas
        marked finished -- a new map per arena (indoor / outdoor by cfg.regen_indoor_ratio), its distance field
        (and rect records / costmap when those buffers exist), start / goal table, robot, pedestrians, the
        per-episode env_param draws and the first observation.  Runs in chunks of arenas so that the scratch
        stays below `scratch_bytes`.  new_episode: bump every arena's episode counter first (a second reset()
        must not reproduce the maps of the first)."""
        import torch
        E = self.cfg.n_envs
        self._choose_regen_helper()
        if new_episode:
            self.t["episode"] += 1
        cfg = self.cfg.copy()
        cfg.regen_min_steps = 0                 # a reset of everything: whatever the last episodes' lengths
        ws = self._regen_chunk(cfg, scratch_bytes)
        done = torch.zeros(E, dtype=torch.uint8, device=self.device)
        for a in range(0, E, cfg.regen_cap):
            done.zero_()
            done[a:a + cfg.regen_cap] = 1
            self._call_regen(cfg, ws, None, "navsim_regen (reset of all arenas)", done=done)
        for b in self.out_buf:                             # nobody is finished after a reset (NEXT_STEP: the next launch's reset mask)
            b["done"].zero_()
            if "truncated" in b:
                b["truncated"].zero_()
        self.clear_episode_stats()
        torch.cuda.current_stream().synchronize()          # `ws` and `done` are released on return
        return self.obs

    def counters(self, reset=False):
        """navsim_state.counters as a dict (abi.COUNTERS): arenas / pedestrians the calls served and what their caps
        (cfg.regen_cap, replan's max_queries, cfg.max_waypoints) left waiting or cut.  One device -> host copy."""
        v = self.t["counters"].cpu().numpy()
        if reset:
            self.t["counters"].zero_()
        return {k: int(v[i]) for i, k in enumerate(abi.COUNTERS)}

    # ---- episode statistics: return, length, path, clearance, discomfort and outcome of every finished episode, kept on the
    # device by one launch behind the step (include/navsim.h navsim_episode_stats_update)
    def enable_episode_stats(self):
        """Allocates the per-arena accumulators, the totals and two sets of published rows (ep_*: they flip with self.cur, so
        the rows episode_stats() returns stay intact through the next step like everything else a step returns).  From now on
        reset_obs(mask) / reset_arenas / regenerate_all clear the accumulators of the arenas they reset."""
        import torch
        if self.cfg.auto_reset == abi.AUTORESET_SAME_STEP and self.final_buf is None:
            raise ValueError("episode statistics under same-step auto-reset read the terminal rows: NavSim(final_obs=True)")
        if self.ep_acc is None:
            E = self.cfg.n_envs
            make = lambda d, n=E: torch.zeros(n, dtype=_dtype(d), device=self.device)
            self.ep_acc = {k: make(d) for k, d in abi.EPISODE_ACCUMULATORS.items()}
            self.ep_buf = [{k: make(d) for k, d in abi.EPISODE_PUBLISHED.items()} for _ in range(2)]
            self.ep_totals = make("int64", len(abi.EPISODE_TOTALS))     # uint64 on the device; far below 2^63
            self._ep_args = {}
        self.ep_totals.zero_()
        self.clear_episode_stats()

    def _episode_struct(self, parity):
        """navsim_episode_stats with the accumulators, the totals and the published rows of one parity."""
        stats = abi.NavsimEpisodeStats()
        for k, v in list(self.ep_acc.items()) + list(self.ep_buf[parity].items()):
            setattr(stats, k, v.data_ptr())
        stats.totals = self.ep_totals.data_ptr()
        return stats

    def _episode_args(self):
        """(io, stats) of navsim_episode_stats_update for the current parity: the buffers of the LATEST step, taken from the
        properties -- not from self.io, whose pointers the graph replay and the install paths do not keep current.
        Built once per parity and kept (a ctypes struct per call costs the host as much as the launch).  That rests on an
        invariant of this class: obs_buf, out_buf, final_buf, ep_acc, ep_buf, ep_totals, cfg and st are allocated once, in
        __init__ / enable_episode_stats, and only ever written in place.  Whoever reallocates one of them must empty
        self._ep_args."""
        args = self._ep_args.get(self.cur)
        if args is None:
            io = abi.NavsimStepIO()
            io.obs = self.obs.data_ptr()
            for k in ("reward", "done", "is_success", "is_crash", "truncated"):
                if k in self.out:
                    setattr(io, k, self.out[k].data_ptr())
            if self.final is not None:
                io.final_obs = self.final["final_obs"].data_ptr()
            if self.next_step:
                io.reset_mask = self.reset_flags.data_ptr()
            stats = self._episode_struct(self.cur)
            args = self._ep_args[self.cur] = (io, stats, C.byref(io), C.byref(stats), C.byref(self.cfg), C.byref(self.st))
        return args

    def episode_stats(self):
        """navsim_episode_stats_update behind the latest step (and its regen() / replan()) on the current stream: one launch.
        Returns the published rows: ep_return, ep_length, ep_path_length, ep_min_clearance, ep_discomfort_steps, ep_outcome --
        valid where that step's done flag is set, intact through the next step."""
        if self.ep_acc is None:
            raise RuntimeError("call enable_episode_stats() first")
        a = self._episode_args()
        rc = self.lib.navsim_episode_stats_update(a[4], a[5], a[2], a[3], _stream())
        if rc:
            check(rc, "navsim_episode_stats_update")
        return self.ep_buf[self.cur]

    def clear_episode_stats(self, mask=None):
        """The accumulators of the masked arenas (None: all) back to "no step yet"; nothing without enable_episode_stats()."""
        if self.ep_acc is None:
            return
        stats = self._episode_struct(self.cur)            # (clear touches the accumulators only: either parity's struct does)
        check(self.lib.navsim_episode_stats_clear(C.byref(self.cfg), C.byref(stats), _ptr(mask), _stream()),
              "navsim_episode_stats_clear")

    def episode_totals(self, reset=False):
        """The running totals over finished episodes as a dict (abi.EPISODE_TOTALS).  One device -> host copy."""
        if self.ep_acc is None:
            raise RuntimeError("call enable_episode_stats() first")
        v = self.ep_totals.cpu().numpy()
        if reset:
            self.ep_totals.zero_()
        return {k: int(v[i]) for i, k in enumerate(abi.EPISODE_TOTALS)}

    # ---- the launches behind the step that follow: each enable_* call leaves one _StepProduct in self.products
    def _product(self, name):
        """The record of an enabled product.  (The four call methods ask the dict themselves first, `self.products.get(name) or
        self._product(name)`: per step the guard is a function call only when it raises.)"""
        p = self.products.get(name)
        if p is None:
            raise RuntimeError("call enable_%s() first" % name)
        return p

    # the two parameter structs that callers outside this class read by name (a specification run beside the device's call takes
    # the struct the call uses): read-only views of the records, None while the product is not enabled
    @property
    def obs_params(self):
        p = self.products.get("ped_observe")
        return p and p.params

    @property
    def local_map_params(self):
        p = self.products.get("local_map")
        return p and p.params

    # ---- observed pedestrians: the K nearest pedestrians in the robot's line of sight, in its frame, from one launch behind the
    # step (include/navsim.h navsim_ped_observe)
    def enable_ped_observe(self, params=None):
        """Allocates two sets of outputs (state [E,K,5], index [E,K], count [E], visible [E,N]: they flip with self.cur, so what
        ped_observe() returned stays intact through the next step like everything else a step returns).  params: an
        abi.NavsimPedObserveParams, a dict of overrides of ped_observe_defaults(cfg), or None."""
        if self.cfg.ped_model == abi.PED_NONE:
            raise ValueError("observed pedestrians need a pedestrian model")
        p = params if isinstance(params, abi.NavsimPedObserveParams) else ped_observe_params(self.cfg, params)
        if not 1 <= p.max_obs <= abi.MAX_PEDS:
            raise ValueError("max_obs must lie in 1..%d, not %d" % (abi.MAX_PEDS, p.max_obs))
        # (the four arrays in abi.PED_OBSERVATION's order: 4-byte types first)
        self.products["ped_observe"] = _StepProduct(self, p, ped_observation_layout(self.cfg.n_envs, p.max_obs, self.cfg.max_peds),
                                                    abi.NavsimPedObservation)

    def ped_observation_host(self):
        """The current set of ped_observe()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("ped_observe").host(self.cur)

    def ped_observe(self, skip=None):
        """navsim_ped_observe of the current state on the current stream: one launch.  skip: uint8 / bool [E], arenas whose rows
        come back empty (None: none).  Returns the current set {'state', 'index', 'count', 'visible'}, intact through the next
        step."""
        p, cur = self.products.get("ped_observe") or self._product("ped_observe"), self.cur
        rc = self.lib.navsim_ped_observe(p.cfg, p.st, p.par, _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_ped_observe")
        return p.buf[cur]

    # ---- goal path: a distance-to-goal field per arena on the 5 x 5-cell navigation grid, the robot's path distance and a steering
    # sub-goal read from it -- two launches behind the step (include/navsim.h navsim_goal_path)
    def enable_goal_path(self, params=None):
        """Allocates the field (uint16 [E, H/5, W/5]), its keys (int64 [E,3], -1 = never built), the rebuild counter and two sets
        of outputs (distance [E], subgoal [E,2], status [E]: they flip with self.cur like everything a step returns).  params: an
        abi.NavsimGoalPathParams, a dict of overrides of goal_path_defaults(cfg), or None."""
        import torch
        cfg = self.cfg
        p = params if isinstance(params, abi.NavsimGoalPathParams) else goal_path_params(cfg, params)
        nbytes = self.lib.navsim_goal_field_bytes(C.byref(cfg))
        if nbytes == 0 and cfg.n_envs > 0:
            raise ValueError("the goal path needs maps of at least 5 x 5 cells")
        field = dict(dist=torch.full((cfg.n_envs, cfg.map_h // 5, cfg.map_w // 5), abi.GOAL_FIELD_INF - 65536, dtype=torch.int16,
                                     device=self.device).view(torch.uint16),
                     key=torch.full((cfg.n_envs, 3), -1, dtype=torch.int64, device=self.device),
                     rebuilds=torch.zeros(1, dtype=torch.int64, device=self.device))
        self.products["goal_path"] = _StepProduct(self, p, goal_path_layout(cfg.n_envs), abi.NavsimGoalPathOut, extra=field,
                                                  extra_struct=abi.NavsimGoalField(**{k: v.data_ptr() for k, v in field.items()}))

    def goal_path(self, rebuild=None, skip=None):
        """navsim_goal_path of the current state on the current stream: two launches, no copy.  rebuild: uint8 / bool [E], arenas
        whose field is rebuilt whatever their key says (None: the keys alone decide -- every in-launch restart changes them);
        skip: uint8 / bool [E], arenas that are neither rebuilt nor read and come back (0, (0, 0), 0).  Returns the current set
        {'distance', 'subgoal', 'status'}, intact through the next step."""
        p, cur = self.products.get("goal_path") or self._product("goal_path"), self.cur
        rc = self.lib.navsim_goal_path(p.cfg, p.st, p.par, _ptr(rebuild), _ptr(skip), p.extra_ref, p.out[cur], _stream())
        if rc:
            check(rc, "navsim_goal_path")
        return p.buf[cur]

    def goal_path_host(self):
        """The current set of goal_path()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("goal_path").host(self.cur)

    def goal_field(self):
        """The distance-to-goal fields on the device: uint16 [E, H/5, W/5] in map cells (5 a straight hop, 7 a diagonal one),
        0xFFFF = impassable, unreachable or farther than 65534; as of each arena's latest rebuild."""
        return self._product("goal_path").extra["dist"]

    def goal_path_rebuilds(self):
        """Fields rebuilt since enable_goal_path().  One device -> host copy."""
        return int(self._product("goal_path").extra["rebuilds"].item())

    # ---- local planner: a dynamic-window action per arena -- candidates rolled out against the distance field and the pedestrians,
    # the best one returned -- one launch behind the step (include/navsim.h navsim_dwa)
    def enable_dwa(self, params=None, scores=False, robot_type="keti"):
        """Allocates two sets of outputs (twist [E,2], action [E,2], clearance [E], best [E], status [E]; with scores=True also
        scores [E,C] and first_hit [E,C], every candidate's values: they flip with self.cur like everything a step returns).
        params: an abi.NavsimDwaParams, a dict of overrides of dwa_defaults(cfg, robot_type), or None."""
        p = params if isinstance(params, abi.NavsimDwaParams) else dwa_params(self.cfg, params, robot_type)
        if not (1 <= p.n_v <= 16 and 1 <= p.n_w <= 32 and 1 <= p.horizon <= 32):
            raise ValueError("n_v must lie in 1..16, n_w in 1..32, horizon in 1..32, not %d, %d, %d" % (p.n_v, p.n_w, p.horizon))
        self.products["dwa"] = _StepProduct(self, p, dwa_layout(self.cfg.n_envs, p.n_v * p.n_w, scores=scores), abi.NavsimDwaOut)

    def dwa(self, subgoal=None, skip=None):
        """navsim_dwa of the current state on the current stream: one launch, no copy.  subgoal: float32 [E,2] targets in the
        robot's frame (goal_path()'s 'subgoal'; None: the arena's goal); skip: uint8 / bool [E], arenas that are not read and come
        back all 0.  Returns the current set {'twist', 'action', 'clearance', 'best', 'status'[, 'scores', 'first_hit']}, intact
        through the next step."""
        p, cur = self.products.get("dwa") or self._product("dwa"), self.cur
        rc = self.lib.navsim_dwa(p.cfg, p.st, p.par, _ptr(subgoal), _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_dwa")
        return p.buf[cur]

    def dwa_host(self):
        """The current set of dwa()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("dwa").host(self.cur)

    # ---- egocentric local map: wall and pedestrian grids per arena in the robot's frame, one launch behind the step
    # (include/navsim.h navsim_local_map)
    def enable_local_map(self, size, params=None):
        """Allocates two outputs float32 [E, C, size, size] (they flip with self.cur like everything a step returns).  params: an
        abi.NavsimLocalMapParams (its own size counts), a dict of overrides of local_map_defaults(cfg), or None."""
        p = params if isinstance(params, abi.NavsimLocalMapParams) else local_map_params(self.cfg, params, size)
        if not 1 <= p.size <= abi.LOCAL_MAP_MAX:
            raise ValueError("the local map's size must lie in 1 .. %d, not %d" % (abi.LOCAL_MAP_MAX, p.size))
        if p.channels not in (1, 2, 4):
            raise ValueError("the local map has 1, 2 or 4 channels, not %d" % p.channels)
        # (a layout of one array, at the start of its allocation: navsim_local_map picks its four-cell kernel by out's alignment)
        self.products["local_map"] = _StepProduct(self, p, blob_layout(abi.LOCAL_MAP_OUT, self.cfg.n_envs, {"C": p.channels, "G": p.size}))

    def local_map(self, skip=None, visible=None):
        """navsim_local_map of the current state on the current stream: one launch, no copy, no allocation.  skip: uint8 / bool
        [E], arenas that are not read and come back all 0; visible: uint8 / bool [E,N], the pedestrians that count
        (ped_observe()'s 'visible'; None: all of them).  Returns the current tensor [E, C, G, G], intact through the next step."""
        p, cur = self.products.get("local_map") or self._product("local_map"), self.cur
        rc = self.lib.navsim_local_map(p.cfg, p.st, p.par, _ptr(visible), _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_local_map")
        return p.buf[cur]["map"]

    # ---- scan ground truth: the robot's scan without noise and per beam what it fell on, one launch behind the step
    # (include/navsim.h navsim_scan_labels)
    def enable_scan_labels(self):
        """Allocates two sets of outputs (range [E,B] float32, label [E,B] uint8, index [E,B] int8 and, with a pedestrian model,
        hits [E,N] int32: they flip with self.cur like everything a step returns).  The rule has no parameters."""
        cfg = self.cfg
        omit = ("hits",) if cfg.ped_model == abi.PED_NONE else ()
        self.products["scan_labels"] = _StepProduct(self, None, blob_layout(abi.SCAN_LABELS_OUT, cfg.n_envs,
                                                                            {"B": cfg.n_beams, "N": cfg.max_peds}, omit=omit),
                                                    abi.NavsimScanLabelsOut)

    def scan_labels(self, skip=None):
        """navsim_scan_labels of the current state on the current stream: one launch, no copy, no allocation.  skip: uint8 / bool
        [E], arenas that are not read and come back empty (range 0, label 0, index -1, hits 0).  Returns the current set {'range',
        'label', 'index'[, 'hits']}, intact through the next step.  label: abi.BEAM_NONE / BEAM_WALL / BEAM_PED_BODY / BEAM_PED_LEG."""
        p, cur = self.products.get("scan_labels") or self._product("scan_labels"), self.cur
        rc = self.lib.navsim_scan_labels(p.cfg, p.st, _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_scan_labels")
        return p.buf[cur]

    def scan_labels_host(self):
        """The current set of scan_labels()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("scan_labels").host(self.cur)

    # ---- action lookahead: what step() would return for each of K candidate actions per arena, one launch that only reads the
    # state (include/navsim.h navsim_lookahead)
    def enable_lookahead(self, K, params=None):
        """Allocates two sets of outputs (abi.LOOKAHEAD_OUT, [E,K,...] and status [E]: they flip with self.cur like everything a
        step returns), an action buffer float64 [E,K,2] and a command buffer float64 [E,N,2].  params: a dict of overrides of
        lookahead_defaults(cfg), or None.  The thresholds live on the device, so rule 5's lower bound on the cap is checked here
        (one device -> host copy of their maximum): a range outside [max scan_discomfort + 0.1, range_max] raises ValueError."""
        import torch
        cfg = self.cfg
        if not 1 <= int(K) <= abi.LOOKAHEAD_MAX:
            raise ValueError("lookahead evaluates 1 .. %d actions per arena, not %r" % (abi.LOOKAHEAD_MAX, K))
        dmax = float(self.t["scan_discomfort"].max().item())
        d = _overridden(lookahead_defaults(cfg, dmax), params, "lookahead", LOOKAHEAD_KEYS)
        R = float(d["range"])
        if not lookahead_range_min(dmax) <= R <= cfg.range_max:
            raise ValueError("the lookahead's range must lie in [%g, %g] (0.1 m above the largest discomfort threshold .. range_max), "
                             "not %g" % (lookahead_range_min(dmax), cfg.range_max, R))
        p = abi.NavsimLookaheadParams(n_actions=int(K), range=R)
        extra = dict(actions=torch.zeros((cfg.n_envs, int(K), 2), dtype=torch.float64, device=self.device),
                     ped_cmd=torch.zeros((cfg.n_envs, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        self.products["lookahead"] = _StepProduct(self, p, blob_layout(abi.LOOKAHEAD_OUT, cfg.n_envs, {"K": int(K)}),
                                                  abi.NavsimLookaheadOut, extra=extra)

    def lookahead(self, actions, ped_cmd=None, skip=None):
        """navsim_lookahead of the current state on the current stream: one launch, no device -> host copy, no allocation, and the
        state is only read.  actions: [E,K,2] in cfg.action_kind's form (copied into the product's buffer unless it already is a
        contiguous float64 tensor on the device); ped_cmd: [E,N,2] commands that stand for the state's under PED_EXTERNAL (None:
        the state's own); skip: uint8 / bool [E], arenas that are not read and come back all 0 with status 0.  Returns the current
        set {'reward', 'done', 'is_success', 'is_crash', 'discomfort', 'distance', 'margin', 'pose', 'status'}, intact through
        the next step."""
        import torch
        p, cur = self.products.get("lookahead") or self._product("lookahead"), self.cur
        buf = p.extra["actions"]
        if not (torch.is_tensor(actions) and actions.device == buf.device and actions.dtype == buf.dtype and actions.is_contiguous()
                and actions.shape == buf.shape):
            buf.copy_(torch.as_tensor(actions).to(device=buf.device, dtype=buf.dtype).reshape(buf.shape), non_blocking=True)
            actions = buf
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_lookahead(p.cfg, p.st, p.par, _ptr(actions), _ptr(ped_cmd), _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_lookahead")
        return p.buf[cur]

    def lookahead_host(self):
        """The current set of lookahead()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("lookahead").host(self.cur)

    # ---- lookahead observations: the WHOLE return of step() -- row, goals, reward, done, truncated, flags -- for each of K
    # candidate actions per arena, one launch that only reads the state (include/navsim.h navsim_lookahead_obs)
    def enable_lookahead_obs(self, K, params=None):
        """Allocates two sets of outputs (abi.LOOKAHEAD_OBS_OUT, [E,K,...] and status [E]: they flip with self.cur like everything
        a step returns), an action buffer float64 [E,K,2] and a command buffer float64 [E,N,2].  params: a dict of overrides of
        lookahead_obs_defaults(), or None -- noise 'step' (the draw the step itself would make) or 'off'; rows 'full' (the rows
        [E,K,S*B+7] as `obs`: E*K*(S*B+7)*4 bytes per set) or 'scan' (no `obs`: scan [E,K,B] and tail [E,K,7] only)."""
        import torch
        cfg = self.cfg
        if not 1 <= int(K) <= abi.LOOKAHEAD_MAX:
            raise ValueError("lookahead_obs evaluates 1 .. %d actions per arena, not %r" % (abi.LOOKAHEAD_MAX, K))
        d = _overridden(lookahead_obs_defaults(), params, "lookahead_obs", LOOKAHEAD_OBS_KEYS)
        noise, rows = lookahead_obs_choice(d)
        p = abi.NavsimLookaheadObsParams(n_actions=int(K), noise=noise)
        extra = dict(actions=torch.zeros((cfg.n_envs, int(K), 2), dtype=torch.float64, device=self.device),
                     ped_cmd=torch.zeros((cfg.n_envs, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        sym = {"K": int(K), "B": cfg.n_beams, "D": cfg.n_scan_stack * cfg.n_beams + abi.OBS_TAIL}
        layout = blob_layout(abi.LOOKAHEAD_OBS_OUT, cfg.n_envs, sym, omit=() if rows == "full" else ("obs",))
        self.products["lookahead_obs"] = _StepProduct(self, p, layout, abi.NavsimLookaheadObsOut, extra=extra)

    def lookahead_obs(self, actions, ped_cmd=None, skip=None):
        """navsim_lookahead_obs of the current state and the current observation (self.obs: what the next step takes as
        obs_prev) on the current stream: one launch, no device -> host copy, no allocation, and the state is only read.
        actions, ped_cmd, skip: as lookahead()'s.  Returns the current set -- lookahead()'s nine arrays, 'scan' [E,K,B], 'tail'
        [E,K,7], 'goals' [E,K,4], 'truncated' [E,K] and, with rows='full', 'obs' [E,K,S*B+7] -- intact through the next step."""
        import torch
        p, cur = self.products.get("lookahead_obs") or self._product("lookahead_obs"), self.cur
        buf = p.extra["actions"]
        if not (torch.is_tensor(actions) and actions.device == buf.device and actions.dtype == buf.dtype and actions.is_contiguous()
                and actions.shape == buf.shape):
            buf.copy_(torch.as_tensor(actions).to(device=buf.device, dtype=buf.dtype).reshape(buf.shape), non_blocking=True)
            actions = buf
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_lookahead_obs(p.cfg, p.st, p.par, _ptr(actions), _ptr(ped_cmd), _ptr(self.obs_buf[cur]), _ptr(skip),
                                           p.out[cur], _stream())
        if rc:
            check(rc, "navsim_lookahead_obs")
        return p.buf[cur]

    def lookahead_obs_host(self):
        """The current set of lookahead_obs()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("lookahead_obs").host(self.cur)

    # ---- action-sequence rollout: what the next H step() calls would return for each of K action sequences per arena, one launch
    # that only reads the state (include/navsim.h navsim_rollout)
    def enable_rollout(self, K, H, params=None):
        """Allocates two sets of outputs (abi.ROLLOUT_OUT, [E,K,...] and status [E]: they flip with self.cur like everything a
        step returns), an action buffer float64 [E,K,H,2] and a command buffer float64 [E,N,2].  params: a dict of overrides of
        rollout_defaults(cfg) -- range, gamma -- or None.  The lower bound on the cap is the lookahead's and is checked here the
        same way: a range outside [max scan_discomfort + 0.1, range_max] or a gamma outside [0, 1] raises ValueError."""
        import torch
        cfg = self.cfg
        if not 1 <= int(K) <= abi.ROLLOUT_MAX_K:
            raise ValueError("rollout evaluates 1 .. %d sequences per arena, not %r" % (abi.ROLLOUT_MAX_K, K))
        if not 1 <= int(H) <= abi.ROLLOUT_MAX_H:
            raise ValueError("rollout looks 1 .. %d steps ahead, not %r" % (abi.ROLLOUT_MAX_H, H))
        dmax = float(self.t["scan_discomfort"].max().item())
        d = _overridden(rollout_defaults(cfg, dmax), params, "rollout", ROLLOUT_KEYS)
        R, gamma = float(d["range"]), float(d["gamma"])
        if not lookahead_range_min(dmax) <= R <= cfg.range_max:
            raise ValueError("the rollout's range must lie in [%g, %g] (0.1 m above the largest discomfort threshold .. range_max), "
                             "not %g" % (lookahead_range_min(dmax), cfg.range_max, R))
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("the rollout's gamma must lie in [0, 1], not %g" % gamma)
        p = abi.NavsimRolloutParams(n_seq=int(K), horizon=int(H), range=R, gamma=gamma)
        extra = dict(actions=torch.zeros((cfg.n_envs, int(K), int(H), 2), dtype=torch.float64, device=self.device),
                     ped_cmd=torch.zeros((cfg.n_envs, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        self.products["rollout"] = _StepProduct(self, p, blob_layout(abi.ROLLOUT_OUT, cfg.n_envs, {"K": int(K), "H": int(H)}),
                                                abi.NavsimRolloutOut, extra=extra)

    def rollout(self, actions, ped_cmd=None, skip=None):
        """navsim_rollout of the current state on the current stream: one launch, no device -> host copy, no allocation, and the
        state is only read.  actions: [E,K,H,2] in cfg.action_kind's form (copied into the product's buffer unless it already is a
        contiguous float64 tensor on the device); ped_cmd: [E,N,2] commands held for the whole horizon under PED_EXTERNAL (None:
        the state's own); skip: uint8 / bool [E], arenas that are not read and come back all 0 with status 0.  Returns the current
        set (abi.ROLLOUT_OUT's keys), intact through the next step."""
        import torch
        p, cur = self.products.get("rollout") or self._product("rollout"), self.cur
        buf = p.extra["actions"]
        if not (torch.is_tensor(actions) and actions.device == buf.device and actions.dtype == buf.dtype and actions.is_contiguous()
                and actions.shape == buf.shape):
            buf.copy_(torch.as_tensor(actions).to(device=buf.device, dtype=buf.dtype).reshape(buf.shape), non_blocking=True)
            actions = buf
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_rollout(p.cfg, p.st, p.par, _ptr(actions), _ptr(ped_cmd), _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_rollout")
        return p.buf[cur]

    def rollout_host(self):
        """The current set of rollout()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("rollout").host(self.cur)

    # ---- rollout observations: the WHOLE return of the next H step() calls -- row, goals, reward, pose, outcome -- for each of K
    # action sequences per arena, one launch that only reads the state (include/navsim.h navsim_rollout_obs)
    def enable_rollout_obs(self, K, H, params=None):
        """Allocates two sets of outputs (abi.ROLLOUT_OBS_OUT, [E,K,...] and status [E]: they flip with self.cur like everything a
        step returns), an action buffer float64 [E,K,H,2] and a command buffer float64 [E,N,2].  params: a dict of overrides of
        rollout_obs_defaults(), or None -- gamma in [0, 1]; noise 'step' (the draw each future step itself would make) or 'off';
        rows 'last' (obs_last [E,K,S*B+7] and goals_last [E,K,4] only) or 'all' (obs_all [E,K,H,S*B+7] and goals_all [E,K,H,4] as
        well: E*K*H*(S*B+7)*4 bytes per set).  Independent of enable_rollout and enable_lookahead_obs."""
        import torch
        cfg = self.cfg
        if not 1 <= int(K) <= abi.ROLLOUT_MAX_K:
            raise ValueError("rollout_obs evaluates 1 .. %d sequences per arena, not %r" % (abi.ROLLOUT_MAX_K, K))
        if not 1 <= int(H) <= abi.ROLLOUT_MAX_H:
            raise ValueError("rollout_obs looks 1 .. %d steps ahead, not %r" % (abi.ROLLOUT_MAX_H, H))
        d = _overridden(rollout_obs_defaults(), params, "rollout_obs", ROLLOUT_OBS_KEYS)
        gamma, noise, rows = rollout_obs_choice(d)
        p = abi.NavsimRolloutObsParams(n_seq=int(K), horizon=int(H), noise=noise, gamma=gamma)
        extra = dict(actions=torch.zeros((cfg.n_envs, int(K), int(H), 2), dtype=torch.float64, device=self.device),
                     ped_cmd=torch.zeros((cfg.n_envs, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        sym = {"K": int(K), "H": int(H), "D": cfg.n_scan_stack * cfg.n_beams + abi.OBS_TAIL}
        layout = blob_layout(abi.ROLLOUT_OBS_OUT, cfg.n_envs, sym, omit=() if rows == "all" else ("obs_all", "goals_all"))
        self.products["rollout_obs"] = _StepProduct(self, p, layout, abi.NavsimRolloutObsOut, extra=extra)

    def rollout_obs(self, actions, ped_cmd=None, skip=None):
        """navsim_rollout_obs of the current state and the current observation (self.obs: what the next step takes as obs_prev)
        on the current stream: one launch, no device -> host copy, no allocation, and the state is only read.  actions, ped_cmd,
        skip: as rollout()'s.  Returns the current set -- rollout()'s ten arrays, 'obs_last' [E,K,S*B+7], 'goals_last' [E,K,4]
        and, with rows='all', 'obs_all' [E,K,H,S*B+7] and 'goals_all' [E,K,H,4] -- intact through the next step."""
        import torch
        p, cur = self.products.get("rollout_obs") or self._product("rollout_obs"), self.cur
        buf = p.extra["actions"]
        if not (torch.is_tensor(actions) and actions.device == buf.device and actions.dtype == buf.dtype and actions.is_contiguous()
                and actions.shape == buf.shape):
            buf.copy_(torch.as_tensor(actions).to(device=buf.device, dtype=buf.dtype).reshape(buf.shape), non_blocking=True)
            actions = buf
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_rollout_obs(p.cfg, p.st, p.par, _ptr(actions), _ptr(ped_cmd), _ptr(self.obs_buf[cur]), _ptr(skip),
                                         p.out[cur], _stream())
        if rc:
            check(rc, "navsim_rollout_obs")
        return p.buf[cur]

    def rollout_obs_host(self):
        """The current set of rollout_obs()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("rollout_obs").host(self.cur)

    # ---- MPPI local planner: sampled plans, the rollout's launch and the weighted update on the device, 3 launches an iteration
    # (include/navsim.h navsim_mppi).  Independent of enable_rollout: its K and H are its own
    def enable_mppi(self, params=None, robot_type="keti"):
        """Allocates the workspace ONCE -- plan [E,H,2], plan_key [E,2] (-1: no plan yet), actions [E,K,H,2], cost [E,K] and
        navsim_rollout's ten arrays: it persists from call to call -- and two sets of outputs (abi.MPPI_OUT: they flip with
        self.cur like everything a step returns).  params: an abi.NavsimMppiParams, a dict of overrides of mppi_defaults(cfg,
        robot_type), or None.  The lower bound on the rollout's cap is checked here as enable_rollout checks it."""
        import torch
        cfg, E = self.cfg, self.cfg.n_envs
        dmax = float(self.t["scan_discomfort"].max().item())
        p = params if isinstance(params, abi.NavsimMppiParams) else mppi_params(cfg, params, robot_type, dmax)
        if not lookahead_range_min(dmax) <= p.range <= cfg.range_max:
            raise ValueError("the planner's range must lie in [%g, %g] (0.1 m above the largest discomfort threshold .. range_max), "
                             "not %g" % (lookahead_range_min(dmax), cfg.range_max, p.range))
        if not 0.0 <= p.gamma <= 1.0:
            raise ValueError("the planner's gamma must lie in [0, 1], not %g" % p.gamma)
        sym = {"K": p.n_samples, "H": p.horizon}
        ws = {k: torch.zeros((E,) + tuple(sym.get(s, s) for s in shape), dtype=_dtype(d), device=self.device)
              for k, (d, shape) in abi.MPPI_WS.items()}
        ws["plan_key"][:, 0] = -1
        roll_blob = torch.zeros(blob_layout(abi.ROLLOUT_OUT, E, sym)[-1][3], dtype=torch.uint8, device=self.device)
        roll = {k: roll_blob[lo:hi].view(_dtype(d)).view(shape) for k, d, lo, hi, shape in blob_layout(abi.ROLLOUT_OUT, E, sym)[:-1]}
        struct = abi.NavsimMppiWs(roll=abi.NavsimRolloutOut(**{k: v.data_ptr() for k, v in roll.items()}),
                                  **{k: v.data_ptr() for k, v in ws.items()})
        extra = dict(ws, roll=roll, roll_blob=roll_blob,
                     ped_cmd=torch.zeros((E, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        self.products["mppi"] = _StepProduct(self, p, blob_layout(abi.MPPI_OUT, E), abi.NavsimMppiOut, extra=extra, extra_struct=struct)

    def mppi(self, field=None, ped_cmd=None, skip=None):
        """navsim_mppi of the current state on the current stream: 3 launches per iteration, no device -> host copy, no
        allocation; the state is only read.  field: True = the terminal cost reads the goal field of enable_goal_path() -- call
        goal_path() for this state first, the field's keys are not looked at here --, None / False = the straight-line distance;
        ped_cmd: [E,N,2] commands held for the whole horizon under PED_EXTERNAL (None: the state's own); skip: uint8 / bool [E],
        arenas that are not read, whose plan stays and whose rows come back all 0.  Returns the current set {'action', 'best',
        'cost_best', 'ess', 'status'}, intact through the next step."""
        import torch
        p, cur = self.products.get("mppi") or self._product("mppi"), self.cur
        gf = gp = None
        if field:
            g = self.products.get("goal_path") or self._product("goal_path")
            gf, gp = g.extra_ref, g.par
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_mppi(p.cfg, p.st, p.par, gf, gp, _ptr(ped_cmd), _ptr(skip), p.extra_ref, p.out[cur], _stream())
        if rc:
            check(rc, "navsim_mppi")
        return p.buf[cur]

    def mppi_host(self):
        """The current set of mppi()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("mppi").host(self.cur)

    def mppi_plan(self):
        """The plans on the device: float64 [E,H,2], as the latest mppi() left them."""
        return self._product("mppi").extra["plan"]

    # ---- pedestrian forecast: each arena's pedestrians over the next H steps, one launch that only reads the state
    # (include/navsim.h navsim_ped_forecast)
    def enable_ped_forecast(self, H, params=None):
        """Allocates two sets of outputs (abi.FORECAST_OUT, time-major [E,H,N,...]: they flip with self.cur like everything a step
        returns), an action buffer float64 [E,H,2] and a command buffer float64 [E,N,2].  params: a dict of overrides of
        ped_forecast_defaults(cfg) -- robot, model -- or None."""
        cfg = self.cfg
        if cfg.ped_model == abi.PED_NONE:
            raise ValueError("the pedestrian forecast needs a pedestrian model")
        if not 1 <= int(H) <= abi.FORECAST_MAX_H:
            raise ValueError("the pedestrian forecast looks 1 .. %d steps ahead, not %r" % (abi.FORECAST_MAX_H, H))
        d = _overridden(ped_forecast_defaults(cfg), params, "pedestrian forecast", PED_FORECAST_KEYS)
        if d["robot"] not in PED_FORECAST_ROBOT:
            raise ValueError("the pedestrian forecast's robot is one of %s, not %r" % (", ".join(PED_FORECAST_ROBOT), d["robot"]))
        if d["model"] not in PED_FORECAST_MODEL:
            raise ValueError("the pedestrian forecast's model is one of %s, not %r" % (", ".join(PED_FORECAST_MODEL), d["model"]))
        self.products["ped_forecast"] = self._ped_forecast_product(int(H), PED_FORECAST_ROBOT[d["robot"]], PED_FORECAST_MODEL[d["model"]])

    def _ped_forecast_product(self, H, robot, model):
        import torch
        cfg = self.cfg
        p = abi.NavsimPedForecastParams(horizon=H, robot=robot, model=model)
        extra = dict(actions=torch.zeros((cfg.n_envs, H, 2), dtype=torch.float64, device=self.device),
                     ped_cmd=torch.zeros((cfg.n_envs, max(cfg.max_peds, 1), 2), dtype=torch.float64, device=self.device))
        return _StepProduct(self, p, blob_layout(abi.FORECAST_OUT, cfg.n_envs, {"H": H, "N": cfg.max_peds}),
                            abi.NavsimPedForecastOut, extra=extra)

    def ped_forecast(self, actions=None, ped_cmd=None, skip=None, query=False):
        """navsim_ped_forecast of the current state on the current stream: one launch, no device -> host copy, and the state is
        only read.  actions: [E,H,2] in cfg.action_kind's form -- required when the forecast was enabled with robot='actions'
        (copied into the product's buffer unless it already is a contiguous float64 tensor on the device); ped_cmd: [E,N,2]
        commands held for the whole horizon under PED_EXTERNAL with model='true' (None: the state's own); skip: uint8 / bool
        [E], arenas that are not read and come back all 0 with status 0.  query=True: the call takes `actions` whatever robot
        the forecast was enabled with (None: that robot) and writes into a buffer set of its own -- made at the first such call
        -- so that what the call behind the step returned stays intact.  Returns the current set (abi.FORECAST_OUT's keys),
        intact through the next step."""
        import torch
        p, cur = self.products.get("ped_forecast") or self._product("ped_forecast"), self.cur
        if query:
            robot = p.params.robot if actions is None else abi.FORECAST_ACTIONS
            q = self.products.get("ped_forecast_query")
            if q is None or q.params.robot != robot:
                q = self.products["ped_forecast_query"] = self._ped_forecast_product(p.params.horizon, robot, p.params.model)
            p = q
        if p.params.robot == abi.FORECAST_ACTIONS:
            if actions is None:
                raise ValueError("a pedestrian forecast with robot='actions' needs actions")
            buf = p.extra["actions"]
            if not (torch.is_tensor(actions) and actions.device == buf.device and actions.dtype == buf.dtype and actions.is_contiguous()
                    and actions.shape == buf.shape):
                buf.copy_(torch.as_tensor(actions).to(device=buf.device, dtype=buf.dtype).reshape(buf.shape), non_blocking=True)
                actions = buf
        else:
            actions = None
        if ped_cmd is not None:
            cmd = p.extra["ped_cmd"]
            cmd.copy_(torch.as_tensor(ped_cmd).to(device=cmd.device, dtype=cmd.dtype).reshape(cmd.shape), non_blocking=True)
            ped_cmd = cmd
        rc = self.lib.navsim_ped_forecast(p.cfg, p.st, p.par, _ptr(actions), _ptr(ped_cmd), _ptr(skip), p.out[cur], _stream())
        if rc:
            check(rc, "navsim_ped_forecast")
        return p.buf[cur]

    def ped_forecast_host(self, query=False):
        """The current set of ped_forecast()'s outputs as NumPy arrays, from ONE device -> host copy."""
        return self._product("ped_forecast_query" if query else "ped_forecast").host(self.cur)

    def occupancy(self, e=0):
        """uint8 [H, W] occupancy grid (1 = occupied) of arena e, read back from its distance field
        (a cell is occupied exactly when its distance is 0)."""
        H, W = self.cfg.map_h, self.cfg.map_w
        if "map_slot" in self.t:                        # where the arena's map lies (enable_pregen(install=True, map_slots=True))
            e = int(self.t["map_slot"][e].item())
        if self.cfg.field_format == abi.FIELD_F32:
            return (self.t["field"][e] == 0).to(_dtype("uint8")).cpu().numpy()
        tpr, tpc = (W + 7) // 8, (H + 7) // 8
        per = tpr * tpc * 64
        blob = self.t["field"].reshape(-1)[e * per:(e + 1) * per].cpu().numpy().view(np.uint16)
        tiles = blob.reshape(tpc, tpr, 8, 8).transpose(0, 2, 1, 3).reshape(tpc * 8, tpr * 8)
        return (tiles[:H, :W] == 0).astype(np.uint8)

    def replan(self, max_queries=1024, flags=True):
        """navsim_replan (env.py:667-680): pedestrians standing on their final waypoint get a new goal and
        the waypoints of a planned path.  Needs the resident costmap (world.make_world(plan_paths=True)).
        flags=True: the candidates are the pedestrians the last step flagged (navsim_state.ped_due); False: the call
        finds them by its own pass over the state (after the caller moved pedestrians by hand)."""
        ws = self._replan_ws(max_queries)
        self._latest_flags()
        st = self.st
        if not flags:
            st = abi.NavsimState()
            C.memmove(C.byref(st), C.byref(self.st), C.sizeof(st))
            st.ped_due = None
        check(self.lib.navsim_replan(C.byref(self.cfg), C.byref(st), max_queries, _ptr(ws), ws.numel(), _stream()),
              "navsim_replan")

    # ---- navsim_replan beside the step (round 5).  env.py:667-680 plans a new route inside step() for the pedestrian that
    # reached its goal; here that is one breadth-first search per arrived pedestrian (~2 % of the arenas per step), a chain of
    # dependent levels that used to sit serially behind every step (c3 world through the gym API: 166 us of step + 98 us of
    # re-plan).  The arenas WITHOUT a waiting pedestrian do not need its result: navsim_step_part steps them on the caller's
    # stream while a side stream runs the re-plan of the previous step and then steps the arenas that waited for it.
    # Same kernels on the same per-arena inputs in the same per-arena order -- step(t), replan(t), step(t + 1) -- so every
    # result is what the serial sequence gives.
    replan_in_step = True             # planned routes: navsim_step_replan (one launch) instead of the two-stream overlap

    overlap_big_first = False         # which stream takes the big launch (launch_step_overlapped); A/B: profiles/r05_replan/

    def _overlap_streams(self):
        import torch
        if self._side is None:
            self._side = concurrent_stream(self.device, priority=-1 if self.overlap_big_first else 0)
        return torch.cuda.current_stream(self.device), self._side

    def launch_step_overlapped(self, replan_cap=1024, reorder=True):
        """navsim_step_part(NOT_DUE) beside [navsim_replan of the PREVIOUS step's flags -> navsim_step_part(DUE)], on two
        streams, joined at the end.  Needs the costmap (planned routes).
        Which stream takes what (overlap_big_first = False, measured: profiles/r05_replan/README.md): the re-plan chain runs on
        the caller's stream, where nothing has to be waited for, and the big launch on a side stream behind an event -- a few us
        later, so the searches' workgroups are resident before 4096 arena workgroups take every slot of the chip
        (c3 world through the gym API: 19.2-19.4 M env-steps/s; the other way round 18.6 M; serial, round 4: 15.5 M)."""
        if self.replan_in_step:
            if reorder:
                self._reorder()
            self._flush_sort()
            self._flip()
            rc = self.lib.navsim_step_replan(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), int(replan_cap), _stream())
            if rc == 0:
                self.cur = 1 - self.cur
                return
            if rc != abi.E_UNSUPPORTED:
                check(rc, "navsim_step_replan")
            self.replan_in_step = False             # a costmap of more words than the arena's workgroup has threads: two streams
            self._flip()                            # (idempotent: the same parity)
            reorder = False
        main, side = self._overlap_streams()
        big, chain = (main, side) if self.overlap_big_first else (side, main)
        ws = self._replan_ws(replan_cap)
        if reorder:
            self._reorder()
        self._flush_sort()
        for s_ in {big, chain} - {main}:            # the previous step (both parts were joined on `main`), regen, the actions
            s_.wait_stream(main)
        # the re-plan reads st.ped_due = the flags the previous step wrote: launched BEFORE the buffers flip
        self._latest_flags()
        rc = self.lib.navsim_replan(C.byref(self.cfg), C.byref(self.st), replan_cap, _ptr(ws), ws.numel(), C.c_void_p(chain.cuda_stream))
        if rc:
            check(rc, "navsim_replan")
        self._flip()
        rc = self.lib.navsim_step_part(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), abi.STEP_NOT_DUE, C.c_void_p(big.cuda_stream))
        if rc:
            check(rc, "navsim_step_part (not due)")
        rc = self.lib.navsim_step_part(C.byref(self.cfg), C.byref(self.st), C.byref(self.io), abi.STEP_DUE, C.c_void_p(chain.cuda_stream))
        if rc:
            check(rc, "navsim_step_part (due)")
        for s_ in {big, chain} - {main}:
            main.wait_stream(s_)
        self.cur = 1 - self.cur

    def step_overlapped(self, action=None, replan_cap=1024):
        """step() of a world with planned pedestrian routes: replan (of the previous step) + step, overlapped
        (launch_step_overlapped).  The sequence of calls  step_overlapped, step_overlapped, ...  equals
        step, replan, step, replan, ...  shifted by one replan: finish a rollout with replan() to leave the same state."""
        if action is not None:
            self._set_action(action)
        self.launch_step_overlapped(replan_cap)
        return self.obs, self.out

    def set_policy(self, weights):
        """HumanPolicy actor weights: dict of arrays / tensors named like abi.POLICY_FIELDS, or a reference
        state_dict (human_policy.py names, e.g. torch.load('human_policy.pth'))."""
        import torch
        named = {abi.POLICY_STATE_DICT.get(k, k): v for k, v in weights.items()}
        self.policy_t = {}
        self.policy_w = abi.NavsimPolicyWeights()
        for k in abi.POLICY_FIELDS:
            t = torch.as_tensor(named[k]).detach().to(device=self.device, dtype=torch.float32).reshape(abi.POLICY_SHAPES[k]).contiguous()
            self.policy_t[k] = t
            setattr(self.policy_w, k, t.data_ptr())
        nbytes = self.lib.navsim_ped_policy_workspace_bytes(C.byref(self.cfg))
        self.t["policy_ws"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if "policy_prev_actions" not in self.t:
            self.t["policy_prev_actions"] = torch.zeros((self.cfg.n_envs, self.cfg.max_peds, 2), dtype=torch.float32,
                                                        device=self.device)

    def _ped_policy_pipelined(self, n_slices):
        """scans -> network in slices of arenas on two streams (round 5; MEASURED AND NOT THE DEFAULT): the scans of slice
        k + 1 beside the network of slice k, same kernels on the same rows.  The round-4 verdict's idea -- a latency-bound
        march beside a layer at 0.8 of the f32 MFMA peak -- loses: 3.26 / 3.54 / 5.5 ms for 3 / 6 / 12 slices against 3.0 ms for
        the two calls at c3 size (profiles/r05_policy/): the march's waves and the layer's share the CUs' issue slots and LDS,
        smaller slices run the layer below its peak, and every slice costs two cross-stream waits."""
        import torch
        main = torch.cuda.current_stream(self.device)
        if self._scan_stream is None:
            self._scan_stream = torch.cuda.Stream(device=self.device)
            self.t["ped_scan_rows"] = torch.zeros((self.cfg.n_envs, self.cfg.max_peds, self.cfg.ped_n_beams), dtype=torch.float32,
                                                  device=self.device)
        side, rows, ws, E = self._scan_stream, self.t["ped_scan_rows"], self.t["policy_ws"], self.cfg.n_envs
        bounds = [E * k // n_slices for k in range(n_slices + 1)]
        side.wait_stream(main)                      # the state the scans read
        events = []
        for k in range(n_slices):
            e0, n_e = bounds[k], bounds[k + 1] - bounds[k]
            check(self.lib.navsim_ped_scans_part(C.byref(self.cfg), C.byref(self.st), _ptr(rows), e0, n_e, C.c_void_p(side.cuda_stream)),
                  "navsim_ped_scans_part")
            ev = torch.cuda.Event()
            ev.record(side)
            events.append(ev)
        for k in range(n_slices):
            e0, n_e = bounds[k], bounds[k + 1] - bounds[k]
            main.wait_event(events[k])
            check(self.lib.navsim_ped_policy_part(C.byref(self.cfg), C.byref(self.st), C.byref(self.policy_w), _ptr(rows),
                                                  _ptr(self.t["policy_prev_actions"]), _ptr(self.t["ped_cmd"]), _ptr(ws), ws.numel(),
                                                  e0, n_e, C.c_void_p(main.cuda_stream)), "navsim_ped_policy_part")
        return self.t["ped_cmd"], self.t["policy_prev_actions"]

    def ped_policy(self, scans=None, fused=False, scans_out=None, pipeline=None):
        """navsim_ped_policy (env.py:617-662): pedestrian scans -> HumanPolicy actor -> ped_cmd for a
        NAVSIM_PED_EXTERNAL step.  Returns (ped_cmd [E,N,2] float64, clip(mean) [E,N,2] float32).
        scans=None: the scans of the current state (navsim_ped_scans first; pipeline=n: taken and consumed in n slices of
        arenas on two streams, _ped_policy_pipelined -- measured slower, kept as an option).
        fused=True: navsim_ped_scan_policy -- every
        scan is taken inside the pass by the workgroup that convolves it and only written to HBM when scans_out (float32
        [E,N,512]) is given; bit-identical, saves the [E,N,512] buffer, measured 1 % slower than the two calls."""
        ws = self.t["policy_ws"]
        if scans is None and not fused and pipeline:
            return self._ped_policy_pipelined(int(pipeline) if int(pipeline) > 1 else 3)
        if fused:
            check(self.lib.navsim_ped_scan_policy(C.byref(self.cfg), C.byref(self.st), C.byref(self.policy_w),
                                                  _ptr(scans_out) if scans_out is not None else None,
                                                  _ptr(self.t["policy_prev_actions"]), _ptr(self.t["ped_cmd"]), _ptr(ws),
                                                  ws.numel(), _stream()), "navsim_ped_scan_policy")
            return self.t["ped_cmd"], self.t["policy_prev_actions"]
        if scans is None:
            scans = self.ped_scans()
        check(self.lib.navsim_ped_policy(C.byref(self.cfg), C.byref(self.st), C.byref(self.policy_w), _ptr(scans),
                                         _ptr(self.t["policy_prev_actions"]), _ptr(self.t["ped_cmd"]), _ptr(ws),
                                         ws.numel(), _stream()), "navsim_ped_policy")
        return self.t["ped_cmd"], self.t["policy_prev_actions"]

    def _ped_orca_struct(self, params):
        if isinstance(params, abi.NavsimPedOrcaParams):
            return params
        if params is None:
            if self._orca_default is None:
                self._orca_default = ped_orca_params(self.cfg, None)
            return self._orca_default
        return ped_orca_params(self.cfg, params)

    def ped_orca(self, params=None):
        """navsim_ped_orca: ORCA pedestrians from the simulator's own state -> ped_cmd for a NAVSIM_PED_EXTERNAL step, one
        kernel on the simulator's stream (waypoint pop, preferred velocity, neighbours out of LDS, the linear programs).
        params: None, a dict (ped_orca_params: unknown keys raise ValueError) or a ready abi.NavsimPedOrcaParams.
        Returns ped_cmd [E,N,2] float64; rows of slots >= n_peds[e] are left as they were."""
        params = self._ped_orca_struct(params)
        check(self.lib.navsim_ped_orca(C.byref(self.cfg), C.byref(self.st), C.byref(params), _ptr(self.t["ped_cmd"]), _stream()),
              "navsim_ped_orca")
        return self.t["ped_cmd"]

    def ped_orca_walls(self, params=None, max_rects=8, dropped=None):
        """navsim_ped_orca_walls: ped_orca() with the arena's listed rectangles (the list of its t['rect_index'] row) as ORCA
        obstacles -- every pedestrian avoids the max_rects (<= 32) nearest of them within time_horizon_obst * v_pref + radius.
        params as for ped_orca() (a dict's max_obst_rects is ignored: max_rects says it); dropped: None or an int32 [E,N]
        tensor that receives, per live pedestrian, how many rectangles in range were not kept.  max_rects = 0 is ped_orca().
        Returns ped_cmd [E,N,2] float64."""
        import torch
        params = self._ped_orca_struct(params)
        if dropped is not None and (dropped.dtype != torch.int32 or not dropped.is_contiguous() or
                                    tuple(dropped.shape) != (self.cfg.n_envs, self.cfg.max_peds) or
                                    dropped.device != self.t["ped_cmd"].device):
            raise ValueError("dropped must be a contiguous int32 [E,N] tensor on the simulator's device")
        check(self.lib.navsim_ped_orca_walls(C.byref(self.cfg), C.byref(self.st), C.byref(params), int(max_rects),
                                             _ptr(self.t["ped_cmd"]), None if dropped is None else _ptr(dropped), _stream()),
              "navsim_ped_orca_walls")
        return self.t["ped_cmd"]

    def ped_scans(self):
        """Scan of every pedestrian (env.py:685-693) from the current state -> float32 [E, N, 512]."""
        import torch
        out = torch.zeros((self.cfg.n_envs, self.cfg.max_peds, self.cfg.ped_n_beams), dtype=torch.float32,
                          device=self.device)
        check(self.lib.navsim_ped_scans(C.byref(self.cfg), C.byref(self.st), _ptr(out), _stream()), "navsim_ped_scans")
        return out

    # ---- hipGraph replay of a whole step (round 4).  A step of a world that draws new maps is four or five launches
    # (navsim_step, navsim_regen's three, navsim_replan's three) whose gaps are launch-bound: c5 4.77 -> 5.08 M env-steps/s.
    def enable_graphs(self, regen=False, replan_cap=0, overlap=True):
        """Capture a whole step once per observation-buffer parity and replay it in step_graphed():
        [navsim_step, navsim_regen (regen=True)], and with replan_cap > 0 the re-plan -- overlap=True (default): the re-plan
        of the PREVIOUS step beside this step's launch (launch_step_overlapped: a fork and a join inside the graph), False:
        navsim_replan behind the step as in round 4.  Actions go through the simulator's own action buffer (a graph's
        arguments are frozen), the longest-first launch order is not re-sorted (graphs are for the launches of one
        generation, where it does not matter).  Same kernels, same arguments, same per-arena order: same results.
        The configuration is captured BY VALUE: step_graphed() re-captures when self.cfg has changed since."""
        import torch
        if self.pregen:
            raise ValueError("enable_graphs and enable_pregen are alternatives")
        if regen:
            self._choose_regen_helper()                   # (timed with host synchronisation: before the capture)
        check(self.lib.navsim_prepare(C.byref(self.cfg), C.byref(self.st), C.byref(self._io_copy(obs=self.obs))), "navsim_prepare")
        if regen:                                         # (the workspaces: allocated before the capture)
            self._regen_ws()
        if replan_cap:
            self._replan_ws(replan_cap)
        self.io.action = self.action.data_ptr()
        self._graph_args = (bool(regen), int(replan_cap), bool(overlap))
        overlap = bool(overlap) and replan_cap > 0
        if overlap:
            self._overlap_streams()
        self._flush_sort()                                # (a sort that is due runs now: a captured launch's buffers are frozen)
        torch.cuda.synchronize(self.device)
        cur0, self._graphs = self.cur, {}
        for p in (0, 1):
            self.cur = p
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if overlap:
                    self.launch_step_overlapped(replan_cap, reorder=False)
                else:
                    self.launch_step(reorder=False)
                if regen:
                    self.regen()
                if replan_cap and not overlap:
                    self.replan(replan_cap)
            self._graphs[p] = g
        self.cur = cur0
        # a captured launch holds navsim_config BY VALUE (round-4 advisor: _override_reward_factor after the capture changed
        # compute_rewards() but not the step): remember what was captured, step_graphed() compares
        self._graph_cfg = bytes(self.cfg)
        torch.cuda.synchronize(self.device)

    def step_graphed(self, action=None):
        """step() (+ regen + replan, as captured by enable_graphs) as ONE graph launch."""
        if bytes(self.cfg) != self._graph_cfg:      # the configuration changed since the capture: capture again
            self.enable_graphs(*self._graph_args)
        if action is not None:
            self.action.copy_(self._as(action, self.action))
        self._graphs[self.cur].replay()
        self.cur = 1 - self.cur
        return self.obs, self.out

    def launch_step(self, reorder=True):
        """step() without the action copy: inputs already resident (bench inner loop).  reorder=False: the
        caller has already called _reorder() (bench.py keeps it outside its per-kernel events)."""
        if reorder:
            self._reorder()
        self._flip()
        self._launch()
        self.cur = 1 - self.cur

    def set_ped_cmd(self, cmd):
        self.t["ped_cmd"].copy_(self._as(cmd, self.t["ped_cmd"]))

    def _as(self, a, like):
        import torch
        if not isinstance(a, torch.Tensor):          # numpy >= 2 arrays also carry a `.device`
            a = torch.as_tensor(np.asarray(a))
        return a.to(device=self.device, dtype=like.dtype).reshape(like.shape)

    def by_arena(self, name):
        """t[name] with one entry per arena: the per-map arrays of a world with slot tables (2 E slots, a packed field being one
        flat blob) gathered through t['map_slot']; every other array as it is."""
        v = self.t[name]
        slots = self.t.get("map_slot")
        if slots is None or name not in self.MAPS:
            return v
        n_slots = 2 * self.cfg.n_envs
        rows = v.reshape(n_slots, -1)[slots.long()]
        return rows.reshape(-1) if v.dim() == 1 else rows.reshape((self.cfg.n_envs,) + tuple(v.shape[1:]))

    def numpy_state(self, *names):
        """State arrays on the host.  "ped_due": the latest step's "waits for navsim_replan" flags (they flip, so not in t)."""
        out = {n: self.by_arena(n).detach().cpu().numpy() for n in (names or self.t.keys()) if n != "ped_due"}
        if self.due is not None and (not names or "ped_due" in names):
            out["ped_due"] = self.due[self.cur].detach().cpu().numpy()
        return out
