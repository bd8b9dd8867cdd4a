"""What NavSim.enable_pregen leaves, over a grid of worlds, configurations and keyword arguments: one JSON line per combination.

  python compare.py dump --package DIR --out FILE    on a GPU; DIR holds the nav_gym_amd package of the tree under test (a checkout
                                                     of the parent commit, or this tree); NAVSIM_LIB may name the built library
  python compare.py diff PARENT.jsonl NEW.jsonl      on the host: the differences, and every combination of PARENT.jsonl held
                                                     against sim.pregen_plan of this tree (no device)

A combination is a fresh NavSim on a shared world, one enable_pregen call, and a snapshot: the ValueError's text if the call was
refused, and in either case what the object holds afterwards.  `off` is the snapshot before the call."""
import argparse
import gc
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, map kind, arenas, map side): the caps' E // 64 and E // 128 branches pass 8 at 576 and 1152 arenas, so 6 and 1280;
# the corridor world only small; t_* are the worlds of the named rows of tests/test_host_logic.py's table
WORLDS = [("outdoor", "outdoor", 6, 200), ("outdoor", "outdoor", 1280, 200), ("costmap", "costmap", 6, 300),
          ("costmap", "costmap", 1280, 300), ("corridor", "corridor", 6, 260),
          ("t_abc", "outdoor", 512, 200), ("t_d", "corridor", 1024, 260), ("t_fg", "outdoor", 48, 200)]

INSTALL = dict(pipeline=4, install=True)
# keyword arguments of enable_pregen; "cfg_cap": cfg.regen_cap (default: n_envs)
CALLS = [dict(), dict(pipeline=4), dict(pipeline=3, cfg_cap=8), dict(cfg_cap=8), dict(pipeline=-1), dict(pipeline=4, stage_cap=3),
         dict(pipeline=4, stage_lanes=2), dict(fallback=True), dict(pipeline=4, fallback=True), dict(install=True),
         dict(INSTALL), dict(pipeline=1, install=True), dict(INSTALL, cfg_cap=3), dict(INSTALL, late_beside=True),
         dict(INSTALL, fallback_poll=False), dict(INSTALL, fallback_poll=True), dict(INSTALL, stage_lanes=1),
         dict(INSTALL, stage_lanes=2), dict(INSTALL, stage_lanes=3), dict(INSTALL, stage_cap=3), dict(INSTALL, fallback_cap=4),
         dict(INSTALL, map_slots=False), dict(INSTALL, fallback=False), dict(INSTALL, fallback=True),
         dict(INSTALL, fallback=True, late_beside=True, fallback_cap=4, stage_lanes=2)]
TABLE_CALLS = {"t_abc": [dict(INSTALL), dict(INSTALL, late_beside=True)], "t_d": [dict(INSTALL)],
               "t_fg": [dict(pipeline=3, cfg_cap=8), dict(cfg_cap=8)]}


def grid():
    """(world index, auto_reset, regen_min_steps, call) of every combination; regen_min_steps 0 and 4 P (P > 0), 12 for row f."""
    for w, (name, kind, E, size) in enumerate(WORLDS):
        calls = TABLE_CALLS.get(name, CALLS)
        for mode, call in itertools.product((1, 2), calls):
            P = int(call.get("pipeline", 0))
            for rms in ((0, 4 * P) if P > 0 else (0,)):
                yield w, mode, rms, call
        yield w, 0, 0, dict()                                     # no auto-reset: refused


def snapshot(g):
    flags = ("pregen", "pg_install", "pg_period", "pg_k", "pg_passes", "stage_cap", "late_cap", "late_poll", "lone", "rs_cap")
    s = {k: getattr(g, k) for k in flags}
    s["none"] = sorted(k for k in ("late", "late2", "ready", "urgent", "_regen_helper", "side", "stage_st", "stage_obs", "want", "mark",
                                   "stage_ws", "late_ws", "ev_staged", "ev_stepped") if getattr(g, k) is None)
    s["stage_cfg_cap"] = None if g.stage_cfg is None else g.stage_cfg.regen_cap
    s["late_cfg"] = None if g.late_cfg is None else [g.late_cfg.regen_cap, g.late_cfg.defer_reset_scan]
    s["lanes"] = len(g.stage_lane)
    s["lane_helpers"] = [ln["helper"] is not None for ln in g.stage_lane]
    s["lane0_is_self"] = bool(g.stage_lane) and all(g.stage_lane[0][k] is v for k, v in (
        ("want", g.want), ("io", g.stage_io), ("ws", g.stage_ws), ("side", g.side), ("helper", g._regen_helper)))
    s["mark"] = None if g.mark is None else g.mark.numel()
    s["ws_bytes"] = [None if t is None else t.numel() for t in (g.stage_ws, g.late_ws)]
    s["map_slot"] = "map_slot" in g.t
    s["field_rows"] = g.t["field"].shape[0]
    s["stage_t"] = sorted(g.stage_t)
    s["side_priority"] = None if g.side is None else g.side.priority
    return s


def make_world(kind, E, size, torch, abi, lib, robots, sim, world):
    """cfg and arrays of a small world of `kind` (tests/gpu_support.py regen_layout's, with 64 beams); 64 maps, repeated"""
    kw = dict(n_envs=E, map_h=size, map_w=size, auto_reset=1, n_spawn=6, seed=31, min_goal_dist=3.0, max_goal_dist=8.0,
              spawn_clearance=0.9, ped_min_robot_dist=2.0, ped_min_goal_dist=4.0, field_format=abi.FIELD_U16T, regen_cap=E)
    if kind == "outdoor":
        cfg = lib.default_config(max_peds=2, ped_model=abi.PED_SFM, regen_plan=0, regen_indoor_ratio=0.0, **kw)
        n_peds, wkw, n_obst = 2, {}, 10
    elif kind == "costmap":
        cfg = lib.default_config(max_peds=6, ped_model=abi.PED_SFM, regen_plan=1, regen_indoor_ratio=0.0, obstacle_number=6, **kw)
        n_peds, wkw, n_obst = 5, dict(plan_paths=True, v_pref_range=(0.5, 0.6)), 6
    else:
        cfg = lib.default_config(max_peds=6, ped_model=abi.PED_SFM, regen_plan=1, regen_indoor_ratio=0.5, **kw)
        n_peds, wkw, n_obst = 5, dict(plan_paths=True), 10
    world.lidar_full_circle(cfg, 64)
    import numpy as np
    occ = world.make_maps(min(E, 64), size, 31, n_obstacles=n_obst)
    occ = np.concatenate([occ] * ((E + 63) // 64))[:E]
    arrays = world.make_world(cfg, occ, n_peds=n_peds, **wkw)
    for key, name in (("scan_threshold", "threshold_footprint"), ("scan_discomfort", "discomfort_threshold_footprint")):
        arrays[key] = sim.scan_threshold(cfg, torch.from_numpy(robots.footprint_array("keti", name)).to("cuda:0"))
    return cfg, arrays


def dump(package, out):
    sys.path.insert(0, package)
    import torch
    from nav_gym_amd import abi, lib, robots, sim, world
    rows, built = list(grid()), {}
    with open(out, "w") as f:
        f.write(json.dumps(dict(source_hash=lib.source_hash(), package=os.path.basename(os.path.abspath(package)))) + "\n")
        for i, (w, mode, rms, call) in enumerate(rows):
            name, kind, E, size = WORLDS[w]
            if w not in built:
                built.clear()                                     # one world resident at a time
                gc.collect(); torch.cuda.empty_cache()
                built[w] = make_world(kind, E, size, torch, abi, lib, robots, sim, world)
            cfg, arrays = built[w]
            kw = dict(call)
            c = cfg.copy()
            c.auto_reset, c.regen_min_steps, c.regen_cap = mode, rms, min(E, kw.pop("cfg_cap", E))
            g = sim.NavSim(c, {k: v.clone() for k, v in arrays.items()})
            g.reset_obs()
            rec = dict(world=name, kind=kind, E=E, auto_reset=mode, regen_min_steps=rms, regen_cap=c.regen_cap, regen_plan=c.regen_plan,
                       regen_indoor_ratio=c.regen_indoor_ratio, costmap="costmap" in g.t, call=call, off=snapshot(g), error=None)
            try:
                g.enable_pregen(**kw)
            except ValueError as e:
                rec["error"] = str(e)
            torch.cuda.synchronize()
            rec["after"] = snapshot(g)
            f.write(json.dumps(rec, sort_keys=True) + "\n")
            f.flush()
            g.close()
            del g
            gc.collect()
            if i % 50 == 0:
                print("%d / %d" % (i, len(rows)), flush=True)
    print("%d combinations -> %s" % (len(rows), out))


def plan_view(rec):
    """What sim.pregen_plan of THIS tree says the snapshot of a successful call must hold (no device)."""
    sys.path.insert(0, os.path.join(HERE, "..", "..", "nav-gym_amd"))
    from nav_gym_amd import abi, sim
    cfg = abi.NavsimConfig()
    cfg.n_envs, cfg.auto_reset, cfg.regen_min_steps, cfg.regen_cap = rec["E"], rec["auto_reset"], rec["regen_min_steps"], rec["regen_cap"]
    cfg.regen_plan, cfg.regen_indoor_ratio = rec["regen_plan"], rec["regen_indoor_ratio"]
    kw = {k: v for k, v in rec["call"].items() if k != "cfg_cap"}
    try:
        p = sim.pregen_plan(cfg, rec["auto_reset"] == abi.AUTORESET_NEXT_STEP, rec["costmap"], **kw)
    except ValueError as e:
        return str(e), None
    return None, dict(pg_install=p.install, pg_period=p.period, stage_cap=p.stage_cap, stage_cfg_cap=p.stage_cap, late_cap=p.late_cap,
                      late_poll=p.poll, lone=p.lone, lanes=p.lanes, lane_helpers=[p.helper] * p.lanes, map_slot=p.shared_maps,
                      field_rows=rec["off"]["field_rows"] * (2 if p.shared_maps else 1), side_priority=p.side_priority,
                      late=p.fallback, late2=p.beside, urgent=p.beside, ready=p.period > 0, _regen_helper=p.helper,
                      late_cfg_cap=p.late_cap if p.fallback else None, late_defer=p.late_defer_scan)


def diff(parent, new):
    a, b = ([json.loads(ln) for ln in open(p)] for p in (parent, new))
    print("PARENT %s, NEW %s" % (json.dumps(a[0]), json.dumps(b[0])))
    a, b = a[1:], b[1:]
    assert len(a) == len(b)
    key = lambda r: (r["world"], r["E"], r["auto_reset"], r["regen_min_steps"], json.dumps(r["call"], sort_keys=True))
    assert [key(r) for r in a] == [key(r) for r in b]
    n_ok = n_err = d_ok = d_err = left = touched = plan_bad = 0
    for ra, rb in zip(a, b):
        assert ra["off"] == rb["off"]
        if ra["error"] is None and rb["error"] is None:
            n_ok += 1
            if ra["after"] != rb["after"]:
                d_ok += 1
                print("DIFFERS", key(ra), {k: (ra["after"][k], rb["after"].get(k)) for k in ra["after"] if ra["after"][k] != rb["after"].get(k)})
        else:
            n_err += 1
            d_err += ra["error"] != rb["error"]
            left += ra["after"] != ra["off"]                       # the parent: a refused call that left something behind
            touched += rb["after"] != rb["off"]                    # this tree: must be 0
        err, want = plan_view(ra)                                   # the parent's file against pregen_plan on the host
        s = ra["after"]
        if err is not None or ra["error"] is not None:
            plan_bad += err != ra["error"]
        else:
            have = dict(s, late="late" not in s["none"], late2="late2" not in s["none"], urgent="urgent" not in s["none"],
                        ready="ready" not in s["none"], _regen_helper="_regen_helper" not in s["none"],
                        late_cfg_cap=s["late_cfg"] and s["late_cfg"][0],
                        late_defer=bool(s["late_cfg"] and s["late_cfg"][1]))
            bad = {k: (have[k], v) for k, v in want.items() if have[k] != v}
            plan_bad += bool(bad)
            if bad:
                print("PLAN", key(ra), bad)
    print("the worlds of tests/test_host_logic.py's table rows, as PARENT left them:")
    for r in a:
        if r["world"].startswith("t_") and r["auto_reset"]:
            s = r["after"]
            print("  %s E=%d auto_reset=%d regen_min_steps=%d regen_cap=%d %s -> %s" % (
                r["world"], r["E"], r["auto_reset"], r["regen_min_steps"], r["regen_cap"], json.dumps(r["call"], sort_keys=True),
                r["error"] or json.dumps(dict({k: s[k] for k in ("pg_period", "pg_install", "stage_cap", "late_cap", "late_poll", "lone", "lanes",
                                                                 "lane_helpers", "map_slot", "side_priority", "late_cfg")},
                                              late="late" not in s["none"], late2="late2" not in s["none"]), sort_keys=True)))
    print("%d combinations: %d enabled, %d of them differ; %d refused, %d messages differ" % (len(a), n_ok, d_ok, n_err, d_err))
    print("refused calls that left state behind: PARENT %d, NEW %d" % (left, touched))
    print("PARENT's snapshots and messages against sim.pregen_plan on the host: %d differ" % plan_bad)
    return d_ok + d_err + touched + plan_bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump"); d.add_argument("--package", required=True); d.add_argument("--out", required=True)
    c = sub.add_parser("diff"); c.add_argument("parent"); c.add_argument("new")
    args = ap.parse_args()
    sys.exit(dump(args.package, args.out) if args.cmd == "dump" else diff(args.parent, args.new))
