"""navsim_reset_install (include/navsim.h): reset() of some arenas on a simulator with staged worlds, one launch.  No GPU here:
the export, the unchanged ABI, and every refusal the entry point makes before it touches the device."""
import ctypes as C

from nav_gym_amd import abi


def test_abi_stays_7_with_one_new_export():
    from nav_gym_amd import lib
    L = lib.load()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()
    assert C.sizeof(abi.NavsimState) == L.navsim_sizeof_state()
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    assert abi.NavsimConfig._fields_[-1][0] == "max_episode_steps" and abi.NavsimStepIO._fields_[-1][0] == "truncated"
    assert "navsim_reset_install" in abi.EXPORTS and hasattr(L, "navsim_reset_install")
    assert len(L.navsim_reset_install.argtypes) == 10


def _valid(lib, **cfg_kw):
    """A call that passes every check: the pointers all name one host buffer, which nothing may ever read -- every case below is
    refused, or has no arena to launch for."""
    kw = dict(n_envs=4, map_h=160, map_w=160, max_peds=1, ped_model=abi.PED_NONE, n_spawn=4, auto_reset=abi.AUTORESET_SAME_STEP,
              field_format=abi.FIELD_U16T, regen_cap=4)
    kw.update(cfg_kw)
    cfg = lib.default_config(**kw)
    buf = (C.c_double * 64)()
    ptr = C.addressof(buf)
    live, stage, io = abi.NavsimState(), abi.NavsimState(), abi.NavsimStepIO()
    for st in (live, stage):
        for name in ("field", "scan_threshold", "scan_discomfort", "robot_pose", "robot_goal", "prev_action", "prev_pose", "n_hist",
                     "episode", "steps", "spawn_pose", "spawn_goal", "done_steps"):
            setattr(st, name, ptr)
    io.obs = ptr
    io.obs_prev = ptr
    args = dict(stage=stage, stage_obs=ptr, mark=ptr, ready=ptr, mask=ptr, late=ptr)
    return cfg, live, io, args, buf


def _call(L, cfg, live, io, args):
    a = dict(args)
    stage = a.pop("stage")
    return L.navsim_reset_install(C.byref(cfg), C.byref(live), C.byref(io), None if stage is None else C.byref(stage),
                                  a["stage_obs"], a["mark"], a["ready"], a["mask"], a["late"], None)


def test_argument_refusals_without_gpu():
    from nav_gym_amd import lib
    L = lib.load()
    # nothing to launch for: the one call here that is not refused
    cfg, live, io, args, buf = _valid(lib, n_envs=0, regen_cap=1)
    assert _call(L, cfg, live, io, args) == abi.OK
    # a NULL argument
    for name in ("stage", "stage_obs", "mark", "ready", "mask", "late"):
        cfg, live, io, args, buf = _valid(lib)
        args[name] = None
        assert _call(L, cfg, live, io, args) == abi.E_ARG, name
    cfg, live, io, args, buf = _valid(lib)
    live.done_steps = None
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    assert L.navsim_reset_install(None, C.byref(live), C.byref(io), C.byref(args["stage"]), args["stage_obs"], args["mark"],
                                  args["ready"], args["mask"], args["late"], None) == abi.E_ARG
    # mark[] is consumed in 32-bit words
    for off in (1, 2, 3):
        cfg, live, io, args, buf = _valid(lib)
        args["mark"] = C.addressof(buf) + off
        assert _call(L, cfg, live, io, args) == abi.E_ARG, off
    # the two states hold different optional buffers
    for name in ("field_overflow", "rect_table", "costmap", "ped_goal"):
        for which in ("live", "stage"):
            cfg, live, io, args, buf = _valid(lib)
            setattr(live if which == "live" else args["stage"], name, C.addressof(buf))
            assert _call(L, cfg, live, io, args) == abi.E_ARG, (name, which)
    # slot tables: both states or neither, two tables over the same per-map arrays
    cfg, live, io, args, buf = _valid(lib)
    live.map_slot = C.addressof(buf)
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    cfg, live, io, args, buf = _valid(lib)
    args["stage"].map_slot = C.addressof(buf)
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    cfg, live, io, args, buf = _valid(lib)
    live.map_slot = args["stage"].map_slot = C.addressof(buf)                    # one table for both
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    cfg, live, io, args, buf = _valid(lib)
    live.map_slot, args["stage"].map_slot = C.addressof(buf), C.addressof(buf) + 64
    args["stage"].field = C.addressof(buf) + 128                                 # two tables, but not over the same field
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    # nothing restarts by itself: there are no staged worlds to follow the episodes
    cfg, live, io, args, buf = _valid(lib, auto_reset=abi.AUTORESET_NONE)
    assert _call(L, cfg, live, io, args) == abi.E_ARG
    # a float32 field; a first scan deferred to navsim_regen
    cfg, live, io, args, buf = _valid(lib, field_format=abi.FIELD_F32)
    assert _call(L, cfg, live, io, args) == abi.E_UNSUPPORTED
    cfg, live, io, args, buf = _valid(lib, defer_reset_scan=1)
    assert _call(L, cfg, live, io, args) == abi.E_UNSUPPORTED
    for mode in (abi.AUTORESET_SAME_STEP, abi.AUTORESET_NEXT_STEP):              # both restart modes pass the checks (no arenas)
        cfg, live, io, args, buf = _valid(lib, n_envs=0, regen_cap=1, auto_reset=mode)
        assert _call(L, cfg, live, io, args) == abi.OK
