"""GPU: what the step's entry points answer when they refuse a call (include/navsim.h navsim_step_part, navsim_step_replan,
navsim_step_install*, navsim_prepare) -- the return code of every refusal path between the C ABI and the launch, and that
such a call launches nothing: every output and state array is as it was.  The codes are those the library returned before
the launch path was rewritten around one descriptor (csrc/step_plan.hpp StepLaunch); the worlds are zero-filled buffers of
the right shapes (2 arenas, a 40 x 40 map, 64 beams), since no call here may reach a kernel.  One case needs another map:
"more costmap words than threads per arena" takes a costmap of at least 65 rows (one 64-bit word per row against the 64
threads of the narrowest workgroup), so it runs on a 325 x 40 map."""
import ctypes as C

import pytest

from gpu_support import gpu  # noqa: F401  (the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

E, SIDE, BEAMS, N = 2, 40, 64, 4
TALL = 325
OK, ARG, UNSUPPORTED = abi.OK, abi.E_ARG, abi.E_UNSUPPORTED


def _copy(s):
    o = type(s)()
    C.memmove(C.byref(o), C.byref(s), C.sizeof(s))
    return o


class _World:
    """A NavSim over zero-filled arrays, what the install calls need beside it, and a copy of everything a launch could write."""

    def __init__(self, gpu, H):
        torch = gpu.torch
        cfg = gpu.lib.default_config(n_envs=E, map_h=H, map_w=SIDE, max_peds=N, ped_model=abi.PED_SFM, n_spawn=2,
                                     auto_reset=abi.AUTORESET_SAME_STEP, seed=3, field_format=abi.FIELD_U16T, regen_cap=E,
                                     regen_min_steps=8)
        gpu.world.lidar_full_circle(cfg, BEAMS)
        arrays = gpu.world.empty_world(cfg, device=gpu.dev, plan_paths=True)
        arrays["scan_threshold"] = torch.zeros(BEAMS, dtype=torch.float32, device=gpu.dev)
        arrays["scan_discomfort"] = torch.zeros(BEAMS, dtype=torch.float32, device=gpu.dev)
        self.g = g = gpu.sim.NavSim(cfg, arrays)
        g._flip()                                                   # io as a step's launch finds it
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=gpu.dev)
        self.x = dict(stage_obs=torch.zeros_like(g.obs_buf[0]), mark=z(4, torch.uint8), ready=z(E, torch.int64), late=z(E, torch.uint8),
                      field_f32=z((E, H, SIDE), torch.float32), map_slot=torch.arange(E, dtype=torch.int32, device=gpu.dev))
        for t in g.obs_buf + [v for b in g.out_buf for v in b.values()]:
            t.fill_(7)                                              # (a launch writes zeros and ones over most of these)
        torch.cuda.synchronize()
        self.watched = list(g.t.values()) + g.obs_buf + [v for b in g.out_buf for v in b.values()] + g.due + list(self.x.values())
        self.before = [t.clone() for t in self.watched]

    def unchanged(self, torch):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(self.watched, self.before))

    def call(self, name, *tail, cfg=None, st=None, **state):
        """lib.<name>(cfg, st, io, *tail) with the given config fields / state pointers replaced in copies."""
        g = self.g
        c, s = g.cfg.copy(), _copy(g.st)
        for k, v in (cfg or {}).items():
            setattr(c, k, v)
        for k, v in dict(st or {}, **state).items():
            setattr(s, k, None if v is None else self.x[v].data_ptr())
        tail = [C.byref(s) if a == "stage" else (C.c_void_p(self.x[a].data_ptr()) if isinstance(a, str) else a) for a in tail]
        return getattr(g.lib, name)(C.byref(c), C.byref(s), C.byref(g.io), *tail)


@pytest.fixture(scope="module")
def worlds(gpu):
    return {"square": _World(gpu, SIDE), "tall": _World(gpu, TALL)}


INSTALL = ("stage", "stage_obs", "mark", "ready", "late")          # navsim_step_install's arguments behind io
F32 = dict(cfg=dict(field_format=abi.FIELD_F32), field="field_f32")
NO_PEDS = dict(ped_model=abi.PED_NONE)
WIDE = dict(angle_min=-3.5, angle_last=3.5)                        # 7 rad > 2 pi

CASES = [
    # navsim_step_part
    ("part_3", "square", ("navsim_step_part", 3, None), {}, ARG),
    ("part_negative", "square", ("navsim_step_part", -1, None), {}, ARG),
    ("part_without_pedestrians", "square", ("navsim_step_part", abi.STEP_NOT_DUE, None), dict(cfg=NO_PEDS), ARG),
    ("part_not_due_ped_split", "square", ("navsim_step_part", abi.STEP_NOT_DUE, None), dict(cfg=dict(ped_split=2)), UNSUPPORTED),
    ("part_due_ped_split", "square", ("navsim_step_part", abi.STEP_DUE, None), dict(cfg=dict(ped_split=2)), UNSUPPORTED),
    ("part_not_due_map_slot", "square", ("navsim_step_part", abi.STEP_NOT_DUE, None), dict(map_slot="map_slot"), UNSUPPORTED),
    ("part_due_map_slot", "square", ("navsim_step_part", abi.STEP_DUE, None), dict(map_slot="map_slot"), UNSUPPORTED),
    # navsim_step_replan
    ("replan_ped_split", "square", ("navsim_step_replan", 8, None), dict(cfg=dict(ped_split=2)), UNSUPPORTED),
    ("replan_negative_cap", "square", ("navsim_step_replan", -1, None), {}, ARG),
    ("replan_without_costmap", "square", ("navsim_step_replan", 8, None), dict(costmap=None), ARG),
    ("replan_without_pedestrians", "square", ("navsim_step_replan", 8, None), dict(cfg=NO_PEDS), ARG),
    ("replan_block_below_plan_words", "tall", ("navsim_step_replan", 8, None), dict(cfg=dict(step_block=64)), UNSUPPORTED),
    ("replan_map_slot", "square", ("navsim_step_replan", 8, None), dict(map_slot="map_slot"), UNSUPPORTED),
    # navsim_step_install, navsim_step_install_replan
    ("install_f32", "square", ("navsim_step_install",) + INSTALL + (None,), F32, UNSUPPORTED),
    ("install_cap_below_n_envs", "square", ("navsim_step_install",) + INSTALL + (None,), dict(cfg=dict(regen_cap=1)), UNSUPPORTED),
    ("install_ped_split", "square", ("navsim_step_install",) + INSTALL + (None,), dict(cfg=dict(ped_split=2)), UNSUPPORTED),
    ("install_replan_without_costmap", "square", ("navsim_step_install_replan",) + INSTALL + (8, None), dict(costmap=None), ARG),
    ("install_replan_without_pedestrians", "square", ("navsim_step_install_replan",) + INSTALL + (8, None), dict(cfg=NO_PEDS), ARG),
    ("install_replan_block_below_plan_words", "tall", ("navsim_step_install_replan",) + INSTALL + (8, None),
     dict(cfg=dict(step_block=64)), UNSUPPORTED),
    # the lone form (NEXT_STEP without a fallback: an arena regenerates its own world inside the launch) draws square maps only
    ("install_lone_not_square", "tall", ("navsim_step_install", "stage", "stage_obs", "mark", "ready", None, None),
     dict(cfg=dict(auto_reset=abi.AUTORESET_NEXT_STEP, regen_min_steps=0, step_block=256), costmap=None), UNSUPPORTED),
    # navsim_prepare launches nothing whatever it is given; a form the configuration cannot use is skipped without an error
    ("prepare_all_forms", "square", ("navsim_prepare",), {}, OK),
    ("prepare_no_part_replan_install_lone", "square", ("navsim_prepare",),
     dict(cfg=dict(NO_PEDS, field_format=abi.FIELD_F32, regen_cap=0), field="field_f32"), OK),
    ("prepare_ped_split", "square", ("navsim_prepare",), dict(cfg=dict(ped_split=2)), OK),
    ("prepare_without_costmap", "square", ("navsim_prepare",), dict(costmap=None), OK),
    ("prepare_block_below_plan_words", "tall", ("navsim_prepare",), dict(cfg=dict(step_block=64)), OK),
    ("prepare_map_slot_without_pedestrians", "square", ("navsim_prepare",), dict(cfg=NO_PEDS, map_slot="map_slot"), OK),
    # (a state with slot tables has no navsim_step_part form, and navsim_prepare says so instead of skipping it)
    ("prepare_map_slot_with_pedestrians", "square", ("navsim_prepare",), dict(map_slot="map_slot"), UNSUPPORTED),
    # a lidar wider than one turn in a world with pedestrians (include/navsim.h angle_last): refused by dispatch_step, which
    # every step and reset entry passes through, ahead of ped_update_kernel; without pedestrians the same lidar is served
    # (tests/test_gpu_ped_edge_scenes.py runs it against the oracle)
    ("step_lidar_above_one_turn", "square", ("navsim_step", None), dict(cfg=WIDE), UNSUPPORTED),
    ("step_lidar_far_above_one_turn", "square", ("navsim_step", None), dict(cfg=dict(angle_min=-3.2, angle_last=6.2)), UNSUPPORTED),
    ("step_lidar_above_one_turn_ped_split", "square", ("navsim_step", None), dict(cfg=dict(WIDE, ped_split=2)), UNSUPPORTED),
    ("step_lidar_above_one_turn_external", "square", ("navsim_step", None), dict(cfg=dict(WIDE, ped_model=abi.PED_EXTERNAL)), UNSUPPORTED),
    ("step_part_lidar_above_one_turn", "square", ("navsim_step_part", abi.STEP_DUE, None), dict(cfg=WIDE), UNSUPPORTED),
    ("step_replan_lidar_above_one_turn", "square", ("navsim_step_replan", 8, None), dict(cfg=WIDE), UNSUPPORTED),
    ("step_install_lidar_above_one_turn", "square", ("navsim_step_install",) + INSTALL + (None,), dict(cfg=WIDE), UNSUPPORTED),
    ("reset_obs_lidar_above_one_turn", "square", ("navsim_reset_obs", None, None), dict(cfg=WIDE), UNSUPPORTED),
    ("prepare_lidar_above_one_turn", "square", ("navsim_prepare",), dict(cfg=WIDE), UNSUPPORTED),
    ("prepare_lidar_above_one_turn_without_pedestrians", "square", ("navsim_prepare",), dict(cfg=dict(WIDE, **NO_PEDS)), OK),
]


@pytest.mark.parametrize("world,call,changes,code", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal_code_and_nothing_launched(gpu, worlds, world, call, changes, code):
    w = worlds[world]
    rc = w.call(*call, **changes)
    assert rc == code, "%s returned %d" % (call[0], rc)
    assert w.unchanged(gpu.torch), "%s wrote to the outputs or the state" % call[0]


def test_pedestrian_scan_entries_refuse_a_lidar_above_one_turn(gpu):
    """include/navsim.h ped_angle_last: navsim_ped_scans, navsim_ped_scans_part and navsim_ped_scan_policy return
    NAVSIM_E_UNSUPPORTED for ped_angle_last - ped_angle_min > 2 pi and write nothing.  (Exactly 2 pi is served:
    tests/test_gpu_ped_edge_scenes.py runs it against the oracle.)"""
    torch = gpu.torch
    w = _World(gpu, SIDE)
    g = w.g
    g.set_policy({k: torch.zeros(abi.POLICY_SHAPES[k]) for k in abi.POLICY_FIELDS})
    ws = g.t["policy_ws"]
    ws.zero_()
    scans = torch.full((E, N, g.cfg.ped_n_beams), 7.0, dtype=torch.float32, device=gpu.dev)
    prev, cmd = g.t["policy_prev_actions"], g.t["ped_cmd"]
    extra = [scans, ws, prev] + list(g.policy_t.values())
    before = [t.clone() for t in extra]
    P = lambda t: C.c_void_p(t.data_ptr())
    c = g.cfg.copy()
    c.ped_angle_min, c.ped_angle_last = -3.5, 3.5
    calls = dict(
        navsim_ped_scans=lambda c: g.lib.navsim_ped_scans(C.byref(c), C.byref(g.st), P(scans), None),
        navsim_ped_scans_part=lambda c: g.lib.navsim_ped_scans_part(C.byref(c), C.byref(g.st), P(scans), 0, E, None),
        navsim_ped_scan_policy=lambda c: g.lib.navsim_ped_scan_policy(C.byref(c), C.byref(g.st), C.byref(g.policy_w), P(scans), P(prev),
                                                                      P(cmd), P(ws), ws.numel(), None))
    for name, call in calls.items():
        assert call(c) == UNSUPPORTED, name
        assert w.unchanged(torch) and all(torch.equal(a, b) for a, b in zip(extra, before)), "%s wrote something" % name
