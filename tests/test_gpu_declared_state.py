"""GPU: a NavSim that has NOT been through any enable_* call -- the path the big equality tests never take.  Its state is
declared in __init__ at the "not enabled" values, the reset calls run on it as it is, and enable_pregen() leaves what its
arguments say."""
import pytest

from gpu_support import gpu, device_sim, regen_layout, seeded_action  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

OFF = dict(pregen=False, pg_install=False, pg_period=0, pg_k=0, pg_passes=0, stage_cap=0, pg_open=[], pg_swapped=[], pg_staged=[],
           stage_lane=[], stage_t={}, stage_st=None, stage_cfg=None, stage_obs=None, stage_io=None, stage_ws=None, want=None,
           mark=None, ready=None, side=None, ev_swapped=None, ev_staged=None,
           late=None, late_cfg=None, late_ws=None, late_cap=0, late_poll=False, lone=False,
           late2=None, urgent=None, ev_stepped=None, ev_urgent=None,
           pg_replan_cap=0, pg_replan_in_step=True, _side=None, _regen_helper=None, _action_ref=None, _graphs={}, _graph_args=None,
           _graph_cfg=None, policy_t={}, policy_w=None, _scan_stream=None, _orca_default=None)


def test_a_simulator_without_any_enable_call(gpu):
    torch = gpu.torch
    cfg, occ, _, wkw = regen_layout(gpu, "float32-smallest")       # its map and spawn rules; smaller, packed, with pedestrians
    E = 6                                                           # no multiple of 4: the last word of `mark` is padding
    cfg.n_envs, cfg.regen_cap, cfg.max_peds, cfg.ped_model, cfg.field_format = E, E, 2, abi.PED_SFM, abi.FIELD_U16T
    gpu.world.lidar_full_circle(cfg, 64)
    g = device_sim(gpu, cfg, occ[:E], 2, **wkw)
    for k, v in OFF.items():
        assert getattr(g, k) == v and type(getattr(g, k)) is type(v), k
    g.close(); g.close()
    # the reset calls of an object that has not been through enable_pregen / enable_graphs
    g.step(seeded_action(gpu, E, 1))
    g.out["done"].fill_(1)
    goals = g.t["spawn_goal"].clone()
    g.regen()
    assert int((g.t["spawn_goal"] != goals).flatten(1).any(1).sum()) == E
    goals = g.t["spawn_goal"].clone()
    mask = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.uint8)
    g.reset_arenas(mask, new_world=True)
    assert (g.t["spawn_goal"] != goals).flatten(1).any(1).cpu().tolist() == mask.bool().tolist()
    goals = g.t["spawn_goal"].clone()
    g.regenerate_all(new_episode=True)
    assert int((g.t["spawn_goal"] != goals).flatten(1).any(1).sum()) == E
    assert not g.pregen and g.stage_lane == [] and "regen_ws" in g.t
    # ... and then the pipelined reset path: what enable_pregen leaves is what its arguments say
    g.enable_pregen(pipeline=1, install=True)
    assert g.pregen is True and g.pg_install is True and g.pg_period == 1 and len(g.stage_lane) == 1
    assert g.mark.numel() == 8 and g.stage_lane[0]["side"] is g.side and g.stage_lane[0]["ws"] is g.stage_ws
    assert g.late is not None and g.late.shape == (E,)              # regen_min_steps = 0 < 4 P: the fallback
    assert g.late2 is None and g.lone is False and g.late_poll is False    # same-step restarts, outdoor maps, no planning
    for k in (2, 3, 4):
        obs, out = g.step(seeded_action(gpu, E, k))
        g.regen()
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and g.pg_k == 3 and g.pg_passes == 3
    g.close()


def test_a_refused_enable_pregen_leaves_the_simulator_as_it_was(gpu):
    """enable_pregen decides everything (sim.pregen_plan) before it touches the object: a call it refuses -- the last of its
    checks (stage_lanes) or an early one -- leaves every attribute at its "not enabled" value, no plan, no slot table and the
    maps where they were; a valid call on the same object then works."""
    torch = gpu.torch
    cfg, occ, _, wkw = regen_layout(gpu, "float32-smallest")
    E = 6
    cfg.n_envs, cfg.regen_cap, cfg.max_peds, cfg.ped_model, cfg.field_format = E, E, 2, abi.PED_SFM, abi.FIELD_U16T
    gpu.world.lidar_full_circle(cfg, 64)
    g = device_sim(gpu, cfg, occ[:E], 2, **wkw)
    field = g.t["field"]
    for kw, text in ((dict(pipeline=1, install=True, stage_lanes=3), "stage_lanes=3"), (dict(fallback=True), "fallback=True")):
        with pytest.raises(ValueError, match=text):
            g.enable_pregen(**kw)
        for k, v in OFF.items():
            assert getattr(g, k) == v and type(getattr(g, k)) is type(v), (kw, k)
        assert g.pg_plan is None and "map_slot" not in g.t and g.t["field"] is field
    g.enable_pregen(pipeline=1, install=True)
    assert g.pregen is True and g.pg_install is True and g.pg_period == 1 and len(g.stage_lane) == 1
    assert g.pg_plan == gpu.sim.pregen_plan(g.cfg, False, False, pipeline=1, install=True)
    assert g.pg_plan.fallback and g.late is not None and g.late_cap == g.pg_plan.late_cap == E and g.stage_cap == g.pg_plan.stage_cap == E
    assert "map_slot" in g.t and g.stage_lane[0]["side"] is g.side and g.stage_lane[0]["ws"] is g.stage_ws
    for k in (2, 3, 4):
        obs, out = g.step(seeded_action(gpu, E, k))
        g.regen()
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and g.pg_k == 3 and g.pg_passes == 3
    g.close()
