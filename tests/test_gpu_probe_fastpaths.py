"""The wave-uniform short form of a probe round (kernels_step.hpp probe_round, RECT = 2 without pedestrians; profiles/r14_probe/).

A round leaves out the tile's second rectangle when no live lane's tile has one.  That is a choice of a whole wavefront, so
each scene below puts the lanes of ONE wavefront where a round must take the short form, the long form, or change between
them (tests/probe_fastpaths_spec.py), and asserts with a NumPy census of the same rounds that it does.  Every output and state
array of a rollout must equal the CPU oracle's bit for bit, noise off.
"""
import numpy as np
import pytest

import probe_fastpaths_spec as spec
import ref
from gpu_support import gpu, device_world, eq, host_arrays, state_equal, to_device  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

STEPS = 12
RULES = {"f32": abi.MARCH_F32, "f32_fma": abi.MARCH_F32_FMA, "f64": abi.MARCH_F64}


def _actions(E, t):
    """straight ahead at full speed, with a slow turn every fourth step: the arenas that start facing a wall crash into it"""
    act = np.tile(np.array([[0.5, 0.0]]), (E, 1))
    if t % 4 == 3:
        act[:, 0] = 0.3; act[:, 1] = 0.4
    return act


def _world(gpu, kind, B, step_block, rule):
    """The scene's four arenas in the HIP step and in the oracle, every spawn pose a pose of the scene."""
    occ1, poses = spec.scene(kind)
    E, size = len(poses), occ1.shape[0]
    occ = np.repeat(occ1[None], E, axis=0)
    cfg = gpu.lib.default_config(n_envs=E, map_h=size, map_w=size, max_peds=1, n_scan_stack=1, ped_model=abi.PED_NONE,
                                 auto_reset=1, n_spawn=2, seed=14, step_block=step_block, rect_lds=2, march_rule=rule,
                                 field_format=abi.FIELD_U16T)
    spec.lidar(cfg, B)
    arrays = device_world(gpu, cfg, occ, 0, robot_clearance=0.3)
    assert cfg.closed_maps == 1 and "rect_index" in arrays, "the scene does not take the LDS form of the march (RECT = 2)"
    xy = spec.poses_xy(cfg, poses)
    spawn = np.stack([xy, np.roll(xy, 1, axis=0)], axis=1)                  # [E, 2, 3]: the arena's own pose and its neighbour's
    goal = np.repeat(spec.goals_xy(cfg, poses, size)[:, None], 2, axis=1).copy()   # (out of reach)
    arrays["spawn_pose"] = to_device(gpu, spawn); arrays["spawn_goal"] = to_device(gpu, goal)
    arrays["robot_pose"] = to_device(gpu, spawn[:, 0]); arrays["robot_goal"] = to_device(gpu, goal[:, 0])
    host = host_arrays(arrays, occ)
    tiles = (size + 7) // 8
    pairs = arrays["rect_index"].cpu().numpy().reshape(E, -1)[:, 2048:2048 + tiles * tiles * 2].copy().view(np.uint16).reshape(E, tiles, tiles)
    return cfg, gpu.sim.NavSim(cfg, arrays), ref.RefSim(cfg, host), host["field"], pairs


def _rollout(gpu, kind, B, step_block, rule):
    cfg, g, r, field, pairs = _world(gpu, kind, B, step_block, RULES[rule])
    E = cfg.n_envs
    eq(g.reset_obs().cpu().numpy(), r.reset_obs(), "reset obs")
    scans = [(e,) + tuple(r.a["robot_pose"][e]) for e in range(E)]
    crashes = 0
    for t in range(STEPS):
        act = _actions(E, t)
        go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
        ro, rout = r.step(act)
        for k in rout:
            eq(gout[k].cpu().numpy(), rout[k], "%s at step %d" % (k, t))
        eq(go.cpu().numpy(), ro, "obs at step %d" % t)
        crashes += int((rout["is_crash"] != 0).sum())
        scans += [(e,) + tuple(r.a["robot_pose"][e]) for e in range(E)]
    state_equal(g, r, "at the end")
    assert crashes > 0, "no arena of the oracle's run crashed and restarted"
    park = 16 if step_block == 256 else 0                                   # (kernels_step.hpp step_parks)
    return spec.round_forms(cfg, field, pairs, scans, park, ref.beam_dirs)


CASES = [(B, blk, rule) for B in (65, 127, 1081) for blk in (64, 256, 512) for rule in ("f32", "f32_fma", "f64")]
case_ids = ["B%d-block%d-%s" % c for c in CASES]


@pytest.mark.parametrize("B,step_block,rule", CASES, ids=case_ids)
def test_bare_room_takes_the_short_form(gpu, B, step_block, rule):
    """(a) a 64 x 64 room with nothing in it: away from the room's diagonals a tile has one wall nearest, so most rounds
    leave the second rectangle out."""
    n = _rollout(gpu, "bare_room", B, step_block, rule)
    assert n["one_rect"] > n["two_rect"], "one rectangle is not the common case of this scene: %d of %d rounds" % (n["one_rect"], n["rounds"])


@pytest.mark.parametrize("B,step_block,rule", CASES, ids=case_ids)
def test_box_grid_takes_the_second_rectangle(gpu, B, step_block, rule):
    """(b) boxes of 2-3 cells on a 9-cell pitch around a clearing: tiles with two rectangles everywhere, the long form of
    the rectangle part in most rounds."""
    n = _rollout(gpu, "box_grid", B, step_block, rule)
    assert n["two_rect"] > n["one_rect"], "the second rectangle is not the common case of this scene: %d of %d rounds" % (n["two_rect"], n["rounds"])


@pytest.mark.parametrize("B,step_block,rule", CASES, ids=case_ids)
def test_one_box_mixes_the_forms_inside_a_chunk(gpu, B, step_block, rule):
    """(c) one box in a room: a 64-beam fan straddles the bisector between the box and a wall, so one chunk's march has
    rounds with and rounds without the second rectangle."""
    n = _rollout(gpu, "one_box", B, step_block, rule)
    mixed = [c for c, forms in n["by_chunk"].items() if forms == {False, True}]
    assert mixed, "no chunk of the census changes between the one- and the two-rectangle form"
