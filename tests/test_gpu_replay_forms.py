"""GPU: every (field format, march rule, rect records) form of the four kernels that replay the step through the shared pieces of
csrc/kernels_replay.hpp -- navsim_lookahead, navsim_lookahead_obs, navsim_rollout, navsim_rollout_obs -- against navsim_step
itself, bit for bit, on one small world.  The families' own tests reach a float32 world and a packed world with rect records;
here the template arguments that travel through the shared functions are all exercised, so a dropped or swapped one shows.

The world is the smallest that can still go wrong: E = 2; B = 65 beams (one full 64-beam chunk plus a remainder of one, and a
256-stride pass with idle threads); 3 pedestrian slots with 2 present under the social force, slot 0 with legs and slot 1 without
(both kinds of primitive, and a ballot with a gap); a scan stack of 2; K = 2 (both parity buffers of the lookahead pair); H = 2
(one carry of the rollout pair); scan noise on for the two observation entries.  navsim_scan_labels on the same state shows
that a pedestrian's body and a pedestrian's leg are both seen, so no comparison passes for want of pedestrians."""
import numpy as np
import pytest

import lookahead_call as lc
import lookahead_obs_call as loc
import rollout_call as rc
import rollout_obs_call as roc
import scan_labels_call
from gpu_support import eq, gpu, random_actions, same_bits, to_device   # noqa: F401
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

E, B, N, S, K, H = 2, 65, 3, 2, 2, 2
SIZE = 120                                                          # cells: a 6 m room
ROBOT = (3.0, 3.0)
BODY_DIST = 1.6                                                     # outside the Keti crash thresholds (0.60 - 0.86 m)
LEG_BEAM, LEG_DIST = 16, 1.0                                        # the beam at -91 degrees, to the robot's right
RULES = (abi.MARCH_F64, abi.MARCH_F32, abi.MARCH_F32_FMA)          # (tests/test_gpu_scan_labels.py's)
FORMS = [(abi.FIELD_F32, rule, False) for rule in RULES] + [(abi.FIELD_U16T, rule, rects) for rule in RULES for rects in (False, True)]
IDS = ["%s-rule%d-%s" % ("f32" if f == abi.FIELD_F32 else "u16t", r, "rects" if x else "norects") for f, r, x in FORMS]

ACTIONS = np.broadcast_to(np.array([(0.5, 0.0), (0.2, 0.5)]), (E, K, 2)).copy()
SEQUENCES = np.broadcast_to(np.array([[(0.5, 0.0), (0.4, -0.4)], [(0.1, 0.6), (0.3, 0.2)]]), (E, K, H, 2)).copy()


def world(gpu, fmt, rule, rects, noise):
    """The world of the module docstring in a NavSim, warmed by five steps (prev_action, waypoint heads, leg odometry and the scan
    stack are live), then the robot and the two pedestrians put where the scan sees both: one leg of pedestrian 0 centred on
    beam LEG_BEAM at LEG_DIST (its angular width, 3.4 degrees, is below the beam spacing of 5.5: it has to sit on a beam),
    pedestrian 1's body BODY_DIST away at 120 degrees.  Arena 1 starts from an empty scan history."""
    cfg = gpu.lib.default_config(n_envs=E, map_h=SIZE, map_w=SIZE, max_peds=N, ped_model=abi.PED_SFM, n_scan_stack=S, seed=13,
                                 field_format=fmt, march_rule=rule, lidar_legs=1, n_spawn=4)
    gpu.world.lidar_full_circle(cfg, B)
    occ = lc.room(E, SIZE, SIZE, 3, (20, 26, 20, 30))
    g = (loc if noise else lc).sim_world(gpu, cfg, occ, 2, rect_table=rects)
    assert ("rect_table" in g.t) == bool(rects), sorted(g.t)
    rng = np.random.default_rng(3)
    for _ in range(5):
        g.step(to_device(gpu, random_actions(rng, E)))
    for e in range(E):
        lc.place(g, g.cfg, e, ROBOT[0], ROBOT[1], goal=(2.0, 1.0))
    g.t["n_peds"][:] = 2
    g.t["ped_has_legs"][:, 0] = 1
    g.t["ped_has_legs"][:, 1] = 0
    g.t["ped_dist"][:, 0] = 0.0                                     # legs at (0.3, 0.2) and (-0.3, -0.2) of a pedestrian heading 0
    th = -np.pi + LEG_BEAM * 2 * np.pi / B
    leg = np.array([ROBOT[0] + LEG_DIST * np.cos(th), ROBOT[1] + LEG_DIST * np.sin(th)])
    g.t["ped_pose"][:, 0] = to_device(gpu, np.array([leg[0] - 0.3, leg[1] - 0.2, 0.0]))
    g.t["ped_pose"][:, 1] = to_device(gpu, np.array([ROBOT[0] + BODY_DIST * np.cos(2.1), ROBOT[1] + BODY_DIST * np.sin(2.1), 0.5]))
    g.t["n_hist"][1] = 0
    return g


def capped_entries(gpu, fmt, rule, rects):
    """navsim_lookahead and navsim_rollout under the default cap R, against the step without scan noise."""
    g = world(gpu, fmt, rule, rects, noise=False)
    cfg = g.cfg
    R = gpu.sim.lookahead_defaults(cfg, float(g.t["scan_discomfort"].max().item()))["range"]
    assert R < cfg.range_max
    labels = scan_labels_call.call(gpu, cfg, g.st)["label"]
    for e in range(E):
        assert abi.BEAM_PED_BODY in labels[e] and abi.BEAM_PED_LEG in labels[e], "arena %d sees %s" % (e, sorted(set(labels[e].tolist())))
    thr, dthr = g.t["scan_threshold"].cpu().numpy(), g.t["scan_discomfort"].cpu().numpy()
    saved = lc.save_state(g)

    look = lc.call(gpu, cfg, g.st, ACTIONS, R)                                       # navsim_lookahead: K steps from the state
    step = rc.steps_of(gpu, g, saved, ACTIONS[:, :, None, :], labels=True)
    for name in lc.STEP_KEYS:
        same_bits(look[name], step[name][:, :, 0], "lookahead: %s" % name)
    assert (look["status"] == 1).all()
    ok = step["is_crash"][:, :, 0] == 0
    assert ok.any()
    same_bits(look["pose"][ok], step["pose"][:, :, 0][ok], "lookahead: pose")
    ranges = step["range"][:, :, 0]
    same_bits(look["margin"][ok], (np.minimum(ranges, np.float32(R)) - thr).min(axis=2)[ok], "lookahead: margin")
    eq(look["discomfort"][ok], (ranges < dthr).any(axis=2)[ok].astype(np.uint8), "lookahead: discomfort")
    assert ((look["margin"] < 0) == (look["is_crash"] != 0)).all()

    roll = rc.call(gpu, cfg, g.st, SEQUENCES, R, gamma=0.9)                          # navsim_rollout: K sequences of H steps
    step = rc.steps_of(gpu, g, saved, SEQUENCES, labels=True)
    assert (roll["exact_steps"] == H).all() and (roll["length"] == H).any(), (roll["exact_steps"], roll["length"])
    rows = rc.same_as_steps(roll, step, "rollout", gamma=0.9, thr=thr, dthr=dthr, R=R)
    assert rows == int(roll["length"].sum())
    for k, v in lc.save_state(g).items():                                            # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the calls" % k)


def observation_entries(gpu, fmt, rule, rects):
    """navsim_lookahead_obs and navsim_rollout_obs against the step with its scan noise."""
    g = world(gpu, fmt, rule, rects, noise=True)
    cfg = g.cfg
    assert cfg.add_scan_noise and (g.t["scan_noise_std"].cpu().numpy() > 0).all()
    thr = g.t["scan_threshold"].cpu().numpy()
    saved, obs0 = lc.save_state(g), g.obs.clone()

    look = loc.call(gpu, cfg, g.st, ACTIONS, obs0)                                   # navsim_lookahead_obs
    step = loc.steps_of(gpu, g, saved, obs0, ACTIONS)
    for name in loc.STEP_KEYS:
        same_bits(look[name], step[name], "lookahead_obs: %s" % name)
    assert not look["truncated"].any() and (look["status"] == 1).all()
    same_bits(look["obs"], step["obs"], "lookahead_obs: row")
    same_bits(look["goals"], step["goals"], "lookahead_obs: goals")
    same_bits(look["scan"], look["obs"][:, :, (S - 1) * B:S * B], "lookahead_obs: scan against the row's newest slot")
    same_bits(look["tail"], look["obs"][:, :, S * B:], "lookahead_obs: tail against the row's")
    ok = step["is_crash"] == 0
    assert ok.any()
    same_bits(look["margin"][ok], (step["obs"][:, :, (S - 1) * B:S * B] - thr).min(axis=2)[ok], "lookahead_obs: margin")
    clean = lc.call(gpu, cfg, g.st, ACTIONS, cfg.range_max)
    same_bits(look["pose"], clean["pose"], "lookahead_obs: pose against navsim_lookahead's")
    assert not np.array_equal(look["margin"], clean["margin"]), "the noise changed nothing"

    roll = roc.call(gpu, cfg, g.st, SEQUENCES, obs0, gamma=0.9)                      # navsim_rollout_obs
    step = roc.steps_of(gpu, g, saved, obs0, SEQUENCES)
    assert (roll["exact_steps"] == H).all() and (roll["length"] == H).any(), (roll["exact_steps"], roll["length"])
    rows = roc.same_as_steps(roll, step, "rollout_obs", gamma=0.9)
    assert rows == int(roll["length"].sum())
    for k, v in lc.save_state(g).items():                                            # the state is only read
        same_bits(v.cpu().numpy(), saved[k].cpu().numpy(), "state %s after the calls" % k)
    same_bits(g.obs.cpu().numpy(), obs0.cpu().numpy(), "the observation after the calls")


@pytest.mark.parametrize("fmt,rule,rects", FORMS, ids=IDS)
def test_all_four_entries_equal_the_step(gpu, fmt, rule, rects):
    capped_entries(gpu, fmt, rule, rects)
    observation_entries(gpu, fmt, rule, rects)
