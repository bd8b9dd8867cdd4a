"""CPU: the oracle against the independent float64 references of tests/ped_edge_f64.py on the scenes of
tests/ped_edge_scenes.py -- pedestrians in the robot's and the pedestrians' scans at the edges of the device's bearing cull,
and the social force in its degenerate branches.  (tests/test_gpu_ped_edge_scenes.py holds the device to the oracle bit for
bit on the same worlds.)

Lidar.  Every beam of every scene is compared, except silhouette beams (ped_edge_f64.SILHOUETTE: the float64 ray passes
within 1e-5 rad of a vertex's bearing or a disc's tangent); each world asserts that they are at most 0.1 % of its hit beams.
    measured, oracle (float32) against float64, all 22 worlds, 3 observations + the pedestrian scans:
        largest |range difference| over 360 817 hit beams (silhouettes apart)   LIDAR_MEASURED = 1.5672e-5 m
        (the 4000-beam lidar 0.5 mm from a vertex; every other world stays below 3.8e-6 m)
        allowed: twice that                                                      LIDAR_TOL      = 3.1344e-5 m
Social force.  No scene is left out; pose and velocity after one and after three steps.
    measured over both worlds (max_peds 64 and 11) and their perturbed twins, the larger of the two instants:
        positions 8.882e-16 m, velocities 7.772e-16 m/s, headings 4.441e-15 rad SFM_MEASURED
        allowed: four times that                                                 SFM_TOL = 3.553e-15 m, 3.109e-15 m/s, 1.776e-14 rad
    (An ulp of a position near 7 m is 8.9e-16 m: the oracle's own sin / cos / atan2 / exp and libm's agree to the last bits.
    The first comparison read 3 mm per step in the first free cell of a row: DESIGN.md section 5 did not say that the
    obstacle force saturates inside the agent's radius.  It does now, and so does the reference.)
Every test prints its figures (pytest -s)."""
import math

import numpy as np
import pytest

import ped_edge_f64 as f64
import ped_edge_scenes as ps
import ref
from ped_edge_runs import LIDAR_WORLDS, WIDE_WORLDS, lidar_world, run, sfm_world

LIDAR_MEASURED = 1.5672e-5
LIDAR_TOL = 2 * LIDAR_MEASURED
SFM_MEASURED = dict(pos=8.882e-16, vel=7.772e-16, yaw=4.441e-15)
SFM_TOL = {k: 4 * v for k, v in SFM_MEASURED.items()}


# ---- lidar -------------------------------------------------------------------------------------------------------------------------
def _walls(cfg, field, xy, headings, clip):
    """The walls' ranges from the oracle's march: xy [E, 2] lidar positions, headings float32 [E, n] -> metres float32 [E, n]"""
    E, n = headings.shape
    q = np.zeros((E, n, 3), np.float32)
    for e in range(E):
        q[e, :, :2] = f64.origin_cell(cfg, xy[e])
    q[:, :, 2] = headings
    r = ref.cast_static(field, q, float(cfg.map_h * cfg.map_w), cfg.march_rule) * np.float32(cfg.resolution)
    return np.minimum(r, np.float32(clip))


def compare_lidar(name):
    """-> dict(hit=, left_out=, worst=, where=) of one world: the oracle's robot scans of the first observation and of two
    steps, and its pedestrian scans, against the float64 reference."""
    cfg, occ, world, names = lidar_world(name)
    rec, r = run(cfg, world, (0.0, 0.0))
    E, B, S, N, PB = cfg.n_envs, cfg.n_beams, cfg.n_scan_stack, cfg.max_peds, cfg.ped_n_beams
    tot = dict(hit=0, left_out=0, worst=0.0, where=None, crashes=int(sum(x["out"]["is_crash"].sum() for x in rec[1:])))

    def tally(got, want, sil, clip, what):
        hit = (want < clip) | (got < np.float32(clip))
        tot["hit"] += int(hit.sum()); tot["left_out"] += int((hit & sil).sum())
        d = np.abs(got.astype(np.float64) - want)[~sil]
        if d.size and d.max() > tot["worst"]:
            tot["worst"], tot["where"] = float(d.max()), what
    for t, x in enumerate(rec):
        st = x["state"]
        heads = np.stack([f64.beam_headings(cfg.angle_min, cfg.angle_last, B, st["robot_pose"][e, 2]) for e in range(E)])
        wall = _walls(cfg, world["field"], st["robot_pose"][:, :2], heads, cfg.range_max)
        for e in range(E):
            want, sil = f64.robot_scan(cfg, st, e, wall[e])
            tally(x["obs"][e, (S - 1) * B:S * B], want, sil, cfg.range_max, "%s, observation %d, robot" % (names[e], t))
    st = rec[-1]["state"]
    got = r.ped_scans()
    for e in range(E):
        n = min(int(st["n_peds"][e]), N)
        if n == 0:
            continue
        heads = np.stack([f64.beam_headings(cfg.ped_angle_min, cfg.ped_angle_last, PB, st["ped_pose"][e, i, 2]) for i in range(n)])
        cells = np.stack([f64.origin_cell(cfg, st["ped_pose"][e, i, :2]) for i in range(n)])
        q = np.zeros((1, n * PB, 3), np.float32)
        q[0, :, :2] = np.repeat(cells, PB, axis=0); q[0, :, 2] = heads.reshape(-1)
        wall = np.minimum(ref.cast_static(world["field"][e:e + 1], q, float(cfg.map_h * cfg.map_w), cfg.march_rule) * np.float32(cfg.resolution),
                          np.float32(cfg.ped_range_max)).reshape(n, PB)
        for i in range(n):
            want, sil = f64.ped_scan(cfg, st, e, i, wall[i])
            tally(got[e, i], want, sil, cfg.ped_range_max, "%s, pedestrian %d's scan" % (names[e], i))
        assert not got[e, n:].any()
    return tot


@pytest.mark.parametrize("name", list(LIDAR_WORLDS) + list(WIDE_WORLDS))
def test_oracle_scans_against_float64(name):
    tot = compare_lidar(name)
    print("%s: %d hit beams, %d left out as silhouettes, worst difference %.3e m at %s; %d crashes" % (
        name, tot["hit"], tot["left_out"], tot["worst"], tot["where"], tot["crashes"]))
    assert tot["hit"] > 0 and tot["crashes"] > 0, "the near scenes crash"
    assert tot["left_out"] <= 0.001 * tot["hit"], "more than 0.1 % of the hit beams are silhouette beams"
    assert tot["worst"] <= LIDAR_TOL, tot


def test_lidar_scenes_are_what_they_say():
    """The placements, from the geometry alone: distances to the nearest side / vertex / leg of the near scenes, the nearest
    point of the far scenes, the angles of the sides seen under almost pi."""
    scenes = {s["name"]: s for s in ps.lidar_scenes(ps.LIDARS["reference_1081"])}
    L = np.array(ps.CENTRE)

    def seg_dist(p, q):
        d = q - p
        u = np.clip(np.dot(L - p, d) / np.dot(d, d), 0, 1)
        return float(np.linalg.norm(p + u * d - L))

    def rect_of(sc, k=0):
        v = f64.rectangle(sc["peds"][k][0]).astype(np.float64)
        return [(v[i], v[(i + 1) % 4]) for i in range(4)]
    for name, want in (("near: 0.5 mm from a side", 0.0005), ("near: 2 mm from a side", 0.002),
                       ("near: 0.5 mm from a vertex", 0.0005), ("near: 2 mm from a vertex", 0.002)):
        got = min(seg_dist(p, q) for p, q in rect_of(scenes[name]))
        assert abs(got - want) < 2e-6, (name, got)
        if "vertex" in name:
            assert abs(min(np.linalg.norm(p - L) for p, _ in rect_of(scenes[name])) - want) < 2e-6
    for name, k in (("near: inside a leg disc", 0.0), ("near: 1.04 radii from a leg", 1.04), ("near: 1.06 radii from a leg", 1.06)):
        d = min(np.linalg.norm(c.astype(np.float64) - L) for c in f64.leg_centres(scenes[name]["peds"][0][0], (0, 0, 0)))
        assert (d < 0.03) if k == 0.0 else abs(d / 0.03 - k) < 2e-3, (name, d)
    for ang in (2.9, 3.05, 3.13):
        best = max(abs(f64._wrap(math.atan2(*(q - L)[::-1]) - math.atan2(*(p - L)[::-1]))) for p, q in rect_of(scenes["near: a side under %.2f rad" % ang]))
        assert abs(best - ang) < 0.02 and (best > 3.0) == (ang > 3.0), (ang, best)
    for name, D in (("range_max - 1 cm", ps.RANGE_MAX - 0.01), ("range_max", ps.RANGE_MAX), ("rcull - 1 mm", ps.RCULL - 0.001),
                    ("rcull + 1 mm", ps.RCULL + 0.001), ("rcull + 0.5 m", ps.RCULL + 0.5)):
        sc = scenes["far: a side and a leg at " + name]
        assert abs(min(seg_dist(p, q) for p, q in rect_of(sc, 0)) - D) < 5e-6, name
        leg = min(np.linalg.norm(c.astype(np.float64) - L) for c in f64.leg_centres(sc["peds"][1][0], (0, 0, 0))) - 0.03
        assert abs(leg - D) < 5e-6, (name, leg)
    crowd = scenes["crowd: two rings of 32"]
    assert len(crowd["peds"]) == 64 and sum(l for _, l in crowd["peds"]) == 32


# ---- social force ------------------------------------------------------------------------------------------------------------------
def compare_sfm(max_peds, nudge):
    """-> (worst differences after one and three steps, the reference's report of the first step per scene, the smallest
    non-zero |theta| of each step)"""
    cfg, occ, world, scenes = sfm_world(max_peds, nudge)
    rec, r = run(cfg, world, ps.SFM_ACTION, steps=3)
    E, N = cfg.n_envs, cfg.max_peds
    worst = {1: dict(pos=0.0, vel=0.0, yaw=0.0), 3: dict(pos=0.0, vel=0.0, yaw=0.0)}
    reports, min_theta = [], {1: math.inf, 2: math.inf, 3: math.inf}
    for e in range(E):
        n = min(int(world["n_peds"][e]), N)
        pos, vel, yaw = world["ped_pose"][e, :, :2].copy(), world["ped_vel"][e].copy(), world["ped_pose"][e, :, 2].copy()
        for t in (1, 2, 3):
            before = rec[t - 1]["state"]            # the robot as the oracle's step finds it: its pose and its previous action
            p, v, y, rep, mt = f64.sfm_step(cfg, world["field"][e], before["robot_pose"][e], before["prev_action"][e, 0], pos, vel, yaw,
                                            world["ped_v_pref"][e], world["ped_waypoints"][e, :, 0], n)
            pos[:n], vel[:n], yaw[:n] = p, v, y
            min_theta[t] = min(min_theta[t], mt)
            if t == 1:
                reports.append(rep)
            if t in worst and n:
                after = rec[t]["state"]
                w = worst[t]
                w["pos"] = max(w["pos"], float(np.abs(after["ped_pose"][e, :n, :2] - pos[:n]).max()))
                w["vel"] = max(w["vel"], float(np.abs(after["ped_vel"][e, :n] - vel[:n]).max()))
                w["yaw"] = max(w["yaw"], float(np.abs(f64._wrap(after["ped_pose"][e, :n, 2] - yaw[:n])).max()))
        after = rec[3]["state"]                     # rows beyond the arena's pedestrians are not touched
        assert np.array_equal(after["ped_pose"][e, n:], world["ped_pose"][e, n:]) and np.array_equal(after["ped_vel"][e, n:], world["ped_vel"][e, n:])
    return worst, reports, min_theta


@pytest.mark.parametrize("max_peds", [64, 11])
def test_oracle_social_force_against_float64(max_peds):
    scenes = ps.sfm_scenes(max_peds)
    pairs = {"coincident", "il0", "theta0"}
    for nudge in (False, True):
        worst, reports, min_theta = compare_sfm(max_peds, nudge)
        print("max_peds %d%s: worst after 1 step %s, after 3 steps %s; smallest non-zero |theta| per step %s" % (
            max_peds, ", perturbed twin" if nudge else "", worst[1], worst[3], min_theta))
        for t in (1, 3):
            for k, bound in SFM_TOL.items():
                assert worst[t][k] <= bound, (t, k, worst[t][k], bound)
        # as placed, no pair is near the sgn(theta) discontinuity unless its scene says theta == 0; in the second and third
        # step the geometry is the model's own (64 pedestrians come as near as 6e-5 rad): 1e-5 rad is ten orders above the
        # rounding of theta, so its sign is the same in any arithmetic.  (The perturbed twins sit 1e-6 m beside theta == 0.)
        assert min_theta[1] > (1e-8 if nudge else 1e-3) and min(min_theta[2], min_theta[3]) > 1e-5, min_theta
        for sc, rep in zip(scenes, reports):
            got = set(rep)
            want = set(sc["expect"])
            if not nudge:
                assert want <= got, (sc["name"], sorted(want - got, key=str))
                # nothing degenerate between two agents where the scene does not say so
                assert {x for x in got if x[0] in pairs} == {x for x in want if x[0] in pairs}, (sc["name"], sorted(got, key=str))
            elif sc["nudge"] is not None:
                k = sc["nudge"]
                moved = {x for x in want if x[1] == k or x[2] == k}
                assert moved and not (moved & got), (sc["name"], sorted(moved & got, key=str))
                assert (want - moved) <= got
    assert sum(len(s["expect"]) for s in scenes) >= 25
