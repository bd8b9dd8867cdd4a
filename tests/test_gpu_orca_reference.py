"""GPU: crowd_orca_kernel (navsim_crowd_orca) and ped_orca_kernel (navsim_ped_orca) against the independent float64 solver of
tests/orca_f64.py.  Every test asserts on the device's output (a) equality bit for bit with the CPU oracle, resp. with
tests/ped_orca_spec.py, (b) the comparison with the float64 reference under the bounds of tests/orca_scenes.py (taken from
the CPU oracle's error, tests/test_orca_reference.py), (c) a census of the branches its inputs reach.  The inputs are the
ones tests/test_orca_reference.py runs through the oracle, so a failure here is the kernel's."""
import numpy as np
import pytest

import orca_f64 as f64
import orca_scenes as sc
import ped_orca_spec as spec
import ref
from gpu_support import gpu, eq, orca_pair, small_orca_config, to_device, ORCA_SENTINEL as SENTINEL  # noqa: F401  (gpu: the module's fixture)

pytestmark = pytest.mark.gpu


# ---- crowd_orca_kernel ------------------------------------------------------------------------------------------------------
def _crowd(gpu, p, ag, pv, na=None, verts=None, what="ORCA velocity"):
    """navsim_crowd_orca on the device, equal to the oracle bit for bit -> velocities"""
    gv, _ = gpu.sim.crowd_orca(p, to_device(gpu, ag), to_device(gpu, pv), None if verts is None else to_device(gpu, verts),
                               None if na is None else to_device(gpu, na))
    gv = gv.cpu().numpy()
    eq(gv, ref.crowd_orca(p, ag, pv, verts, na)[0], what)
    return gv


@pytest.mark.parametrize("name", ["worlds", "ragged"])
def test_crowd_kernel_vs_float64_reference(gpu, name):
    """worlds: 500 queries of each of the four worlds.  ragged: 2 x 1000 queries with 1 .. 12 agents, a list of 3 entries and
    a range of 2.5 m."""
    sc.crowd_check(name, lambda p, ag, pv, na: _crowd(gpu, p, ag, pv, na, what="ORCA velocity (%s)" % name))


@pytest.mark.parametrize("n", [1, 5])
def test_crowd_kernel_obstacles_swept_disc_keeps_clear(gpu, n):
    """The two boxes with 1 and with 5 agents, 1 000 queries each: the disc swept along the device's velocity for
    time_horizon_obst keeps clear of both boxes to CLEAR_BOUND, and the boxes and agents do bend the answer."""
    ag, pv = sc.obstacle_scene(n, 200 + n, 1000)
    v = _crowd(gpu, sc.ORCA_P, ag, pv, verts=sc.BOXES[None], what="ORCA velocity around the boxes")
    a32 = ag.astype(np.float32).astype(np.float64)
    clear = f64.swept_clearance(a32[:, 0, :2], v, sc.RADIUS, sc.ORCA_P["time_horizon_obst"], sc.BOXES)
    differs = np.sqrt(((v - sc.clipped(pv, ag[:, 0, 5])) ** 2).sum(1)) > 1e-3
    print("device, obstacles, %d agent(s): the swept disc enters a box by %.3g m at most; the answer differs from the clipped "
          "preferred velocity in %.1f %% of %d queries" % (n, max(-clear.min(), 0.0), 100 * differs.mean(), len(v)))
    assert np.isfinite(v).all()
    assert -clear.min() <= sc.CLEAR_BOUND
    assert differs.mean() >= 0.25


def test_crowd_kernel_degenerate_inputs(gpu):
    """The degenerate table: decided by comparisons with NaN, which the device must decide like the oracle.  And two
    neighbours exactly equally far with room for one: the first of the list stays."""
    ag, pv = sc.degenerate_batch()
    v = _crowd(gpu, sc.ORCA_P, ag, pv, what="degenerate table")
    assert v.tobytes() == sc.DEGENERATE_ANSWERS.tobytes(), v
    sc.tie_check(lambda p, ag, pv, na: _crowd(gpu, p, ag, pv, what="equally distant neighbours"))


# ---- ped_orca_kernel --------------------------------------------------------------------------------------------------------
KEYS = ("ped_pose", "ped_vel", "ped_v_pref", "ped_waypoints", "ped_n_waypoints", "ped_wp_head", "robot_pose", "prev_action",
        "n_peds")


class _Arenas:
    """One simulator and one oracle of E arenas x N pedestrians whose state every call overwrites with a scene."""

    def __init__(self, gpu, E, N):
        self.gpu, self.cfg = gpu, small_orca_config(gpu, E, N)
        self.g, self.r = orca_pair(gpu, self.cfg, N, moving=False)

    def answer(self, s, kw):
        gpu, g, r = self.gpu, self.g, self.r
        a = sc.ped_state(s, self.cfg.max_waypoints)
        for k in KEYS:
            r.a[k][...] = a[k]
            g.t[k].copy_(to_device(gpu, r.a[k]))
        g.t["ped_cmd"].fill_(SENTINEL)
        r.a["ped_cmd"][...] = SENTINEL
        p = spec.params(self.cfg, **kw)
        want, head, _ = spec.ped_orca(self.cfg, r.a, p)
        got = g.ped_orca({k: p[k] for k in spec.KEYS}).cpu().numpy()
        what = "E %d N %d %s" % (self.cfg.n_envs, self.cfg.max_peds, kw)
        eq(got, want, "ped_cmd (%s)" % what)                          # live rows, and dead rows still holding the sentinel
        eq(g.numpy_state("ped_wp_head")["ped_wp_head"], head, "ped_wp_head (%s)" % what)
        live = np.arange(self.cfg.max_peds)[None, :] < r.a["n_peds"][:, None]
        assert (got[~live] == SENTINEL).all() and np.isfinite(got[live]).all()
        return got, self.cfg.time_step, p


@pytest.mark.parametrize("name", list(sc.PED_CASES))
def test_ped_kernel_vs_float64_reference(gpu, name):
    """The shapes at which the kernel packs its wavefronts differently (45 x 8: 8 arenas per wavefront, the last one partial,
    ragged n_peds with 0 and 1; 11 x 12: 5 per wavefront, 4 idle lanes; 7 x 20; 5 x 33 and 4 x 63: one arena per wavefront),
    arenas from 2 m to 11 m wide; on 45 x 8 and 11 x 12 also max_neighbors 0, 1, 3, neighbor_dist 1.5 and the robot unseen,
    so that lanes of one wavefront hold empty, partial and truncated lists.  The velocity is recovered from ped_cmd as
    speed (cos, sin)(theta + omega dt).  The census counts, besides classes, optimum locations and list events, infeasible
    programs and displaced list entries on lanes behind a wavefront's first arena and in the last, partial wavefront."""
    E, N, _ = sc.ped_calls(name)
    sc.ped_check(name, _Arenas(gpu, E, N).answer)


def test_ped_kernel_lists_of_63(gpu):
    """max_neighbors 63 on 4 x 63: bit for bit on every lane, the float64 comparison on a sample of 200 queries."""
    sc.ped_full_lists(_Arenas(gpu, 4, 63).answer)


def test_ped_kernel_degenerate_arenas(gpu):
    """Two pedestrians at one pose with zero velocity, at one pose with different velocities, a pedestrian exactly on the
    robot, v_pref 0: ped_cmd equals the specification's (and is finite)."""
    _Arenas(gpu, 4, 3).answer(sc.ped_degenerate(), {})
