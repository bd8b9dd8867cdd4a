"""What the step kernel does with a finished ray (kernels_step.hpp: the `finish` of scan_beams_pred, finish_beams).

Every lane of a wavefront runs that code outside divergent control flow; a lane mask decides which lanes may vote for
crash / discomfort and store.  The directed tests put the only beam that can vote at the places where a mask that DROPS
lanes goes wrong (the first and last lane of a chunk, the partial last chunk): done / is_crash / reward then differ from the
oracle's.  They cannot see a lane that votes without the right to: a lane past the last beam runs along on beam B - 1 and
holds that beam's value, and a ray that is still marching carries the miss range, which clips to range_max and is below no
threshold -- that a wrong mask of this kind changes nothing is a property of the kernel, by construction.  The rollouts
compare every output and state array with the oracle bit for bit; the noise test compares two launch shapes, because
which wavefront finishes a ray must not matter."""
import numpy as np
import pytest

import ref
from gpu_support import gpu, device_world, eq, random_actions, sim_and_oracle, state_equal  # noqa: F401  (gpu: the module's fixture)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu



def _lidar(gpu, cfg, B):
    if B == 1081:
        gpu.world.lidar_1081(cfg)
    else:
        gpu.world.lidar_full_circle(cfg, B)


def _step_both(gpu, g, r, act, what):
    go, gout = g.step(gpu.torch.from_numpy(act).to(gpu.dev))
    ro, rout = r.step(act)
    for k in rout:
        eq(gout[k].cpu().numpy(), rout[k], "%s %s" % (k, what))
    eq(go.cpu().numpy(), ro, "obs %s" % what)
    return ro, rout


@pytest.fixture(scope="module")
def directed_maps(gpu):
    return gpu.world.make_maps(4, 120, 31)


def _flag_cases():
    for B in (65, 127, 1081):
        for kstar in sorted({0, 63, 64, B - 1}):
            yield B, kstar


@pytest.mark.parametrize("step_block", [64, 256])
@pytest.mark.parametrize("which", ["crash", "discomfort"])
@pytest.mark.parametrize("B,kstar", list(_flag_cases()))
def test_one_beam_decides_the_flag(gpu, directed_maps, B, kstar, which, step_block):
    """4 arenas, 120 x 120 outdoor maps, one step.  The crash (or the discomfort) threshold is 0 at every beam but beam
    k*, where it is 100 m: a range is never below 0 and always below 100 m, so the flag fires iff beam k*'s lane votes.
    k* = 0, 63, 64 and B - 1 are the first and last lane of the first chunk, the first lane of the second and the last
    valid lane of the scan (B = 65: the only valid lane of its chunk).  64 threads per arena march every chunk to the
    end, 256 park rays and finish them in a second place."""
    E = 4
    cfg = gpu.lib.default_config(n_envs=E, map_h=120, map_w=120, max_peds=1, n_scan_stack=1, ped_model=abi.PED_NONE,
                                 auto_reset=0, n_spawn=4, seed=31, step_block=step_block)
    _lidar(gpu, cfg, B)
    flagged = np.zeros(B, np.float32); flagged[kstar] = 100.0
    zero = np.zeros(B, np.float32)
    thr, dthr = (flagged, zero) if which == "crash" else (zero, flagged)
    g, r, host = sim_and_oracle(gpu, cfg, directed_maps, 0, thr=thr, dthr=dthr)
    act = np.tile(np.array([[0.2, 0.1]]), (E, 1))
    ro, rout = _step_both(gpu, g, r, act, "with beam %d of %d flagged" % (kstar, B))
    # the oracle itself must have seen the flag: against its own run with both arrays zero
    r0 = ref.RefSim(cfg, dict(host, scan_threshold=zero, scan_discomfort=zero))
    r0.reset_obs()
    _, rout0 = r0.step(act)
    assert not rout0["is_crash"].any()
    if which == "crash":
        assert rout["is_crash"].all() and rout["done"].all()
    else:
        assert not rout["is_crash"].any()
        assert (rout["reward"] != rout0["reward"]).all(), "the discomfort penalty is missing from the oracle's reward"


ROLLOUT_SEED, ROLLOUT_CLEARANCE = 11, 0.5      # chosen with the oracle on the CPU: every world below crashes, comes close without a
                                               # crash, restarts and has quiet steps within 30 steps (asserted on the oracle's outputs)


@pytest.fixture(scope="module")
def rollout_maps(gpu):
    return gpu.world.make_maps(8, 120, ROLLOUT_SEED)


def _rollout(gpu, occ, S, B, step_block, ped_model, n_peds, steps=30):
    E = 8
    cfg = gpu.lib.default_config(n_envs=E, map_h=120, map_w=120, max_peds=4 if n_peds else 1, n_scan_stack=S, ped_model=ped_model,
                                 auto_reset=1, n_spawn=8, seed=ROLLOUT_SEED, step_block=step_block)
    _lidar(gpu, cfg, B)
    g, r, _ = sim_and_oracle(gpu, cfg, occ, n_peds, robot_clearance=ROLLOUT_CLEARANCE)
    dthr = r.a["scan_discomfort"]
    rng = np.random.default_rng(5)
    n = dict(crash=0, discomfort=0, restart=0, neither=0)
    for t in range(steps):
        ro, rout = _step_both(gpu, g, r, random_actions(rng, E, t), "at step %d" % t)
        done = rout["done"] != 0
        # an arena that did not finish keeps its scan as the newest row: below the discomfort threshold somewhere, and no crash
        close = (ro[:, (S - 1) * B:S * B] < dthr[None, :]).any(axis=1) & ~done
        n["crash"] += int((rout["is_crash"] != 0).sum()); n["restart"] += int(done.sum())
        n["discomfort"] += int(close.sum()); n["neither"] += int((~close & ~done).sum())
    state_equal(g, r, "at the end")
    assert min(n.values()) > 0, "the oracle's run lacks one of crash / discomfort alone / restart / neither: %s" % n


@pytest.mark.parametrize("step_block", [64, 256])
@pytest.mark.parametrize("B", [127, 1081])
@pytest.mark.parametrize("S", [1, 3])
def test_rollout_without_pedestrians(gpu, rollout_maps, S, B, step_block):
    """8 arenas x 30 steps with restarts in place, stacks of 1 and 3 scans (the stack fill of a fresh episode), a partial
    last chunk, rays finished at the end of their chunk (64 threads) and after parking (256): all equal to the oracle."""
    _rollout(gpu, rollout_maps, S, B, step_block, abi.PED_NONE, 0)


def test_rollout_with_pedestrians(gpu, rollout_maps):
    """The pedestrian variants finish their beams in the dense pass behind the merge (finish_beams)."""
    _rollout(gpu, rollout_maps, 3, 1081, 256, abi.PED_SFM, 4)


def test_noise_does_not_depend_on_the_launch_shape(gpu, rollout_maps):
    """Noise on (sigma = 0.02 m): 64 and 256 threads per arena give identical observations and outputs over 10 steps."""
    E, S, B = 8, 3, 1081
    runs = []
    for step_block, noise, steps in ((64, 1, 10), (256, 1, 10), (64, 0, 0)):      # the third: the noise-free first observation
        cfg = gpu.lib.default_config(n_envs=E, map_h=120, map_w=120, max_peds=1, n_scan_stack=S, ped_model=abi.PED_NONE,
                                     auto_reset=1, n_spawn=8, seed=ROLLOUT_SEED, step_block=step_block, add_scan_noise=noise)
        _lidar(gpu, cfg, B)
        g = gpu.sim.NavSim(cfg, device_world(gpu, cfg, rollout_maps, 0, robot_clearance=ROLLOUT_CLEARANCE, noise_std_range=(0.02, 0.02)))
        out = [g.reset_obs().cpu().numpy().copy()]
        rng = np.random.default_rng(5)
        for t in range(steps):
            go, gout = g.step(gpu.torch.from_numpy(random_actions(rng, E, t)).to(gpu.dev))
            out.append(go.cpu().numpy().copy())
            out.append(np.concatenate([gout[k].cpu().numpy().astype(np.float64).reshape(E, -1) for k in sorted(gout)], axis=1))
        runs.append(out)
    assert (runs[0][0] != runs[2][0]).any(), "the noise is not on"
    for i, (a, b) in enumerate(zip(runs[0], runs[1])):
        eq(a, b, "array %d of the run (64 vs 256 threads per arena)" % i)
