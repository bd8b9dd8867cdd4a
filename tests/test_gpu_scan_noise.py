"""GPU: every noisy range of the fused step against the float64 model of its draw (tests/scan_noise_f64.py).

Per step the state and the observation are read back BEFORE the launch; gpu_support.NoisyStep steps the oracle from that
snapshot for the clean scans and the noise-free outputs, draws the noise from the model and lets the model's noisy first
scan alone decide crash / restart / truncation.  Then, per arena:
  * the returned row (obs; final_obs where the arena restarted inside the step) is the model's within TOL = 1e-5 m, with
    the first scan's key, or the re-scan's after a crash; beams whose clean value is range_max equal range_max bit for bit;
    arenas with std 0 equal the clean row bit for bit;
  * a restarted or reset arena's row is the new episode's first observation in every slot;
  * history slots are the previous observation's slots bit for bit, filled slots the newest slot bit for bit;
  * is_crash, is_success, done, truncated are the model's; without a crash no beam of the returned row is below its crash
    threshold; the reward is reward_scalar's sum in float64 with the discomfort term taken from the DEVICE's returned row
    (atol 1e-9); distance, goals, the rows' tails and every state array equal the oracle's bit for bit.
An arena-step whose noisy first scan comes within TOL of a crash threshold is undecidable: it is skipped and counted, and a
case may have at most 1 % of them (tests/test_scan_noise.py measures the worlds' share on the CPU: none).

Cases (gpu_support.NOISE_CASES; 24 arenas, 30 steps, random_actions with its crash bursts, range_max 3 m):
  mode                    S  B                 pedestrians                      step_block  extras
  NONE                    1  77 (fan)          none                             64          FIELD_F32
  SAME_STEP + final_obs   3  200 full circle   SFM, 5 of 6, some legs           256         env_index_base 1000, seed 2^40 + 99, packed field + rect index
  NEXT_STEP               2  1081              EXTERNAL                         0           packed field + rect index
  SAME_STEP + final_obs   2  77 (fan)          none                             256         max_episode_steps 7

The last test evaluates nv::gauss_noise alone (debug function 17) at the corners of its two 24-bit fields."""
import math

import numpy as np
import pytest

import scan_noise_f64 as model
from gpu_support import (NOISE_CASES, TOL, NoisyStep, device_map_arrays, gpu, noise_coverage, noise_coverage_met,  # noqa: F401  (gpu: the module's fixture)
                         noise_inputs, noise_world, same_bits, to_device, to_numpy)
from nav_gym_amd import abi

pytestmark = pytest.mark.gpu

G_TOL = TOL / 0.05              # the range bar over the reference's largest std


class _Worst(object):
    """the largest deviation of a noisy range from the model, in metres and as |dg| = |d range| / std"""

    def __init__(self):
        self.m, self.g, self.n = 0.0, 0.0, 0

    def add(self, d, std):
        if d.size:
            self.m, self.g, self.n = max(self.m, float(d.max())), max(self.g, float(d.max()) / float(std)), self.n + d.size


def _scan_is(dev, want, clean, old, prev, std, rmax, worst, what):
    """dev float32 [S,B] against want float64 [S,B]: history slots (old[j]) are prev's slot j + 1 bit for bit, the others the
    model's row -- range_max beams and a std of 0 bit for bit, noisy beams within TOL -- and equal to the newest slot bit for bit"""
    S = dev.shape[0]
    far = clean == np.float32(rmax)
    for j in range(S):
        if old[j]:
            same_bits(dev[j], prev[j + 1], "%s: history slot %d" % (what, j))
            continue
        same_bits(dev[j], dev[S - 1], "%s: filled slot %d against the newest" % (what, j))
        same_bits(dev[j][far], clean[far], "%s: beams at range_max, slot %d" % (what, j))
        if std == 0.0:
            same_bits(dev[j], clean, "%s: std 0, slot %d" % (what, j))
            continue
        d = np.abs(dev[j].astype(np.float64) - want[j])[~far]
        worst.add(d, std)
        assert (d <= TOL).all(), "%s, slot %d: %d noisy ranges off by more than %g m, worst %.3e m at noisy beam %d (std %g)" % (
            what, j, int((d > TOL).sum()), TOL, d.max(), int(np.argmax(d)), std)


def _device(gpu, name):
    cfg, occ, host = noise_world(gpu.lib.default_config, name)
    arrays = device_map_arrays(gpu, cfg, occ, {k: to_device(gpu, v) for k, v in host.items() if k != "field"}, rects=True)
    final = cfg.auto_reset == abi.AUTORESET_SAME_STEP
    return cfg, host, gpu.sim.NavSim(cfg, arrays, final_obs=final), final


@pytest.mark.parametrize("name", sorted(NOISE_CASES))
def test_every_noisy_range_is_the_models(gpu, name):
    cfg, host, g, final = _device(gpu, name)
    E, S, B, T = cfg.n_envs, cfg.n_scan_stack, cfg.n_beams, cfg.max_episode_steps
    rmax = cfg.range_max
    ns = NoisyStep(cfg, host)
    names = [k for k in ns.keys if k in g.t] + (["ped_due"] if g.due is not None else [])
    thr = ns.thr
    worst = _Worst()
    scan_of = lambda row: row[:, :S * B].reshape(E, S, B)
    none_old = np.zeros(S, bool)

    def state_is(got, want, who, what):
        for k in names:
            same_bits(got[k][who], want[k][who].astype(got[k].dtype), "state %s %s" % (k, what))

    # ---- the construction-time first observation
    before = g.numpy_state(*names)
    first = g.reset_obs().cpu().numpy()
    scan, clean, tail, state1 = ns.first_obs(before, np.zeros_like(first))
    for e in range(E):
        _scan_is(scan_of(first)[e], scan[e], clean[e], none_old, None, float(before["scan_noise_std"][e]), rmax, worst, "first observation, arena %d" % e)
    same_bits(first[:, S * B:], tail, "first observation: tail")
    state_is(g.numpy_state(*names), state1, np.ones(E, bool), "after reset_obs")

    rng = np.random.default_rng(5)
    n = {}
    for t in range(30):
        act, cmd = noise_inputs(cfg, rng, t)
        if cmd is not None:
            g.set_ped_cmd(cmd)
        before, prev = g.numpy_state(*names), g.obs.cpu().numpy().copy()
        pending = g.out["done"].cpu().numpy() != 0 if g.next_step else None
        go, gout = g.step(to_device(gpu, act))
        go, gout = go.cpu().numpy(), to_numpy(gout)
        fin = to_numpy(g.final) if final else None
        after = g.numpy_state(*names)
        x = ns.expect(before, prev, act, pending)
        noise_coverage(n, x, rmax)
        std = before["scan_noise_std"]
        live = ~x["pending"]
        crashed = gout["is_crash"] != 0
        # ---- from the device's own rows, no exclusions: without a crash nothing of the returned row is below its crash threshold
        restarted_dev = (gout["done"] != 0) & live if final else np.zeros(E, bool)
        ret = np.where(restarted_dev[:, None], scan_of(fin["final_obs"])[:, S - 1] if final else 0.0, scan_of(go)[:, S - 1]).astype(np.float32)
        below = (ret < thr[None, :]).any(axis=1)
        assert not (below & ~crashed & live).any(), "step %d: arenas %s returned a row below the crash threshold without a crash" % (
            t, np.flatnonzero(below & ~crashed & live))
        ok = ~x["undecided"]
        what = "step %d" % t
        # ---- flags and the noise-free outputs
        for k, want in (("is_crash", x["crash"] & live), ("is_success", x["out"]["is_success"] != 0), ("done", x["done"])):
            assert np.array_equal((gout[k] != 0)[ok], want[ok]), "%s %s: arenas %s" % (what, k, np.flatnonzero(((gout[k] != 0) != want) & ok))
        if T > 0:
            assert np.array_equal((gout["truncated"] != 0)[ok], x["trunc"][ok]), "%s truncated" % what
        for k in ("distance", "achieved_goal", "desired_goal"):
            same_bits(gout[k][ok], x["out"][k][ok].astype(gout[k].dtype), "%s %s" % (what, k))
        for e in np.flatnonzero(ok):
            want = 0.0 if x["pending"][e] else ns.reward(x, e, bool(x["crash"][e]), ret[e])
            assert abs(gout["reward"][e] - want) <= 1e-9, "%s reward of arena %d: %.12g, expected %.12g (crash %s)" % (
                what, e, gout["reward"][e], want, x["crash"][e])
        # ---- the rows
        for e in np.flatnonzero(ok):
            old = none_old if x["fresh"][e] else x["old"][e]
            _scan_is(scan_of(go)[e], x["obs_scan"][e], x["obs_clean"][e], old, scan_of(prev)[e], float(std[e]), rmax, worst,
                     "%s, arena %d%s" % (what, e, " (first observation of its next episode)" if x["fresh"][e] else ""))
            if x["restarted"][e]:
                _scan_is(scan_of(fin["final_obs"])[e], x["view_scan"][e], x["view_clean"][e], x["old"][e], scan_of(prev)[e], float(std[e]),
                         rmax, worst, "%s, arena %d, final_obs (crash %s)" % (what, e, x["crash"][e]))
        same_bits(go[ok, S * B:], x["obs_tail"][ok], "%s: tail of obs" % what)
        who = x["restarted"] & ok
        if final and who.any():
            same_bits(fin["final_obs"][who, S * B:], x["view_tail"][who], "%s: tail of final_obs" % what)
            same_bits(fin["final_goals"][who], x["view_goals"][who], "%s: final_goals" % what)
        assert np.array_equal(restarted_dev[ok], x["restarted"][ok])
        state_is(after, x["state"], ok, "after " + what)
    print("%s: %s; %d noisy ranges compared, worst |range - model| %.3e m, worst |dg| %.3e" % (name, n, worst.n, worst.m, worst.g))
    noise_coverage_met(n, cfg)


def test_gauss_noise_at_the_corners_of_its_fields(gpu):
    """nv::gauss_noise(stream, beam = i) for streams the model's inverse finaliser builds: u1 = 2^-24 (|g| = 5.77 at a2 = 0 and
    next to pi), u1 = 1 (g exactly 0 whatever a2), a2 around pi / 2 and 3 pi / 2 (the cosine changes sign) at the largest and at
    middling radii, a2 = 0 and the largest a2, and 2^22 random streams behind them.  |g - model| <= TOL / 0.05 = 2e-4."""
    F = 0xFFFFFF
    corners = [(0, 0), (0, 1 << 23), (0, F), (F, 0), (F, 1 << 22), (F, F), (F, 12345), (1, 0), (F - 1, F)]
    for radius in (0, 1, 1000, 1 << 20, 1 << 23):
        for quarter in (1 << 22, 3 << 22):
            corners += [(radius, quarter + d) for d in (-2, -1, 0, 1, 2)]
    rng = np.random.default_rng(17)
    n_rand = 1 << 22
    low8 = rng.integers(0, 256, (len(corners), 2))
    streams = [model.stream_for_fields(fa << 8 | int(l[0]), fb << 8 | int(l[1]), i) for i, ((fa, fb), l) in enumerate(zip(corners, low8))]
    streams = np.concatenate([np.array(streams, dtype=np.uint64), rng.integers(0, 1 << 64, n_rand, dtype=np.uint64)])
    beams = np.arange(len(streams))
    fa, fb = model.beam_fields(streams, beams)
    assert [(int(a), int(b)) for a, b in zip(fa[:len(corners)], fb[:len(corners)])] == corners
    want = model.gauss_from_fields(fa, fb)
    lo, hi = (streams & np.uint64(0xFFFFFFFF)).astype(np.float64), (streams >> np.uint64(32)).astype(np.float64)
    got = gpu.sim.debug_math(17, to_device(gpu, lo), to_device(gpu, hi)).cpu().numpy()
    d = np.abs(got - want)
    print("gauss_noise: %d inputs, worst |g - model| %.3e at input %d (u1 field %d, a2 field %d, g %.6f); corners alone %.3e" % (
        len(d), d.max(), int(np.argmax(d)), fa[np.argmax(d)], fb[np.argmax(d)], want[np.argmax(d)], d[:len(corners)].max()))
    assert abs(want[0] - math.sqrt(48 * math.log(2))) < 1e-12 and abs(want[1] + want[0]) < 1e-6      # +-5.768: the largest |g|
    one = fa == F
    assert one[:len(corners)].sum() >= 4 and (got[one] == 0.0).all(), "u1 = 1 must give exactly 0"
    assert (d <= G_TOL).all(), "%d of %d draws differ from the model by more than %g, worst %.3e" % ((d > G_TOL).sum(), len(d), G_TOL, d.max())
