"""CPU: the float64 model of the scan noise (tests/scan_noise_f64.py) -- its statistics over an index set shaped like a batch,
the key schedule's properties, and the share of arena-steps of the GPU test's cases whose crash the model cannot decide.

tests/test_gpu_scan_noise.py ties every draw of the device to this model, so the model's statistics are the device's."""
import math

import numpy as np
import pytest

import ref
import scan_noise_f64 as m
from gpu_support import NOISE_CAP, NOISE_CASES, TOL, noise_coverage, noise_coverage_met, noise_emulation, noise_world, same_bits

SEED = 99


@pytest.fixture(scope="module")
def batch():
    """g of 64 arenas x 40 consecutive scan keys (first scans and re-scans of steps 1 .. 20 of episode 0) x 1081 beams"""
    keys = np.array([m.step_key(0, 1) + i for i in range(40)], dtype=np.uint64)
    return m.gauss(m.noise_stream(SEED, np.arange(64)[:, None], keys[None, :]), np.arange(1081))


def test_moments_of_a_batch(batch):
    n = batch.size
    assert n == 2767360
    mean, std, kurt = m.moments(batch)
    print("mean %.3e (bound %.3e), std %.5f, kurtosis %.4f" % (mean, 3 / math.sqrt(n), std, kurt))
    assert abs(mean) < 3 / math.sqrt(n)
    assert abs(std - 1.0) < 2e-3
    assert 2.97 <= kurt <= 3.03


def test_neighbours_are_uncorrelated(batch):
    bound = 3 / math.sqrt(batch.size)
    lag = dict(beams=m.correlation(batch[:, :, :-1], batch[:, :, 1:]), keys=m.correlation(batch[:, :-1], batch[:, 1:]),
               arenas=m.correlation(batch[:-1], batch[1:]))
    print(lag, "bound %.3e" % bound)
    for k, v in lag.items():
        assert abs(v) < bound, (k, v)
    beams = np.arange(100000)
    key = m.step_key(0, 1)
    c = m.correlation(m.gauss(m.noise_stream(SEED, 0, key), beams), m.gauss(m.noise_stream(SEED, 0, key + 1), beams))
    print("first scan against re-scan: %.3e (bound %.3e)" % (c, 3 / math.sqrt(1e5)))
    assert abs(c) < 3 / math.sqrt(1e5)


def test_float_inputs_are_exact_float32_values():
    """u1 and a2 at the ends of their 24-bit fields; the inverse of the finalisers finds a stream for any pair of fields"""
    for fa, fb, beam in ((0, 0, 0), (0xFFFFFF, 0xFFFFFF, 5), (0x123456, 0x400000, 1080)):
        s = m.stream_for_fields(fa << 8 | 0x5A, fb << 8 | 0xA5, beam)
        ga, gb = m.beam_fields(np.array(s, dtype=np.uint64), np.array([beam]))
        assert (int(ga[0]), int(gb[0])) == (fa, fb)
    u1, a2 = m.uniform_inputs(np.array([0, 0xFFFFFF], np.uint32), np.array([0, 0xFFFFFF], np.uint32))
    assert u1.dtype == np.float32 and a2.dtype == np.float32
    assert float(u1[0]) == 2.0 ** -24 and float(u1[1]) == 1.0
    assert float(a2[0]) == 0.0 and float(a2[1]) == float(np.float32(0xFFFFFF) * m.TWO_PI_24) < 2 * math.pi
    g = m.gauss_from_fields(np.array([0, 0xFFFFFF], np.uint32), np.array([0, 0], np.uint32))
    assert abs(g[0] - math.sqrt(2 * 24 * math.log(2))) < 1e-12 and g[1] == 0.0


def test_noisy_keeps_range_max_and_zero_std():
    clean = np.array([0.5, 3.0, 2.999, 0.0, 3.0], np.float32)
    out = m.noisy(clean, np.float32(0.05), m.noise_stream(1, 2, 3), 3.0)
    assert out[1] == 3.0 and out[4] == 3.0 and (out[[0, 2, 3]] != clean[[0, 2, 3]]).all()
    assert np.array_equal(m.noisy(clean, np.float32(0.0), m.noise_stream(1, 2, 3), 3.0), clean.astype(np.float64))
    g = m.gauss(m.noise_stream(1, 2, 3), np.arange(5))
    assert np.array_equal(out[[0, 2, 3]], clean[[0, 2, 3]].astype(np.float64) + float(np.float32(0.05)) * g[[0, 2, 3]])


def test_keys_of_an_episode_and_its_neighbours_are_distinct():
    keys = []
    for ep in range(4):
        keys.append(m.first_obs_key(ep))
        for steps in range(1, 200):
            keys += [m.step_key(ep, steps), m.rescan_key(ep, steps)]
    assert len(set(keys)) == len(keys)
    assert m.step_key(3, 1) == (3 << 32) + 2 and m.rescan_key(3, 1) == (3 << 32) + 3 and m.first_obs_key(3) == 3 << 32


def test_streams_differ_between_arenas_seeds_and_keys():
    beams = np.arange(256)
    base = m.gauss(m.noise_stream(7, 10, m.step_key(0, 1)), beams)
    others = dict(arena=m.noise_stream(7, 11, m.step_key(0, 1)), seed_above_bit_32=m.noise_stream(7 + (1 << 40), 10, m.step_key(0, 1)),
                  rescan=m.noise_stream(7, 10, m.rescan_key(0, 1)), next_step=m.noise_stream(7, 10, m.step_key(0, 2)),
                  episode=m.noise_stream(7, 10, m.step_key(1, 1)), arena_far=m.noise_stream(7, 1010, m.step_key(0, 1)))
    for k, s in others.items():
        g = m.gauss(s, beams)
        assert (g != base).mean() > 0.99, k
        assert abs(m.correlation(g, base)) < 4 / math.sqrt(len(beams)), k


@pytest.mark.parametrize("name", sorted(NOISE_CASES))
def test_cases_of_the_gpu_test_are_decidable_and_meet_their_purpose(name):
    """The GPU test's rollout with the model in the device's place: the arena-steps whose noisy first scan comes within TOL of a
    crash threshold are at most a quarter of the cap the GPU test allows, and the run has the crashes, restarts, truncations,
    range_max beams and crossings that the case is for.  (A case that fails here gets other worlds, not another cap.)"""
    cfg, occ, host = noise_world(ref.default_config, name)
    n = {}
    for t, x in noise_emulation(cfg, host):
        noise_coverage(n, x, cfg.range_max)
        assert (np.abs(x["margin"][x["undecided"]]) <= TOL).all()
    print(name, n)
    assert n["undecided"] <= 0.25 * NOISE_CAP * n["arena_steps"], n
    noise_coverage_met(n, cfg)


@pytest.mark.parametrize("name", sorted(NOISE_CASES))
def test_without_noise_the_expectation_is_the_oracles_own_rollout(name):
    """NoisyStep pieces a step together from two oracles that never restart (clean scans, both branches, the restart, the
    terminal row, NEXT_STEP's resets).  With every std 0 the pieces must add up to the oracle's own run of the case, with its
    real thresholds and its own restarts: rows, final rows, outputs and state, bit for bit, at every step."""
    cfg, occ, host = noise_world(ref.default_config, name)
    cfg.max_episode_steps = 0                                    # (the oracle has no time limit)
    host["scan_noise_std"][:] = 0.0
    S, B = cfg.n_scan_stack, cfg.n_beams
    r = ref.RefSim(cfg, host)
    r.reset_obs()
    n = 0
    for t, x in noise_emulation(cfg, host):
        act, cmd = x["inputs"]
        if cmd is not None:
            r.set_ped_cmd(cmd)
        ro, rout = r.step(act)
        what = "%s step %d" % (name, t)
        same_bits(ro, np.concatenate([x["obs_scan"].reshape(len(ro), -1).astype(np.float32), x["obs_tail"]], axis=1), what + " obs")
        for k, want in (("is_crash", x["crash"]), ("done", x["done"])):
            assert np.array_equal(rout[k] != 0, want), (what, k)
        for k in ("distance", "is_success", "achieved_goal", "desired_goal"):
            same_bits(rout[k], x["out"][k].astype(rout[k].dtype), "%s %s" % (what, k))
        live = np.flatnonzero(~x["pending"])
        want = np.array([ns_reward(x, e) for e in live])
        assert np.abs(rout["reward"][live] - want).max() <= 1e-9, what
        who = x["restarted"]
        if who.any():
            same_bits(r.final["final_obs"][who], np.concatenate([x["view_scan"].reshape(len(ro), -1).astype(np.float32), x["view_tail"]], axis=1)[who],
                      what + " final_obs")
            same_bits(r.final["final_goals"][who], x["view_goals"][who], what + " final_goals")
        for k, v in x["state"].items():
            same_bits(r.a[k], v.astype(r.a[k].dtype), "%s state %s" % (what, k))
        n += int(who.sum()) + int(x["pending"].sum())
    assert n >= 3 or cfg.auto_reset == 0


def ns_reward(x, e):
    return x["reward_of"](e, bool(x["crash"][e]), x["view_scan"][e, -1].astype(np.float32))
