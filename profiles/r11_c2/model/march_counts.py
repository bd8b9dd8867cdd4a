"""Per-ray probe counts of the c2 scan, without a GPU.

Marches the 1081 beams of one scan on each of 160 c2 maps (world.make_maps(160, 500, 1234): 500 x 500 outdoor maps) the
way the kernel does -- float32 t, t += max(0.999f * d, 1), d the exact Euclidean distance to the nearest occupied cell
(SciPy), the ray ends on an occupied cell or at the march limit -- from a free cell at least 1.2 m from every obstacle,
heading drawn uniformly.  Saves, per ray, the number of probes and how many of them were unit steps (d <= 1 / 0.999:
the only probes whose next sample does not depend on the distance read), as counts.npz beside this file.

    python profiles/r11_c2/model/march_counts.py [n_maps]
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "nav-gym_amd"))
from nav_gym_amd import world  # noqa: E402

SIZE, B, RES, RANGE_MAX, SEED = 500, 1081, 0.05, 25.0, 1234


def march(d, i0, j0, heading):
    ang = np.linspace(-0.75 * np.pi, 0.75 * np.pi, B)
    h = (ang + heading).astype(np.float32).astype(np.float64)
    dx, dy = np.cos(h).astype(np.float32), np.sin(h).astype(np.float32)
    x0, y0 = np.float32(i0), np.float32(j0)
    limit = np.float32(RANGE_MAX / RES + 4.0)
    t = np.zeros(B, np.float32); n = np.zeros(B, np.int32); unit = np.zeros(B, np.int32)
    act = np.ones(B, bool)
    while act.any():
        x = (x0 + dx * t).astype(np.int32); y = (y0 + dy * t).astype(np.int32)
        act &= (x >= 0) & (x < SIZE) & (y >= 0) & (y < SIZE)
        dd = np.where(act, d[np.clip(y, 0, SIZE - 1), np.clip(x, 0, SIZE - 1)], np.float32(0))
        n += act
        act &= dd > 0
        step = np.maximum(np.float32(0.999) * dd, np.float32(1.0))
        unit += act & (step == np.float32(1.0))
        t = np.where(act, t + step, t).astype(np.float32)
        act &= t < limit
    return n, unit


def main():
    n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 160
    occ = world.make_maps(n_maps, SIZE, SEED)
    rng = np.random.default_rng(SEED)
    probes = np.zeros((n_maps, B), np.int32); units = np.zeros((n_maps, B), np.int32)
    for e in range(n_maps):
        d = ndimage.distance_transform_edt(occ[e] == 0).astype(np.float32)
        free = np.argwhere(d >= 1.2 / RES)
        if len(free) == 0:
            free = np.argwhere(d >= 0.6 * d.max())
        j0, i0 = free[rng.integers(len(free))]
        probes[e], units[e] = march(d, int(i0), int(j0), rng.uniform(-np.pi, np.pi))
    np.savez_compressed(os.path.join(HERE, "counts.npz"), probes=probes, units=units)
    chunks = [probes[:, c:c + 64].max(axis=1) for c in range(0, B, 64)]
    rounds = np.stack(chunks, axis=1)
    print("%d scans: %.2f probes per ray, %.2f rounds per 64-beam chunk, useful lanes %.3f, p99 %d, slowest ray of a scan %.1f"
          % (n_maps, probes.mean(), rounds.mean(), probes.sum() / 64.0 / rounds.sum(), np.percentile(probes, 99), probes.max(axis=1).mean()))
    print("unit steps: %.3f of all probes" % (units.sum() / probes.sum()))
    for lo in (20, 50):
        m = probes > lo
        print("  rays longer than %d probes: unit steps %.3f of their probes" % (lo, units[m].sum() / max(probes[m].sum(), 1)))


if __name__ == "__main__":
    main()
