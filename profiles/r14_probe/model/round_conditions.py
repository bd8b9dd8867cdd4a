"""How often may a probe round of the c2 scan take a short form?  Modelled on the CPU, no GPU.

Marches one scan on each of 40 c2 maps (world.make_maps(40, 500, 1234)) the way navsim_step_kernel<256, ...> does:
64-beam chunks, a chunk is left when at most 16 lanes still march, the parked rays are marched 64 at a time; float32 t,
t += max(0.999f * sqrt(d2), 1), d2 the exact integer squared distance; one pose per map on a free cell at least 1.2 m
from every obstacle.  Lanes that are not live run along as in the kernel: a finished lane stays where it stopped, the
lanes past beam B - 1 of the last chunk sit on beam B - 1's first sample, the lanes past the last parked ray on the
group's first ray as it was parked.

Per round it records the wave-uniform conditions of profiles/r14_probe:
  item 1  no voting lane stands in a tile whose record needs two rectangles (ia != ib).  The records are rebuilt here
          by the builder's own first greedy round (kernels_rect.hpp rect_tile_build: maximal rectangles, both growth
          orders, around a nearest obstacle of the tile's first and last cell; one-rectangle when a candidate
          reproduces d2 on all 64 cells), so this is the records' condition, not the component proxy.  The proxy
          (all 64 cells of the tile share one nearest obstacle component) is printed beside it.
  item 2  no voting lane has d2 >= N, for N = 256 .. 4096.
Each with only the LIVE lanes voting and with ALL 64 lanes voting.

    python profiles/r14_probe/model/round_conditions.py [n_maps]
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "nav-gym_amd"))
from nav_gym_amd import world  # noqa: E402

SIZE, B, RES, RANGE_MAX, SEED, PARK = 500, 1081, 0.05, 25.0, 1234, 16
NS = (256, 512, 1024, 2048, 4096)
ROUND_VALU, RECT_B_VALU, STEP_VALU = 33, 6, 8


class Records:
    """one-rectangle / two-rectangle verdict per 8x8 tile, by the builder's first greedy round, on demand"""

    def __init__(self, occ, d2):
        self.occ, self.d2 = occ != 0, d2
        H, W = occ.shape
        idx = np.arange(W)
        free = ~self.occ
        lastf = np.maximum.accumulate(np.where(free, idx[None, :], -1), axis=1)
        nextf = np.minimum.accumulate(np.where(free, idx[None, :], W)[:, ::-1], axis=1)[:, ::-1]
        self.hl = np.where(free, 32767, lastf + 1); self.hr = np.where(free, -1, nextf - 1)
        idy = np.arange(H)
        lastf = np.maximum.accumulate(np.where(free, idy[:, None], -1), axis=0)
        nextf = np.minimum.accumulate(np.where(free, idy[:, None], H)[::-1, :], axis=0)[::-1, :]
        self.vt = np.where(free, 32767, lastf + 1); self.vb = np.where(free, -1, nextf - 1)
        self.memo = {}

    def nearest(self, px, py):                                  # rect_nearest_obstacle: smallest dx first, signs ++ -+ +- --
        d2 = int(self.d2[py, px])
        if d2 == 0:
            return px, py
        H, W = self.occ.shape
        dx = np.arange(int(np.sqrt(d2)) + 2)
        rem = d2 - dx * dx
        dy = np.floor(np.sqrt(np.maximum(rem, 0))).astype(np.int64)
        ok = (rem >= 0) & (dy * dy == rem)
        for a, b in zip(dx[ok], dy[ok]):
            for s in range(4):
                x = px + (-a if s & 1 else a); y = py + (-b if s & 2 else b)
                if 0 <= x < W and 0 <= y < H and self.occ[y, x]:
                    return int(x), int(y)
        raise RuntimeError("inconsistent distance field")

    @staticmethod
    def _span(ok, at):                                          # the run of True around index `at`
        bad = np.flatnonzero(~ok)
        lo = bad[bad < at]; hi = bad[bad > at]
        return (lo[-1] + 1 if len(lo) else 0), (hi[0] - 1 if len(hi) else len(ok) - 1)

    def grow(self, ox, oy, order):                              # rect_grow
        if order == 0:
            xl, xr = self.hl[oy, ox], self.hr[oy, ox]
            y0, y1 = self._span((self.hl[:, ox] <= xl) & (self.hr[:, ox] >= xr), oy)
            return xl, xr, y0, y1
        yt, yb = self.vt[oy, ox], self.vb[oy, ox]
        x0, x1 = self._span((self.vt[oy, :] <= yt) & (self.vb[oy, :] >= yb), ox)
        return x0, x1, yt, yb

    def one_rect(self, tx, ty):
        key = (tx, ty)
        if key in self.memo:
            return self.memo[key]
        H, W = self.occ.shape
        ys, xs = np.mgrid[ty * 8:min(ty * 8 + 8, H), tx * 8:min(tx * 8 + 8, W)]
        want = self.d2[ys, xs]
        verdict = False
        for leader in ((xs[0, 0], ys[0, 0]), (xs[-1, -1], ys[-1, -1])):
            ox, oy = self.nearest(int(leader[0]), int(leader[1]))
            for order in (0, 1):
                x0, x1, y0, y1 = self.grow(ox, oy, order)
                ddx = np.maximum(np.maximum(x0 - xs, xs - x1), 0); ddy = np.maximum(np.maximum(y0 - ys, ys - y1), 0)
                if np.array_equal(ddx * ddx + ddy * ddy, want):
                    verdict = True
                    break
            if verdict:
                break
        self.memo[key] = verdict
        return verdict


class Tally:
    def __init__(self):
        self.rounds = 0; self.live = 0; self.probes = 0; self.probes_one = 0; self.probes_lt1024 = 0
        self.one = {"live": 0, "all": 0}; self.proxy = {"live": 0, "all": 0}
        self.lt = {"live": np.zeros(len(NS), np.int64), "all": np.zeros(len(NS), np.int64)}
        self.last_chunk_rounds = 0; self.last_chunk_lt1024 = {"live": 0, "all": 0}


def march_group(d2, rec, same_comp, x0, y0, dx, dy, t, active, limit, stop_at, tally, last_chunk=False):
    """rounds of one wavefront over 64 lanes until at most stop_at lanes are live; returns t, active"""
    n = len(t)
    while active.sum() > stop_at:
        x = (x0 + dx * t).astype(np.int32); y = (y0 + dy * t).astype(np.int32)
        x = np.clip(x, 0, SIZE - 1); y = np.clip(y, 0, SIZE - 1)    # closed maps: never taken (kernel: no bounds test)
        dd = d2[y, x]
        one = np.array([rec.one_rect(int(a) >> 3, int(b) >> 3) for a, b in zip(x, y)])
        prox = same_comp[y >> 3, x >> 3]
        tally.rounds += 1; tally.live += int(active.sum()); tally.probes += int(active.sum())
        tally.probes_one += int(one[active].sum()); tally.probes_lt1024 += int((dd[active] < 1024).sum())
        for who, m in (("live", active), ("all", np.ones(n, bool))):
            tally.one[who] += bool(one[m].all()); tally.proxy[who] += bool(prox[m].all())
            tally.lt[who] += np.array([bool((dd[m] < N).all()) for N in NS])
            if last_chunk:
                tally.last_chunk_lt1024[who] += bool((dd[m] < 1024).all())
        tally.last_chunk_rounds += last_chunk
        occ = active & (dd == 0)
        step = np.maximum(np.float32(0.999) * np.sqrt(dd.astype(np.float32)), np.float32(1.0))
        go = active & ~occ
        tn = (t + step).astype(np.float32)
        t = np.where(go, tn, t).astype(np.float32)
        active = go & (tn < limit)
    return t, active


def scan(occ, d2, i0, j0, heading, tally):
    lab, _ = ndimage.label(occ != 0)
    near = ndimage.distance_transform_edt(occ == 0, return_distances=False, return_indices=True)
    comp = lab[near[0], near[1]]                                 # nearest obstacle component of every cell
    T = (SIZE + 7) // 8
    pad = np.pad(comp, ((0, T * 8 - SIZE), (0, T * 8 - SIZE)), mode="edge").reshape(T, 8, T, 8)
    same_comp = (pad.max(axis=(1, 3)) == pad.min(axis=(1, 3)))
    rec = Records(occ, d2)
    ang = np.linspace(-0.75 * np.pi, 0.75 * np.pi, B)
    h = (ang + heading).astype(np.float32).astype(np.float64)
    dxs, dys = np.cos(h).astype(np.float32), np.sin(h).astype(np.float32)
    x0, y0 = np.float32(i0), np.float32(j0)
    limit = np.float32(RANGE_MAX / RES + 4.0)
    t1 = np.maximum(np.float32(0.999) * np.sqrt(np.float32(d2[j0, i0])), np.float32(1.0))
    parked = []
    for c in range(0, B, 64):
        k = np.minimum(np.arange(c, c + 64), B - 1)
        valid = np.arange(c, c + 64) < B
        t = np.full(64, t1, np.float32)
        t, act = march_group(d2, rec, same_comp, x0, y0, dxs[k], dys[k], t, valid.copy() & bool(t1 < limit), limit, PARK, tally,
                             last_chunk=not valid.all())
        parked += [(dxs[kk], dys[kk], tt) for kk, tt in zip(k[act], t[act])]
    for g in range(0, len(parked), 64):
        grp = parked[g:g + 64]
        valid = np.arange(64) < len(grp)
        grp = grp + [grp[0]] * (64 - len(grp))
        dx = np.array([p[0] for p in grp], np.float32); dy = np.array([p[1] for p in grp], np.float32)
        t = np.array([p[2] for p in grp], np.float32)
        march_group(d2, rec, same_comp, x0, y0, dx, dy, t, valid, limit, 0, tally)
    return len(parked)


def main():
    n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    occ = world.make_maps(n_maps, SIZE, SEED)
    rng = np.random.default_rng(SEED)
    tally = Tally(); n_parked = 0
    for e in range(n_maps):
        d = ndimage.distance_transform_edt(occ[e] == 0)
        d2 = np.rint(d * d).astype(np.int64)
        free = np.argwhere(d >= 1.2 / RES)
        if len(free) == 0:
            free = np.argwhere(d >= 0.6 * d.max())
        j0, i0 = free[rng.integers(len(free))]
        n_parked += scan(occ[e], d2, int(i0), int(j0), rng.uniform(-np.pi, np.pi), tally)
    R = float(tally.rounds)
    print("%d scans: %.1f rounds per scan, %.1f live lanes per round, %.0f parked rays per scan" % (n_maps, R / n_maps, tally.live / R, n_parked / n_maps))
    print("by probe: one-rectangle tile %.3f, d2 < 1024 %.3f" % (tally.probes_one / tally.probes, tally.probes_lt1024 / tally.probes))
    for who in ("live", "all"):
        print("%s lanes vote:" % who.upper())
        print("  item 1, no lane in a two-rectangle tile: %.3f of the rounds (component proxy %.3f)" % (tally.one[who] / R, tally.proxy[who] / R))
        print("  item 2, no lane with d2 >= " + " / ".join(str(N) for N in NS) + ": " + " / ".join("%.3f" % (v / R) for v in tally.lt[who]))
    L = max(tally.last_chunk_rounds, 1)
    print("rounds of the last chunk (7 lanes past beam B - 1): %.3f of all; d2 < 1024 on every lane in %.3f of them (live vote %.3f)"
          % (tally.last_chunk_rounds / R, tally.last_chunk_lt1024["all"] / L, tally.last_chunk_lt1024["live"] / L))
    f1 = tally.one["live"] / R
    f2l, f2a = tally.lt["live"][2] / R, tally.lt["all"][2] / R
    print("priced, vector instructions per round of %d:" % ROUND_VALU)
    print("  item 1 (live vote: one compare):                        %.3f x %d - 1 = %+.2f" % (f1, RECT_B_VALU, f1 * RECT_B_VALU - 1))
    print("  item 2, all lanes vote (compare + shift):               %.3f x %d - 1 = %+.2f" % (f2a, STEP_VALU - 1, f2a * (STEP_VALU - 1) - 1))
    print("  item 2, live lanes vote, read predicated (+ one and):   %.3f x %d - 1 = %+.2f" % (f2l, STEP_VALU - 2, f2l * (STEP_VALU - 2) - 1))
    best2 = max(f2a * (STEP_VALU - 1) - 1, f2l * (STEP_VALU - 2) - 1)
    print("  together %.2f per round, %.0f per arena-step of %.0f rounds" % (f1 * RECT_B_VALU - 1 + best2, (f1 * RECT_B_VALU - 1 + best2) * R / n_maps, R / n_maps))


if __name__ == "__main__":
    main()
