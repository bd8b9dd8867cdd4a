"""Vector instructions per arena-step of the c2 scan under different march schedules, from the per-ray probe counts of
march_counts.py (counts.npz) and static instruction counts of the kernel's listing.

A wavefront marches a group of rays until the group's exit condition; a probe round costs the same whether 1 or 64 lanes
are still marching.  Priced per group: directions, probe rounds, the finish, and for parked rays a park and a fetch.

    python profiles/r11_c2/model/price_schedules.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROUND, DIRS, FINISH, PARK, FETCH = 33, 45, 75, 10, 8        # vector instructions (listing of the c2 kernel)
OTHER = 0                                                    # phases outside the scan: the same under every schedule


def chunks_of(n):
    return [n[c:c + 64] for c in range(0, len(n), 64)]


def no_parking(n):
    return sum(DIRS + ROUND * int(v.max()) + FINISH for v in chunks_of(n))


def park(n, T, cascade=False):
    """Leave a chunk when at most T rays march; parked rays 64 at a time (cascade: those groups re-park at <= T too)."""
    cost = 0
    pool = []
    for v in chunks_of(n):
        s = np.sort(v)[::-1]
        if len(s) <= T:
            cost += DIRS + ROUND * int(s[0]) + FINISH
            continue
        r_exit = int(s[T])
        rem = [int(x) - r_exit for x in s[:T] if x > r_exit]
        cost += DIRS + ROUND * r_exit + FINISH + (PARK if rem else 0)
        pool += rem
    while pool:
        grp, pool = pool[:64], pool[64:]
        s = np.sort(np.array(grp))[::-1]
        if cascade and len(s) > T:                          # at most T of the group go back to the pool, each shorter than before
            r_exit = int(s[T])
            rem = [int(x) - r_exit for x in s[:T] if x > r_exit]
            cost += FETCH + ROUND * r_exit + FINISH + (PARK if rem else 0)
            pool += rem
        else:
            cost += FETCH + ROUND * int(s[0]) + FINISH
    return cost


def all_lanes_busy(n):
    return int(np.ceil(n.sum() / 64.0)) * ROUND + len(chunks_of(n)) * (DIRS + FINISH)


def main():
    probes = np.load(os.path.join(HERE, "counts.npz"))["probes"]
    rows = [("no parking", no_parking),
            ("park at <= 16 lanes, parked rays 64 at a time (the kernel)", lambda n: park(n, 16)),
            ("park at <= 12 lanes", lambda n: park(n, 12)),
            ("park at <= 16 lanes, parked pool cascaded (re-park at <= 16)", lambda n: park(n, 16, cascade=True)),
            ("every lane always busy (unreachable)", all_lanes_busy)]
    for name, fn in rows:
        v = np.mean([fn(n) for n in probes]) + OTHER
        print("%-66s %8.0f" % (name, v))
    print("(scan only; the kernel's other phases add the same count to every row)")


if __name__ == "__main__":
    main()
