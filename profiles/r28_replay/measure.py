"""Device-event times of the four entries that share csrc/kernels_replay.hpp, on the library that is loaded (NAVSIM_LIB selects
another build, e.g. the parent commit's), for an A/B in which the two libraries alternate process by process.

    python profiles/r28_replay/measure.py events c2|c3 TAG     # reset() + ten steps, then per entry and shape one warm launch and
                                                               # REPS launches between two device events each; prints and
                                                               # appends one JSON line {tag, world, times: {name: median ms}}
    python profiles/r28_replay/measure.py table FILE           # the JSON lines of FILE (tags 'parent' and 'head') as a table:
                                                               # medians over the processes, the parent's spread (max - min of
                                                               # its own values), and whether head <= parent + spread

Shapes: the lookahead pair at K = 9 and 64 (navsim_lookahead under the default cap, navsim_lookahead_obs with rows='scan'), the
rollout pair at (K, H) = (16, 8) and (64, 16) (navsim_rollout under the default cap, navsim_rollout_obs with rows='last'); the
worlds are profiles/r27_rollout_obs/measure.py's.  NAVSIM_OUT overrides the output directory, NAVSIM_ONLY=lookahead|rollout
measures that pair alone."""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r28_replay"))
E = int(os.environ.get("NAVSIM_ENVS", "4096"))
B = 1081
LOOK_K = (9, 64)
ROLL_KH = ((16, 8), (64, 16))
REPS = int(os.environ.get("NAVSIM_REPS", "5"))
ONLY = os.environ.get("NAVSIM_ONLY", "")                               # "lookahead" or "rollout": that pair alone


def table(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    for world in sorted({r["world"] for r in rows}):
        side = {tag: [r["times"] for r in rows if r["world"] == world and r["tag"] == tag] for tag in ("parent", "head")}
        print("%s-shaped world, %d arenas x %d beams: %d parent and %d head processes, alternating; ms per launch" %
              (world, E, B, len(side["parent"]), len(side["head"])))
        print("  %-24s %10s %10s %10s %10s %8s  %s" % ("entry and shape", "parent", "head", "head/par", "spread", "+spread", "verdict"))
        for name in side["parent"][0]:
            p = sorted(t[name] for t in side["parent"]); h = sorted(t[name] for t in side["head"])
            pm, hm, spread = p[len(p) // 2], h[len(h) // 2], p[-1] - p[0]
            print("  %-24s %10.3f %10.3f %10.4f %10.3f %8.3f  %s" % (name, pm, hm, hm / pm, spread, pm + spread,
                                                                  "ok" if hm <= pm + spread else "SLOWER by %.3f ms" % (hm - pm)))


if len(sys.argv) > 2 and sys.argv[1] == "table":
    table(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch, nav_gym_env

WORLDS = dict(c3=dict(num_envs=E, n_beams=B, map_size=500, indoor_ratio=0.0, pedestrian_model="sfm", num_humans=20, device="cuda:0", seed=1234),
              c2=dict(num_envs=E, n_beams=B, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234))


def actions(n, k=64):
    g = torch.Generator(device="cuda:0"); g.manual_seed(78)
    a = torch.rand((k, n, 2), generator=g, device="cuda:0", dtype=torch.float64)
    a[..., 0] *= 0.5; a[..., 1] = a[..., 1] * 1.28 - 0.64
    return a


def sequences(acts, K, H):
    """[E,K,H,2]: sequence k repeats candidate k's action, turning the other way every fourth step"""
    seq = acts[:K].permute(1, 0, 2)[:, :, None, :].repeat(1, 1, H, 1)
    seq[:, :, 3::4, 1] *= -1.0
    return seq.contiguous()


def timed(call):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


world, tag = sys.argv[2], sys.argv[3]
env = nav_gym_env.make("NavGym-v0", **WORLDS[world])
env.reset()
acts = actions(E)
for t in range(10):
    env.step(acts[t])
sim = env.sim
times = {}
for K in (LOOK_K if ONLY != "rollout" else ()):
    cand = acts[:K].permute(1, 0, 2).contiguous()
    sim.enable_lookahead(K)
    times["lookahead K=%d" % K] = timed(lambda: sim.lookahead(cand))
    sim.products.pop("lookahead", None)
    sim.enable_lookahead_obs(K, dict(rows="scan"))
    times["lookahead_obs K=%d" % K] = timed(lambda: sim.lookahead_obs(cand))
    sim.products.pop("lookahead_obs", None)
    torch.cuda.empty_cache()
for K, H in (ROLL_KH if ONLY != "lookahead" else ()):
    seq = sequences(acts, K, H)
    sim.enable_rollout(K, H)
    times["rollout (%d, %d)" % (K, H)] = timed(lambda: sim.rollout(seq))
    sim.products.pop("rollout", None)
    sim.enable_rollout_obs(K, H, dict(rows="last"))
    times["rollout_obs (%d, %d)" % (K, H)] = timed(lambda: sim.rollout_obs(seq))
    sim.products.pop("rollout_obs", None)
    torch.cuda.empty_cache()
line = json.dumps(dict(tag=tag, world=world, lib=os.path.basename(os.environ.get("NAVSIM_LIB", "in-tree")), times=times))
print(line, flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "events.jsonl"), "a") as f:
    f.write(line + "\n")
env.close()
