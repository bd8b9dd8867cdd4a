"""What info['episode'] costs through NavGymEnv.step() on the c2-shaped world (4096 arenas, 1081 beams, 500 x 500 maps, no
pedestrians, same-step auto-reset with terminal observations): three environments of the same world alternate in one process,

    off     episode_stats=False
    on      episode_stats=True: one launch behind the step (navsim_episode_stats_update)
    torch   episode_stats=False, and the SAME quantities (return, length, path length, minimum clearance, discomfort steps,
            outcome, the published rows, the totals) composed from torch ops behind the step

in windows of NAVSIM_WINDOW steps, NAVSIM_REPS windows each, a host clock around a window that ends in a device synchronise.
Writes profiles/r13_episode_stats/summary.txt (NAVSIM_OUT overrides the directory): per variant the median, minimum and
maximum window, and the ratio to `off`.

    python profiles/_diag/episode_stats_steps.py                    # the three variants
    python profiles/_diag/episode_stats_steps.py --ten-steps [on]   # reset() + ten steps of `off` (or `on`), nothing else: run it
                                                                    # under rocprofv3 --kernel-trace --stats to see that `off`
                                                                    # launches nothing new, and what the kernel of `on` takes
    python profiles/_diag/episode_stats_steps.py --kernels CSV off|on   # the kernels of such a run (its kernel_stats.csv or
                                                                    # kernel_trace.csv), counted, appended to the summary
"""
import collections, csv, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
OUT = os.environ.get("NAVSIM_OUT", os.path.join(ROOT, "profiles", "r13_episode_stats"))
os.makedirs(OUT, exist_ok=True)

if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    names, avg_us = collections.Counter(), {}
    with open(sys.argv[2]) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name") or "?"
            names[name] += int(row["Calls"]) if "Calls" in row else 1
            if "AverageNs" in row:
                avg_us[name] = float(row["AverageNs"]) / 1e3
    variant = sys.argv[3] if len(sys.argv) > 3 else "off"
    with open(os.path.join(OUT, "summary.txt"), "a") as f:
        f.write("\nkernels of reset() + ten steps of `%s` (rocprofv3 --kernel-trace --stats): launches, average us, name\n" % variant)
        for k, n in sorted(names.items(), key=lambda kv: -kv[1]):
            f.write("  %6d  %9s  %s\n" % (n, "%.2f" % avg_us[k] if k in avg_us else "", k.replace("(anonymous namespace)::", "")[:140]))
        f.write("  launches of kernels with 'episode' in their name: %d\n" % sum(n for k, n in names.items() if "episode" in k))
    sys.exit(0)

import numpy as np
import torch, torch.utils._python_dispatch, nav_gym_env

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
window, reps = int(os.environ.get("NAVSIM_WINDOW", "200")), int(os.environ.get("NAVSIM_REPS", "7"))
kw = dict(num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, pedestrian_model="none", num_humans=0, device="cuda:0", seed=1234)
g = torch.Generator(device="cuda:0"); g.manual_seed(78)
acts = torch.rand((64, E, 2), generator=g, device="cuda:0", dtype=torch.float64)
acts[..., 0] *= 0.5; acts[..., 1] = acts[..., 1] * 1.28 - 0.64

if len(sys.argv) > 1 and sys.argv[1] == "--ten-steps":
    env = nav_gym_env.make("NavGym-v0", episode_stats=sys.argv[2:3] == ["on"], **kw)
    env.reset()
    for t in range(10):
        env.step(acts[t])
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)


class TorchStats(object):
    """The quantities of navsim_episode_stats_update from what step() returns, in torch ops (same-step auto-reset)."""

    def __init__(self, env):
        c = env.cfg
        self.B, self.S = c.n_beams, c.n_scan_stack
        self.thr, self.dthr = env.scan_threshold, env.scan_discomfort_threshold
        self.thr64 = self.thr.double()
        z = lambda d: torch.zeros(E, dtype=d, device="cuda:0")
        self.ret, self.length, self.path, self.dsteps = z(torch.float64), z(torch.int32), z(torch.float64), z(torch.int32)
        self.clear = torch.full((E,), float("inf"), dtype=torch.float64, device="cuda:0")
        self.ep = {k: z(d) for k, d in (("r", torch.float64), ("l", torch.int32), ("path_length", torch.float64),
                                        ("min_clearance", torch.float64), ("discomfort_steps", torch.int32), ("outcome", torch.uint8))}
        self.totals = torch.zeros(5, dtype=torch.int64, device="cuda:0")
        self.inf = torch.full((), float("inf"), dtype=torch.float64, device="cuda:0")

    def update(self, obs, reward, done, info):
        B, S = self.B, self.S
        o, f = obs["observation"], info["final_observation"]["observation"]
        lo, hi = (S - 1) * B, S * B
        scan = torch.where(done[:, None], f[:, lo:hi], o[:, lo:hi])
        tail = torch.where(done[:, None], f[:, hi:hi + 4], o[:, hi:hi + 4]).double()
        self.length += 1
        self.ret += reward
        self.path += torch.hypot(tail[:, 2] - tail[:, 0], tail[:, 3] - tail[:, 1])
        self.clear = torch.minimum(self.clear, (scan.double() - self.thr64).amin(dim=1))
        crash_row = (scan < self.thr).any(dim=1)
        self.dsteps += ((scan < self.dthr).any(dim=1) & ~crash_row).to(torch.int32)
        succ, crash = info["is_success"] != 0, info["is_crash"] != 0
        outcome = succ.to(torch.uint8) | (crash.to(torch.uint8) << 1)
        if "TimeLimit.truncated" in info:
            outcome = outcome | (info["TimeLimit.truncated"].to(torch.uint8) << 2)
        for k, v in (("r", self.ret), ("l", self.length), ("path_length", self.path), ("min_clearance", self.clear),
                     ("discomfort_steps", self.dsteps), ("outcome", outcome)):
            self.ep[k] = torch.where(done, v, self.ep[k])
        limit = (outcome & 4) != 0
        self.totals[:4] += torch.stack([done, done & succ, done & crash, done & limit]).sum(dim=1)
        self.totals[4] += (self.length * done).sum()
        keep = ~done
        self.ret *= keep; self.length *= keep; self.path *= keep; self.dsteps *= keep
        self.clear = torch.where(done, self.inf, self.clear)
        return self.ep


envs = {"off": nav_gym_env.make("NavGym-v0", **kw), "on": nav_gym_env.make("NavGym-v0", episode_stats=True, **kw),
        "torch": nav_gym_env.make("NavGym-v0", **kw)}
for env in envs.values():
    env.reset()
composed = TorchStats(envs["torch"])


def run(name, n, k0):
    env = envs[name]
    if name == "torch":
        for t in range(n):
            obs, reward, done, info = env.step(acts[(k0 + t) % 64])
            info["episode"] = composed.update(obs, reward, done, info)
    else:
        for t in range(n):
            env.step(acts[(k0 + t) % 64])


for name in envs:                                            # warm-up: every variant, every shape
    run(name, 30, 0)
torch.cuda.synchronize()


class CountOps(torch.utils._python_dispatch.TorchDispatchMode):
    """How many aten operations one update of the torch composition dispatches (views and slices included)."""

    def __init__(self):
        super().__init__()
        self.n, self.names = 0, collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        self.names[str(func).split(".")[1]] += 1
        return func(*args, **(kwargs or {}))


obs, reward, done, info = envs["torch"].step(acts[30])
with CountOps() as ops:
    composed.update(obs, reward, done, info)
envs["on"].step(acts[30]); envs["off"].step(acts[30])        # (the three stay on the same rollout)
VIEWS = ("slice", "select", "unsqueeze", "view", "expand", "alias", "detach", "as_strided", "_unsafe_view", "t")
launching = sum(n for k, n in ops.names.items() if k not in VIEWS)
# the two forms agree on what they count (the totals; the torch form's path length goes through hypot, so rows may differ in the last bit)
on, tt = envs["on"].episode_totals(reset=False), composed.totals.cpu().numpy()
assert [on[k] for k in ("episodes", "successes", "crashes", "time_limits", "steps")] == tt.tolist(), (on, tt)
times = {name: [] for name in envs}
k0 = 31
for r in range(reps):
    for name in envs:                                        # alternating: the three share whatever else the machine does
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(name, window, k0)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / window)
    k0 += window
lines = ["NavGymEnv.step() on the c2-shaped world, %d arenas, %d windows of %d steps per variant, variants alternating in one process"
         % (E, reps, window),
         "(host clock around a window that ends in a device synchronise; us per step, M env-steps/s from the median)"]
base = np.median(times["off"])
for name in envs:
    t = np.array(times[name]) * 1e6
    lines.append("  %-6s median %7.1f us  min %7.1f  max %7.1f   %6.2f M env-steps/s   x %.3f of off   (+%.1f us)"
                 % (name, np.median(t), t.min(), t.max(), E / np.median(t), np.median(t) / (base * 1e6), np.median(t) - base * 1e6))
lines.append("  episode totals of `on` after the run: %s" % envs["on"].episode_totals(reset=False))
lines.append("  the torch composition dispatches %d aten operations per step, %d of them other than views / slices: %s"
             % (ops.n, launching, ", ".join("%s x%d" % kv for kv in sorted(ops.names.items(), key=lambda kv: -kv[1]))))
lines.append("  (it computes ALL the quantities of info['episode'] and the totals, with two [E, B] selections between the row and the")
lines.append("   terminal row; return, length, success and crash alone would be about a dozen operations -- at the 3-5 us of host time an")
lines.append("   operation costs here, still several times the +%.1f us of `on`)" % (np.median(times["on"]) * 1e6 - base * 1e6))
on_us, torch_us = np.median(times["on"]) * 1e6, np.median(times["torch"]) * 1e6
lines.append("  required: `on` faster than the torch composition -- %.1f us < %.1f us: %s" % (on_us, torch_us, "yes" if on_us < torch_us else "NO"))
text = "\n".join(lines) + "\n"
print(text)
with open(os.path.join(OUT, "summary.txt"), "w") as f:
    f.write(text)
for env in envs.values():
    env.close()
assert on_us < torch_us, "episode_stats=True is not faster than the torch composition"
