"""The reference's README usage loop (README.md:47-55) on this build, then the same loop batched.

    python examples/usage.py            # needs a MI355X; there is no CPU fallback
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nav-gym_amd"))
import nav_gym_env  # noqa: E402  registers 'NavGym-v0'

# ---- exactly the reference's loop ---------------------------------------------------------------------
env = nav_gym_env.make("NavGym-v0")
obs = env.reset()
done, steps = False, 0
while not done and steps < 200:
    action = env.action_space.sample()            # your agent code here
    obs, reward, done, info = env.step(action)
    steps += 1
print("single arena: %d steps, last reward %.3f, info %s" % (steps, reward, info))
img = env.render(mode="rgb_array")                # env.py:833-1050: float32 BGR [800, 800, 3] (no window here)
print("render:", img.shape, img.dtype)

# ---- 4096 arenas per call --------------------------------------------------------------------------------
import torch  # noqa: E402

E = 4096
benv = nav_gym_env.make("NavGym-v0", num_envs=E, n_beams=1081, map_size=500, pedestrian_model="sfm", num_humans=10,
                        episode_stats=True)       # info['episode'] / episode_totals(): kept on the device, one launch per step
# (pedestrian_model="orca", orca_params=dict(max_obst_rects=8, time_horizon_obst=2.0): ORCA pedestrians that also avoid walls)
obs = benv.reset()
actions = torch.rand((E, 2), dtype=torch.float64, device="cuda:0")
actions[:, 0] *= 0.5
actions[:, 1] = actions[:, 1] * 1.28 - 0.64
for _ in range(20):
    benv.step(actions)
torch.cuda.synchronize()
benv.episode_totals()                                 # (reset=True: count from here)
t0 = time.perf_counter()
n = 200
finished = 0
returns = torch.zeros((), dtype=torch.float64, device="cuda:0")
for _ in range(n):
    obs, reward, done, info = benv.step(actions)      # your batched agent here
    finished += done.sum()
    returns += (info["episode"]["r"] * info["_episode"]).sum()      # rows of the arenas that finished in this step
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d arenas: %.2f M env-steps/s, %d episodes finished, observation %s on %s"
      % (E, E * n / dt / 1e6, int(finished), tuple(obs["observation"].shape), obs["observation"].device))
totals = benv.episode_totals()                        # the only device -> host copy of the statistics
print("episodes %d: success rate %.3f, crash rate %.3f, mean return %.3f, mean length %.1f"
      % (totals["episodes"], totals["successes"] / max(totals["episodes"], 1), totals["crashes"] / max(totals["episodes"], 1),
         float(returns) / max(totals["episodes"], 1), totals["steps"] / max(totals["episodes"], 1)))

# ---- the reference's own world, batched: every registered default, a new map at every episode end ----------
# (512 beams, 1000 x 1000 corridor / 400 x 400 outdoor maps, 5-15 pedestrians on planned routes).  For such worlds the
# env stages every arena's next world ahead of time on a side stream (pregen_pipeline=8 by default: the same rollout
# as pregen_pipeline=0, bit for bit, about 2.4 x the throughput); env.counters() says how many arenas were served.
E = 1024
renv = nav_gym_env.make("NavGym-v0", num_envs=E, map_size="reference", randomize_maps=True)
renv.reset()
actions = actions[:E].contiguous()
for _ in range(20):
    renv.step(actions)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(100):
    obs, reward, done, info = renv.step(actions)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("reference defaults, %d arenas: %.2f M env-steps/s (pregen_pipeline=%d); %s" % (E, E * 100 / dt / 1e6, renv.pregen_pipeline, renv.counters()))

# ---- the path to the goal on that world: its corridors make the straight line point through walls ---------------------------
# goal_path=True keeps a distance-to-goal field per arena on the device (rebuilt whenever an arena gets a new goal or map) and
# returns, two launches behind the step, the PATH distance and a sub-goal 2 m down the path in the robot's frame.
genv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size="reference", randomize_maps=True, goal_path=True)
genv.reset()
obs, reward, done, info = genv.step(actions[:64].contiguous())
g = info["goal_path"]
for e in range(4):
    print("arena %d: straight line %.2f m, path %.2f m, sub-goal (%.2f, %.2f) m in the robot's frame, status %d"
          % (e, float(info["distance"][e]), float(g["distance"][e]), float(g["subgoal"][e, 0]), float(g["subgoal"][e, 1]), int(g["status"][e])))
print("fields rebuilt so far: %d" % genv.sim.goal_path_rebuilds())

# ---- a baseline controller on the same batch: the dynamic-window local planner ------------------------------------------------
# local_planner='dwa' returns, one launch behind the step (and behind the goal path, whose sub-goal it then steers for), the
# action a classical planner would take in every arena: candidates around the last twist rolled out against the arena's distance
# field and its pedestrians.  Feeding it back drives the batch without a policy.
penv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, indoor_ratio=0.0, min_goal_dist=3.0, max_goal_dist=8.0,
                        goal_path=True, local_planner="dwa")
penv.reset()
plan = penv.planner_action()                               # valid after reset() too
successes = crashes = 0
for _ in range(150):
    obs, reward, done, info = penv.step(plan["action"])    # a float64 [E,2] tensor on the device, read in place
    successes += int(((info["is_success"] > 0) & done).sum())
    crashes += int(((info["is_crash"] > 0) & done).sum())
    plan = info["planner"]
print("planner-driven, 64 arenas x 150 steps: %d successes, %d crashes; now %d arenas blocked, clearance of arena 0 %.2f m"
      % (successes, crashes, int((plan["status"] == 2).sum()), float(plan["clearance"][0])))

# ---- a safety shield: try K candidate actions before committing to one ---------------------------------------------------------
# lookahead=K evaluates K candidate actions per arena in one launch that only reads the state: what step() would return for each.
senv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, lookahead=4)
senv.reset()
for _ in range(50):
    cand = torch.cat([actions[:256].reshape(64, 4, 2)[:, :3], torch.zeros(64, 1, 2, dtype=torch.float64, device="cuda:0")], dim=1).contiguous()
    safe = (senv.lookahead(cand)["is_crash"] == 0).to(torch.uint8).argmax(dim=1)         # the first candidate that does not crash
    obs, reward, done, info = senv.step(cand[torch.arange(64, device="cuda:0"), safe].contiguous())
print("shielded, 64 arenas x 50 steps: %d crashes in the last step" % int((info["is_crash"] > 0).sum()))

# ---- a one-step TD target over K actions: r + gamma * max_a' V(obs') with obs' from the exact model -------------------------------
# lookahead_obs=K returns the WHOLE return of step() per candidate -- the observation too, with the scan noise the step will draw.
qenv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, lookahead_obs=4)
qenv.reset()
value = lambda rows: -rows[..., -7:-5].sub(rows[..., -5:-3]).norm(dim=-1)                # a stand-in for a learned V(obs): minus the last move
cand = actions[:256].reshape(64, 4, 2).contiguous()
nxt = qenv.lookahead_obs(cand)                                                           # 'observation' {'observation' [E,K,D], ...}, 'reward', 'done', ...
target = nxt["reward"] + 0.99 * value(nxt["observation"]["observation"]).double() * (~nxt["done"])
obs, reward, done, info = qenv.step(cand[torch.arange(64, device="cuda:0"), target.argmax(dim=1)].contiguous())
print("TD targets, 64 arenas x 4 actions: best target of arena 0 %.3f, the step's reward for it %.3f" % (float(target[0].max()), float(reward[0])))

# ---- random shooting: roll K action sequences H steps ahead, execute the first action of the best one --------------------------------
# rollout=K evaluates K sequences per arena over the next H steps in one launch that only reads the state: what step() would return.
renv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, rollout=8, rollout_params=dict(horizon=6))
renv.reset()
for _ in range(50):
    seq = torch.rand(64, 8, 6, 2, dtype=torch.float64, device="cuda:0") * torch.tensor([0.5, 1.28], device="cuda:0") - torch.tensor([0.0, 0.64], device="cuda:0")
    seq[:, -1] = 0.0                                                                     # standing still is always on offer
    out = renv.rollout(seq)                                                            # 'ret' [E,K], 'outcome' [E,K] (bit 1: crash), ...
    best = torch.where((out["outcome"] & 2) == 0, out["ret"], torch.full_like(out["ret"], -1e300)).argmax(dim=1)
    obs, reward, done, info = renv.step(seq[torch.arange(64, device="cuda:0"), best, 0].contiguous())
print("random shooting, 64 arenas x 50 steps: %d crashes in the last step" % int((info["is_crash"] > 0).sum()))

# ---- MPPI: the planner on top of the rollout, all on the device -------------------------------------------------------------------
# local_planner='mppi' keeps a plan per arena, samples K sequences around it, rolls them out with the step's own arithmetic and
# takes the weighted mean; with goal_path=True the cost's distance follows the goal field around the walls.
menv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, goal_path=True, local_planner="mppi")
menv.reset()
reached = torch.zeros(64, dtype=torch.bool, device="cuda:0")
for _ in range(100):
    plan = menv.planner_action()                                                       # valid after reset() too
    obs, reward, done, info = menv.step(plan["action"].clone())
    reached |= info["is_success"] > 0
print("MPPI, 64 arenas x 100 steps: %d reached a goal, %d crashes in the last step, mean effective sample size %.1f"
      % (int(reached.sum()), int((info["is_crash"] > 0).sum()), float(info["planner"]["ess"].mean())))

# ---- pedestrian forecast: where the crowd will be over the next H steps ---------------------------------------------------------------
# ped_forecast=H puts every pedestrian's next H poses into info['ped_forecast'], time-major [E,H,N,...], from one launch behind the
# step: the step's own pedestrian model (model='true', bit-equal to the next steps up to 'exact_steps') or the constant-velocity
# baseline (model='const_vel'); 'rel' is the position in the robot's current frame, 'min_dist' the predicted closest approach.
fenv = nav_gym_env.make("NavGym-v0", num_envs=64, map_size=400, num_humans=8, ped_forecast=8, observe_humans=4)
fenv.reset()
for _ in range(20):
    obs, reward, done, info = fenv.step(actions[:64].contiguous())
f = info["ped_forecast"]                                                               # = fenv.ped_forecast()
near = f["min_dist"].min(dim=1).values                                                 # +inf in an arena without pedestrians
print("forecast, 64 arenas: closest predicted approach within 1.6 s %.2f m; futures of the observed pedestrians %s; a query with "
      "the robot standing still: %s" % (float(near.min()), tuple(f["humans_rel"].shape),
                                        tuple(fenv.ped_forecast(actions=torch.zeros(8, 2, dtype=torch.float64))["pose"].shape)))
