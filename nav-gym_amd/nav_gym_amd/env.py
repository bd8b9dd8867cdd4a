"""NavGymEnv: the reference's gym.Env API (nav_gym_env/env.py:30-831) over E batched arenas.

Same constructor keywords as the registered NavGym-v0 (nav_gym_env/__init__.py:6-38), same methods
(reset, step, compute_reward(s), compute_terminals, compute_done, compute_info,
_override_reward_factor), same observation dict keys and layout.  Build additions are keyword-only
and default to the reference's behaviour for num_envs == 1:

    num_envs        arenas stepped per call (leading axis of every returned array)
    n_beams, lidar  lidar geometry (default: KetiRobot's 512 beams over 2*pi)
    map_size        cells per side of every arena (default 400, the reference's outdoor size)
    randomize_maps  True: an arena that finishes an episode restarts on a NEW random outdoor map,
                    generated on the device inside step() (navsim_regen); False: it respawns in place
    plan_paths      True (default): pedestrians follow the waypoints of planned shortest paths and re-plan
                    at their goal (env.py:667-680, 788-804; navsim_replan after every step); with
                    randomize_maps new starts / goals are sampled on the costmap and kept only when the
                    planner joins them (env.py:342-383, 756-762).  False: straight-line goals.
                    Maps above 1000 cells per side fall back to False (the search lives in LDS).
    pedestrian_model 'policy' (the reference's HumanPolicy actor on the device, env.py:617-662; needs
                    policy_weights = the state_dict of human_policy.pth, a path to it, or a dict of arrays),
                    'sfm' (build-defined social force), 'orca' (build-defined: reciprocal velocity obstacles among the
                    arena's pedestrians and the robot toward the current waypoint, NavSim.ped_orca in front of every step;
                    orca_params = dict overriding sim.ped_orca_defaults, unknown keys raise ValueError; with the default
                    max_obst_rects = 0 static obstacles are not ORCA obstacles, max_obst_rects = K in 1 .. 32 makes every
                    pedestrian avoid the K nearest LISTED rectangles of its arena (NavSim.ped_orca_walls: the border ring and
                    the boxes of outdoor maps, within time_horizon_obst * v_pref + radius; needs the packed field's rect
                    records -- a world without them raises ValueError at construction; set time_horizon_obst = 2 or less
                    with it: the pinned default of 5 s puts more rectangles in range than are kept and is the setting
                    DESIGN.md section 5 lists as NOT bounded);
                    ordered like 'policy': no graphs, no pregen_pipeline), 'external' (caller
                    supplies (v, w) per pedestrian -- the slot the reference fills with HumanPolicy) or 'none'
    action_kind     'twist' (default): action = (v, omega) like the reference (env.py:591); 'wheels': action = the
                    angular speeds (left, right) of a skid-steer base's wheel pairs in rad/s, converted on the device
                    with the robot's wheel radius / track (robots.py; Husky: husky.urdf.xacro:61-67)
    clip_actions    True: the twist is clamped to linvel_range x rotvel_range on the device (the reference only prints
                    a warning and never clips, env.py:606-613: default False)
    regen_min_steps, pregen_pipeline   (randomize_maps) pregen_pipeline = P > 0 (default: 4; for worlds of corridor maps with
                    planned starts the passes alternate between two side streams; 0 where the pipeline is not available): the next world of every arena is staged ahead
                    of time on a side stream (a pass every P steps) and installed inside the step's own launch.  With
                    regen_min_steps = 0 (default) the rollout is EXACTLY the one without the pipeline: an arena that finishes
                    before its world is staged is generated on the spot (counters()['regen_late']).  regen_min_steps >= 4 P
                    drops that fallback's launches (fastest): an episode shorter than regen_min_steps restarts on its old map,
                    which the reference never does (it draws a map at every reset) -- counted in counters()['regen_short'].
                    The on-the-spot fallback serves at most max(8, num_envs // 128) arenas per step: more late arenas than
                    that in ONE step keep their old map for the next episode and are counted in counters()['regen_unserved']
                    (not seen in the soaks of profiles/r05_pipe/: a pass every P steps leaves a handful of late arenas per step)
    pregen_fallback_poll   (pregen_pipeline, regen_min_steps < 4 P) True: step() reads one byte back from the device -- "did this step
                    leave an arena without its staged world?" -- and launches the on-the-spot generation only then, instead of
                    enqueueing its launches blind behind every step.  A host wait per step; default (None): on for worlds of
                    corridor maps or planned starts, whose fallback is ~18 launches (the reference's configuration: 2.74 -> 3.25 M env-steps/s at 1024 arenas, 3.74 -> 4.07 M at 4096),
                    off otherwise.  Same rollout either way.
    use_graphs      replay a step's launches (navsim_step, navsim_regen, navsim_replan) as one captured hipGraph; None
                    (default) = when randomize_maps makes a step several launches (c5: +6 %) and navsim_regen does not fork
                    (corridor maps with planned starts: plain launches are as fast or faster); results are identical
    max_waypoints   waypoints kept per pedestrian route (default 64 = 128 m at the 2 m interval; the reference keeps
                    all of them, env.py:788-804); longer routes are stored cut, counted, and continued to the same goal
    device, seed, env_index_base (global index of arena 0: sharding), auto_reset, field_format
    autoreset_mode  (auto_reset) 'same_step' (default): the step() that ends an arena's episode also restarts it -- the returned
                    observation row is the FIRST of the new episode, and the observation the reference's step() returns with
                    done = True (env.py:700-728: the last one of the episode, after a crash the re-scan at the reverted pose)
                    is info['final_observation'] (same keys as the observation dict; rows where info['final_mask'] = done);
                    'next_step' (gymnasium's next-step mode): step() returns that terminal observation itself, like the
                    reference, and the arena is reset by the NEXT step() -- its action is ignored, reward 0, done False, the
                    observation is the new episode's first one, info['reset_mask'] marks it.  final_observation=False drops
                    the terminal rows of 'same_step' (and their second scan after a crash).
    max_episode_steps  time limit T (old gym's TimeLimit, per arena, decided inside the fused step): an episode that reaches
                    T steps without success or crash ends with done = True and info['TimeLimit.truncated'] = True (reward
                    and the other info keys are the step's own; success or crash at step T wins, truncated False).  It then
                    restarts like any finished arena under auto_reset -- same_step: info['final_observation'] holds its
                    terminal row; next_step: the next step() resets it (info['reset_mask']).  Without auto_reset an arena
                    stepped past T stays truncated until reset().  info['TimeLimit.truncated'] is a bool (num_envs == 1)
                    or a torch.bool [num_envs] view; None (default): no limit, the reference's behaviour and no such key.
    episode_stats   True: step() keeps every arena's episode statistics on the device, one launch behind the step
                    (navsim_episode_stats_update; gymnasium's RecordEpisodeStatistics) -- info['episode'] = {'r' return, 'l'
                    length, 'path_length' metres, 'min_clearance' smallest scan - scan_threshold of the episode, 'discomfort_steps',
                    'outcome' bit 0 success, bit 1 crash, bit 2 time limit}.  num_envs > 1: torch views [num_envs], rows valid
                    where info['_episode'] (= done) is set, with the lifetime below; num_envs == 1: Python scalars, only in the
                    step that ends the episode.  The terminal step counts (same_step: its row is info['final_observation'], so
                    final_observation=False raises ValueError), the step in which next_step RESETS an arena does not, and
                    reset() / reset(mask) start the arenas' statistics afresh.  With auto_reset=False the caller resets
                    finished arenas (reset(mask=done)) before their next step: an arena stepped on past its `done` may keep the
                    flag, and every such step would count as an episode of one step.  env.episode_totals() reads the running totals
                    -- the only device -> host copy, and only when called.  False (default): nothing is launched.
    observe_humans  K (1 .. the world's pedestrian cap): the K nearest pedestrians the robot has in line of sight, one launch behind
                    the step (navsim_ped_observe; the list SARL / CADRL-style policies take) -- info['humans'] = {'state' [E,K,5]
                    x, y, vx, vy in the robot's frame and the distance d, nearest first; 'index' [E,K] the pedestrian of the row,
                    -1 = unused row; 'count' [E] pedestrians seen, which may exceed K; 'visible' [E,N] bool}.  A pedestrian is
                    seen when it is within sensor_range, inside the lidar's field of view and one of `rays` lines of sight (its
                    centre, its two silhouette points) crosses no wall of the arena's map; other pedestrians do not occlude.
                    observe_params overrides ped_radius, sensor_range, rays (1 | 3), occlusion, fov.  The rows describe the state
                    the returned observation row describes: after a same-step restart the new episode's first state
                    (info['final_observation'] carries no humans: a terminal copy is a follow-up); under next-step auto-reset
                    an arena whose `done` is set has restarted already, and its rows are empty (count 0, index -1) until the
                    step that resets it.  env.observed_humans() returns the same dict, also after reset() / reset(mask).
                    num_envs > 1: torch views with the lifetime below; num_envs == 1: NumPy arrays without the leading axis,
                    from one device -> host copy.  Needs a pedestrian model; None (default): nothing is allocated or launched.
    goal_path       True: a distance-to-goal field per arena on the 5 x 5-cell navigation grid (the costmap's cells), rebuilt on the
                    device whenever the arena gets a new goal or map, and from it the robot's PATH distance and a steering
                    sub-goal -- two launches behind the step (navsim_goal_path), no copy: info['goal_path'] = {'distance' [E]
                    metres along the cheapest path that keeps its clearance from the walls (info['distance'] is the straight
                    line, which points through them); 'subgoal' [E,2] a point `lookahead` metres down that path, in the robot's
                    frame -- the goal itself once it is that near; 'status' [E] uint8: 1 on the field, 3 = the sub-goal is the
                    goal, 4 = the robot stands on no passable cell and the values are the straight line's, 0 = skipped}.
                    goal_path_params overrides hard_clearance (0.3 m), clearance (0.75 m), band_cost (3), lookahead (2.0 m).  The
                    row describes the state the returned observation row describes: after a SAME-STEP restart that is the NEW
                    episode (new goal, new field) -- a reward shaper masks its progress term with `done`; under next-step
                    auto-reset an arena whose `done` is set has restarted already and its row is skipped (all 0) until the step
                    that resets it.  env.goal_path() returns the same dict, also after reset() / reset(mask); env.goal_field() the
                    uint16 [E, H/5, W/5] fields on the device.  num_envs > 1: torch views with the lifetime below; num_envs == 1:
                    NumPy scalars and arrays from one device -> host copy.  False (default): nothing is allocated or launched.
    local_planner   'dwa': a dynamic-window local planner on the device, one launch behind the step (navsim_dwa; behind
                    navsim_goal_path with goal_path=True, whose sub-goal is then its target -- otherwise the goal itself): every
                    arena forms a window of twists it can reach from the twist of its last step, rolls each candidate out with the
                    step's kinematics against its distance field (two discs over the threshold footprint) and its pedestrians
                    (moved at constant velocity), and picks the admissible candidate with the best score --
                    info['planner'] = {'action' [E,2] float64 in action_kind's form: feed it to the next step(); 'twist' [E,2] the
                    same as (v, omega); 'clearance' [E] metres; 'best' [E] the candidate's index; 'status' [E] uint8: 1 = ok, 2 =
                    blocked (no admissible candidate: the one that violates the margin last), 0 = skipped}.  A classical baseline
                    on the same batch: a number to beat, an expert for demonstrations, a check that an arena is solvable.
                    local_planner_params overrides sim.dwa_defaults (acc_lin, acc_rot, body_radius, body_offset, ped_radius,
                    margin, clearance_cap, the four weights, n_v, n_w, horizon, use_peds).  The row describes the state the returned
                    observation row describes; under next-step auto-reset an arena whose `done` is set is skipped (all 0) until
                    the step that resets it.  env.planner_action() returns the same dict, also after reset() / reset(mask).
                    num_envs > 1: torch views with the lifetime below; num_envs == 1: NumPy values from one device -> host copy.
                    None (default): nothing is allocated or launched.
                    'mppi': a sampling-based model-predictive controller on the device (navsim_mppi, 3 launches per iteration
                    behind the step and behind navsim_goal_path): every arena keeps a plan of H actions, perturbs it K times with
                    time-correlated Gaussian noise, evaluates the sequences with the STEP'S OWN arithmetic (navsim_rollout: the
                    scan-based crash test, the social force per sequence), weights them by exp(-cost / lam) and takes the
                    weighted mean as its new plan; the plan is shifted by one action from step to step and starts afresh when
                    the arena's (episode, steps) say it restarted.  cost = w_goal x the distance to the goal at the horizon's
                    end -- along the goal field with goal_path=True, else the straight line -- minus the rollout's return,
                    + w_crash for a crash.  info['planner'] = {'action' [E,2] float64: feed it to the next step(); 'best' [E]
                    the best sequence, one that did not crash whenever there is one; 'cost_best' [E]; 'ess' [E] the effective
                    sample size; 'status' [E] uint8: 1 = ok, 2 = every sequence crashed, 0 = skipped}.  local_planner_params
                    overrides sim.mppi_defaults: n_samples (32), horizon (24), iterations (1), sigma, lam, beta, w_goal, w_crash,
                    off_field_cost, stop_sample, select ('mean': the new plan's first action, 'best': the best sequence's),
                    range, gamma, init_action; the action box is action_space.  env.planner_plan() returns the plans [E,H,2].
                    Not with pedestrian_model 'orca' or 'policy'; 'external': the state's own commands are held.
    observe_local_map  G (1 .. 128): an egocentric grid map per arena, one launch behind the step (navsim_local_map; what a CNN
                    policy over a local costmap or a DRL-VO style pedestrian map reads) -- info['local_map'] = float32
                    [E, C, G, G] in the robot's frame, row r counting forward along the body's x axis and column q to its left,
                    the window's centre `ahead` metres in front of the pose origin: channel 0 the clearance to the walls (metres,
                    saturated at `cap`, 0 outside the map), channel 1 the clearance to the nearest pedestrian's disc, channels 2
                    and 3 the robot-frame velocity of the pedestrian that covers the cell (0 elsewhere).  local_map_params
                    overrides sim.local_map_defaults (cell 0.1 m, ahead 0, cap 2 m, ped_radius 0.3 m, channels 4 with a
                    pedestrian model and 1 without); visible_only=True (needs observe_humans) counts only the pedestrians that
                    launch found in line of sight.  The map describes the state the returned observation row describes; under
                    next-step auto-reset an arena whose `done` is set is skipped (all 0) until the step that resets it;
                    info['final_observation'] carries no map.  env.local_map() returns the same tensor, also after reset() /
                    reset(mask).  num_envs > 1: a torch tensor with the lifetime below; num_envs == 1: a NumPy array [C, G, G]
                    from one device -> host copy.  None (default): nothing is allocated or launched.
    scan_labels     True: the ground truth of the lidar, one launch behind the step (navsim_scan_labels; what a 2D-lidar person or
                    leg detector, a tracker, a policy that masks pedestrian returns or a scan denoiser trains on) --
                    info['scan_labels'] = {'range' [E,B] float32, the robot's scan of the current state WITHOUT noise; 'label'
                    [E,B] uint8, abi.BEAM_NONE 0 (no return: range == range_max) / BEAM_WALL 1 / BEAM_PED_BODY 2 / BEAM_PED_LEG 3;
                    'index' [E,B] int8, the pedestrian a beam of label 2 or 3 fell on, else -1; 'hits' [E,N] int32, the beams
                    that see each pedestrian (only with a pedestrian model)}.  With scan noise off, 'range' equals the newest
                    scan slot of the observation bit for bit; with noise on the two differ by the noise alone, and only where
                    label != 0.  The rows describe the state the returned observation row describes; under next-step auto-reset
                    an arena whose `done` is set is skipped (range 0, label 0, index -1, hits 0) until the step that resets it.
                    env.scan_labels() returns the same dict, also after reset() / reset(mask).  num_envs > 1: torch views with
                    the lifetime below; num_envs == 1: NumPy rows from one device -> host copy.  False (default): nothing is
                    allocated or launched.
    lookahead       K in 1 .. 64: env.lookahead(actions) returns what step() would return for each of K candidate actions per
                    arena -- reward, done, is_success, is_crash, discomfort, distance, the crash margin and the pose -- from one
                    launch that only reads the state (navsim_lookahead): what a safety shield, an action mask or a one-step
                    Q-target asks.  With scan noise off the five values step() also returns are bit-identical to that step's.
                    lookahead_params: dict(range=), the candidates' scan cap in metres (default: the smallest multiple of 0.25 m
                    that lies 0.1 m above the largest discomfort threshold).  Not with pedestrian_model 'orca' or 'policy', whose
                    commands come from a launch in front of the step.  None (default): nothing is allocated or launched.
    lookahead_obs   K in 1 .. 64: env.lookahead_obs(actions) returns the WHOLE return of step() for each of K candidate actions per
                    arena -- lookahead()'s values plus the observation {'observation' [E,K,D], 'achieved_goal', 'desired_goal'
                    [E,K,2]}, 'scan' [E,K,B] (the row's newest slot), 'tail' [E,K,7] and 'truncated' [E,K] -- from one launch that
                    only reads the state (navsim_lookahead_obs): the obs' of a one-step target r + gamma V(obs'), of a full-action
                    backup or of a safety critic.  With scan noise on it draws the noise the step itself will draw, so row, goals,
                    reward, done, truncated and flags are bit-identical to the step's, noise on or off; a candidate that crashes
                    carries the reference's re-scan from the reverted pose.  The first observation of a restarted episode is not
                    modelled: a `done` candidate holds the terminal row (final_observation).  lookahead_obs_params:
                    dict(noise='step' | 'off', rows='full' | 'scan'); rows='scan' leaves 'observation' out and saves its
                    E*K*(S*B+7)*4 bytes per set.  Independent of lookahead=.  Not with pedestrian_model 'orca' or 'policy'.  None
                    (default): nothing is allocated or launched.
    rollout         K in 1 .. 256: env.rollout(actions) returns what the next H step() calls would return if an arena executed each
                    of K action sequences -- per step reward and pose; per sequence the discounted return, the steps evaluated,
                    the outcome bits (1 success, 2 crash, 4 time limit), discomfort steps, the least crash margin, the final
                    distance and exact_steps -- from one launch that only reads the state (navsim_rollout): what random shooting,
                    MPPI, CEM, an n-step target or a multi-step shield asks.  A sequence ends at its first done step; a pedestrian
                    that reaches its last waypoint inside the horizon is not re-planned, and exact_steps says up to which step the
                    rows are the step's own, bit for bit with scan noise off (without pedestrians: the whole horizon).
                    rollout_params: dict(horizon=8, range=, gamma=1.0); range as lookahead_params'.  Not with pedestrian_model
                    'orca' or 'policy'.  None (default): nothing is allocated or launched.
    rollout_obs     K in 1 .. 256: env.rollout_obs(actions) returns the WHOLE return of the next H step() calls for each of K action
                    sequences per arena -- rollout()'s values plus 'observation' {'observation' [E,K,D], 'achieved_goal',
                    'desired_goal' [E,K,2]} of every sequence's last evaluated step -- from one launch that only reads the state
                    (navsim_rollout_obs): the obs of an n-step target sum gamma^h r_h + gamma^H V(obs_H), of a learned value at
                    the leaves of a depth-H search, of terminal-value MPC.  Every step scans at the lidar's full range and draws
                    the noise that future step itself will draw, so rows, goals, rewards and outcomes below exact_steps are
                    bit-identical to the steps', noise on or off; a step that crashes ends its sequence and carries the
                    reference's re-scan from the reverted pose.  rollout_obs_params: dict(horizon=8, gamma=1.0, noise='step' |
                    'off', rows='last' | 'all'); rows='all' adds 'observations', the same three keys with an H axis
                    ([E,K,H,D], [E,K,H,2]: E*K*H*(S*B+7)*4 bytes per set; rows behind a sequence's end are 0).  Independent of
                    rollout= and lookahead_obs=.  Not with pedestrian_model 'orca' or 'policy'.  None (default): nothing is
                    allocated or launched.
    ped_forecast    H in 1 .. 32: info['ped_forecast'] holds where every pedestrian will be after each of the next H step() calls,
                    time-major -- 'pose' [E,H,N,3], 'vel' [E,H,N,2], 'rel' [E,H,N,2] (the position in the robot's CURRENT frame),
                    'robot_pose' [E,H,3] (the robot pose assumed after step h), 'min_dist' / 'min_step' [E,N] (the predicted
                    closest approach and its step), 'exact_steps' [E], 'status' [E] -- from one launch behind the step that only
                    reads the state (navsim_ped_forecast): the observation of a prediction-aware policy, the labels and the
                    constant-velocity baseline of a trajectory predictor, a risk signal.  ped_forecast_params: dict(robot='hold' |
                    'stop' | 'plan', model='true' | 'const_vel').  robot: what the robot is assumed to do -- repeat its previous
                    action, stand still, or execute the first H actions of the MPPI planner's plan (needs local_planner='mppi' with
                    a plan horizon >= H; the launch then runs behind the planner's).  model 'true': the pedestrians' own model with
                    the step's arithmetic -- the rows below exact_steps equal the next steps' states bit for bit; a pedestrian that
                    reaches its last waypoint inside the horizon is not re-planned --; 'const_vel': every pedestrian keeps its
                    velocity (exact_steps 0).  Defaults 'hold' and 'true'; with pedestrian_model 'orca' or 'policy', whose
                    commands come from a launch in front of the step, the default is 'const_vel' and 'true' raises ValueError.
                    With observe_humans=K also 'humans_rel' [E,H,K,2]: `rel` of the observed pedestrians, in info['humans']'s row
                    order.  env.ped_forecast() returns the same dict, also after reset() / reset(mask);
                    env.ped_forecast(actions=, human_actions=) is an explicit query.  None (default): nothing is allocated or
                    launched.
    reset(mask)    reset() of SOME arenas (the reference's reset() is per environment, env.py:730-831): a bool / 0-1 array
                    [num_envs]; the others keep their state and their rows.  On the pipelined reset path the masked arenas install
                    their staged worlds in one launch: the same state and rows as with pregen_pipeline=0.

`env.counters()` reports what the caps of the device-side reset path left unserved (arenas beyond regen_cap,
pedestrians beyond replan_cap, routes cut at max_waypoints) since the last call.

num_envs == 1 returns NumPy float64 arrays with the reference's shapes; num_envs > 1 returns torch
tensors on `device` (float32 observations).  Everything on the step() path runs in the HIP library;
there is no CPU fallback.

Lifetime of what step() returns (num_envs > 1): the observation dict, reward, done and info are views of device buffers
the simulator keeps in PAIRS -- they stay intact through the next step() and are overwritten by the one after
(`obs = next_obs`, `dones.append(done)` across one step are safe; keep a `.clone()` of anything needed longer).

Pickling (env.py:30, 56-78: the reference is an EzPickle): `pickle.dumps(env)` stores the constructor's keyword
arguments; the copy is a fresh environment that has not been reset().  `state_dict()` / `load_state_dict()` move the
simulation state itself.  When `gym` is importable the class is a gym.Env (`unwrapped`, `spec`, `reward_range`).
"""
import collections
import numbers
import operator
import warnings

import numpy as np

from . import abi, robots, world
from .registry import HAVE_GYM, spaces

if HAVE_GYM:                                # the reference's base class (env.py:30), when the package is there
    import gym as _gym
    _EnvBase = _gym.Env
else:
    class _EnvBase(object):                 # what wrappers read of a gym.Env
        reward_range = (-float("inf"), float("inf"))
        spec = None

        @property
        def unwrapped(self):
            return self

        def seed(self, seed=None):
            return [seed]

        def __enter__(self):
            return self

        def __exit__(self, *args):
            self.close()
            return False

DEFAULT_KWARGS = {                       # nav_gym_env/__init__.py:6-38
    'robot_type': 'keti',
    'time_step': 0.2,
    'min_turning_radius': 0,
    'distance_threshold': 0.5,
    'num_scan_stack': 1,
    'linvel_range': [0, 0.5],
    'rotvel_range': [-0.64, 0.64],
    'human_v_pref_range': [0., 0.6],
    'human_has_legs_ratio': 0.5,
    'indoor_ratio': 0.5,
    'min_goal_dist': 10,
    'max_goal_dist': 20,
    'reward_scale': 15.,
    'reward_success_factor': 1,
    'reward_crash_factor': 1,
    'reward_progress_factor': 0.001,
    'reward_forward_factor': 0.0,
    'reward_rotation_factor': 0.005,
    'reward_discomfort_factor': 0.01,
    'env_param_range': dict(
        num_humans=([5, 15], 'int'),
        corridor_width=([3, 4], 'int'),
        iterations=([80, 150], 'int'),
        obstacle_number=([10, 10], 'int'),
        obstacle_width=([0.3, 1.0], 'float'),
        scan_noise_std=([0., 0.05], 'float'),
    ),
}


# one launch behind the step as NavGymEnv runs it: the key in info, the record in NavSim.products, the bound method that makes the
# call (skip, rebuild), the arrays handed out and, where the rows need more than that, what finishes them
_Product = collections.namedtuple("_Product", "key record launch keys finish")


def _check_params(name, params, on, needs, known, hint=""):
    """A feature's dict of overrides (the constructor argument `name`) asks for the feature (`on`; `needs` is how to ask for
    it) and holds `known` keys only."""
    if params is not None and not on:
        raise ValueError("%s needs %s" % (name, needs))
    for k in (params or {}):
        if k not in known:
            raise ValueError("unknown key %r in %s (known: %s%s)" % (k, name, ", ".join(known), hint))


class _AgentView(object):
    """Read-only view of one agent of arena 0 with the attribute names RosEnv reads
    (ros_env.py:83-176): px, py, theta, vx, vy, footprint, ..."""

    def __init__(self, env, kind, index=0):
        self._env, self._kind, self._i = env, kind, index
        spec = robots.ROBOTS[env.robot_type] if kind == "robot" else robots.HUMAN
        for k, v in spec.items():
            setattr(self, k, v)

    def _pose(self):
        t = self._env.sim.t
        p = t["robot_pose"][0] if self._kind == "robot" else t["ped_pose"][0, self._i]
        return p.cpu().numpy()

    px = property(lambda s: float(s._pose()[0]))
    py = property(lambda s: float(s._pose()[1]))
    theta = property(lambda s: float(s._pose()[2]))

    @property
    def vx(self):
        return float(self._env.sim.t["ped_vel"][0, self._i, 0]) if self._kind != "robot" else 0.0

    @property
    def vy(self):
        return float(self._env.sim.t["ped_vel"][0, self._i, 1]) if self._kind != "robot" else 0.0

    @property
    def gx(self):
        return float(self._env.sim.t["robot_goal"][0, 0])

    @property
    def gy(self):
        return float(self._env.sim.t["robot_goal"][0, 1])


class NavGymEnv(_EnvBase):
    metadata = {"render.modes": ["human", "rgb_array"]}
    _warned = set()                         # fallbacks are announced once per process

    @classmethod
    def _warn_once(cls, key, text):
        if key not in cls._warned:
            cls._warned.add(key)
            warnings.warn(text, RuntimeWarning, stacklevel=3)

    def __init__(self, robot_type, time_step, min_turning_radius, distance_threshold, num_scan_stack,
                 linvel_range, rotvel_range, human_v_pref_range, human_has_legs_ratio, indoor_ratio,
                 min_goal_dist, max_goal_dist, reward_scale, reward_success_factor, reward_crash_factor,
                 reward_progress_factor, reward_forward_factor, reward_rotation_factor,
                 reward_discomfort_factor, env_param_range, *,
                 num_envs=1, n_beams=None, lidar=None, map_size=400, pedestrian_model="sfm", policy_weights=None,
                 num_humans=None, device="cuda:0", seed=0, env_index_base=0, auto_reset=None,
                 field_format=abi.FIELD_U16T, n_spawn=None, randomize_maps=False, plan_paths=True,
                 action_kind="twist", clip_actions=False, max_waypoints=64, march_rule=None, use_graphs=None,
                 regen_min_steps=0, pregen_pipeline=None, pregen_stage_cap=None, autoreset_mode="same_step",
                 final_observation=True, pregen_fallback_poll=None, max_episode_steps=None, orca_params=None,
                 episode_stats=False, observe_humans=None, observe_params=None, goal_path=False, goal_path_params=None,
                 local_planner=None, local_planner_params=None, observe_local_map=None, local_map_params=None,
                 scan_labels=False, lookahead=None, lookahead_params=None, lookahead_obs=None, lookahead_obs_params=None,
                 rollout=None, rollout_params=None, rollout_obs=None, rollout_obs_params=None,
                 ped_forecast=None, ped_forecast_params=None):
        # EzPickle (env.py:56-78): what the environment was made with -- this call's own arguments -- is what a pickle of it carries
        self._ctor_kwargs = {k: v for k, v in locals().items() if k != "self"}
        from . import lib
        if robot_type not in robots.ROBOTS:
            raise NotImplementedError(robot_type)            # env.py:772-773
        self.robot_type = robot_type
        self.time_step = time_step
        self.min_turning_radius = min_turning_radius
        self.distance_threshold = distance_threshold
        self.num_scan_stack = num_scan_stack
        self.linvel_range = linvel_range
        self.rotvel_range = rotvel_range
        self.human_v_pref_range = human_v_pref_range
        self.human_has_legs_ratio = human_has_legs_ratio
        self.indoor_ratio = indoor_ratio
        self.min_goal_dist = min_goal_dist
        self.max_goal_dist = max_goal_dist
        self.env_param_range = env_param_range
        self.num_envs = int(num_envs)
        # map_size="reference": the reference's own two sizes (map_generator.py:108-142) -- every arena is allocated at
        # 1000 x 1000 cells, a corridor episode fills it, an outdoor episode draws its 400 x 400 map in the corner
        # [0, 400)^2 (the rest is occupied: nothing behind the border wall is ever seen).  An integer: one size for both.
        self.outdoor_map_size = 0
        if map_size == "reference":
            map_size, self.outdoor_map_size = 1000, 400
        self.map_size = int(map_size)
        self.device = device
        self.seed_value = int(seed)
        self.pedestrian_model = pedestrian_model
        # 'policy' and 'orca' compute the pedestrians' commands in a launch of their own IN FRONT of the step (which then runs
        # as PED_EXTERNAL): that launch reads the routes, so the re-plan stays behind the step, and neither graphs nor the
        # pipelined reset path cover it
        self._cmd_in_front = pedestrian_model in ("policy", "orca")
        from . import sim as _simmod
        if orca_params is not None and pedestrian_model != "orca":
            raise ValueError("orca_params needs pedestrian_model='orca'")
        for k in (orca_params or {}):
            if k not in _simmod.PED_ORCA_KEYS:
                raise ValueError("unknown key %r in orca_params (known: %s)" % (k, ", ".join(_simmod.PED_ORCA_KEYS)))
        self.orca_params = None if orca_params is None else dict(orca_params)
        self._orca_struct = None
        self._orca_rects = int((orca_params or {}).get("max_obst_rects", 0)) if pedestrian_model == "orca" else 0
        if not 0 <= self._orca_rects <= 32:
            raise ValueError("orca_params['max_obst_rects'] must be in 0 .. 32, not %r" % (self._orca_rects,))
        self.auto_reset = (self.num_envs > 1) if auto_reset is None else bool(auto_reset)
        if autoreset_mode not in ("same_step", "next_step"):
            raise ValueError("autoreset_mode must be 'same_step' or 'next_step'")
        self.autoreset_mode = autoreset_mode
        if max_episode_steps is not None and not (isinstance(max_episode_steps, numbers.Integral) and
                                                  not isinstance(max_episode_steps, bool) and max_episode_steps > 0):
            raise ValueError("max_episode_steps must be None or a positive int, not %r" % (max_episode_steps,))
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)
        self.final_observation = bool(final_observation) and self.auto_reset and autoreset_mode == "same_step"
        self.episode_stats = bool(episode_stats)
        if self.episode_stats and self.auto_reset and autoreset_mode == "same_step" and not self.final_observation:
            raise ValueError("episode_stats=True under same-step auto-reset needs final_observation=True: an episode's last "
                             "step is read from its terminal row")
        self._num_humans_fixed = num_humans
        self._episode_batch = 0
        self.randomize_maps = bool(randomize_maps)
        # start / goal pairs kept per arena: what an arena restarts from IN PLACE.  A world that draws a new map per episode
        # only does that for arenas beyond cfg.regen_cap in one step -- 4 pairs there (each is planned at every reset:
        # env.py:342-383), 16 where the map stays
        if n_spawn is None:
            n_spawn = 4 if self.randomize_maps else 16
        self.replan_cap = 1024                              # pedestrians re-planned per step, at most
        self._use_graphs_arg = use_graphs
        # pregen_pipeline = P > 0 (with randomize_maps): the next world of every arena is generated ahead of time by staging
        # passes on a side stream, one every P steps, and a finished arena takes it inside the step's own launch
        # (navsim_step_install) -- navsim_regen leaves the step's critical path.  It rests on regen_min_steps >= 4 P: an
        # episode that ended after fewer steps restarts on its OLD map (the reference draws a map at every reset: opt-in).
        # None (default): the pipelined reset path wherever it is available (packed field, i.e. map_size <= 1024; not with
        # pedestrian_model='policy') -- a pass every 4 steps (a c5-shaped world through this API: 5.4 -> 7.4 M env-steps/s, with planned
        # routes 1.3 -> 3.0 M, profiles/_diag/gym_c5_steps.py); for worlds whose reset is heavy (corridor maps with planned starts, the
        # reference's own kind) the passes alternate between two side streams, each of which starts one every 8 steps
        # (profiles/r05_refdef/pipeline_sweep.txt, profiles/r06_planner/ab_stage_lanes.txt).  With regen_min_steps = 0 it changes no result: the rollout is the one of
        # pregen_pipeline=0, bit for bit.
        self._pregen_auto = pregen_pipeline is None
        if pregen_pipeline is None:
            available = (not self._cmd_in_front and field_format == abi.FIELD_U16T and
                         (map_size == "reference" or int(map_size) <= 1024))
            # (worlds of corridor maps with planned starts: a pass every 4 steps too since round 6 -- their passes alternate between
            #  two side streams, NavSim.enable_pregen stage_lanes, i.e. each stream still starts one every 8 steps)
            pregen_pipeline = 4 if available else 0
            if use_graphs:                         # (asked for: the graph replay of step + navsim_regen is the other form)
                pregen_pipeline = 0
        self.regen_min_steps = int(regen_min_steps)
        self.pregen_stage_cap = pregen_stage_cap        # arenas one staging pass serves at most (None: NavSim.enable_pregen's default)
        self.pregen_fallback_poll = pregen_fallback_poll   # None: NavSim.enable_pregen's default (on for corridor maps / planned starts)
        if self.randomize_maps and self.auto_reset and self._cmd_in_front and int(pregen_pipeline):
            raise ValueError("pregen_pipeline is not available with pedestrian_model=%r" % pedestrian_model)
        self._graphed = False
        self._overlap_replan = False
        # which sequence step() runs and what it launches behind the step (_choose_step_path, at the first reset())
        self._step_path, self._regen_behind, self._replan_behind = None, False, False
        self.plan_paths = bool(plan_paths) and int(map_size) <= 1000
        if plan_paths and not self.plan_paths:
            self._warn_once("plan_paths", "NavGymEnv: map_size %d > 1000: the planner's search lives in LDS (costmaps up to "
                            "200 x 200 cells), plan_paths falls back to False -- pedestrians head straight for their goals"
                            % int(map_size))
        if field_format == abi.FIELD_U16T and int(map_size) > 1024:
            field_format = abi.FIELD_F32     # beyond the rect records' and the packed regeneration's tested range
            self._warn_once("field_format", "NavGymEnv: map_size %d > 1024: the packed uint16 distance field and its rect "
                            "records are not used beyond 1024 cells per side, field_format falls back to FIELD_F32" % int(map_size))
        spec = robots.ROBOTS[robot_type]
        nh_hi = int(env_param_range["num_humans"][0][1]) if num_humans is None else int(num_humans)
        ped = {"none": abi.PED_NONE, "external": abi.PED_EXTERNAL, "sfm": abi.PED_SFM,
               "policy": abi.PED_EXTERNAL, "orca": abi.PED_EXTERNAL}[pedestrian_model]
        if pedestrian_model == "policy" and policy_weights is None:
            raise ValueError("pedestrian_model='policy' needs policy_weights (human_policy.pth is not shipped)")
        self._policy_weights = policy_weights
        if nh_hi == 0:
            ped = abi.PED_NONE
        cfg = lib.default_config(
            n_envs=self.num_envs, map_h=self.map_size, map_w=self.map_size, max_peds=max(nh_hi, 1),
            n_scan_stack=num_scan_stack, ped_model=ped, lidar_legs=1,
            auto_reset=(abi.AUTORESET_NONE if not self.auto_reset else
                        (abi.AUTORESET_NEXT_STEP if autoreset_mode == "next_step" else abi.AUTORESET_SAME_STEP)),
            n_spawn=n_spawn, add_scan_noise=1, env_index_base=env_index_base, field_format=field_format,
            time_step=time_step, axle_offset=spec["axle_offset"], min_turning_radius=float(min_turning_radius),
            distance_threshold=distance_threshold, range_max=spec["range_max"], seed=self.seed_value)
        # reset() -- of the whole batch and, with randomize_maps, of every finished arena -- runs on the device
        # (navsim_regen): planning on the costmap as env.py:342-383 when plan_paths, the map kind by indoor_ratio
        # (env.py:295), and the per-episode draws of env_param_range (env.py:281-292)
        if action_kind not in ("twist", "wheels"):
            raise ValueError("action_kind must be 'twist' or 'wheels'")
        self.action_kind = action_kind
        cfg.action_kind = abi.ACTION_WHEELS if action_kind == "wheels" else abi.ACTION_TWIST
        cfg.clamp_action = int(bool(clip_actions))
        cfg.linvel_lo, cfg.linvel_hi = float(linvel_range[0]), float(linvel_range[1])
        cfg.rotvel_lo, cfg.rotvel_hi = float(rotvel_range[0]), float(rotvel_range[1])
        cfg.wheel_radius = float(spec.get("wheel_radius", robots.HUSKY_WHEEL_RADIUS))
        cfg.wheel_track = float(spec.get("wheel_track", robots.HUSKY_TRACK))
        cfg.max_waypoints = int(max_waypoints)
        if march_rule is not None:                    # include/navsim.h NAVSIM_MARCH_*: the unpinned rounding of range_libc
            cfg.march_rule = int(march_rule)
        cfg.regen_min_steps = self.regen_min_steps if (self.randomize_maps and self.auto_reset) else 0
        cfg.max_episode_steps = self.max_episode_steps or 0     # (0: no limit -- the step's plain form where it has one)
        cfg.regen_plan = int(self.plan_paths)
        cfg.regen_indoor_ratio = float(indoor_ratio)
        # rect records (the march's shortcut around most field reads): always for fixed maps; with a new map per episode
        # only in worlds of outdoor maps, whose records come out of the pass that writes the new field -- corridor maps
        # would need the verified builder for a handful of maps per step, which costs more than the records save
        self._with_rects = (cfg.field_format == abi.FIELD_U16T and self.map_size <= 1024 and
                            (not self.randomize_maps or not cfg.regen_indoor_ratio > 0.0))
        if self._orca_rects and not self._with_rects:
            raise ValueError("orca_params['max_obst_rects'] > 0 needs a world with rect_index rows (the packed field, "
                             "map_size <= 1024, and with randomize_maps outdoor maps only: indoor_ratio = 0)")
        cfg.outdoor_map_size = int(self.outdoor_map_size)
        room = (self.outdoor_map_size or self.map_size) * cfg.resolution
        cfg.min_goal_dist = float(min(min_goal_dist, 0.4 * room))
        cfg.max_goal_dist = float(min(max_goal_dist, 0.8 * room))
        cfg.v_pref_lo, cfg.v_pref_hi = float(human_v_pref_range[0]), float(human_v_pref_range[1])
        cfg.has_legs_ratio = float(human_has_legs_ratio)
        epr = env_param_range
        cfg.obstacle_number, cfg.obstacle_number_hi = [int(x) for x in epr["obstacle_number"][0]]
        cfg.obstacle_width_lo, cfg.obstacle_width_hi = [float(x) for x in epr["obstacle_width"][0]]
        cfg.corridor_width_lo, cfg.corridor_width_hi = [int(x) for x in epr["corridor_width"][0]]
        cfg.iterations_lo, cfg.iterations_hi = [int(x) for x in epr["iterations"][0]]
        cfg.scan_noise_std_lo, cfg.scan_noise_std_hi = [float(x) for x in epr["scan_noise_std"][0]]
        if num_humans is None:
            cfg.num_humans_lo, cfg.num_humans_hi = [int(x) for x in epr["num_humans"][0]]
        else:
            cfg.num_humans_lo = cfg.num_humans_hi = int(num_humans)
        for i, v in enumerate(np.asarray(spec["threshold_footprint"], dtype=np.float64).reshape(-1)):
            cfg.robot_seen_footprint[i] = float(v)
        if lidar is not None:                         # (angle_min, angle_last, n_beams)
            cfg.angle_min, cfg.angle_last, cfg.n_beams = float(lidar[0]), float(lidar[1]), int(lidar[2])
            # the step refuses it (include/navsim.h angle_last): pedestrians are merged into the scan by bearing, one turn at most
            if cfg.ped_model != abi.PED_NONE and cfg.angle_last - cfg.angle_min > 2.0 * np.pi:
                raise ValueError("lidar=(%r, %r, ...) spans more than 2*pi, which worlds with pedestrians do not support "
                                 "(pedestrian_model=%r); use pedestrian_model='none' or num_humans=0, or a lidar of at most "
                                 "one turn" % (lidar[0], lidar[1], pedestrian_model))
        elif n_beams is not None and int(n_beams) == 1081:
            world.lidar_1081(cfg)
        elif n_beams is not None:
            world.lidar_full_circle(cfg, int(n_beams))
        else:                                         # keti_robot.py:44-48, env.py:388-390
            cfg.n_beams = spec["n_angles"]
            cfg.angle_min = spec["angle_min"]
            cfg.angle_last = spec["angle_max"] - spec["angle_increment"]
        # observed pedestrians (navsim_ped_observe): K rows per arena, one launch behind the step
        _check_params("observe_params", observe_params, observe_humans is not None, "observe_humans=K",
                      [k for k in _simmod.PED_OBSERVE_KEYS if k != "max_obs"], hint="; max_obs is observe_humans")
        if observe_humans is not None:
            if not (isinstance(observe_humans, numbers.Integral) and not isinstance(observe_humans, bool) and
                    1 <= observe_humans <= cfg.max_peds):
                raise ValueError("observe_humans must be None or an int in 1 .. %d (the world's pedestrian cap), not %r"
                                 % (cfg.max_peds, observe_humans))
            if cfg.ped_model == abi.PED_NONE:
                raise ValueError("observe_humans needs pedestrians: pedestrian_model=%r with at most %d of them has none"
                                 % (pedestrian_model, nh_hi))
        self.observe_humans = None if observe_humans is None else int(observe_humans)
        self.observe_params = None if observe_params is None else dict(observe_params)
        # goal path (navsim_goal_path): the field per arena, the path distance and the sub-goal, two launches behind the step
        _check_params("goal_path_params", goal_path_params, goal_path, "goal_path=True", _simmod.GOAL_PATH_KEYS)
        self.goal_path_on = bool(goal_path)
        self.goal_path_params = None if goal_path_params is None else dict(goal_path_params)
        self._goal_all = None                               # the goal path's rebuild mask of a reset(): every arena
        # local planner (navsim_dwa): an action per arena, one launch behind the step (and behind the goal path)
        if local_planner not in (None, "dwa", "mppi"):
            raise ValueError("local_planner must be None or 'dwa' or 'mppi', not %r" % (local_planner,))
        _check_params("local_planner_params", local_planner_params, local_planner is not None, "local_planner='dwa' or 'mppi'",
                      self._MPPI_KEYS if local_planner == "mppi" else _simmod.DWA_KEYS)
        if local_planner == "mppi":
            # (navsim_mppi, behind the goal path: its rollouts run the pedestrians' own model, which needs their commands)
            if pedestrian_model in ("orca", "policy"):
                raise ValueError("rollout is not available with pedestrian_model=%r: the pedestrians' commands come from a launch in "
                                 "front of the step that has not run yet (local_planner='mppi' plans with navsim_rollout)"
                                 % pedestrian_model)
            _simmod.mppi_params(cfg, self._mppi_overrides(local_planner_params, linvel_range, rotvel_range, cfg), robot_type)
        self.local_planner = local_planner
        self.local_planner_params = None if local_planner_params is None else dict(local_planner_params)
        # local map (navsim_local_map): a G x G grid per arena in the robot's frame, one launch behind the step
        _check_params("local_map_params", local_map_params, observe_local_map is not None, "observe_local_map=G",
                      _simmod.LOCAL_MAP_KEYS + ("visible_only",), hint="; the size is observe_local_map")
        if observe_local_map is not None:
            if not (isinstance(observe_local_map, numbers.Integral) and not isinstance(observe_local_map, bool) and
                    1 <= observe_local_map <= abi.LOCAL_MAP_MAX):
                raise ValueError("observe_local_map must be None or an int in 1 .. %d, not %r" % (abi.LOCAL_MAP_MAX, observe_local_map))
            channels = (local_map_params or {}).get("channels", _simmod.local_map_defaults(cfg)["channels"])
            if channels not in (1, 2, 4):
                raise ValueError("local_map_params: channels must be 1, 2 or 4, not %r" % (channels,))
            if channels > 1 and cfg.ped_model == abi.PED_NONE:
                raise ValueError("local_map_params: channels=%d needs pedestrians: pedestrian_model=%r with at most %d of them "
                                 "has none" % (channels, pedestrian_model, nh_hi))
            if (local_map_params or {}).get("visible_only") and self.observe_humans is None:
                raise ValueError("local_map_params: visible_only=True needs observe_humans=K")
        self.observe_local_map = None if observe_local_map is None else int(observe_local_map)
        self.local_map_params = None if local_map_params is None else dict(local_map_params)
        self._local_map_visible = bool((local_map_params or {}).get("visible_only"))
        # scan ground truth (navsim_scan_labels): the clean scan and per-beam hit labels, one launch behind the step
        if not isinstance(scan_labels, (bool, np.bool_)):
            raise ValueError("scan_labels must be True or False, not %r" % (scan_labels,))
        self.scan_labels_on = bool(scan_labels)
        # action lookahead (navsim_lookahead): the step's outcomes for K candidate actions per arena, on request (env.lookahead())
        _check_params("lookahead_params", lookahead_params, lookahead is not None, "lookahead=K", _simmod.LOOKAHEAD_KEYS)
        if lookahead is not None:
            if not (isinstance(lookahead, numbers.Integral) and not isinstance(lookahead, bool) and 1 <= lookahead <= abi.LOOKAHEAD_MAX):
                raise ValueError("lookahead must be None or an int in 1 .. %d, not %r" % (abi.LOOKAHEAD_MAX, lookahead))
            if pedestrian_model in ("orca", "policy"):
                raise ValueError("lookahead is not available with pedestrian_model=%r: the pedestrians' commands come from a launch in "
                                 "front of the step that has not run yet" % pedestrian_model)
        self.lookahead_k = None if lookahead is None else int(lookahead)
        self.lookahead_params = None if lookahead_params is None else dict(lookahead_params)
        # lookahead observations (navsim_lookahead_obs): the step's whole return for K candidate actions, on request (env.lookahead_obs())
        _check_params("lookahead_obs_params", lookahead_obs_params, lookahead_obs is not None, "lookahead_obs=K", _simmod.LOOKAHEAD_OBS_KEYS)
        if lookahead_obs is not None:
            if not (isinstance(lookahead_obs, numbers.Integral) and not isinstance(lookahead_obs, bool)
                    and 1 <= lookahead_obs <= abi.LOOKAHEAD_MAX):
                raise ValueError("lookahead_obs must be None or an int in 1 .. %d, not %r" % (abi.LOOKAHEAD_MAX, lookahead_obs))
            _simmod.lookahead_obs_choice(dict(_simmod.lookahead_obs_defaults(), **(lookahead_obs_params or {})))
            if pedestrian_model in ("orca", "policy"):
                raise ValueError("lookahead_obs is not available with pedestrian_model=%r: the pedestrians' commands come from a launch "
                                 "in front of the step that has not run yet" % pedestrian_model)
        self.lookahead_obs_k = None if lookahead_obs is None else int(lookahead_obs)
        self.lookahead_obs_params = None if lookahead_obs_params is None else dict(lookahead_obs_params)
        # action-sequence rollout (navsim_rollout): the next H steps' outcomes for K action sequences per arena, on request (env.rollout())
        _check_params("rollout_params", rollout_params, rollout is not None, "rollout=K", ("horizon",) + _simmod.ROLLOUT_KEYS)
        if rollout is not None:
            if not (isinstance(rollout, numbers.Integral) and not isinstance(rollout, bool) and 1 <= rollout <= abi.ROLLOUT_MAX_K):
                raise ValueError("rollout must be None or an int in 1 .. %d, not %r" % (abi.ROLLOUT_MAX_K, rollout))
            horizon = (rollout_params or {}).get("horizon", self._ROLLOUT_HORIZON)
            if not (isinstance(horizon, numbers.Integral) and not isinstance(horizon, bool) and 1 <= horizon <= abi.ROLLOUT_MAX_H):
                raise ValueError("rollout_params: horizon must be an int in 1 .. %d, not %r" % (abi.ROLLOUT_MAX_H, horizon))
            gamma = (rollout_params or {}).get("gamma", 1.0)
            if not (isinstance(gamma, numbers.Real) and not isinstance(gamma, bool) and 0.0 <= gamma <= 1.0):
                raise ValueError("rollout_params: gamma must lie in [0, 1], not %r" % (gamma,))
            if pedestrian_model in ("orca", "policy"):
                raise ValueError("rollout is not available with pedestrian_model=%r: the pedestrians' commands come from a launch in "
                                 "front of the step that has not run yet" % pedestrian_model)
        self.rollout_k = None if rollout is None else int(rollout)
        self.rollout_h = None if rollout is None else int((rollout_params or {}).get("horizon", self._ROLLOUT_HORIZON))
        self.rollout_params = None if rollout_params is None else dict(rollout_params)
        # rollout observations (navsim_rollout_obs): the next H steps' whole returns for K action sequences, on request (env.rollout_obs())
        _check_params("rollout_obs_params", rollout_obs_params, rollout_obs is not None, "rollout_obs=K",
                      ("horizon",) + _simmod.ROLLOUT_OBS_KEYS)
        if rollout_obs is not None:
            if not (isinstance(rollout_obs, numbers.Integral) and not isinstance(rollout_obs, bool)
                    and 1 <= rollout_obs <= abi.ROLLOUT_MAX_K):
                raise ValueError("rollout_obs must be None or an int in 1 .. %d, not %r" % (abi.ROLLOUT_MAX_K, rollout_obs))
            horizon = (rollout_obs_params or {}).get("horizon", self._ROLLOUT_HORIZON)
            if not (isinstance(horizon, numbers.Integral) and not isinstance(horizon, bool) and 1 <= horizon <= abi.ROLLOUT_MAX_H):
                raise ValueError("rollout_obs_params: horizon must be an int in 1 .. %d, not %r" % (abi.ROLLOUT_MAX_H, horizon))
            _simmod.rollout_obs_choice(dict(_simmod.rollout_obs_defaults(),
                                            **{k: v for k, v in (rollout_obs_params or {}).items() if k != "horizon"}))
            if pedestrian_model in ("orca", "policy"):
                raise ValueError("rollout_obs is not available with pedestrian_model=%r: the pedestrians' commands come from a launch "
                                 "in front of the step that has not run yet" % pedestrian_model)
        self.rollout_obs_k = None if rollout_obs is None else int(rollout_obs)
        self.rollout_obs_h = None if rollout_obs is None else int((rollout_obs_params or {}).get("horizon", self._ROLLOUT_HORIZON))
        self.rollout_obs_params = None if rollout_obs_params is None else dict(rollout_obs_params)
        # pedestrian forecast (navsim_ped_forecast): the pedestrians' next H poses per arena, one launch behind the step
        _check_params("ped_forecast_params", ped_forecast_params, ped_forecast is not None, "ped_forecast=H", self._FORECAST_KEYS)
        self.ped_forecast_h = self.ped_forecast_robot = self.ped_forecast_model = None
        if ped_forecast is not None:
            if not (isinstance(ped_forecast, numbers.Integral) and not isinstance(ped_forecast, bool) and
                    1 <= ped_forecast <= abi.FORECAST_MAX_H):
                raise ValueError("ped_forecast must be None or an int in 1 .. %d, not %r" % (abi.FORECAST_MAX_H, ped_forecast))
            if cfg.ped_model == abi.PED_NONE:
                raise ValueError("ped_forecast needs pedestrians: pedestrian_model=%r with at most %d of them has none"
                                 % (pedestrian_model, nh_hi))
            launched = pedestrian_model in ("orca", "policy")       # their commands come from a launch in front of the step
            robot = (ped_forecast_params or {}).get("robot", "hold")
            model = (ped_forecast_params or {}).get("model", "const_vel" if launched else "true")
            if robot not in self._FORECAST_ROBOT:
                raise ValueError("ped_forecast_params: robot must be one of %s, not %r" % (", ".join(map(repr, self._FORECAST_ROBOT)), robot))
            if model not in _simmod.PED_FORECAST_MODEL:
                raise ValueError("ped_forecast_params: model must be 'true' or 'const_vel', not %r" % (model,))
            if model == "true" and launched:
                raise ValueError("ped_forecast with model='true' is not available with pedestrian_model=%r: the pedestrians' commands "
                                 "come from a launch in front of the step that has not run yet (model='const_vel' is)" % pedestrian_model)
            if robot == "plan":
                if local_planner != "mppi":
                    raise ValueError("ped_forecast_params: robot='plan' needs local_planner='mppi'")
                plan_h = _simmod.mppi_params(cfg, self._mppi_overrides(local_planner_params, linvel_range, rotvel_range, cfg),
                                             robot_type).horizon
                if plan_h < ped_forecast:
                    raise ValueError("ped_forecast_params: robot='plan' needs a plan of at least ped_forecast=%d steps; the planner's "
                                     "horizon is %d" % (ped_forecast, plan_h))
            self.ped_forecast_h, self.ped_forecast_robot, self.ped_forecast_model = int(ped_forecast), robot, model
        self.ped_forecast_params = None if ped_forecast_params is None else dict(ped_forecast_params)
        self._humans_rel = None
        # the launches behind the step (and behind reset() / reset(mask) / load_state_dict), in the order they run -- the planner
        # reads the goal path's sub-goal, the local map the observer's `visible`.  _run_products() runs them; its latest result
        # and, per buffer parity, the views it handed out
        self._products = [row for on, row in (
            (self.observe_humans, _Product("humans", "ped_observe", self._observe, tuple(abi.PED_OBSERVATION), self._humans_row)),
            (self.goal_path_on, _Product("goal_path", "goal_path", self._goal_path, tuple(abi.GOAL_PATH_OUT), None)),
            (self.local_planner == "dwa", _Product("planner", "dwa", self._plan, self._PLANNER_KEYS, None)),
            (self.local_planner == "mppi", _Product("planner", "mppi", self._plan_mppi, tuple(abi.MPPI_OUT), None)),
            (self.observe_local_map, _Product("local_map", "local_map", self._local_map, ("map",), operator.itemgetter("map"))),
            (self.scan_labels_on, _Product("scan_labels", "scan_labels", self._scan_labels,
                                           tuple(k for k in abi.SCAN_LABELS_OUT if k != "hits" or cfg.ped_model != abi.PED_NONE), None)),
            (self.ped_forecast_h, _Product("ped_forecast", "ped_forecast", self._ped_forecast, tuple(abi.FORECAST_OUT),
                                           self._forecast_row if self.observe_humans else None))) if on]
        self._product_out, self._product_views = {}, {}
        self.cfg = cfg
        self.sim = None
        self._choose_reset_path(pregen_pipeline, plain_cap=cfg.regen_cap)      # (without the pipeline: the library's default cap)
        self._override_reward_factor(reward_scale, reward_success_factor, reward_crash_factor,
                                     reward_progress_factor, reward_forward_factor, reward_rotation_factor,
                                     reward_discomfort_factor)
        self.prev_obs = None
        self._bool = None
        self._views = {}                                    # per buffer parity: what step() hands out beside the observation
        self.robot = _AgentView(self, "robot")
        self.humans = []
        self._map_info = None
        self.scan_threshold = None
        self.scan_discomfort_threshold = None
        if action_kind == "wheels":                   # wheel speeds that reach every corner of the twist box
            corners = [robots.wheels_from_twist(v, w, cfg.wheel_radius, cfg.wheel_track)
                       for v in linvel_range for w in rotvel_range]
            lo, hi = float(np.min(corners)), float(np.max(corners))
            self.action_space = spaces.Box(low=np.array([lo, lo]), high=np.array([hi, hi]), dtype=np.float32)
        else:
            self.action_space = spaces.Box(low=np.array([linvel_range[0], rotvel_range[0]]),
                                           high=np.array([linvel_range[1], rotvel_range[1]]), dtype=np.float32)
        D = num_scan_stack * cfg.n_beams + 7
        self.observation_space = spaces.Dict({
            'observation': spaces.Box(-np.inf, np.inf, shape=(D,), dtype=np.float32),
            'achieved_goal': spaces.Box(-np.inf, np.inf, shape=(2,), dtype=np.float32),
            'desired_goal': spaces.Box(-np.inf, np.inf, shape=(2,), dtype=np.float32)})

    # ---- env.py:144-160 -------------------------------------------------------------------------
    def _override_reward_factor(self, reward_scale=15., reward_success_factor=1, reward_crash_factor=1,
                                reward_progress_factor=0.001, reward_forward_factor=0.0,
                                reward_rotation_factor=0.005, reward_discomfort_factor=0.01):
        self.reward_scale = reward_scale
        self.reward_success_factor = reward_success_factor
        self.reward_crash_factor = reward_crash_factor
        self.reward_progress_factor = reward_progress_factor
        self.reward_forward_factor = reward_forward_factor
        self.reward_rotation_factor = reward_rotation_factor
        self.reward_discomfort_factor = reward_discomfort_factor
        for c_ in (self.cfg,) if self.sim is None else (self.cfg, self.sim.cfg):      # (the simulator holds its own copy)
            for k in ("scale", "success_factor", "crash_factor", "progress_factor", "forward_factor",
                      "rotation_factor", "discomfort_factor"):
                setattr(c_, "reward_" + k, float(getattr(self, "reward_" + k)))

    def _choose_reset_path(self, pipeline, plain_cap=None):
        """How finished arenas get their next world, decided in this one place: pregen_pipeline, use_graphs, cfg.defer_reset_scan
        and cfg.regen_cap (self.cfg and the simulator's own copy) from the constructor's facts.  pipeline = P > 0: staging passes
        and navsim_step_install; 0: navsim_regen behind every step, as a hipGraph or as plain launches.
        plain_cap: cfg.regen_cap without the pipeline -- the constructor passes the library's default (64), the memory fallback
        of reset() passes nothing and gets min(num_envs, 64)."""
        regen = self.randomize_maps and self.auto_reset
        # (corridor maps AND planned starts: the worlds whose navsim_regen forks -- sim.pregen_plan's `helper`; its `heavy` is the OR
        #  of the two and decides another thing, the polled fallback and the two staging lanes)
        heavy = self.plan_paths and float(self.indoor_ratio) > 0.0
        self.pregen_pipeline = int(pipeline) if regen else 0
        if self.pregen_pipeline:
            self.use_graphs = False
        elif self._use_graphs_arg is not None:
            self.use_graphs = bool(self._use_graphs_arg)
        else:
            # corridor maps with planned starts: navsim_regen forks its distance transform beside the searches; as fork / join
            # nodes of a hipGraph that gains nothing (reference defaults, 1024 arenas: 0.92 M graphed, 0.96 M plain launches)
            self.use_graphs = self.randomize_maps and not heavy
        for c_ in (self.cfg,) if self.sim is None else (self.cfg, self.sim.cfg):
            if self.pregen_pipeline:
                c_.defer_reset_scan = 0           # a staged world brings its first observation; restarts in place scan in the step
                c_.regen_cap = self.num_envs      # every finished arena decides alone inside the step (navsim_step_install)
            else:
                # every step() is navsim_step + navsim_regen: the restarted arenas' first observations come from regen's masked
                # launch instead of a second scan inside the step (include/navsim.h defer_reset_scan), where a launch is one
                # generation of workgroups -- a few arenas per CU
                c_.defer_reset_scan = int(regen and self.num_envs <= 1024)
                c_.regen_cap = min(self.num_envs, 64) if plain_cap is None else plain_cap

    def _choose_step_path(self):
        """Which of its four sequences step() runs, with the fixed facts they need (at the end of the first reset(): the world's
        arrays and the reset path are known then)."""
        routes = "costmap" in self.sim.t
        self._regen_behind = self.randomize_maps and self.auto_reset      # navsim_regen behind the step
        self._replan_behind = routes                                      # navsim_replan behind the step (or inside / beside it)
        # pedestrians on planned routes: navsim_replan overlaps the step (not with 'policy' / 'orca', whose control block runs in
        # front of every step and reads the routes)
        self._overlap_replan = routes and self.sim.due is not None and not self._cmd_in_front and not self.pregen_pipeline
        if self._graphed:
            self._step_path = "graphed"
        elif self.pregen_pipeline:
            self._step_path = "pipelined"
            if routes and self.sim.pg_replan_cap == 0:      # the re-plan of the previous step's arrivals inside the step's launch
                self.sim.pg_replan_cap = self.replan_cap
        else:
            self._step_path = "overlapped" if self._overlap_replan else "plain"

    # ---- reset (env.py:730-831), all arenas ---------------------------------------------------------
    def reset(self, mask=None):
        """reset() of every arena (env.py:730-831).  Nothing is generated on the host: maps, distance fields,
        costmaps, start / goal pairs (joined by a planned path when plan_paths), pedestrians, the per-episode
        env_param draws and the first observations all come from navsim_regen with every arena marked
        finished (NavSim.regenerate_all).
        mask [num_envs] (bool / 0-1): reset only those arenas -- the reference's reset() is per environment -- the others
        keep their state and their observation rows (NavSim.reset_arenas: next start / goal pair and episode number, first
        observation; with randomize_maps a new world each).  On the pipelined reset path (pregen_pipeline > 0) the masked
        arenas install their staged worlds in one launch (navsim_reset_install; an arena whose world is not staged yet is
        regenerated on the spot): the same state and rows as with pregen_pipeline=0."""
        from . import lib
        lib.require_gpu()                                 # no CPU fallback: fail before any work
        import torch
        if mask is not None:
            if self.sim is None:
                raise RuntimeError("reset(mask) needs one reset() of every arena first")
            m = torch.as_tensor(np.asarray(mask) if not hasattr(mask, "is_cuda") else mask).reshape(self.num_envs)
            if self._graphed:
                torch.cuda.synchronize(self.sim.device)
            self.sim.reset_arenas(m, new_world=self.randomize_maps)
            if "policy_prev_actions" in self.sim.t:       # env.py:739
                self.sim.t["policy_prev_actions"].mul_((m.to(self.sim.device) == 0).to(self.sim.t["policy_prev_actions"].dtype)[:, None, None])
            self._map_info = None
            self._humans_of_episode = None
            # (the goal path of the restarted arenas: their key says so; a new map with the old number would not)
            self._run_products(rebuild=m.to(self.sim.device).ne(0).to(torch.uint8).contiguous() if self.goal_path_on else None)
            return self._obs_dict()
        self._bool = torch.bool
        from . import sim as simmod
        cfg = self.cfg
        first = self.sim is None
        if first:
            dev = torch.device(self.device)
            arrays = world.empty_world(cfg, device=self.device,
                                       plan_paths=self.plan_paths and cfg.ped_model != abi.PED_NONE,
                                       rect_table=self._with_rects)
            for key, name in (("scan_threshold", "threshold_footprint"), ("scan_discomfort", "discomfort_threshold_footprint")):
                arrays[key] = simmod.scan_threshold(cfg, torch.from_numpy(robots.footprint_array(self.robot_type, name)).to(dev))
            # every map of this world comes from navsim_regen, whose generators close their maps with a border wall
            # (map_generator.py:11, 61-93): the LDS form of the march may be used (include/navsim.h closed_maps)
            cfg.closed_maps = int("rect_index" in arrays)
            self.sim = simmod.NavSim(cfg, arrays, device=self.device, final_obs=self.final_observation)
            self._views = {}
            self.scan_threshold = arrays["scan_threshold"]
            self.scan_discomfort_threshold = arrays["scan_discomfort"]
            if self.pedestrian_model == "policy":
                w = self._policy_weights
                if isinstance(w, str):
                    w = torch.load(w, map_location="cpu")
                self.sim.set_policy(w)
            if self.episode_stats:
                self.sim.enable_episode_stats()
            if self.observe_humans:
                self.sim.enable_ped_observe(dict(self.observe_params or {}, max_obs=self.observe_humans))
            if self.goal_path_on:
                self.sim.enable_goal_path(self.goal_path_params)
                self._goal_all = torch.ones(self.num_envs, dtype=torch.uint8, device=dev)
            if self.local_planner == "dwa":
                self.sim.enable_dwa(self.local_planner_params, robot_type=self.robot_type)
            if self.local_planner == "mppi":
                self.sim.enable_mppi(self._mppi_overrides(self.local_planner_params, self.linvel_range, self.rotvel_range, cfg),
                                     robot_type=self.robot_type)
            if self.observe_local_map:
                self.sim.enable_local_map(self.observe_local_map, {k: v for k, v in (self.local_map_params or {}).items()
                                                                   if k != "visible_only"})
            if self.scan_labels_on:
                self.sim.enable_scan_labels()
            if self.lookahead_k:
                self.sim.enable_lookahead(self.lookahead_k, self.lookahead_params)
            if self.lookahead_obs_k:
                self.sim.enable_lookahead_obs(self.lookahead_obs_k, self.lookahead_obs_params)
            if self.rollout_k:
                self.sim.enable_rollout(self.rollout_k, self.rollout_h,
                                        {k: v for k, v in (self.rollout_params or {}).items() if k != "horizon"})
            if self.rollout_obs_k:
                self.sim.enable_rollout_obs(self.rollout_obs_k, self.rollout_obs_h,
                                            {k: v for k, v in (self.rollout_obs_params or {}).items() if k != "horizon"})
            if self.ped_forecast_h:
                self.sim.enable_ped_forecast(self.ped_forecast_h, dict(
                    robot="actions" if self.ped_forecast_robot == "plan" else self.ped_forecast_robot, model=self.ped_forecast_model))
                if self.observe_humans:                   # 'humans_rel' [E,H,K,2], one buffer per set of the step's outputs
                    self._humans_rel = [torch.zeros((self.num_envs, self.ped_forecast_h, self.observe_humans, 2), dtype=torch.float32,
                                                    device=dev) for _ in range(2)]
        elif "policy_prev_actions" in self.sim.t:
            self.sim.t["policy_prev_actions"].zero_()           # env.py:739
        self._episode_batch += 1
        self.sim.regenerate_all(new_episode=not first)
        if self.pregen_pipeline and first and self._pregen_auto:
            # the pipeline keeps a second, staged copy of every array navsim_regen writes (the maps above all) and builds it
            # through a few GB of scratch: where that does not fit, the env's own choice falls back to navsim_regen after every step
            need = 2 * sum(v.numel() * v.element_size() for k, v in self.sim.t.items() if k in self.sim.STAGED) + (6 << 30)
            free = torch.cuda.mem_get_info(torch.device(self.device))[0]
            if need > free:
                self._warn_once("pregen_memory", "NavGymEnv: %.0f GB free on the device, the pipelined reset path would need about "
                                "%.0f GB more than the world itself: pregen_pipeline falls back to 0 (navsim_regen after every step)"
                                % (free / 2 ** 30, need / 2 ** 30))
                self._choose_reset_path(0)
        if self.pregen_pipeline:
            if cfg.field_format != abi.FIELD_U16T:
                raise ValueError("pregen_pipeline needs the packed distance field (map_size <= 1024)")
            if first:
                self.sim.enable_pregen(pipeline=self.pregen_pipeline, install=True, stage_cap=self.pregen_stage_cap,
                                       fallback_poll=self.pregen_fallback_poll)
            else:
                self.sim.restage_all()                    # the worlds behind the ones this reset() just drew
        if first and self.use_graphs and not self._cmd_in_front:
            self.sim.enable_graphs(regen=self.randomize_maps and self.auto_reset,
                                   replan_cap=self.replan_cap if "costmap" in self.sim.t else 0)
            self._graphed = True
        if first:
            self._choose_step_path()
        self._map_info = None                             # read back from the device when somebody asks (map_info)
        self._humans_of_episode = None
        self._run_products(rebuild=self._goal_all)        # (every arena's goal path: a reset() may start the episode numbers again)
        return self._obs_dict()

    @property
    def map_info(self):
        """Arena 0's map as RosEnv reads it (ros_env.py:69-81; env.py:297-310): built on first use after a reset() -- the
        occupancy grid is read back from the device's distance field, which step() and reset() themselves never need
        (round 4 copied it to the host in every reset())."""
        if self.sim is None:
            return None
        if self._map_info is None:
            cfg = self.cfg
            occ0 = self.sim.occupancy(0)
            live = self.map_size
            if self.outdoor_map_size and occ0[self.outdoor_map_size:, :].all() and occ0[:, self.outdoor_map_size:].all():
                live = self.outdoor_map_size              # arena 0 drew an outdoor map: the reference's 400 x 400 array
            self._map_info = {"data": (occ0[:live, :live].astype(np.int8) * 100), "origin": (cfg.origin_x, cfg.origin_y),
                              "resolution": cfg.resolution, "width": live, "height": live}
        return self._map_info

    @property
    def humans(self):
        """Views of arena 0's pedestrians (ros_env.py:120-176), as many as its current episode has."""
        if self.sim is None or "n_peds" not in self.sim.t:
            return []
        if self._humans_of_episode is None:
            self._humans_of_episode = [_AgentView(self, "human", i) for i in range(int(self.sim.t["n_peds"][0]))]
        return self._humans_of_episode

    @humans.setter
    def humans(self, value):
        self._humans_of_episode = list(value)

    def _obs_dict(self):
        # no kernel of its own: the observation rows and the two goal arrays are what the step (or navsim_regen's
        # first-observation launch) wrote (env.py:455-461: achieved_goal = the pose slots, desired_goal = the robot's goal)
        o = self.sim.obs
        d = {"observation": o, "achieved_goal": self.sim.out["achieved_goal"], "desired_goal": self.sim.out["desired_goal"]}
        if self.num_envs == 1:
            d = {k: v[0].double().cpu().numpy() for k, v in d.items()}
        self.prev_obs = d
        return d

    # ---- step (env.py:591-728) -------------------------------------------------------------------------
    def step(self, action, human_actions=None):
        if self.sim is None:
            raise RuntimeError("call reset() before step()")
        if human_actions is not None:
            self.sim.set_ped_cmd(human_actions)
        elif self.pedestrian_model == "policy":
            self.sim.ped_policy()                           # scans -> HumanPolicy actor -> (v, omega)
        elif self.pedestrian_model == "orca":
            if self._orca_struct is None:
                from . import sim as simmod
                self._orca_struct = simmod.ped_orca_params(self.sim.cfg, self.orca_params, self.robot_type)
            if self._orca_rects:                            # ... with the arena's listed rectangles as obstacles
                self.sim.ped_orca_walls(self._orca_struct, self._orca_rects)
            else:
                self.sim.ped_orca(self._orca_struct)        # the simulator's state -> ORCA -> (v, omega), one launch
        a = np.asarray(action, dtype=np.float64).reshape(self.num_envs, 2) if not hasattr(action, "is_cuda") else action
        path = self._step_path
        if path == "graphed":                               # step + regen + replan: one graph launch (NavSim.enable_graphs)
            _, out = self.sim.step_graphed(a)
        elif path == "pipelined":
            # navsim_step_install: finished arenas take their staged worlds; with planned routes the re-plan of the PREVIOUS
            # step's arrivals inside the same launch where the search fits the arena's workgroup (else behind the step: the
            # library may refuse the in-launch search at run time)
            _, out = self.sim.step(a)
            self.sim.regen()                               # ... and every P steps a staging pass goes to the side stream
            if self._replan_behind and not self.sim.pg_replan_in_step:
                self.sim.replan(self.replan_cap)
        elif path == "overlapped":
            # planned routes: the re-plan of the previous step runs beside this step's launch (NavSim.launch_step_overlapped)
            _, out = self.sim.step_overlapped(a, self.replan_cap)
            if self._regen_behind:
                self.sim.regen()
        else:
            _, out = self.sim.step(a)                      # (a float64 tensor on the device is read in place: no copy)
            if self.pedestrian_model == "policy" and self.auto_reset:
                # a new episode starts with prev_human_actions = 0 (env.py:739)
                started = self.sim.reset_flags if self.autoreset_mode == "next_step" else out["done"]
                self.sim.t["policy_prev_actions"].mul_((started == 0).to(self.sim.t["policy_prev_actions"].dtype)[:, None, None])
            if self._regen_behind:
                self.sim.regen()
            if self._replan_behind:
                self.sim.replan(self.replan_cap)           # ('policy', 'orca': the launch in front of the next step reads the routes)
        if self.episode_stats:                             # one launch, behind whatever the step's path queued
            ep = self.sim.episode_stats()
        products = self._run_products()                    # likewise: the state the returned rows describe (the goal path's keys
        #                                                    decide what is rebuilt)
        obs = self._obs_dict()
        # the LAST observation of an episode that ended in this step (env.py:700-728 returns it with done = True): under
        # same-step auto-reset the row above already is the next episode's first one and the terminal one rides in info;
        # next-step auto-reset returns it as the observation and marks the arenas this step reset instead
        fin = self.sim.final
        if self.num_envs == 1:
            info = {"is_success": np.float32(out["is_success"][0].item()),
                    "is_crash": np.float32(out["is_crash"][0].item()),
                    "distance": float(out["distance"][0].item())}
            done = bool(out["done"][0].item())
            if fin is not None and done:
                g = fin["final_goals"][0].double().cpu().numpy()
                info["final_observation"] = {"observation": fin["final_obs"][0].double().cpu().numpy(),
                                             "achieved_goal": g[:2], "desired_goal": g[2:]}
            if self.auto_reset and self.autoreset_mode == "next_step":
                info["reset_mask"] = bool(self.sim.reset_flags[0].item())
            if self.max_episode_steps is not None:
                info["TimeLimit.truncated"] = bool(out["truncated"][0].item())
            if self.episode_stats and done:
                info["episode"] = {name: ep[k][0].item() for name, k in self._EPISODE_KEYS}
            info.update(products)
            return obs, float(out["reward"][0].item()), done, info
        # (views of the buffers the kernel wrote, made ONCE per buffer parity: a step of 4096 arenas is 95 us on the device, and
        #  every tensor slice or .view() costs the host 3-5 us -- round 6 measured 42 -> 36 M env-steps/s through this method
        #  when the terminal rows' three views were built per call)
        v = self._views.get(self.sim.cur)
        if v is None:
            v = {"done": out["done"].view(self._bool)}
            if fin is not None:
                v["final"] = {"observation": fin["final_obs"], "achieved_goal": fin["final_goals"][:, :2],
                              "desired_goal": fin["final_goals"][:, 2:]}
            if self.auto_reset and self.autoreset_mode == "next_step":
                v["reset"] = self.sim.reset_flags.view(self._bool)
            if self.max_episode_steps is not None:
                v["truncated"] = out["truncated"].view(self._bool)
            if self.episode_stats:
                v["episode"] = {name: ep[k] for name, k in self._EPISODE_KEYS}
            self._views[self.sim.cur] = v
        info = {"is_success": out["is_success"], "is_crash": out["is_crash"], "distance": out["distance"]}
        done = v["done"]
        if fin is not None:
            info["final_observation"] = v["final"]
            info["final_mask"] = done
        if "reset" in v:
            info["reset_mask"] = v["reset"]
        if "truncated" in v:
            info["TimeLimit.truncated"] = v["truncated"]
        if "episode" in v:
            info["episode"] = v["episode"]
            info["_episode"] = done
        info.update(products)
        return obs, out["reward"], done, info

    def _run_products(self, rebuild=None):
        """The enabled launches behind whatever was queued, on the same stream and in the constructor's order: the products of the
        state the current observation rows describe.  rebuild: the goal path's mask of arenas whose field is rebuilt whatever its
        key says.  Same-step auto-reset: the row of an arena that finished describes its NEW episode, like the observation beside
        it (a shaper masks with `done`).  Next-step auto-reset: an arena whose `done` is set has its state restarted already
        while its row is the terminal one -- every product skips it (empty rows, all 0) until the call that resets it.
        Returns {info key: value}: dicts of views of the current buffer set, made ONCE per buffer parity (env.step's comment has
        the host cost of a view); num_envs == 1: arena 0's rows as NumPy values, from one device -> host copy per product."""
        sim, one = self.sim, self.num_envs == 1
        cur = sim.cur
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" else None
        for p in self._products:
            p.launch(skip, rebuild)
        res = None if one else self._product_views.get(cur)
        if res is None:
            res = {}
            for p in self._products:
                o = sim.products[p.record].host(cur) if one else sim.products[p.record].buf[cur]
                v = {k: o[k][0] if one else o[k] for k in p.keys}
                res[p.key] = v if p.finish is None else p.finish(v)
            if not one:
                self._product_views[cur] = res
        self._product_out = res
        return res

    # what differs per product: its call with its inputs, and what its rows still need
    def _observe(self, skip, rebuild):
        self.sim.ped_observe(skip=skip)

    def _humans_row(self, v):
        if self.num_envs == 1:                            # (NumPy rows: the count an int, `visible` of dtype bool)
            v["count"], v["visible"] = int(v["count"]), v["visible"].astype(bool)
        else:
            v["visible"] = v["visible"].view(self._bool)
        return v

    def _goal_path(self, skip, rebuild):
        self.sim.goal_path(rebuild=rebuild, skip=skip)

    _PLANNER_KEYS = ("action", "twist", "clearance", "best", "status")

    def _plan(self, skip, rebuild):                      # (the goal path's sub-goal of the current buffer set is the target; without
        sim = self.sim                                    # goal_path the arena's goal)
        sim.dwa(subgoal=sim.products["goal_path"].buf[sim.cur]["subgoal"] if self.goal_path_on else None, skip=skip)

    # local_planner_params under 'mppi': sim.MPPI_KEYS without the action box, which is the environment's own action_space
    _MPPI_KEYS = ("n_samples", "horizon", "iterations", "sigma", "lam", "beta", "w_goal", "w_crash", "off_field_cost", "stop_sample",
                  "select", "range", "gamma", "init_action")

    @staticmethod
    def _mppi_overrides(params, linvel_range, rotvel_range, cfg):
        """local_planner_params with the action box of this environment's action_space added (lo, hi of sim.mppi_defaults)."""
        if cfg.action_kind == abi.ACTION_WHEELS:
            corners = [robots.wheels_from_twist(v, w, cfg.wheel_radius, cfg.wheel_track) for v in linvel_range for w in rotvel_range]
            lo, hi = (float(np.min(corners)),) * 2, (float(np.max(corners)),) * 2
        else:
            lo, hi = (float(linvel_range[0]), float(rotvel_range[0])), (float(linvel_range[1]), float(rotvel_range[1]))
        d = dict(params or {}, lo=lo, hi=hi)
        if "sigma" not in d:
            d["sigma"] = tuple(0.5 * (h - l) for l, h in zip(lo, hi))
        if "init_action" not in d:
            d["init_action"] = tuple(min(max(0.0, l), h) for l, h in zip(lo, hi))
        return d

    def _plan_mppi(self, skip, rebuild):                 # (with goal_path the field that launch just brought up to date is the
        self.sim.mppi(field=self.goal_path_on, skip=skip)  # terminal cost; 'external' pedestrians: the state's own commands)

    def planner_plan(self):
        """The planner's current plans (local_planner='mppi'): float64 [E,H,2] on the device, in action_kind's form; row 0 is
        what info['planner']['action'] holds under select='mean' (num_envs == 1: a NumPy array [H,2])."""
        if self.local_planner != "mppi":
            raise RuntimeError("planner_plan() needs NavGymEnv(local_planner='mppi')")
        if self.sim is None:
            raise RuntimeError("call reset() before planner_plan()")
        plan = self.sim.mppi_plan()
        return plan[0].cpu().numpy() if self.num_envs == 1 else plan

    def _local_map(self, skip, rebuild):                 # (visible_only: the observer's `visible` of the current buffer set is the
        sim = self.sim                                    # pedestrians that count)
        sim.local_map(skip=skip, visible=sim.products["ped_observe"].buf[sim.cur]["visible"] if self._local_map_visible else None)

    def _scan_labels(self, skip, rebuild):
        self.sim.scan_labels(skip=skip)

    # ped_forecast_params: the robot assumed over the horizon ('plan': the first H actions of the MPPI planner's plan) and the model
    _FORECAST_KEYS = ("robot", "model")
    _FORECAST_ROBOT = ("hold", "stop", "plan")

    def _ped_forecast(self, skip, rebuild):              # (behind the planner: robot='plan' reads the plan that launch just left, on
        sim = self.sim                                    # the device; 'external' pedestrians: the state's own commands)
        plan = sim.mppi_plan()[:, :self.ped_forecast_h] if self.ped_forecast_robot == "plan" else None
        out = sim.ped_forecast(actions=plan, skip=skip)
        if self._humans_rel is not None:                  # rel gathered by the observer's index of the same buffer set; 0 where -1
            index = sim.products["ped_observe"].buf[sim.cur]["index"]                       # [E,K] int32
            E, K = index.shape
            at = index.clamp(min=0).long()[:, None, :, None].expand(E, self.ped_forecast_h, K, 2)
            rows = out["rel"].gather(2, at).masked_fill_((index < 0)[:, None, :, None], 0.0)
            self._humans_rel[sim.cur].copy_(rows)

    def _forecast_row(self, v):
        rel = self._humans_rel[self.sim.cur]
        v["humans_rel"] = rel[0].cpu().numpy() if self.num_envs == 1 else rel
        return v

    def ped_forecast(self, actions=None, human_actions=None):
        """Where the pedestrians will be after each of the next H step() calls (NavGymEnv(ped_forecast=H); navsim_ped_forecast, one
        launch that only reads the state), time-major: {'pose' [E,H,N,3] float64, 'vel' [E,H,N,2] float64, 'rel' [E,H,N,2] float32
        (the position in the robot's CURRENT frame, observed_humans()' convention), 'robot_pose' [E,H,3] float64 (the robot pose
        assumed after step h), 'min_dist' [E,N] float64 and 'min_step' [E,N] int32 (the closest approach over the horizon and the
        first step that attains it; +inf / -1 for an unused slot), 'exact_steps' [E] int32 (the leading steps that are the
        step's own: H unless a pedestrian reaches its last waypoint inside the horizon, where the real step would re-plan it; 0
        under model='const_vel'), 'status' [E] uint8 (0 = skipped)}; with observe_humans=K also 'humans_rel' [E,H,K,2] float32,
        `rel` of the observed pedestrians, row for row as info['humans']['index'] lists them (0 where the index is -1).
        Without arguments: what info['ped_forecast'] of the latest step() holds; valid after reset() and reset(mask) too.
        actions / human_actions: an explicit query of the current state into buffers of its own -- actions a float64 device
        tensor [E,H,2] or an array-like [H,2] that every arena takes, in action_kind's form (None: the robot of
        ped_forecast_params); human_actions [E,N,2] with pedestrian_model='external', held for the whole horizon (None: the
        state's own).  Next-step auto-reset: an arena whose `done` is set is skipped (status 0, rows 0) until the step that
        resets it.  num_envs > 1: torch views, intact through the next step(); num_envs == 1: NumPy rows."""
        if actions is None and human_actions is None:
            return self._latest("ped_forecast", self.ped_forecast_h, "ped_forecast", "ped_forecast=H")
        if not self.ped_forecast_h:
            raise RuntimeError("ped_forecast() needs NavGymEnv(ped_forecast=H)")
        if self.sim is None:
            raise RuntimeError("call reset() before ped_forecast()")
        sim, E = self.sim, self.num_envs
        if actions is not None:
            actions = self._forecast_actions(actions, E, self.ped_forecast_h)
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" and sim.out is not None else None
        out = sim.ped_forecast(actions=actions, ped_cmd=human_actions if self.pedestrian_model == "external" else None, skip=skip,
                               query=True)
        if E == 1:
            return {k: v[0] for k, v in sim.ped_forecast_host(query=True).items()}
        return dict(out)

    @staticmethod
    def _forecast_actions(actions, E, H):
        """ped_forecast()'s actions as [E,H,2]: a device tensor stays one ([H,2] expanded), an array-like becomes a float64 host
        tensor ([H,2] broadcast over the arenas)."""
        import torch
        if hasattr(actions, "is_cuda"):
            return actions.expand(E, H, 2) if tuple(actions.shape) == (H, 2) else actions
        a = np.asarray(actions, dtype=np.float64)
        if a.shape == (H, 2):
            a = np.broadcast_to(a, (E, H, 2))
        if a.shape != (E, H, 2):
            raise ValueError("ped_forecast() takes actions of shape (%d, %d, 2) or (%d, 2), not %r" % (E, H, H, a.shape))
        return torch.from_numpy(np.array(a, dtype=np.float64, order="C"))               # (a writable copy)

    def _latest(self, key, on, what, needs):
        """What info[key] of the latest step() holds; valid after reset() and reset(mask) too."""
        if not on:
            raise RuntimeError("%s() needs NavGymEnv(%s)" % (what, needs))
        if self.sim is None:
            raise RuntimeError("call reset() before %s()" % what)
        return self._product_out[key]

    def local_map(self):
        """What info['local_map'] of the latest step() holds (observe_local_map=G); valid after reset() and reset(mask) too:
        float32 [E, C, G, G] in the robot's frame (num_envs == 1: a NumPy array [C, G, G])."""
        return self._latest("local_map", self.observe_local_map, "local_map", "observe_local_map=G")

    def scan_labels(self):
        """What info['scan_labels'] of the latest step() holds (scan_labels=True); valid after reset() and reset(mask) too:
        {'range' [E,B] float32, the scan without noise; 'label' [E,B] uint8 (abi.BEAM_*); 'index' [E,B] int8, the pedestrian of
        a beam with label 2 or 3, else -1; 'hits' [E,N] int32 with a pedestrian model}."""
        return self._latest("scan_labels", self.scan_labels_on, "scan_labels", "scan_labels=True")

    _LOOKAHEAD_BOOL = ("done", "discomfort")

    def lookahead(self, actions, human_actions=None):
        """What step() would return for each of K candidate actions per arena, from the current state, which is only read
        (NavGymEnv(lookahead=K); navsim_lookahead, one launch): {'reward' [E,K] float64, 'done' [E,K] bool (success, crash or time
        limit), 'is_success', 'is_crash' [E,K] float32, 'discomfort' [E,K] bool, 'distance' [E,K] float64, 'margin' [E,K] float32
        (the least range minus crash threshold over the beams: negative iff is_crash), 'pose' [E,K,3] float64 (the pose the step
        would scan from), 'status' [E] uint8 (0 = skipped)}.  With scan noise on the values are the noise-free outcome.
        actions: a float64 device tensor [E,K,2], or an array-like [K,2] that every arena takes, in action_kind's form.
        human_actions: [E,N,2] with pedestrian_model='external' (required there: the commands the step would be given).
        Next-step auto-reset: an arena whose `done` is set is skipped (status 0, rows 0) until the step that resets it.
        num_envs > 1: torch views, intact through the next step(); num_envs == 1: NumPy rows [K,...] from one device -> host copy."""
        if self.lookahead_k is None:
            raise RuntimeError("lookahead() needs NavGymEnv(lookahead=K)")
        if self.pedestrian_model == "external" and human_actions is None:
            raise ValueError("lookahead() with pedestrian_model='external' needs human_actions")
        if self.sim is None:
            raise RuntimeError("call reset() before lookahead()")
        import torch
        sim, E, K = self.sim, self.num_envs, self.lookahead_k
        if not hasattr(actions, "is_cuda"):
            a = np.asarray(actions, dtype=np.float64)
            if a.shape == (K, 2):
                a = np.broadcast_to(a, (E, K, 2))
            actions = torch.from_numpy(np.array(a.reshape(E, K, 2), dtype=np.float64, order="C"))    # (a writable copy)
        elif tuple(actions.shape) == (K, 2):
            actions = actions.expand(E, K, 2)
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" and sim.out is not None else None
        out = sim.lookahead(actions, ped_cmd=human_actions if self.pedestrian_model == "external" else None, skip=skip)
        if E == 1:
            host = sim.lookahead_host()
            return {k: (v[0].astype(bool) if k in self._LOOKAHEAD_BOOL else v[0]) for k, v in host.items()}
        return {k: (v.view(self._bool) if k in self._LOOKAHEAD_BOOL else v) for k, v in out.items()}

    def lookahead_obs(self, actions, human_actions=None):
        """The whole return of step() for each of K candidate actions per arena, from the current state, which is only read
        (NavGymEnv(lookahead_obs=K); navsim_lookahead_obs, one launch): lookahead()'s dict -- here with the scan noise the step
        itself would draw (lookahead_obs_params: noise='step'), so its values are the step's own, noise on or off -- plus
        'observation': {'observation' [E,K,D] float32, 'achieved_goal' [E,K,2], 'desired_goal' [E,K,2]} as step() returns it for
        that action (rows='full' only; behind a crash the reference's re-scan from the reverted pose; for a `done` candidate the
        terminal row, not the first row of the next episode), 'scan' [E,K,B] float32 (the row's newest slot), 'tail' [E,K,7]
        float32 and 'truncated' [E,K] bool.
        actions, human_actions: as lookahead()'s.  Next-step auto-reset: an arena whose `done` is set is skipped (status 0, rows 0).
        num_envs > 1: torch views, intact through the next step(); num_envs == 1: NumPy rows [K,...] from one device -> host copy
        (the three arrays of 'observation' as float64, like step()'s)."""
        if self.lookahead_obs_k is None:
            raise RuntimeError("lookahead_obs() needs NavGymEnv(lookahead_obs=K)")
        if self.pedestrian_model == "external" and human_actions is None:
            raise ValueError("lookahead_obs() with pedestrian_model='external' needs human_actions")
        if self.sim is None:
            raise RuntimeError("call reset() before lookahead_obs()")
        import torch
        sim, E, K = self.sim, self.num_envs, self.lookahead_obs_k
        if not hasattr(actions, "is_cuda"):
            a = np.asarray(actions, dtype=np.float64)
            if a.shape == (K, 2):
                a = np.broadcast_to(a, (E, K, 2))
            actions = torch.from_numpy(np.array(a.reshape(E, K, 2), dtype=np.float64, order="C"))    # (a writable copy)
        elif tuple(actions.shape) == (K, 2):
            actions = actions.expand(E, K, 2)
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" and sim.out is not None else None
        out = sim.lookahead_obs(actions, ped_cmd=human_actions if self.pedestrian_model == "external" else None, skip=skip)
        booleans = self._LOOKAHEAD_BOOL + ("truncated",)
        if E == 1:
            out = {k: (v[0].astype(bool) if k in booleans else v[0]) for k, v in sim.lookahead_obs_host().items()}
            wide = lambda v: v.astype(np.float64)
        else:
            out = {k: (v.view(self._bool) if k in booleans else v) for k, v in out.items()}
            wide = lambda v: v
        goals = out.pop("goals")
        if "obs" in out:
            out["observation"] = {"observation": wide(out.pop("obs")), "achieved_goal": wide(goals[..., :2]),
                                  "desired_goal": wide(goals[..., 2:])}
        return out

    _ROLLOUT_HORIZON = 8

    def rollout(self, actions, human_actions=None):
        """What the next H step() calls would return if an arena executed each of K action sequences, from the current state, which
        is only read (NavGymEnv(rollout=K, rollout_params=dict(horizon=H)); navsim_rollout, one launch): {'reward' [E,K,H] float64
        and 'pose' [E,K,H,3] float64 (the pose the step scans from), both 0 behind the sequence's last evaluated step; 'ret' [E,K]
        float64, the rewards discounted by gamma; 'length' [E,K] int32, the steps evaluated (a sequence ends at its first done
        step); 'outcome' [E,K] uint8 of the last evaluated step (1 success | 2 crash | 4 time limit); 'discomfort_steps' [E,K]
        int32; 'min_margin' [E,K] float32 (negative iff a step crashed); 'distance' [E,K] float64; 'exact_steps' [E,K] int32 (the
        leading steps whose rows are the step's own -- H unless a pedestrian reaches its last waypoint inside the horizon, where
        the real step would re-plan it); 'status' [E] uint8 (0 = skipped)}.  With scan noise on the values are the noise-free
        outcome.
        actions: a float64 device tensor [E,K,H,2], or an array-like [K,H,2] that every arena takes, in action_kind's form.
        human_actions: [E,N,2] with pedestrian_model='external' (required there), held for the whole horizon.
        Next-step auto-reset: an arena whose `done` is set is skipped (status 0, rows 0) until the step that resets it.
        num_envs > 1: torch views, intact through the next step(); num_envs == 1: NumPy rows [K,...] from one device -> host copy."""
        if self.rollout_k is None:
            raise RuntimeError("rollout() needs NavGymEnv(rollout=K)")
        if self.pedestrian_model == "external" and human_actions is None:
            raise ValueError("rollout() with pedestrian_model='external' needs human_actions")
        if self.sim is None:
            raise RuntimeError("call reset() before rollout()")
        import torch
        sim, E = self.sim, self.num_envs
        actions = self._rollout_actions(actions, E, self.rollout_k, self.rollout_h)
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" and sim.out is not None else None
        out = sim.rollout(actions, ped_cmd=human_actions if self.pedestrian_model == "external" else None, skip=skip)
        if E == 1:
            return {k: v[0] for k, v in sim.rollout_host().items()}
        return dict(out)

    def rollout_obs(self, actions, human_actions=None):
        """The whole return of the next H step() calls if an arena executed each of K action sequences, from the current state,
        which is only read (NavGymEnv(rollout_obs=K, rollout_obs_params=dict(horizon=H)); navsim_rollout_obs, one launch):
        rollout()'s dict -- here every step scans at the lidar's full range with the scan noise that future step itself would draw
        (rollout_obs_params: noise='step'), so the values below exact_steps are the steps' own, noise on or off, and 'min_margin'
        is taken on those ranges -- plus 'observation': {'observation' [E,K,D] float32, 'achieved_goal' [E,K,2], 'desired_goal'
        [E,K,2]} as step() returns it at the sequence's last evaluated step (behind a crash the reference's re-scan from the
        reverted pose; for a sequence that ends the terminal row, not the first row of the next episode).  With rows='all' also
        'observations': the same three keys for every step, [E,K,H,D] and [E,K,H,2], 0 behind the last evaluated step.
        actions, human_actions: as rollout()'s.  Next-step auto-reset: an arena whose `done` is set is skipped (status 0, rows 0).
        num_envs > 1: torch views, intact through the next step(); num_envs == 1: NumPy rows [K,...] from one device -> host copy
        (the arrays of 'observation' and 'observations' as float64, like step()'s)."""
        if self.rollout_obs_k is None:
            raise RuntimeError("rollout_obs() needs NavGymEnv(rollout_obs=K)")
        if self.pedestrian_model == "external" and human_actions is None:
            raise ValueError("rollout_obs() with pedestrian_model='external' needs human_actions")
        if self.sim is None:
            raise RuntimeError("call reset() before rollout_obs()")
        sim, E = self.sim, self.num_envs
        actions = self._rollout_actions(actions, E, self.rollout_obs_k, self.rollout_obs_h)
        skip = sim.out["done"] if self.auto_reset and self.autoreset_mode == "next_step" and sim.out is not None else None
        out = sim.rollout_obs(actions, ped_cmd=human_actions if self.pedestrian_model == "external" else None, skip=skip)
        if E == 1:
            out = {k: v[0] for k, v in sim.rollout_obs_host().items()}
            wide = lambda v: v.astype(np.float64)
        else:
            out = dict(out)
            wide = lambda v: v
        obs, goals = out.pop("obs_last"), out.pop("goals_last")
        out["observation"] = {"observation": wide(obs), "achieved_goal": wide(goals[..., :2]), "desired_goal": wide(goals[..., 2:])}
        if "obs_all" in out:
            obs, goals = out.pop("obs_all"), out.pop("goals_all")
            out["observations"] = {"observation": wide(obs), "achieved_goal": wide(goals[..., :2]),
                                   "desired_goal": wide(goals[..., 2:])}
        return out

    @staticmethod
    def _rollout_actions(actions, E, K, H):
        """rollout()'s actions as [E,K,H,2]: a device tensor stays one ([K,H,2] expanded), an array-like becomes a float64 host
        tensor ([K,H,2] broadcast over the arenas)."""
        import torch
        if hasattr(actions, "is_cuda"):
            return actions.expand(E, K, H, 2) if tuple(actions.shape) == (K, H, 2) else actions
        a = np.asarray(actions, dtype=np.float64)
        if a.shape == (K, H, 2):
            a = np.broadcast_to(a, (E, K, H, 2))
        if a.shape != (E, K, H, 2):
            raise ValueError("rollout() takes actions of shape (%d, %d, %d, 2) or (%d, %d, 2), not %r" % (E, K, H, K, H, a.shape))
        return torch.from_numpy(np.array(a, dtype=np.float64, order="C"))               # (a writable copy)

    def planner_action(self):
        """What info['planner'] of the latest step() holds (local_planner='dwa'); valid after reset() and reset(mask) too:
        {'action' [E,2] float64 in action_kind's form, 'twist' [E,2] float64 (v, omega), 'clearance' [E] float32 metres, 'best' [E]
        int32, 'status' [E] uint8}.  local_planner='mppi': {'action' [E,2], 'best' [E] int32, 'cost_best' [E] float64, 'ess' [E]
        float64, 'status' [E] uint8 (1 ok, 2 every sequence crashed, 0 skipped)}."""
        return self._latest("planner", self.local_planner, "planner_action", "local_planner='dwa' or 'mppi'")

    def goal_path(self):
        """What info['goal_path'] of the latest step() holds (goal_path=True); valid after reset() and reset(mask) too:
        {'distance' [E] float32 metres, 'subgoal' [E,2] float32 in the robot's frame, 'status' [E] uint8}."""
        return self._latest("goal_path", self.goal_path_on, "goal_path", "goal_path=True")

    def goal_field(self):
        """The distance-to-goal fields on the device (goal_path=True): uint16 [E, H/5, W/5], NavSim.goal_field()."""
        self._latest("goal_path", self.goal_path_on, "goal_field", "goal_path=True")
        return self.sim.goal_field()

    def observed_humans(self):
        """What info['humans'] of the latest step() holds (observe_humans=K); valid after reset() and reset(mask) too: {'state'
        [E,K,5] x, y, vx, vy in the robot's frame and the distance, nearest first; 'index' [E,K] the pedestrian of the row, -1 =
        unused; 'count' [E] pedestrians seen, which may exceed K; 'visible' [E,N] bool}."""
        return self._latest("humans", self.observe_humans, "observed_humans", "observe_humans=K")

    # info['episode']: gymnasium's names for return and length, the build's own for the rest -> NavSim.episode_stats()'s rows
    _EPISODE_KEYS = (("r", "ep_return"), ("l", "ep_length"), ("path_length", "ep_path_length"),
                     ("min_clearance", "ep_min_clearance"), ("discomfort_steps", "ep_discomfort_steps"), ("outcome", "ep_outcome"))

    def episode_totals(self, reset=True):
        """Finished episodes since the last call (episode_stats=True): {'episodes', 'successes', 'crashes', 'time_limits',
        'steps'} -- steps being those of the finished episodes.  The feature's only device -> host copy."""
        if not self.episode_stats:
            raise RuntimeError("episode_totals() needs NavGymEnv(episode_stats=True)")
        if self.sim is None:
            return {k: 0 for k in abi.EPISODE_TOTALS}
        return self.sim.episode_totals(reset=reset)

    def counters(self, reset=True):
        """What the device-side reset path served and what its caps left waiting since the last call (abi.COUNTERS):
        regen_served / regen_unserved (finished arenas beyond cfg.regen_cap play their next episode on the old map),
        replan_served / replan_unserved (pedestrians beyond replan_cap wait for the next step), routes_cut (routes
        longer than max_waypoints) and routes_resumed (cut routes continued to their own goal)."""
        if self.sim is None:
            return {k: 0 for k in abi.COUNTERS}
        return self.sim.counters(reset=reset)

    def human_scans(self):
        """The pedestrians' own 512-beam half-plane scans (env.py:685-693), float32 [E, N, 512]: what
        the reference stacks and feeds to HumanPolicy.  With pedestrian_model='external' a caller can run
        that policy (or any other) on them and pass the resulting (v, w) to step(human_actions=...)."""
        return self.sim.ped_scans()

    # ---- HER batch API (env.py:464-589) ---------------------------------------------------------------
    def _rd(self, obs):
        import torch
        from . import sim as simmod
        o = torch.as_tensor(np.asarray(obs["observation"])) if not hasattr(obs["observation"], "is_cuda") else obs["observation"]
        g = torch.as_tensor(np.asarray(obs["desired_goal"])) if not hasattr(obs["desired_goal"], "is_cuda") else obs["desired_goal"]
        o = o.to(self.device)
        if o.dtype not in (torch.float32, torch.float64):
            o = o.double()
        return simmod.reward_done(self.sim.cfg, o.reshape(-1, o.shape[-1]), g.to(self.device).reshape(-1, 2),
                                  self.scan_threshold, self.scan_discomfort_threshold)

    def compute_rewards(self, actions, obs, make_render_reward_txt=False):
        return self._rd(obs)["reward"].cpu().numpy()

    def compute_terminals(self, obs):
        """Success or crash of each observation (env.py:491-512).  Terminal only: the time limit (max_episode_steps) is not a
        function of the observation and is not part of it -- step() reports it as info['TimeLimit.truncated']."""
        return self._rd(obs)["done"].cpu().numpy().astype(bool)

    def compute_reward(self, action, obs, make_render_reward_txt=False):
        return self.compute_rewards(np.asarray(action)[None], {k: np.asarray(v)[None] for k, v in obs.items()})[0]

    def compute_done(self, obs):
        """compute_terminals of one observation: success or crash, never the time limit."""
        return self.compute_terminals({k: np.asarray(v)[None] for k, v in obs.items()})[0]

    def compute_info(self, obs):
        r = self._rd({k: np.asarray(v)[None] for k, v in obs.items()})
        return {"is_success": np.float32(r["is_success"][0].item()), "is_crash": np.float32(r["is_crash"][0].item()),
                "distance": float(r["distance"][0].item())}

    def render(self, mode="human", arena=0, text=True):
        """The reference's picture of ONE arena (env.py:833-1050) as a float32 BGR array [800, 800, 3] in [0, 1]:
        map, goal, pedestrians with local goals, robot with its three rectangles, lidar returns.  Host-side NumPy
        (render.py); the debug text (env.py:1035-1046: observation tail and reward terms, `text=False` leaves it out) is drawn
        with a built-in font; the reference's OpenCV window is not opened -- both modes return the image.  `arena`
        selects which arena of the batch is drawn."""
        if self.sim is None:
            raise RuntimeError("call reset() before render()")
        from . import render as rd
        t, e, cfg = self.sim.t, int(arena), self.cfg
        occ = self.sim.occupancy(e)
        map_info = {"data": occ.astype(np.int8) * 100, "origin": (cfg.origin_x, cfg.origin_y),
                    "resolution": cfg.resolution, "width": self.map_size, "height": self.map_size}
        spec = robots.ROBOTS[self.robot_type]
        rp = t["robot_pose"][e].cpu().numpy()
        goal = t["robot_goal"][e].cpu().numpy()
        robot = dict(px=rp[0], py=rp[1], theta=rp[2], gx=goal[0], gy=goal[1], footprint=spec["footprint"],
                     threshold_footprint=spec["threshold_footprint"],
                     discomfort_threshold_footprint=spec["discomfort_threshold_footprint"])
        humans = []
        if "n_peds" in t:
            pp = t["ped_pose"][e].cpu().numpy()
            wp = t["ped_waypoints"][e, :, 0].cpu().numpy()
            for i in range(int(t["n_peds"][e])):
                humans.append(dict(px=pp[i, 0], py=pp[i, 1], theta=pp[i, 2], gx=wp[i, 0], gy=wp[i, 1],
                                   footprint=robots.HUMAN["footprint"]))
        o = self.sim.obs[e].cpu().numpy()
        B = cfg.n_beams
        scan = o[(cfg.n_scan_stack - 1) * B: cfg.n_scan_stack * B]
        img = rd.render_arena(map_info, robot, humans, scan, float(o[-1]),
                              dict(angle_min=cfg.angle_min, angle_last=cfg.angle_last, range_max=np.float32(cfg.range_max)))
        if text:
            self._make_render_txt(e)
            rd.overlay_text(img, self.render_obs_txt, self.render_reward_txt)
        return img

    def _make_render_txt(self, e=0):
        """render_obs_txt / render_reward_txt of arena e (env.py:182-217): the observation's tail and the six terms of
        compute_rewards for it, evaluated on the host from the device's latest observation (render.reward_terms)."""
        from . import render as rd
        cfg = self.cfg
        o = self.sim.obs[e].cpu().numpy().astype(np.float64)
        B, S = cfg.n_beams, cfg.n_scan_stack
        tail = o[S * B:]                                   # prev_pose(2) pose(2) vel(2) yaw (env.py:455)
        goal = self.sim.out["desired_goal"][e].cpu().numpy() if "desired_goal" in self.sim.out else self.sim.t["robot_goal"][e].cpu().numpy()
        steps = int(self.sim.t["steps"][e]) if "steps" in self.sim.t else 0
        self.render_obs_txt = rd.obs_text(steps, tail[0:2], tail[2:4], tail[4:6], tail[6], goal)
        factors = {k: getattr(self, k) for k in ("reward_scale", "reward_success_factor", "reward_crash_factor",
                                                 "reward_progress_factor", "reward_forward_factor", "reward_rotation_factor",
                                                 "reward_discomfort_factor")}
        terms = rd.reward_terms(self.sim.obs[e].cpu().numpy()[(S - 1) * B: S * B], tail[0:2], tail[2:4], tail[4:6], goal,
                                self.scan_threshold.cpu().numpy(), self.scan_discomfort_threshold.cpu().numpy(), factors,
                                self.distance_threshold)
        self.render_reward_txt = rd.reward_text(terms)
        return terms

    def close(self):
        if self.sim is not None:
            self.sim.close()                        # (staging passes in flight on a side stream: wait before the arrays go)
        self.sim = None
        self._views = {}

    # ---- EzPickle (env.py:30, 56-78): a pickle carries the constructor's arguments, the copy is built from them -----------
    def __getstate__(self):
        return {"_ezpickle_kwargs": dict(self._ctor_kwargs)}

    def __setstate__(self, d):
        self.__init__(**d["_ezpickle_kwargs"])

    def __reduce__(self):
        return (_rebuild_env, (type(self), dict(self._ctor_kwargs)))

    def state_dict(self):
        """The simulation itself (every device array of the state, the observation / output buffers, their parity) as
        host tensors: `load_state_dict` on an environment made with the same arguments and reset() once continues the
        rollout bit for bit.  (Not part of the reference's API: its pickles carry the constructor arguments only.)"""
        if self.sim is None:
            raise RuntimeError("call reset() before state_dict()")
        import torch
        torch.cuda.synchronize(self.sim.device)
        # (a world with slot tables -- the pipelined reset path -- holds 2 E map slots, E of them staged worlds that are not part
        #  of the snapshot: the arenas' maps are saved in arena order, the table itself is not)
        sd = {}
        for k in self.sim.t:
            if k.startswith(("replan_ws", "regen_ws", "policy_ws")) or k == "map_slot":
                continue
            sd["t." + k] = self.sim.by_arena(k).detach().cpu().clone()
        for i in (0, 1):
            sd["obs.%d" % i] = self.sim.obs_buf[i].cpu().clone()
            for k, v in self.sim.out_buf[i].items():
                sd["out.%d.%s" % (i, k)] = v.cpu().clone()
            if self.sim.due is not None:
                sd["due.%d" % i] = self.sim.due[i].cpu().clone()
            if self.sim.final_buf is not None:
                for k, v in self.sim.final_buf[i].items():
                    sd["final.%d.%s" % (i, k)] = v.cpu().clone()
        if self.sim.ep_acc is not None:                    # episode statistics: the episodes in progress and the totals
            for k, v in self.sim.ep_acc.items():
                sd["episode." + k] = v.cpu().clone()
            sd["episode.totals"] = self.sim.ep_totals.cpu().clone()
        sd["cur"] = int(self.sim.cur)
        sd["steps_launched"] = int(self.sim._steps_launched)
        sd["episode_batch"] = int(self._episode_batch)
        return sd

    def load_state_dict(self, sd):
        if self.sim is None:
            raise RuntimeError("call reset() once before load_state_dict() (it allocates the device arrays)")
        import torch
        torch.cuda.synchronize(self.sim.device)
        slots = self.sim.t.get("map_slot")
        if slots is not None:                              # the snapshot's maps go to the slots 0 .. E - 1, in arena order
            slots.copy_(torch.arange(self.num_envs, dtype=slots.dtype, device=slots.device))
        for k, v in sd.items():
            if k.startswith("t."):
                dst = self.sim.t[k[2:]]
                if slots is not None and k[2:] in self.sim.MAPS:     # (2 E slots; a packed field is one flat blob)
                    dst.reshape(2 * self.num_envs, -1)[: self.num_envs].copy_(v.reshape(self.num_envs, -1))
                else:
                    dst.copy_(v)
        for i in (0, 1):
            self.sim.obs_buf[i].copy_(sd["obs.%d" % i])
            for k, v in self.sim.out_buf[i].items():
                v.copy_(sd["out.%d.%s" % (i, k)])
            if self.sim.due is not None:
                self.sim.due[i].copy_(sd["due.%d" % i])
            if self.sim.final_buf is not None:
                for k, v in self.sim.final_buf[i].items():
                    if "final.%d.%s" % (i, k) in sd:
                        v.copy_(sd["final.%d.%s" % (i, k)])
        self.sim.cur = int(sd["cur"])
        if self.sim.ep_acc is not None:                    # (a snapshot without them: cleared ones; with them and no feature: ignored)
            if "episode.totals" in sd:
                for k, v in self.sim.ep_acc.items():
                    v.copy_(sd["episode." + k])
                self.sim.ep_totals.copy_(sd["episode.totals"])
            else:
                self.sim.clear_episode_stats()
                self.sim.ep_totals.zero_()
        if self.sim.pregen:                                # the staged worlds are not part of the snapshot: stage them again
            self.sim.restage_all(slots_from_live=True)
        self.sim._steps_launched = int(sd["steps_launched"])
        self._episode_batch = int(sd["episode_batch"])
        self._map_info = None
        self._humans_of_episode = None
        # (no part of the snapshot: functions of the state just loaded, of which the goal path's keys know nothing)
        self._run_products(rebuild=self._goal_all)
        torch.cuda.synchronize(self.sim.device)
        self._obs_dict()


def _rebuild_env(cls, kwargs):
    return cls(**kwargs)
