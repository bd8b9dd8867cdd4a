"""ctypes mirror of include/navsim.h (the C ABI of the batched NavGym step).

Pure declarations: importing this module touches neither the GPU nor the shared library.
Field order and types must match include/navsim.h exactly; tests/test_abi.py compares
``ctypes.sizeof`` with the ``sizeof`` the compiled library reports.
"""
import ctypes as C

ABI_VERSION = 7

OK = 0
E_ARG = -1
E_LAUNCH = -2
E_UNSUPPORTED = -3
E_NODEVICE = -4

PED_NONE = 0
PED_EXTERNAL = 1
PED_SFM = 2

MAX_PEDS = 64
MAX_WAYPOINTS = 256     # upper limit of cfg.max_waypoints (the stride P of ped_waypoints; navsim_default_config: 64)
OBS_TAIL = 7

FIELD_F32 = 0
FIELD_U16T = 1
FIELD_TILE = 8

MARCH_F64 = 0          # t += max(fl32(fl64(d) * 0.999), 1)
MARCH_F32 = 1          # t += max(d * 0.999f, 1): RangeLib.h's float member step_coeff (default since ABI 4)
MARCH_F32_FMA = 2      # MARCH_F32 with the sample position contracted into an FMA (GCC -O3 -march=native on FMA hardware)
MARCH_RULES = (MARCH_F64, MARCH_F32, MARCH_F32_FMA)

STEP_ALL, STEP_NOT_DUE, STEP_DUE = 0, 1, 2      # navsim_step_part

AUTORESET_NONE, AUTORESET_SAME_STEP, AUTORESET_NEXT_STEP = 0, 1, 2      # cfg.auto_reset (include/navsim.h NAVSIM_AUTORESET_*)

ACTION_TWIST = 0       # io.action = (v, omega)
ACTION_WHEELS = 1      # io.action = (omega_left, omega_right) of a skid-steer base, rad/s

N_COUNTERS = 8
COUNTERS = ("regen_served", "regen_unserved", "replan_served", "replan_unserved", "routes_cut", "routes_resumed",
            "regen_short", "regen_late")


class NavsimConfig(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32),
        ("n_beams", C.c_int32),
        ("map_h", C.c_int32),
        ("map_w", C.c_int32),
        ("max_peds", C.c_int32),
        ("n_scan_stack", C.c_int32),
        ("ped_model", C.c_int32),
        ("lidar_legs", C.c_int32),
        ("auto_reset", C.c_int32),
        ("n_spawn", C.c_int32),
        ("add_scan_noise", C.c_int32),
        ("env_index_base", C.c_int32),
        ("field_format", C.c_int32),
        ("shared_field", C.c_int32),
        ("resolution", C.c_double),
        ("origin_x", C.c_double),
        ("origin_y", C.c_double),
        ("time_step", C.c_double),
        ("angle_min", C.c_double),
        ("angle_last", C.c_double),
        ("range_max", C.c_double),
        ("axle_offset", C.c_double),
        ("min_turning_radius", C.c_double),
        ("distance_threshold", C.c_double),
        ("reward_scale", C.c_double),
        ("reward_success_factor", C.c_double),
        ("reward_crash_factor", C.c_double),
        ("reward_progress_factor", C.c_double),
        ("reward_forward_factor", C.c_double),
        ("reward_rotation_factor", C.c_double),
        ("reward_discomfort_factor", C.c_double),
        ("sfm_tau", C.c_double),
        ("sfm_k_desired", C.c_double),
        ("sfm_k_social", C.c_double),
        ("sfm_k_obstacle", C.c_double),
        ("sfm_lambda", C.c_double),
        ("sfm_gamma", C.c_double),
        ("sfm_n", C.c_double),
        ("sfm_n_prime", C.c_double),
        ("sfm_sigma_obstacle", C.c_double),
        ("sfm_agent_radius", C.c_double),
        ("seed", C.c_uint64),
        ("ped_angle_min", C.c_double),
        ("ped_angle_last", C.c_double),
        ("ped_range_max", C.c_double),
        ("ped_n_beams", C.c_int32),
        ("regen_plan", C.c_int32),
        ("robot_seen_footprint", C.c_double * 8),
        ("regen_cap", C.c_int32),
        ("obstacle_number", C.c_int32),
        ("obstacle_width_lo", C.c_double),
        ("obstacle_width_hi", C.c_double),
        ("spawn_clearance", C.c_double),
        ("ped_clearance", C.c_double),
        ("min_goal_dist", C.c_double),
        ("max_goal_dist", C.c_double),
        ("ped_min_robot_dist", C.c_double),
        ("ped_min_goal_dist", C.c_double),
        ("v_pref_lo", C.c_double),
        ("v_pref_hi", C.c_double),
        ("has_legs_ratio", C.c_double),
        ("regen_indoor_ratio", C.c_double),
        ("obstacle_number_hi", C.c_int32),
        ("corridor_width_lo", C.c_int32),
        ("corridor_width_hi", C.c_int32),
        ("iterations_lo", C.c_int32),
        ("iterations_hi", C.c_int32),
        ("num_humans_lo", C.c_int32),
        ("num_humans_hi", C.c_int32),
        ("outdoor_map_size", C.c_int32),
        ("scan_noise_std_lo", C.c_double),
        ("scan_noise_std_hi", C.c_double),
        ("march_rule", C.c_int32),
        ("step_block", C.c_int32),
        ("ped_split", C.c_int32),
        ("regen_check_discomfort", C.c_int32),
        ("rect_lds", C.c_int32),
        ("max_waypoints", C.c_int32),
        ("action_kind", C.c_int32),
        ("clamp_action", C.c_int32),
        ("wheel_radius", C.c_double),
        ("wheel_track", C.c_double),
        ("linvel_lo", C.c_double),
        ("linvel_hi", C.c_double),
        ("rotvel_lo", C.c_double),
        ("rotvel_hi", C.c_double),
        ("closed_maps", C.c_int32),
        ("defer_reset_scan", C.c_int32),
        ("regen_min_steps", C.c_int32),
        ("max_episode_steps", C.c_int32),      # ABI 7 (in the tail padding: the size stays 624 bytes)
    ]

    def copy(self):
        other = NavsimConfig()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(self))
        return other


_P = C.c_void_p


class NavsimState(C.Structure):
    _fields_ = [(name, _P) for name in (
        "field", "field_overflow", "rect_table", "beam_table", "scan_threshold", "scan_discomfort", "scan_noise_std",
        "robot_pose", "robot_goal", "prev_action", "prev_pose", "n_hist", "episode", "steps",
        "n_peds", "ped_pose", "ped_vel", "ped_prev_yaw", "ped_dist", "ped_v_pref", "ped_has_legs",
        "ped_waypoints", "ped_n_waypoints", "ped_cmd",
        "spawn_pose", "spawn_goal", "costmap", "arena_cost", "launch_order", "regen_draws",
        "ped_goal", "counters", "rect_index",
        "ped_wp_head", "ped_due", "ped_due_prev", "done_steps", "map_slot",
    )]


POLICY_FIELDS = ("cv1_w", "cv1_b", "cv2_w", "cv2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "a1_w", "a1_b", "a2_w", "a2_b")
POLICY_SHAPES = {"cv1_w": (32, 3, 5), "cv1_b": (32,), "cv2_w": (32, 32, 3), "cv2_b": (32,), "fc1_w": (256, 4096),
                 "fc1_b": (256,), "fc2_w": (128, 260), "fc2_b": (128,), "a1_w": (128,), "a1_b": (1,), "a2_w": (128,),
                 "a2_b": (1,)}
# reference state_dict names (human_policy.py:24-30) -> fields of navsim_policy_weights
POLICY_STATE_DICT = {"act_fea_cv1.weight": "cv1_w", "act_fea_cv1.bias": "cv1_b", "act_fea_cv2.weight": "cv2_w",
                     "act_fea_cv2.bias": "cv2_b", "act_fc1.weight": "fc1_w", "act_fc1.bias": "fc1_b",
                     "act_fc2.weight": "fc2_w", "act_fc2.bias": "fc2_b", "actor1.weight": "a1_w", "actor1.bias": "a1_b",
                     "actor2.weight": "a2_w", "actor2.bias": "a2_b"}


class NavsimPolicyWeights(C.Structure):
    _fields_ = [(name, _P) for name in POLICY_FIELDS]


class NavsimCrowdParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in (
        "time_step", "discomfort_dist", "map_size_m", "map_resolution", "success_reward", "collision_penalty",
        "discomfort_penalty_factor", "rotation_penalty_factor", "timeout_penalty", "time_limit")]


class NavsimCrowdMapParams(C.Structure):
    _fields_ = [("angular_min", C.c_double), ("angular_max", C.c_double), ("angular_max_range", C.c_double),
                ("angular_dim", C.c_int32), ("normalize", C.c_int32), ("map_size_m", C.c_double),
                ("map_resolution", C.c_double), ("submap_size_m", C.c_double)]


class NavsimOrcaParams(C.Structure):
    _fields_ = [("time_step", C.c_float), ("neighbor_dist", C.c_float), ("time_horizon", C.c_float),
                ("time_horizon_obst", C.c_float), ("max_neighbors", C.c_int32)]


class NavsimPedOrcaParams(C.Structure):
    _fields_ = [("orca", NavsimOrcaParams), ("ped_radius", C.c_double), ("robot_radius", C.c_double),
                ("safety_space", C.c_double), ("robot_visible", C.c_int32)]


# navsim_ped_observe: the rule's parameters, and the four output arrays (dtype, trailing shape behind E; K = max_obs, N = max_peds)
class NavsimPedObserveParams(C.Structure):
    _fields_ = [("ped_radius", C.c_double), ("sensor_range", C.c_double), ("max_obs", C.c_int32), ("rays", C.c_int32),
                ("occlusion", C.c_int32), ("fov", C.c_int32)]


PED_OBSERVATION = {"state": ("float32", ("K", 5)), "index": ("int32", ("K",)), "count": ("int32", ()), "visible": ("uint8", ("N",))}


class NavsimPedObservation(C.Structure):
    _fields_ = [(name, _P) for name in PED_OBSERVATION]


# navsim_goal_path: the rule's parameters, the field with its keys, and the three output arrays (dtype, trailing shape behind E)
class NavsimGoalPathParams(C.Structure):
    _fields_ = [("hard_clearance", C.c_double), ("clearance", C.c_double), ("lookahead", C.c_double), ("band_cost", C.c_int32)]


class NavsimGoalField(C.Structure):
    _fields_ = [("dist", _P), ("key", _P), ("rebuilds", _P)]


GOAL_PATH_OUT = {"distance": ("float32", ()), "subgoal": ("float32", (2,)), "status": ("uint8", ())}


class NavsimGoalPathOut(C.Structure):
    _fields_ = [(name, _P) for name in GOAL_PATH_OUT]


GOAL_PATH_OK, GOAL_PATH_REACHED_GOAL_CELL, GOAL_PATH_OFF_FIELD = 1, 2, 4
GOAL_FIELD_INF = 0xFFFF

# navsim_dwa: the rule's parameters and the output arrays (dtype, trailing shape behind E; C = n_v n_w candidates)
DWA_MAX_DISCS = 4


class NavsimDwaParams(C.Structure):
    _fields_ = [("acc_lin", C.c_double), ("acc_rot", C.c_double), ("body_radius", C.c_double),
                ("body_offset", C.c_double * DWA_MAX_DISCS), ("ped_radius", C.c_double), ("margin", C.c_double),
                ("clearance_cap", C.c_double), ("w_progress", C.c_double), ("w_heading", C.c_double), ("w_clearance", C.c_double),
                ("w_speed", C.c_double), ("n_discs", C.c_int32), ("n_v", C.c_int32), ("n_w", C.c_int32), ("horizon", C.c_int32),
                ("use_peds", C.c_int32)]


DWA_OUT = {"twist": ("float64", (2,)), "action": ("float64", (2,)), "clearance": ("float32", ()), "best": ("int32", ()),
           "status": ("uint8", ()), "scores": ("float64", ("C",)), "first_hit": ("int32", ("C",))}


class NavsimDwaOut(C.Structure):
    _fields_ = [(name, _P) for name in DWA_OUT]


DWA_OK, DWA_BLOCKED = 1, 2

# navsim_local_map: the rule's parameters; the output is one float32 array [E, channels, size, size]
LOCAL_MAP_MAX = 128


class NavsimLocalMapParams(C.Structure):
    _fields_ = [("cell", C.c_double), ("ahead", C.c_double), ("cap", C.c_double), ("ped_radius", C.c_double),
                ("size", C.c_int32), ("channels", C.c_int32)]


LOCAL_MAP_OUT = {"map": ("float32", ("C", "G", "G"))}       # (dtype, trailing shape behind E; C = channels, G = size)

# navsim_scan_labels: the labels of a beam, and the four output arrays (dtype, trailing shape behind E; B = n_beams, N = max_peds)
BEAM_NONE, BEAM_WALL, BEAM_PED_BODY, BEAM_PED_LEG = 0, 1, 2, 3
SCAN_LABELS_OUT = {"range": ("float32", ("B",)), "label": ("uint8", ("B",)), "index": ("int8", ("B",)), "hits": ("int32", ("N",))}


class NavsimScanLabelsOut(C.Structure):
    _fields_ = [(name, _P) for name in SCAN_LABELS_OUT]


# navsim_lookahead: the rule's parameters and the nine output arrays (dtype, trailing shape behind E; K = n_actions; status is [E])
LOOKAHEAD_MAX = 64


class NavsimLookaheadParams(C.Structure):
    _fields_ = [("n_actions", C.c_int32), ("range", C.c_double)]


LOOKAHEAD_OUT = {"reward": ("float64", ("K",)), "done": ("uint8", ("K",)), "is_success": ("float32", ("K",)),
                 "is_crash": ("float32", ("K",)), "discomfort": ("uint8", ("K",)), "distance": ("float64", ("K",)),
                 "margin": ("float32", ("K",)), "pose": ("float64", ("K", 3)), "status": ("uint8", ())}


class NavsimLookaheadOut(C.Structure):
    _fields_ = [(name, _P) for name in LOOKAHEAD_OUT]


# navsim_lookahead_obs: the lookahead's nine arrays, then the row of each candidate (dtype, trailing shape behind E; K = n_actions,
# B = n_beams, D = n_scan_stack * n_beams + OBS_TAIL; obs is optional: the call takes NULL for it)
LOOKOBS_NOISE_OFF, LOOKOBS_NOISE_STEP = 0, 1


class NavsimLookaheadObsParams(C.Structure):
    _fields_ = [("n_actions", C.c_int32), ("noise", C.c_int32)]


LOOKAHEAD_OBS_OUT = dict(LOOKAHEAD_OUT, scan=("float32", ("K", "B")), tail=("float32", ("K", 7)), goals=("float32", ("K", 4)),
                         truncated=("uint8", ("K",)), obs=("float32", ("K", "D")))


class NavsimLookaheadObsOut(C.Structure):
    _fields_ = [(name, _P) for name in LOOKAHEAD_OBS_OUT]


# navsim_rollout: the rule's parameters and the ten output arrays (dtype, trailing shape behind E; K = n_seq, H = horizon; status is [E])
ROLLOUT_MAX_K = 256
ROLLOUT_MAX_H = 32
OUTCOME_SUCCESS, OUTCOME_CRASH, OUTCOME_TIME_LIMIT = 1, 2, 4      # bits of navsim_rollout's outcome (navsim_episode_stats' ep_outcome)


class NavsimRolloutParams(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("horizon", C.c_int32), ("range", C.c_double), ("gamma", C.c_double)]


ROLLOUT_OUT = {"reward": ("float64", ("K", "H")), "pose": ("float64", ("K", "H", 3)), "ret": ("float64", ("K",)),
               "length": ("int32", ("K",)), "outcome": ("uint8", ("K",)), "discomfort_steps": ("int32", ("K",)),
               "min_margin": ("float32", ("K",)), "distance": ("float64", ("K",)), "exact_steps": ("int32", ("K",)),
               "status": ("uint8", ())}


class NavsimRolloutOut(C.Structure):
    _fields_ = [(name, _P) for name in ROLLOUT_OUT]


# navsim_rollout_obs: the rule's parameters, the rollout's ten arrays and the rows (dtype, trailing shape behind E; K = n_seq,
# H = horizon, D = n_scan_stack * n_beams + OBS_TAIL; obs_all and goals_all are optional: the call takes NULL for both)
class NavsimRolloutObsParams(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("horizon", C.c_int32), ("noise", C.c_int32), ("gamma", C.c_double)]


ROLLOUT_OBS_OUT = dict(ROLLOUT_OUT, obs_last=("float32", ("K", "D")), goals_last=("float32", ("K", 4)),
                       obs_all=("float32", ("K", "H", "D")), goals_all=("float32", ("K", "H", 4)))


class NavsimRolloutObsOut(C.Structure):
    _fields_ = [(name, _P) for name in ROLLOUT_OBS_OUT]


# navsim_mppi: the rule's parameters, the persistent workspace (with navsim_rollout's ten arrays inside) and the five output arrays
# (dtype, trailing shape behind E; K = n_samples, H = horizon)
MPPI_MAX_ITERATIONS = 8
MPPI_OK, MPPI_ALL_CRASH = 1, 2


class NavsimMppiParams(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("horizon", C.c_int32), ("iterations", C.c_int32), ("stop_sample", C.c_int32),
                ("select", C.c_int32), ("pad_", C.c_int32), ("range", C.c_double), ("gamma", C.c_double),
                ("sigma", C.c_double * 2), ("lo", C.c_double * 2), ("hi", C.c_double * 2), ("init_action", C.c_double * 2),
                ("beta", C.c_double), ("alpha", C.c_double), ("lam", C.c_double), ("w_goal", C.c_double),
                ("w_crash", C.c_double), ("off_field_cost", C.c_double)]       # lam: the header's `lambda`


MPPI_WS = {"plan": ("float64", ("H", 2)), "plan_key": ("int64", (2,)), "actions": ("float64", ("K", "H", 2)),
           "cost": ("float64", ("K",))}                                       # (+ ROLLOUT_OUT's arrays, in the struct's `roll`)


class NavsimMppiWs(C.Structure):
    _fields_ = [("plan", _P), ("plan_key", _P), ("actions", _P), ("roll", NavsimRolloutOut), ("cost", _P)]


MPPI_OUT = {"action": ("float64", (2,)), "best": ("int32", ()), "cost_best": ("float64", ()), "ess": ("float64", ()),
            "status": ("uint8", ())}


class NavsimMppiOut(C.Structure):
    _fields_ = [(name, _P) for name in MPPI_OUT]


# navsim_ped_forecast: the rule's parameters and the eight output arrays (dtype, trailing shape behind E; H = horizon, N = max_peds;
# exact_steps and status are [E]).  Time-major: a consumer that wants [E,N,H,.] takes a transposed view
FORECAST_MAX_H = 32
FORECAST_HOLD, FORECAST_STOP, FORECAST_ACTIONS = 0, 1, 2          # navsim_ped_forecast_params.robot
FORECAST_TRUE, FORECAST_CONST_VEL = 0, 1                          # navsim_ped_forecast_params.model


class NavsimPedForecastParams(C.Structure):
    _fields_ = [("horizon", C.c_int32), ("robot", C.c_int32), ("model", C.c_int32), ("pad_", C.c_int32)]


FORECAST_OUT = {"pose": ("float64", ("H", "N", 3)), "vel": ("float64", ("H", "N", 2)), "rel": ("float32", ("H", "N", 2)),
                "robot_pose": ("float64", ("H", 3)), "min_dist": ("float64", ("N",)), "min_step": ("int32", ("N",)),
                "exact_steps": ("int32", ()), "status": ("uint8", ())}


class NavsimPedForecastOut(C.Structure):
    _fields_ = [(name, _P) for name in FORECAST_OUT]


ORCA_MAX_AGENTS = 64
ORCA_MAX_EDGES = 128
CROWD_MAX_VERTS = 8
CROWD_INFO = ("Nothing", "Timeout", "ReachGoal", "Collision", "CollisionOtherAgent", "Danger")


class NavsimStepIO(C.Structure):
    _fields_ = [(name, _P) for name in (
        "action", "obs_prev", "obs", "achieved_goal", "desired_goal",
        "reward", "done", "is_success", "is_crash", "distance",
        "final_obs", "final_goals", "reset_mask",          # ABI 6
        "truncated",                                       # ABI 7
    )]


# navsim_episode_stats: the accumulators of the episode in progress, what the latest update published for the arenas that
# finished (EPISODE_PUBLISHED: kept in pairs like everything a step returns), the running totals
EPISODE_ACCUMULATORS = {"ret": "float64", "length": "int32", "path_length": "float64", "min_clearance": "float64",
                        "discomfort_steps": "int32"}
EPISODE_PUBLISHED = {"ep_return": "float64", "ep_length": "int32", "ep_path_length": "float64", "ep_min_clearance": "float64",
                     "ep_discomfort_steps": "int32", "ep_outcome": "uint8"}
EPISODE_TOTALS = ("episodes", "successes", "crashes", "time_limits", "steps")
EPISODE_SUCCESS, EPISODE_CRASH, EPISODE_TIME_LIMIT = 1, 2, 4      # bits of ep_outcome


class NavsimEpisodeStats(C.Structure):
    _fields_ = [(name, _P) for name in tuple(EPISODE_ACCUMULATORS) + tuple(EPISODE_PUBLISHED) + ("totals",)]


# dtype / trailing shape of every state array, in units of (E, N, B, S, K, P, H, W)
STATE_LAYOUT = {
    "field": ("float32", ("E", "H", "W")),          # FIELD_F32; a uint8 blob for packed formats
    "field_overflow": ("float32", ("E", "H", "W")),
    "rect_table": ("int32", ("E", "T", 4)),         # 16-byte two-rectangle records of the 8x8 tiles
    "beam_table": ("float64", ("B", 2)),
    "scan_threshold": ("float32", ("B",)),
    "scan_discomfort": ("float32", ("B",)),
    "scan_noise_std": ("float32", ("E",)),
    "robot_pose": ("float64", ("E", 3)),
    "robot_goal": ("float64", ("E", 2)),
    "prev_action": ("float64", ("E", 2)),
    "prev_pose": ("float64", ("E", 3)),
    "n_hist": ("int32", ("E",)),
    "episode": ("int64", ("E",)),
    "steps": ("int64", ("E",)),
    "n_peds": ("int32", ("E",)),
    "ped_pose": ("float64", ("E", "N", 3)),
    "ped_vel": ("float64", ("E", "N", 2)),
    "ped_prev_yaw": ("float64", ("E", "N")),
    "ped_dist": ("float64", ("E", "N", 3)),
    "ped_v_pref": ("float64", ("E", "N")),
    "ped_has_legs": ("uint8", ("E", "N")),
    "ped_waypoints": ("float64", ("E", "N", "P", 2)),
    "ped_n_waypoints": ("int32", ("E", "N")),
    "ped_cmd": ("float64", ("E", "N", 2)),
    "spawn_pose": ("float64", ("E", "K", 3)),
    "spawn_goal": ("float64", ("E", "K", 2)),
    "costmap": ("uint8", ("E", "Hc", "Wc")),
    "arena_cost": ("int32", ("E",)),
    "launch_order": ("int32", ("E",)),
    "regen_draws": ("float64", ("E", 464)),         # tests only: draws supplied (NAVSIM_DRAW_* layout)
    "ped_goal": ("float64", ("E", "N", 2)),         # goal of every pedestrian's current route
    "counters": ("int64", (N_COUNTERS,)),           # uint64 on the device; the totals stay far below 2^63
    "rect_index": ("uint8", ("E", "R")),            # index form of rect_table: 256 rectangles x 8 B + 2 B per tile, per arena
    "ped_wp_head": ("int32", ("E", "N")),           # ABI 5: index of every pedestrian's current waypoint (the pop advances it)
    "ped_due": ("int64", ("E",)),                   # uint64 on the device: bit i = pedestrian i waits for navsim_replan (written by the step)
    "ped_due_prev": ("int64", ("E",)),              # the flags of the previous step (navsim_step_part)
    "done_steps": ("int32", ("E",)),                # length of the episode that ended last (cfg.regen_min_steps)
    "map_slot": ("int32", ("E",)),                  # slot of the five per-map arrays that holds arena e's map (NULL: e)
}

IO_LAYOUT = {
    "action": ("float64", ("E", 2)),
    "obs_prev": ("float32", ("E", "D")),
    "obs": ("float32", ("E", "D")),
    "achieved_goal": ("float32", ("E", 2)),
    "desired_goal": ("float32", ("E", 2)),
    "reward": ("float64", ("E",)),
    "done": ("uint8", ("E",)),
    "is_success": ("float32", ("E",)),
    "is_crash": ("float32", ("E",)),
    "distance": ("float64", ("E",)),
}


# ABI 6: the terminal observation of arenas that restart inside the step that ends their episode (NAVSIM_AUTORESET_SAME_STEP)
FINAL_LAYOUT = {
    "final_obs": ("float32", ("E", "D")),
    "final_goals": ("float32", ("E", 4)),           # achieved_goal (2), desired_goal (2) of that observation
}


# ABI 7: the arenas whose episode cfg.max_episode_steps cut in the step.  Allocated (and wired into io.truncated) only for a
# state made with a limit, so that what a step returns without one keeps its ABI-6 keys; the oracle has no limit and no such array
LIMIT_LAYOUT = {
    "truncated": ("uint8", ("E",)),
}


def rect_index_row_bytes(H, W):
    """navsim_rect_index_bytes(1, H, W): 256 list entries of 8 bytes, then 2 bytes per 8x8 tile (padded to 16)."""
    return 256 * 8 + ((((H + 7) // 8) * ((W + 7) // 8) * 2 + 15) // 16) * 16


def resolve_shape(shape, cfg):
    """Turns a symbolic shape of STATE_LAYOUT / IO_LAYOUT into integers for `cfg`."""
    sym = {
        "E": cfg.n_envs, "N": cfg.max_peds, "B": cfg.n_beams, "S": cfg.n_scan_stack,
        "K": max(cfg.n_spawn, 1), "P": cfg.max_waypoints, "H": cfg.map_h, "W": cfg.map_w,
        "D": cfg.n_scan_stack * cfg.n_beams + OBS_TAIL, "Hc": cfg.map_h // 5, "Wc": cfg.map_w // 5,
        "T": ((cfg.map_h + 7) // 8) * ((cfg.map_w + 7) // 8),
        "R": rect_index_row_bytes(cfg.map_h, cfg.map_w),
    }
    return tuple(sym[s] if isinstance(s, str) else s for s in shape)


def declare(lib, suffix=""):
    """Attaches argtypes/restypes for every entry point of include/navsim.h to `lib`.

    suffix="" is the HIP library (trailing stream argument); suffix="_cpu" is the oracle.
    """
    stream = [] if suffix else [_P]
    i32, f32, f64 = C.c_int32, C.c_float, C.c_double
    cfgp, stp, iop = C.POINTER(NavsimConfig), C.POINTER(NavsimState), C.POINTER(NavsimStepIO)

    def sig(name, args, res=C.c_int):
        fn = getattr(lib, name + suffix)
        fn.argtypes = args
        fn.restype = res
        return fn

    sig("navsim_default_config", [cfgp])
    if suffix:
        sig("navsim_build_dt", [_P, i32, i32, i32, _P])
    else:
        sig("navsim_build_dt", [_P, i32, i32, i32, _P, _P, C.c_size_t, _P])
    if not suffix:
        sig("navsim_field_bytes", [i32, i32, i32, i32], C.c_size_t)
        sig("navsim_build_field", [_P, i32, i32, i32, i32, _P, _P, _P, _P, C.c_size_t, _P])
        sig("navsim_rect_table_bytes", [i32, i32, i32], C.c_size_t)
        sig("navsim_build_rects_workspace_bytes", [i32, i32, i32], C.c_size_t)
        sig("navsim_build_rects", [_P, i32, i32, i32, _P, i32, _P, _P, _P, C.c_size_t, _P])
        sig("navsim_rect_index_bytes", [i32, i32, i32], C.c_size_t)
        sig("navsim_build_rect_index", [_P, i32, i32, i32, _P, _P, _P])
        sig("navsim_maps_closed", [_P, i32, i32, i32, _P, _P])
        sig("navsim_world_closed", [cfgp, stp, _P, _P])
    sig("navsim_cast_static", [_P, i32, i32, i32, _P, i32, f32, i32, _P] + stream)
    sig("navsim_render_polys", [_P, _P, i32, i32, _P, _P, i32, _P] + stream)
    sig("navsim_render_legs", [_P, _P, i32, i32, _P, _P, i32, _P] + stream)
    sig("navsim_integrate", [_P, _P, _P, i32, f64, f64] + stream)
    sig("navsim_reward_done", [cfgp, _P, _P, i32, i32, _P, _P, _P, _P, _P, _P, _P] + stream)
    sig("navsim_scan_threshold", [cfgp, _P, i32, _P] + stream)
    if not suffix:
        sig("navsim_beam_table", [cfgp, _P, _P])
        sig("navsim_debug_xy_to_ij", [cfgp, _P, i32, _P, i32, _P])
        sig("navsim_debug_kernarg_layout", [_P])
    sig("navsim_ped_scans", [cfgp, stp, _P] + stream)
    if not suffix:
        sig("navsim_ped_scans_part", [cfgp, stp, _P, i32, i32, _P])
        sig("navsim_ped_policy_part", [cfgp, stp, C.POINTER(NavsimPolicyWeights), _P, _P, _P, _P, C.c_size_t, i32, i32, _P])
    if suffix:
        sig("navsim_regen", [cfgp, stp, iop])
        sig("navsim_replan", [cfgp, stp, i32])
        sig("navsim_ped_policy", [cfgp, stp, C.POINTER(NavsimPolicyWeights), _P, _P, _P])
    else:
        sig("navsim_ped_policy_workspace_bytes", [cfgp], C.c_size_t)
        sig("navsim_ped_policy", [cfgp, stp, C.POINTER(NavsimPolicyWeights), _P, _P, _P, _P, C.c_size_t, _P])
        sig("navsim_ped_scan_policy", [cfgp, stp, C.POINTER(NavsimPolicyWeights), _P, _P, _P, _P, C.c_size_t, _P])
        sig("navsim_launch_order", [_P, _P, i32, _P])
        sig("navsim_replan_workspace_bytes", [cfgp, i32], C.c_size_t)
        sig("navsim_replan", [cfgp, stp, i32, _P, C.c_size_t, _P])
        sig("navsim_costmap", [_P, i32, i32, i32, _P, _P])
        sig("navsim_plan", [_P, _P, i32, i32, i32, f64, f64, f64, _P, _P, f64, i32, _P, _P, _P, _P, _P])
        sig("navsim_regen_workspace_bytes", [cfgp], C.c_size_t)
        sig("navsim_regen", [cfgp, stp, iop, _P, C.c_size_t, _P])
        sig("navsim_regen_swap", [cfgp, stp, stp, iop, _P, _P, _P, _P, _P])
        sig("navsim_regen_stage", [cfgp, stp, iop, _P, _P, _P, _P, C.c_size_t, _P])
        sig("navsim_regen_stage_part", [cfgp, stp, iop, _P, _P, _P, _P, C.c_size_t, i32, i32, _P])
        sig("navsim_step_install", [cfgp, stp, iop, stp, _P, _P, _P, _P, _P])
        sig("navsim_regen_helper", [_P])
        sig("navsim_step_install_replan", [cfgp, stp, iop, stp, _P, _P, _P, _P, C.c_int32, _P])
        sig("navsim_step_install_next", [cfgp, stp, iop, stp, _P, _P, _P, _P, _P, C.c_int32, _P])
        sig("navsim_reset_install", [cfgp, stp, iop, stp, _P, _P, _P, _P, _P, _P])
    sig("navsim_crowd_check", [C.POINTER(NavsimCrowdParams), i32, i32, i32, _P, _P, _P, _P, _P, _P, _P, _P, _P] + stream)
    mpp = C.POINTER(NavsimCrowdMapParams)
    sig("navsim_crowd_angular_map", [mpp, i32, i32, i32, _P, _P, _P, _P] + stream)
    sig("navsim_crowd_local_map", [mpp, i32, i32, _P, _P, i32, _P] + stream)
    sig("navsim_crowd_orca", [C.POINTER(NavsimOrcaParams), i32, i32, _P, _P, _P, i32, i32, _P, _P, _P, _P, _P, _P] + stream)
    sig("navsim_crowd_agent_step", [_P, _P, _P, i32, f64] + stream)
    if not suffix:
        sig("navsim_ped_orca", [cfgp, stp, C.POINTER(NavsimPedOrcaParams), _P, _P])
        sig("navsim_ped_orca_walls", [cfgp, stp, C.POINTER(NavsimPedOrcaParams), i32, _P, _P, _P])
    if not suffix:
        sig("navsim_prepare", [cfgp, stp, iop])
    sig("navsim_step", [cfgp, stp, iop] + stream)
    if not suffix:
        sig("navsim_step_part", [cfgp, stp, iop, i32, _P])
        sig("navsim_step_replan", [cfgp, stp, iop, i32, _P])
        # (a library built before the export existed -- NAVSIM_LIB, A/B runs -- loads without it: NavSim falls back to navsim_launch_order)
        if hasattr(lib, "navsim_step_sorted"):
            sig("navsim_step_sorted", [cfgp, stp, iop, _P, _P, _P])
    if not suffix and hasattr(lib, "navsim_episode_stats_update"):      # (as above: an older library of an A/B run loads without)
        sig("navsim_episode_stats_update", [cfgp, stp, iop, C.POINTER(NavsimEpisodeStats), _P])
        sig("navsim_episode_stats_clear", [cfgp, C.POINTER(NavsimEpisodeStats), _P, _P])
    if not suffix and hasattr(lib, "navsim_ped_observe"):               # (likewise; the oracle has no twin of it)
        sig("navsim_ped_observe", [cfgp, stp, C.POINTER(NavsimPedObserveParams), _P, C.POINTER(NavsimPedObservation), _P])
    if not suffix and hasattr(lib, "navsim_goal_path"):                 # (likewise)
        sig("navsim_goal_path", [cfgp, stp, C.POINTER(NavsimGoalPathParams), _P, _P, C.POINTER(NavsimGoalField),
                                 C.POINTER(NavsimGoalPathOut), _P])
        sig("navsim_goal_field_bytes", [cfgp], C.c_size_t)
        sig("navsim_debug_goal_path_sweeps", [_P])
    if not suffix and hasattr(lib, "navsim_dwa"):                       # (likewise)
        sig("navsim_dwa", [cfgp, stp, C.POINTER(NavsimDwaParams), _P, _P, C.POINTER(NavsimDwaOut), _P])
    if not suffix and hasattr(lib, "navsim_local_map"):                 # (likewise)
        sig("navsim_local_map", [cfgp, stp, C.POINTER(NavsimLocalMapParams), _P, _P, _P, _P])
    if not suffix and hasattr(lib, "navsim_scan_labels"):               # (likewise)
        sig("navsim_scan_labels", [cfgp, stp, _P, C.POINTER(NavsimScanLabelsOut), _P])
    if not suffix and hasattr(lib, "navsim_lookahead"):                 # (likewise)
        sig("navsim_lookahead", [cfgp, stp, C.POINTER(NavsimLookaheadParams), _P, _P, _P, C.POINTER(NavsimLookaheadOut), _P])
    if not suffix and hasattr(lib, "navsim_lookahead_obs"):             # (likewise)
        sig("navsim_lookahead_obs", [cfgp, stp, C.POINTER(NavsimLookaheadObsParams), _P, _P, _P, _P,
                                     C.POINTER(NavsimLookaheadObsOut), _P])
    if not suffix and hasattr(lib, "navsim_rollout"):                   # (likewise)
        sig("navsim_rollout", [cfgp, stp, C.POINTER(NavsimRolloutParams), _P, _P, _P, C.POINTER(NavsimRolloutOut), _P])
    if not suffix and hasattr(lib, "navsim_mppi"):                      # (likewise)
        sig("navsim_mppi", [cfgp, stp, C.POINTER(NavsimMppiParams), C.POINTER(NavsimGoalField), C.POINTER(NavsimGoalPathParams),
                            _P, _P, C.POINTER(NavsimMppiWs), C.POINTER(NavsimMppiOut), _P])
    if not suffix and hasattr(lib, "navsim_ped_forecast"):              # (likewise)
        sig("navsim_ped_forecast", [cfgp, stp, C.POINTER(NavsimPedForecastParams), _P, _P, _P, C.POINTER(NavsimPedForecastOut), _P])
    if not suffix and hasattr(lib, "navsim_rollout_obs"):               # (likewise)
        sig("navsim_rollout_obs", [cfgp, stp, C.POINTER(NavsimRolloutObsParams), _P, _P, _P, _P,
                                   C.POINTER(NavsimRolloutObsOut), _P])
    sig("navsim_reset_obs", [cfgp, stp, iop, _P] + stream)
    sig("navsim_restart", [cfgp, stp, _P] + stream)
    return lib


# every symbol include/navsim.h declares (tests check the .so exports all of them)
EXPORTS = (
    "navsim_abi_version", "navsim_error_string", "navsim_last_hip_error", "navsim_default_config",
    "navsim_build_dt_workspace_bytes", "navsim_build_dt", "navsim_field_bytes", "navsim_build_field",
    "navsim_rect_table_bytes", "navsim_build_rects_workspace_bytes", "navsim_build_rects",
    "navsim_rect_index_bytes", "navsim_build_rect_index", "navsim_maps_closed", "navsim_world_closed",
    "navsim_cast_static",
    "navsim_render_polys", "navsim_render_legs", "navsim_integrate", "navsim_reward_done",
    "navsim_scan_threshold", "navsim_beam_table", "navsim_ped_scans", "navsim_ped_scans_part", "navsim_ped_policy_part", "navsim_regen_workspace_bytes", "navsim_regen", "navsim_regen_swap", "navsim_regen_stage", "navsim_regen_stage_part", "navsim_step_install", "navsim_regen_helper", "navsim_step_install_replan", "navsim_step_install_next",
    "navsim_costmap", "navsim_plan", "navsim_launch_order", "navsim_replan_workspace_bytes", "navsim_replan", "navsim_ped_policy_workspace_bytes", "navsim_ped_policy", "navsim_ped_scan_policy",
    "navsim_crowd_check", "navsim_crowd_angular_map", "navsim_crowd_local_map", "navsim_crowd_orca", "navsim_crowd_agent_step", "navsim_ped_orca", "navsim_ped_orca_walls",
    "navsim_step", "navsim_step_sorted", "navsim_step_part", "navsim_step_replan", "navsim_prepare", "navsim_reset_obs", "navsim_restart", "navsim_reset_install", "navsim_step_kernel_name",
    "navsim_episode_stats_update", "navsim_episode_stats_clear", "navsim_ped_observe",
    "navsim_goal_path", "navsim_goal_field_bytes", "navsim_debug_goal_path_sweeps", "navsim_dwa", "navsim_local_map",
    "navsim_scan_labels", "navsim_lookahead", "navsim_lookahead_obs", "navsim_rollout", "navsim_mppi", "navsim_ped_forecast",
    "navsim_rollout_obs",
    "navsim_sizeof_config", "navsim_sizeof_state", "navsim_sizeof_step_io", "navsim_debug_math", "navsim_debug_xy_to_ij",
    "navsim_debug_gather", "navsim_debug_kernarg_layout", "navsim_debug_set_stamps", "navsim_debug_spawn_decisions",
)
