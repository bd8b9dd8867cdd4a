/* navsim.h -- C ABI of the MI355X-native batched NavGym step().
 *
 * This is the drop-in boundary for the hot path of leekwoon/nav-gym
 * (NavGymEnv.step, nav_gym/src/nav_gym_env/env.py:591-728).  The reference has no
 * FFI of its own: its hot arithmetic lives behind four pip packages
 * (range_libc, CMap2D, pose2d, pyastar2d; env.py:12-15).  Every entry point below
 * names the reference call site it replaces.  All pointers are DEVICE pointers
 * owned by the caller (torch tensors in the Python host); the library never
 * allocates or frees caller-visible memory, never synchronises the device, and
 * never throws: every function returns 0 on success or a negative NAVSIM_E_* code.
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *
 * The CPU oracle (oracle/navsim_ref.h) exports the same functions with a `_cpu`
 * suffix, host pointers and no stream argument.  The oracle is test
 * infrastructure; nothing in this library calls it.
 *
 * Conventions:
 *   occupancy[y][x] row-major, x = column = "i", y = row = "j"; cell (i,j) covers
 *   world [ox + i*res, ox + (i+1)*res) x [oy + j*res, ...).  Angles are CCW from +x.
 */
#ifndef NAVSIM_H
#define NAVSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAVSIM_ABI_VERSION 7

/* error codes */
#define NAVSIM_OK            0
#define NAVSIM_E_ARG        -1   /* null pointer / bad size */
#define NAVSIM_E_LAUNCH     -2   /* hipGetLastError() after a launch was not hipSuccess */
#define NAVSIM_E_UNSUPPORTED -3  /* configuration outside compiled limits */
#define NAVSIM_E_NODEVICE   -4   /* no HIP device visible */

/* pedestrian update model (navsim_config.ped_model) */
#define NAVSIM_PED_NONE      0   /* n_peds ignored, no pedestrians */
#define NAVSIM_PED_EXTERNAL  1   /* (v, omega) per pedestrian supplied by the caller: the slot the
                                    reference fills with HumanPolicy (env.py:650-662) */
#define NAVSIM_PED_SFM       2   /* build-defined social-force model */

/* distance-field storage (navsim_config.field_format, navsim_build_field) */
#define NAVSIM_FIELD_F32     0   /* float32 [E,H,W] row-major, distance in cells (what range_libc holds) */
#define NAVSIM_FIELD_U16T    1   /* uint16 squared distance in 8x8-cell tiles (128-B lines), 0xFFFF =
                                    "d2 >= 65535, read the float32 overflow plane"; d = sqrtf(d2) is
                                    bit-identical to the float32 field */
#define NAVSIM_FIELD_TILE    8

/* How range_libc's RayMarching::calc_range (env.py:425) rounds its sphere-tracing step `d * step_coeff` and its sample
 * position `x0 + ray_direction_x * t` (navsim_config.march_rule).  The package's source is not in the reference tree,
 * so which of these the upstream BINARY computes is UNPINNED; all are implemented on both sides
 * and the switch is this one field.  DESIGN.md records how many rays change their hit cell between them.
 *   The published header (RangeLib.h, class RayMarching) declares the coefficient as a float data member
 *   (`float step_coeff = 0.999;`, beside `float distThreshold = 0.0;`), so `d * step_coeff` is a float32 product:
 *   NAVSIM_MARCH_F32 is the reading of the SOURCE and the default since ABI 4 (rounds 1-3 defaulted to the double
 *   reading, NAVSIM_MARCH_F64, kept as a switch).  What the source cannot settle is the compiler: upstream's
 *   setup.py builds with -O3 -march=native -ffast-math, and GCC contracts a * b + c into one fused multiply-add
 *   wherever the target has FMA (-ffp-contract=fast is GCC's default outside ISO mode), i.e. the sample position
 *   becomes fmaf(dir, t, x0) on every x86 since Haswell: NAVSIM_MARCH_F32_FMA.  (The hit distance
 *   sqrtf(xd * xd + yd * yd) is unaffected: xd, yd are integers below 2^12, both products are exact.)
 *   A fourth family of last-bit differences has NO switch: upstream takes the ray direction from the C library's cosf / sinf
 *   of the float heading, this build from the correctly rounded fl32(cos64(fl64(heading))).  Measured (round 6,
 *   tests/test_oracle_crosscheck.py direction_rounding_sensitivity, 10^7 rays on twenty 500 x 500 maps, glibc 2.35): the two
 *   differ in dx or dy for 2.6 % of the headings, and 2 rays in 10^7 then change their hit cell (one ulp on either component
 *   changes about 100 in 10^7) -- an order of magnitude below the rules above (26 and 62 in 10^7). */
#define NAVSIM_MARCH_F64     0   /* t += max(fl32(fl64(d) * 0.999), 1): a double coefficient */
#define NAVSIM_MARCH_F32     1   /* t += max(d * 0.999f, 1): the float member `step_coeff` of the source (default) */
#define NAVSIM_MARCH_F32_FMA 2   /* NAVSIM_MARCH_F32 with the sample position contracted: px = (int)fmaf(dx, t, x0) */

/* compiled limits */
#define NAVSIM_MAX_PEDS      64
#define NAVSIM_MAX_WAYPOINTS 256 /* upper limit of navsim_config.max_waypoints (the stride P of ped_waypoints) */
#define NAVSIM_OBS_TAIL      7   /* prev_pose(2) pose(2) vel(2) yaw(1): env.py:455 */

/* ------------------------------------------------------------------------------------------
 * Simulator configuration: the registered kwargs of NavGym-v0 (__init__.py:6-38) plus the
 * batch geometry.  Plain data, passed by pointer, copied by the callee.
 * ---------------------------------------------------------------------------------------- */
typedef struct navsim_config {
    int32_t n_envs;          /* E: independent arenas in this shard */
    int32_t n_beams;         /* B: KetiRobot.n_angles (keti_robot.py:48); 512 native, 1081 bench */
    int32_t map_h;           /* H cells (rows, y) */
    int32_t map_w;           /* W cells (cols, x) */
    int32_t max_peds;        /* N: stride of the per-pedestrian arrays, <= NAVSIM_MAX_PEDS */
    int32_t n_scan_stack;    /* S: num_scan_stack (__init__.py:11) */
    int32_t ped_model;       /* NAVSIM_PED_* */
    int32_t lidar_legs;      /* robot scan renders legs of has_legs pedestrians (env.py:695-698) */
    int32_t auto_reset;      /* NAVSIM_AUTORESET_*: what happens to an arena whose episode ends (below) */
    int32_t n_spawn;         /* K: spawn table entries per env (auto_reset) */
    int32_t add_scan_noise;  /* 1: Gaussian noise on beams != range_max (env.py:437-440) */
    int32_t env_index_base;  /* global index of local env 0 (multi-GPU sharding; seeds RNG) */
    int32_t field_format;    /* NAVSIM_FIELD_* of navsim_state.field */
    int32_t shared_field;    /* 1: every arena reads arena 0's field (one map for the whole batch) */

    double resolution;       /* metres per cell (map_generator.py:116) */
    double origin_x, origin_y;
    double time_step;        /* __init__.py:8 */
    double angle_min;        /* first beam angle in the robot frame (keti_robot.py:45) */
    double angle_last;       /* last beam angle = angle_max - angle_increment (env.py:388-390).  With pedestrians
                              * (ped_model != NAVSIM_PED_NONE) angle_last - angle_min > 2 pi is NAVSIM_E_UNSUPPORTED from every
                              * step and reset entry, before anything is launched: the bearing-culled merge of pedestrians
                              * into the scan visits the 2 pi aliases of a bearing up to one turn.  Exactly 2 pi, a reversed
                              * lidar (angle_last < angle_min) and, without pedestrians, any field of view are served. */
    double range_max;        /* keti_robot.py:47 */
    double axle_offset;      /* 0.14474 for KetiRobot (keti_robot.py:72-90); 0 = plain unicycle */
    double min_turning_radius;   /* env.py:595-600 */
    double distance_threshold;   /* __init__.py:10 */
    double reward_scale;
    double reward_success_factor;
    double reward_crash_factor;
    double reward_progress_factor;
    double reward_forward_factor;
    double reward_rotation_factor;
    double reward_discomfort_factor;

    /* social-force parameters (NAVSIM_PED_SFM only) */
    double sfm_tau;          /* relaxation time, s */
    double sfm_k_desired;
    double sfm_k_social;
    double sfm_k_obstacle;
    double sfm_lambda;       /* lambdaImportance */
    double sfm_gamma;
    double sfm_n;
    double sfm_n_prime;
    double sfm_sigma_obstacle;
    double sfm_agent_radius;

    uint64_t seed;           /* counter-based RNG key (scan noise, spawn choice) */

    /* pedestrian lidar (human.py:12-16) and the robot as pedestrians see it (env.py:404-405):
     * only used by navsim_ped_scans */
    double ped_angle_min, ped_angle_last, ped_range_max;   /* ped_angle_last - ped_angle_min > 2 pi: NAVSIM_E_UNSUPPORTED from
                                                            * navsim_ped_scans(_part) and navsim_ped_scan_policy (as angle_last) */
    int32_t ped_n_beams;
    int32_t regen_plan;               /* navsim_regen: 1 = sample on the costmap and keep only start/goal pairs
                                         joined by a path (env.py:342-383), pedestrians get path waypoints */
    double robot_seen_footprint[8];   /* threshold_footprint, 4 x (x, y) in the robot frame */

    /* device-side reset of finished arenas with a NEW map (navsim_regen):
     * the per-episode ranges of the reference (__init__.py:14-15, 17-18, 26-37; env.py:748-806) */
    int32_t regen_cap;                /* arenas regenerated per call at most (the rest keep their map) */
    int32_t obstacle_number;          /* env_param_range['obstacle_number'] */
    double obstacle_width_lo, obstacle_width_hi;   /* env_param_range['obstacle_width'] */
    double spawn_clearance;           /* robot start / goal cells keep this distance to obstacles, m */
    double ped_clearance;             /* same for pedestrians */
    double min_goal_dist, max_goal_dist;           /* __init__.py:17-18 */
    double ped_min_robot_dist;        /* env.py:372: 4 m */
    double ped_min_goal_dist;         /* env.py:788-791: 10 m */
    double v_pref_lo, v_pref_hi;      /* human_v_pref_range */
    double has_legs_ratio;            /* human_has_legs_ratio */
    double regen_indoor_ratio;        /* navsim_regen: probability that a new map is a corridor map
                                         (create_indoor_map, map_generator.py:97-123) instead of an outdoor one;
                                         env.py:742 indoor_ratio.  0 = outdoor only */

    /* The other per-episode ranges of env_param_range (__init__.py:28-37), drawn by navsim_regen for every new
     * episode like _sample_env_param does (env.py:281-292: 'int' = uniform over lo..hi inclusive, 'float' =
     * uniform(lo, hi)), hash-keyed by (seed, global arena, episode). */
    int32_t obstacle_number_hi;       /* 'obstacle_number' = obstacle_number .. obstacle_number_hi boxes (<= 64);
                                         below obstacle_number (the default 0): always obstacle_number */
    int32_t corridor_width_lo, corridor_width_hi;   /* 'corridor_width' (3, 4) */
    int32_t iterations_lo, iterations_hi;           /* 'iterations' (80, 150) */
    int32_t num_humans_lo, num_humans_hi;           /* 'num_humans': navsim_regen rewrites n_peds[e] (clipped to
                                                       max_peds); hi = 0: n_peds[e] is kept */
    int32_t outdoor_map_size;         /* navsim_regen: side of an OUTDOOR map in cells when it differs from the arena's
                                         allocation (the reference draws outdoor maps at 400 x 400 and corridor maps at
                                         1000 x 1000, map_generator.py:108-142): the map occupies cells [0, size)^2 of the
                                         map_h x map_w arena, the rest is occupied.  0 = map_w */
    double scan_noise_std_lo, scan_noise_std_hi;    /* 'scan_noise_std': navsim_regen rewrites scan_noise_std[e];
                                                       hi < 0: kept */

    int32_t march_rule;               /* NAVSIM_MARCH_* */
    /* Launch geometry of the fused step.  Validated plain data: the library reads no environment variable. */
    int32_t step_block;               /* threads per arena: 0 = chosen from the batch size,
                                         else 64, 256, 512 or 1024 */
    int32_t ped_split;                /* pedestrian update in its own kernel (a pack of arenas per workgroup) ahead of the
                                         step: 0 or 1 = no, inside the step on one wavefront beside the scan (faster at every
                                         batch size since round 3), 2 = yes (the pack shrinks to what fits 64 KB of LDS: one
                                         arena per workgroup at 64 pedestrians) */
    int32_t regen_check_discomfort;   /* navsim_regen: 1 (default) = a robot start whose FIRST scan (no pedestrians, no noise) has a
                                         beam inside the discomfort zone is dropped and the next start / goal pair of the
                                         spawn table takes its place, like reset() re-draws the robot (env.py:776-781) */
    int32_t rect_lds;                 /* fused step with rect records: 0 = the library stages the index form of an arena's record
                                         table (navsim_state.rect_index) in LDS whenever it is present and fits beside the step's
                                         other LDS at the launch's residency, 1 = never (records from global
                                         memory), 2 = whenever it fits one workgroup per CU */
    int32_t max_waypoints;            /* P: waypoints kept per pedestrian = stride of navsim_state.ped_waypoints, 1 ..
                                         NAVSIM_MAX_WAYPOINTS.  The reference keeps EVERY waypoint of a route
                                         (path_to_waypoints, env.py:1261-1277; env.py:788-804); navsim_default_config
                                         sets 64 = 128 m of route at the 2 m interval (a 1000 x 1000 map is 50 m wide).
                                         A longer route is stored cut after P waypoints, counted in
                                         counters[NAVSIM_COUNTER_ROUTES_CUT], and -- when navsim_state.ped_goal is
                                         present -- continued to the SAME goal by navsim_replan when the pedestrian
                                         reaches the cut */

    /* The action's form (round 4; BUILD-DEFINED like the Husky model itself: the reference drives KetiRobot with
     * (v, omega) only).  NAVSIM_ACTION_WHEELS: io->action holds the angular speeds (left, right) of a skid-steer
     * base's wheel pairs in rad/s, converted on the device as v = r (wl + wr) / 2, omega = r (wr - wl) / track
     * (third_party/husky_description/urdf/husky.urdf.xacro:61-67: track 0.5708, wheel radius 0.1651).
     * clamp_action = 1 clamps the twist to [linvel_lo, linvel_hi] x [rotvel_lo, rotvel_hi] before anything else
     * (the reference only prints a warning and never clips, env.py:606-613: 0 is the default).  The twist after
     * conversion and clamp is what the step integrates and what the observation's `vel` slots carry. */
    int32_t action_kind;              /* NAVSIM_ACTION_* */
    int32_t clamp_action;
    double wheel_radius, wheel_track;
    double linvel_lo, linvel_hi, rotvel_lo, rotvel_hi;   /* __init__.py:12-13 linvel_range, rotvel_range */
    int32_t closed_maps;              /* 1 = the caller asserts that EVERY map of the world has a ring of at least 3 occupied cells
                                         around it (all of the reference's maps have 5, map_generator.py:11, 61-93; every map
                                         navsim_regen draws is closed): set it from navsim_maps_closed's answers.
                                         The LDS form of the march (navsim_state.rect_index) needs it -- a ray of a closed map
                                         never leaves the map, so that form carries no bounds test -- and is not used without.
                                         A wrong assertion reads outside the tables. */
    int32_t defer_reset_scan;         /* 1 = navsim_step leaves the FIRST OBSERVATION of an arena it restarted (auto_reset) to the
                                         navsim_regen call that must follow it: the step does the restart's bookkeeping (pose, goal,
                                         episode, counters, tail of the row) and skips the second scan, navsim_regen produces the
                                         first observation of EVERY arena whose done flag is set -- those it gives a new world and
                                         those beyond regen_cap that restart in place -- in one masked launch over all arenas.
                                         Between the two calls the scan rows of a finished arena's observation are unspecified.
                                         Worth it where a launch is one generation of workgroups and lasts as long as its slowest
                                         arena (c5: the restarted arenas' second scans were 10 of the step's 49 us); the masked
                                         launch costs ~4 ns per arena, so not for thousands of arenas per GPU.  0 = the step scans
                                         itself (default).  Not with navsim_regen_swap. */
    int32_t regen_min_steps;          /* > 0: an arena whose episode ended after FEWER steps than this restarts in place (same map,
                                         next entry of its start / goal table) instead of receiving a new world from navsim_regen /
                                         navsim_regen_swap; counted in counters[NAVSIM_COUNTER_REGEN_SHORT].  A rule of the
                                         simulation's own history (navsim_state.done_steps), whatever the timing: it is what lets
                                         worlds be generated AHEAD of time several steps deep (nav_gym_amd/sim.py enable_pregen
                                         with a pipeline) and still be installed deterministically -- a world staged when an
                                         arena restarts is guaranteed complete regen_min_steps steps later.  0 (default): every
                                         finished arena is eligible.  Needs st->done_steps. */
    /* ---- ABI 7 ---- */
    int32_t max_episode_steps;        /* T > 0: time limit (old gym's TimeLimit, per arena).  An arena whose step count after
                                         this step's increment (navsim_state.steps) reaches T and which neither succeeded nor
                                         crashed in this step is TRUNCATED: io->done = 1, io->truncated = 1; reward, is_success
                                         (0), is_crash (0) and distance are the step's own.  Success or crash at step T wins
                                         (done 1, truncated 0).  A truncated arena is then every other finished arena: cfg.auto_reset
                                         restarts it (SAME_STEP: io->final_obs, done_steps = T; NEXT_STEP: the next call's
                                         io->reset_mask), navsim_regen / the staged worlds key on its done flag.  Under
                                         NAVSIM_AUTORESET_NONE an arena stepped past T stays truncated.  Reset-only launches and
                                         the resets of io->reset_mask are not steps.  0 (default): no limit, the outputs of ABI 6
                                         bit for bit.  (Sits in the structure's tail padding: sizeof(navsim_config) is unchanged.)
                                         The CPU oracle (oracle/) ignores the field. */
} navsim_config;

/* navsim_config.auto_reset.  The reference's step() returns the LAST observation of an episode together with done = True
 * (env.py:700-728: after a crash the re-scan at the reverted pose) and leaves reset() to its caller (env.py:730).
 *   NONE       exactly that: nothing restarts; the caller resets (navsim_restart + navsim_reset_obs / navsim_regen).
 *   SAME_STEP  (build-defined vector-env reset, the default of a batch) the step that ends an episode also restarts the arena
 *              -- next start / goal pair of its spawn table, next episode number -- and io->obs holds the FIRST observation of
 *              the new episode; the terminal observation the reference would have returned goes to io->final_obs /
 *              io->final_goals when those are given (rows of the arenas whose done flag this call sets).
 *   NEXT_STEP  (gymnasium's next-step mode) the step that ends an episode returns the terminal observation in io->obs like
 *              the reference, and restarts the arena in the STATE only (pose, goal, episode number, step counter); the arena's
 *              next call must be a reset: the caller passes io->reset_mask = the done flags of the previous call, the arena's
 *              action is ignored, its workgroup produces the first observation (or installs the staged world,
 *              navsim_step_install; or leaves the row to the navsim_regen that follows, cfg.defer_reset_scan) and the call
 *              returns reward 0, done 0, info 0 for it.  A navsim_regen for such arenas takes io->done = that same mask. */
#define NAVSIM_AUTORESET_NONE      0
#define NAVSIM_AUTORESET_SAME_STEP 1
#define NAVSIM_AUTORESET_NEXT_STEP 2

#define NAVSIM_ACTION_TWIST  0   /* io->action = (v, omega): the reference's action (env.py:591) */
#define NAVSIM_ACTION_WHEELS 1   /* io->action = (omega_left, omega_right) in rad/s */

/* ------------------------------------------------------------------------------------------
 * Per-shard simulator state: structure of device arrays, env-major.  E = n_envs, N = max_peds,
 * B = n_beams, S = n_scan_stack, K = n_spawn, P = cfg.max_waypoints.
 * Poses are float64 like the reference's Python floats; scans are float32 like env.py:387.
 * ---------------------------------------------------------------------------------------- */
typedef struct navsim_state {
    /* world */
    const void*   field;            /* distance field of every arena in cfg.field_format
                                       (navsim_build_dt / navsim_build_field) */
    const float*  field_overflow;   /* [E,H,W] float32 distances, read only where the packed field
                                       holds 0xFFFF; may be NULL when navsim_build_field reported
                                       no saturated cell (NAVSIM_FIELD_U16T only) */
    const void*   rect_table;       /* [E, ceil(H/8)*ceil(W/8)] 16-byte two-rectangle records of the 8x8-cell tiles
                                       (navsim_build_rects); optional accelerator of the packed field
                                       (NAVSIM_FIELD_U16T only): a probe in a tile with a valid record gets its
                                       exact integer d2 from the record instead of the field.  NULL = every probe
                                       reads the field.  Results are unchanged.  navsim_regen keeps it current. */
    const double* beam_table;       /* [B,2] cos, sin of the robot-frame beam angles (navsim_beam_table);
                                       optional accelerator, NULL = evaluate every beam direction in full */
    const float*  scan_threshold;   /* [B] env.py:162-170 */
    const float*  scan_discomfort;  /* [B] env.py:172-180 */
    float*        scan_noise_std;   /* [E] env_param['scan_noise_std'] (env.py:439); navsim_regen redraws it per episode
                                       when cfg.scan_noise_std_hi >= 0 */

    /* robot */
    double*  robot_pose;            /* [E,3] px, py, theta in [0, 2pi) */
    double*  robot_goal;            /* [E,2] gx, gy */
    double*  prev_action;           /* [E,2] env.py:725 */
    double*  prev_pose;             /* [E,3] x, y, wrapped yaw of prev_obs (env.py:710-717) */
    int32_t* n_hist;                /* [E] len(prev_obs_queue), 0..S-1 (env.py:257-279) */
    int64_t* episode;               /* [E] episodes finished so far (spawn / RNG counter) */
    int64_t* steps;                 /* [E] steps_since_reset */

    /* pedestrians (ignored when ped_model == NAVSIM_PED_NONE) */
    int32_t* n_peds;                /* [E] live pedestrians, <= N; navsim_regen redraws it per episode when
                                       cfg.num_humans_hi > 0 (env_param['num_humans'], env.py:786) */
    double*  ped_pose;              /* [E,N,3] */
    double*  ped_vel;               /* [E,N,2] world vx, vy (human.py:35-36) */
    double*  ped_prev_yaw;          /* [E,N] wrapped yaw of the pedestrian's previous obs (env.py:245-247) */
    double*  ped_dist;              /* [E,N,3] leg odometry (env.py:255) */
    const double*  ped_v_pref;      /* [E,N] */
    const uint8_t* ped_has_legs;    /* [E,N] */
    double*  ped_waypoints;         /* [E,N,P,2] the waypoints of every pedestrian's current route as its planner stored them
                                       (path_to_waypoints, env.py:1261-1277); entry ped_wp_head is the current local goal.
                                       Written only by whoever plans a route (the caller, navsim_regen, navsim_replan, the
                                       step's table draw): the waypoint pop of env.py:633-642 advances ped_wp_head
                                       instead of shifting the list (ABI 5).  P = cfg.max_waypoints */
    int32_t* ped_n_waypoints;       /* [E,N] >= 1: waypoints STORED for the current route; entry n - 1 is the final one */
    const double*  ped_cmd;         /* [E,N,2] (v, omega) for NAVSIM_PED_EXTERNAL, else NULL */

    /* auto-reset tables */
    const double* spawn_pose;       /* [E,K,3] */
    const double* spawn_goal;       /* [E,K,2] */

    /* planning costmap of every arena, [E, H/5, W/5] uint8 (navsim_costmap), or NULL.  When present a
     * pedestrian that reaches its final waypoint waits for navsim_replan (env.py:667-680) instead of
     * drawing a straight-line goal from the spawn table, and navsim_regen refreshes it (regen_plan). */
    uint8_t* costmap;

    /* Scheduling hints for the fused step, both optional and without effect on any result.  arena_cost [E]:
     * the step writes how long each arena's workgroup lived (ticks of the chip-wide 100 MHz clock).
     * launch_order [E]: a permutation of the arenas; workgroup b then works on arena launch_order[b].
     * navsim_launch_order sorts arenas by descending cost, so that the longest ones start first and the
     * kernel does not end on a few stragglers. */
    uint32_t*      arena_cost;
    const int32_t* launch_order;

    /* TESTS ONLY ("draws supplied"): [E, NAVSIM_DRAWS_PER_ARENA] uniforms in [0, 1) that navsim_regen uses INSTEAD of
     * its hash-keyed ones for the per-episode parameters and the map generators, laid out as NAVSIM_DRAW_* below, so
     * that the reference's own generators can be replayed on the same draws (tests/golden/make_golden.py reset).
     * NULL (always, outside those tests) = hash-keyed draws. */
    const double* regen_draws;

    /* ---- ABI 4 ---- */
    /* [E,N,2] or NULL: the goal of every pedestrian's current route, written by whoever plans it (navsim_regen,
     * navsim_replan; the caller for routes it supplies).  A route was stored cut exactly when its last stored
     * waypoint differs from this goal (path_to_waypoints closes every list with the goal cell's centre, env.py:1273);
     * navsim_replan then plans from where the pedestrian stands to the SAME goal instead of drawing a new one.
     * NULL: a pedestrian that reaches the end of a cut list draws a new goal there. */
    double*  ped_goal;
    /* [NAVSIM_N_COUNTERS] uint64 or NULL: running totals, incremented on the device, zeroed by the caller when it
     * likes.  They make the library's caps observable: no call ever fails or blocks because of a cap. */
    unsigned long long* counters;
    /* [E, navsim_rect_index_bytes(1, H, W)] or NULL: the INDEX form of rect_table (navsim_build_rect_index) -- per arena the
     * distinct rectangles of its records (at most 255, 8 bytes each) and two list indices per 8x8 tile, 10 KB for a
     * 500 x 500 map.  The fused step copies the arena's row into LDS and its scans probe LDS instead of global memory
     * ("map tiles staged through LDS"; cfg.rect_lds).  Needs rect_table (other kernels keep reading the records);
     * navsim_regen keeps it current.  Results are unchanged. */
    void* rect_index;

    /* ---- ABI 5 ---- */
    /* [E,N]: index of the pedestrian's current waypoint in its row of ped_waypoints, 0 <= head < ped_n_waypoints.  The
     * reference pops a reached waypoint off the front of a Python list (env.py:633-642); here the pop is head += 1 and the
     * list stays where its planner put it.  Every planner resets it to 0.  Required with pedestrians. */
    int32_t* ped_wp_head;
    /* [E] or NULL: written by navsim_step for every arena it steps -- bit i set = pedestrian i stands within 0.5 m of its
     * final waypoint after this step's update, i.e. it is due for navsim_replan (env.py:667-680).  When present
     * navsim_replan takes its candidates from here instead of scanning the state itself (every candidate is re-checked
     * against the current state, so flags of pedestrians that were served or regenerated meanwhile are harmless), and
     * navsim_regen clears the word of every arena it gives a new world. */
    unsigned long long* ped_due;
    /* [E] or NULL: the flags the PREVIOUS step wrote (the caller alternates two buffers between ped_due and ped_due_prev).
     * Read by navsim_step_part only: it splits a step into the arenas with and without a pedestrian waiting for
     * navsim_replan, so that the re-plan of step t runs beside step t + 1 of all the other arenas. */
    const unsigned long long* ped_due_prev;
    /* [E] or NULL: written by navsim_step when an arena finishes (cfg.auto_reset): the number of steps its episode lasted.
     * Read by navsim_regen / navsim_regen_swap for cfg.regen_min_steps. */
    int32_t* done_steps;
    /* [E] or NULL: the slot of the five per-map arrays (field, field_overflow, rect_table, rect_index, costmap) that holds
     * arena e's map; NULL = slot e.  Those arrays then have max(map_slot) + 1 entries.  For navsim_step_install without map
     * copies: the live and the staged state point at the SAME five arrays of 2 E slots, each with its own table (live
     * 0 .. E-1, staged E .. 2E-1 to begin with), and an install exchanges the two states' entries for the arena.  Every
     * entry point that reads or writes a map goes through the table (the step through the instantiations navsim_step_install
     * uses, whatever the call: packed fields only, and navsim_step_part / navsim_step_replan return NAVSIM_E_UNSUPPORTED);
     * not with cfg.shared_field. */
    int32_t* map_slot;
} navsim_state;

#define NAVSIM_N_COUNTERS              8
#define NAVSIM_COUNTER_REGEN_SERVED    0   /* arenas given a new world by navsim_regen / installed by navsim_regen_swap */
#define NAVSIM_COUNTER_REGEN_UNSERVED  1   /* finished arenas a navsim_regen / navsim_regen_swap call left beyond
                                              cfg.regen_cap (or not staged yet): they play their next episode in place */
#define NAVSIM_COUNTER_REPLAN_SERVED   2   /* pedestrians navsim_replan planned for (whether or not a path was found) */
#define NAVSIM_COUNTER_REPLAN_UNSERVED 3   /* pedestrians due for a re-plan beyond max_queries: counted in every call that
                                              leaves them waiting */
#define NAVSIM_COUNTER_ROUTES_CUT      4   /* routes longer than cfg.max_waypoints, stored cut (navsim_regen with
                                              regen_plan, navsim_replan) */
#define NAVSIM_COUNTER_ROUTES_RESUMED  5   /* cut routes navsim_replan continued to their own goal (ped_goal) */
#define NAVSIM_COUNTER_REGEN_SHORT     6   /* finished arenas whose episode was shorter than cfg.regen_min_steps: restarted in place */
#define NAVSIM_COUNTER_REGEN_LATE      7   /* navsim_regen_swap (pipelined): eligible arenas whose staged world was not complete --
                                              the caller's pipeline is deeper than cfg.regen_min_steps covers; they restart in
                                              place and this stays 0 when the caller keeps the documented order */

#define NAVSIM_DRAWS_PER_ARENA      464
#define NAVSIM_DRAW_KIND            0   /* np.random.random() < indoor_ratio             (env.py:295) */
#define NAVSIM_DRAW_OBSTACLE_NUMBER 1   /* env_param 'obstacle_number', 'int'            (env.py:281-292) */
#define NAVSIM_DRAW_NUM_HUMANS      2   /* env_param 'num_humans', 'int' */
#define NAVSIM_DRAW_SCAN_NOISE_STD  3   /* env_param 'scan_noise_std', 'float' */
#define NAVSIM_DRAW_OBSTACLE_WIDTH  4   /* env_param 'obstacle_width', 'float' */
#define NAVSIM_DRAW_CORRIDOR_WIDTH  5   /* env_param 'corridor_width', 'int' */
#define NAVSIM_DRAW_ITERATIONS      6   /* env_param 'iterations', 'int' */
#define NAVSIM_DRAW_MAP             8   /* the generator's own draws in its own order: create_outdoor_map (x, y) per
                                           obstacle (map_generator.py:129-131); create_indoor_map (x, y, coin) per
                                           iteration (map_generator.py:101-106, 61) */

/* What step() returns (env.py:728) with a leading env axis. */
typedef struct navsim_step_io {
    const double* action;           /* [E,2] (linvel, rotvel) -- not clipped (env.py:611-613) */
    const float*  obs_prev;         /* [E,S*B+7] observation returned by the previous step/reset */
    float*   obs;                   /* [E,S*B+7] scan stack, prev_pose, pose, vel, yaw (env.py:455) */
    float*   achieved_goal;         /* [E,2] */
    float*   desired_goal;          /* [E,2] */
    double*  reward;                /* [E] */
    uint8_t* done;                  /* [E] */
    float*   is_success;            /* [E] info['is_success'] (env.py:475) */
    float*   is_crash;              /* [E] info['is_crash']   (env.py:476) */
    double*  distance;              /* [E] info['distance']   (env.py:474) */
    /* ---- ABI 6 ---- */
    /* [E, S*B+7] or NULL: the TERMINAL observation of every arena whose done flag this call sets under
     * NAVSIM_AUTORESET_SAME_STEP -- what the reference's step() returns with done = True (env.py:700-728): scan stack, tail
     * and, after a crash, the re-scan at the reverted pose -- written BEFORE the arena restarts; rows of other arenas are not
     * touched.  (NONE / NEXT_STEP: io->obs itself is that row; nothing is written here.) */
    float*   final_obs;
    /* [E,4] or NULL: achieved_goal (2) and desired_goal (2) of that terminal observation (env.py:455-461) */
    float*   final_goals;
    /* [E] uint8 or NULL: arenas to RESET instead of stepping (NAVSIM_AUTORESET_NEXT_STEP: the done flags of the previous
     * call; their state was restarted when they finished).  Must not alias io->done. */
    const uint8_t* reset_mask;
    /* ---- ABI 7 ---- */
    /* [E] uint8 or NULL: 1 = the arena's episode was cut by cfg.max_episode_steps in this call (done is 1 as well), 0 for every
     * other arena the call steps; NEXT_STEP resets (io->reset_mask) write 0 beside their zeroed done.  Written only when
     * cfg.max_episode_steps > 0; untouched otherwise.  The CPU oracle (oracle/) never writes it. */
    uint8_t* truncated;
} navsim_step_io;

/* ---- library ---------------------------------------------------------------------------- */
int         navsim_abi_version(void);
const char* navsim_error_string(int code);
/* Fills a config with the registered NavGym-v0 defaults (__init__.py:6-38, keti_robot.py:44-48). */
int         navsim_default_config(navsim_config* cfg);
/* hipGetErrorString of the launch failure behind the last NAVSIM_E_LAUNCH on the calling thread */
const char* navsim_last_hip_error(void);

/* ---- a3: range_libc.PyOMap + PyRayMarching.__init__ (env.py:337-340) -------------------- */
/* Exact Euclidean distance transform of `occ` (nonzero = occupied), float32 cells.
 * workspace: navsim_build_dt_workspace_bytes() bytes of device scratch. */
size_t navsim_build_dt_workspace_bytes(int32_t n_maps, int32_t map_h, int32_t map_w);
int    navsim_build_dt(const uint8_t* occ, int32_t n_maps, int32_t map_h, int32_t map_w,
                       float* field, void* workspace, size_t workspace_bytes, void* stream);

/* Same transform, written in `format` (the layout the fused step streams).  `field` needs
 * navsim_field_bytes() bytes.  `overflow` (float32 [n,H,W], may be NULL) receives the exact float
 * distance of every cell; `n_saturated` (device int32, may be NULL) is incremented once per cell whose
 * squared distance does not fit the packed format -- when it stays 0 the overflow plane is never read
 * and may be dropped. */
size_t navsim_field_bytes(int32_t n_maps, int32_t map_h, int32_t map_w, int32_t format);
int    navsim_build_field(const uint8_t* occ, int32_t n_maps, int32_t map_h, int32_t map_w, int32_t format,
                          void* field, float* overflow, int32_t* n_saturated,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Two-rectangle records of the distance field's 8x8-cell tiles (navsim_state.rect_table).  Obstacles of the
 * reference's maps are unions of axis-aligned rectangles of cells (map_generator.py:97-143), and the squared
 * distance of a cell to such a rectangle is max(x0-px, px-x1, 0)^2 + max(y0-py, py-y1, 0)^2.  A record holds two
 * rectangles of occupied cells (4 x int16 each: x0, y0, x1, y1) with d2(cell) = min over the two for EVERY in-map
 * cell of the tile -- the builder checks that cell by cell against `field` and marks the tile invalid (x0 of the
 * first rectangle = 0x7FFF) when no such pair is found.  Any map is accepted; maps that are not rectangle unions
 * just get fewer valid records.  `field` / `format` / `overflow` as produced by navsim_build_field for the same
 * occupancy grids (overflow may be NULL: tiles holding a saturated cell are then invalid).  H, W <= 1024. */
size_t navsim_rect_table_bytes(int32_t n_maps, int32_t map_h, int32_t map_w);
/* The index form of `table` (navsim_state.rect_index): per map the distinct rectangles of its valid records and two list
 * indices per tile.  n_rects [n_maps] int32 or NULL receives the number of distinct rectangles found (tiles naming one
 * beyond the 255th get no index and are read from the field). */
size_t navsim_rect_index_bytes(int32_t n_maps, int32_t map_h, int32_t map_w);
int    navsim_build_rect_index(const void* table, int32_t n_maps, int32_t map_h, int32_t map_w, void* index,
                               int32_t* n_rects, void* stream);
/* closed [n_maps] int32: 1 where every cell of the map's outer ring of 3 cells is occupied (navsim_config.closed_maps may
 * be set when all are 1). */
int    navsim_maps_closed(const uint8_t* occ, int32_t n_maps, int32_t map_h, int32_t map_w, int32_t* closed, void* stream);
/* The same test on a WORLD: *n_open (device int32, zeroed by the caller) receives the number of arenas of st->field whose
 * outer ring of 3 cells has a free cell (a cell is occupied exactly when its distance is 0).  cfg->closed_maps is an
 * assertion the march of the LDS form relies on without testing it: a caller who assembles a world checks it with this
 * (nav_gym_amd/sim.py NavSim does, once, at construction); every map navsim_regen draws is closed by construction. */
int    navsim_world_closed(const navsim_config* cfg, const navsim_state* st, int32_t* n_open, void* stream);
size_t navsim_build_rects_workspace_bytes(int32_t n_maps, int32_t map_h, int32_t map_w);
int    navsim_build_rects(const uint8_t* occ, int32_t n_maps, int32_t map_h, int32_t map_w, const void* field,
                          int32_t format, const float* overflow, void* table, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- a4: PyRayMarching.calc_range_many (env.py:425) ------------------------------------- */
/* queries [E, n_per_env, 3] float32 (x, y, theta) in cell units, out [E, n_per_env] in cells;
 * march_rule = NAVSIM_MARCH_*. */
int navsim_cast_static(const float* field, int32_t n_envs, int32_t map_h, int32_t map_w,
                       const float* queries, int32_t n_per_env, float max_range, int32_t march_rule,
                       float* out, void* stream);

/* ---- a5: CMap2D.flatten_contours + render_contours_in_lidar (env.py:430-431) ------------ */
/* ranges [E,B] in/out (metres); angles [E,B] float64; verts [E,V,3] float32 (contour id, x, y),
 * n_verts [E] live vertices per env (<= V); origin [E,2] float32. */
int navsim_render_polys(float* ranges, const double* angles, int32_t n_envs, int32_t n_beams,
                        const float* verts, const int32_t* n_verts, int32_t max_verts,
                        const float* origin, void* stream);

/* ---- a6: CSimAgent + CMap2D.render_agents_in_lidar (env.py:402, 432) -------------------- */
/* agents [E,A,8] float32: pos(3) dist(3) vel(2); n_agents [E] (<= A). */
int navsim_render_legs(float* ranges, const double* angles, int32_t n_envs, int32_t n_beams,
                       const float* agents, const int32_t* n_agents, int32_t max_agents,
                       const float* origin, void* stream);

/* ---- a8 / a9: Human.set_vel (human.py:32-41), KetiRobot.set_vel (keti_robot.py:64-93) --- */
/* pose [n,3] in/out, cmd [n,2] (v, omega), vel_out [n,2] world (vx, vy) or NULL.
 * axle_offset = 0 gives Human.set_vel, 0.14474 gives KetiRobot.set_vel. */
int navsim_integrate(double* pose, const double* cmd, double* vel_out, int32_t n,
                     double time_step, double axle_offset, void* stream);

/* ---- a12 / a13: compute_rewards, compute_terminals, compute_info (env.py:464-589) ------- */
/* HER batch API.  obs [n, S*B+7] float32 or float64 (obs_is_f64), goals [n,2] same dtype.
 * Any output pointer may be NULL. */
int navsim_reward_done(const navsim_config* cfg, const void* obs, const void* goals,
                       int32_t obs_is_f64, int32_t n,
                       const float* scan_threshold, const float* scan_discomfort,
                       double* reward, uint8_t* done, float* is_success, float* is_crash,
                       double* distance, void* stream);

/* ---- a14: _make_scan_threshold / _make_scan_discomfort_threshold (env.py:162-180) ------- */
/* footprint [n_vert,2] float32 (un-closed polygon in the robot frame), out [B]. */
int navsim_scan_threshold(const navsim_config* cfg, const float* footprint, int32_t n_vert,
                          float* out, void* stream);

/* cos / sin (float64, DESIGN.md section 4 functions) of np.linspace(angle_min, angle_last, B): lets the
 * step derive each beam direction by one angle addition and prove, per beam, that the float32
 * rounding equals the full evaluation's (falling back to it otherwise) -- results are unchanged. */
int navsim_beam_table(const navsim_config* cfg, double* table, void* stream);

/* ---- a1: NavGymEnv.step (env.py:591-728), fused ----------------------------------------- */
/* One launch: pedestrian update, robot integration, scan, reward/done/info, crash revert (or
 * respawn) with re-scan, observation packing.  State is updated in place. */
int navsim_step(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                void* stream);

/* navsim_step for a PART of the arenas (ABI 5), chosen by the flags the previous step left in st->ped_due_prev:
 * NAVSIM_STEP_NOT_DUE steps the arenas none of whose pedestrians waits for navsim_replan, NAVSIM_STEP_DUE the others;
 * the two calls together are exactly one navsim_step (arenas are independent; every arena is stepped by one of them),
 * NAVSIM_STEP_ALL is navsim_step.  What it is for: navsim_replan is a chain of dependent breadth-first levels that serves
 * ~2 % of the arenas per step and used to sit serially behind every step (env.py:667-680 plans inside step()); with
 *     stream A:  navsim_step_part(NOT_DUE)                                    } step t + 1
 *     stream B:  navsim_replan (of step t) -> navsim_step_part(DUE)            }
 * the re-plan runs beside the step of the arenas that do not need it (nav_gym_amd/sim.py NavSim.step_overlapped).
 * Both calls use the same io (rows of arenas a call does not step are not touched) and the same two flag buffers. */
#define NAVSIM_STEP_ALL     0
#define NAVSIM_STEP_NOT_DUE 1
#define NAVSIM_STEP_DUE     2
int navsim_step_part(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io, int32_t part,
                     void* stream);

/* ---- env.py:685-693: the scan of every pedestrian (input of the reference's HumanPolicy) --------- */
/* out [E, N, ped_n_beams] float32 metres: static map from the pedestrian's integer cell, the robot as its
 * threshold footprint and the other pedestrians as footprint rectangles (lidar_legs=False), clipped to
 * ped_range_max, no noise.  Uses the CURRENT state (call it after navsim_step / navsim_reset_obs).
 * Rows of pedestrians >= n_peds[e] are left untouched. */
int navsim_ped_scans(const navsim_config* cfg, const navsim_state* st, float* out, void* stream);
/* The same for the arenas [e0, e0 + n_e) only (rows of the other arenas are not touched).  With navsim_ped_policy_part it
 * lets a caller pipeline the two: the scans of the next slice of arenas -- a latency-bound march -- run on one stream beside
 * the network of the current slice -- FMA / MFMA-bound -- on another (nav_gym_amd/sim.py NavSim.ped_policy, round 5). */
int navsim_ped_scans_part(const navsim_config* cfg, const navsim_state* st, float* out, int32_t e0, int32_t n_e, void* stream);

/* ---- reset() of finished arenas on the device, with a new random map ------------ */
/* For every arena with done[e] != 0 (at most cfg.regen_cap, lowest indices first): a fresh outdoor map
 * (create_outdoor_map, map_generator.py:126-143, counter-based RNG keyed by seed / global arena /
 * episode), its distance field, a new table of start / goal pairs (clearance and distance rules of
 * env.py:748-783 without the A* path test), the robot placed on one of them, every pedestrian re-drawn
 * (start >= 4 m from the robot, goal >= 10 m away, v_pref, has_legs: env.py:786-806) and the first
 * observation of the new episode (env.py:808-831) written to io->obs.  Call it right after navsim_step on
 * the same stream with the same io.  Mutates field, spawn tables and pedestrian parameters in place.
 * Square maps; FIELD_F32, or FIELD_U16T.  A packed world of at most 520 cells per side has no overflow plane (no
 * cell of such a map can be 256 cells from every obstacle) and must not be given one; a larger packed world MUST
 * carry st->field_overflow, which is regenerated together with the field (NAVSIM_E_UNSUPPORTED otherwise).
 * cfg->regen_plan = 1: starts and goals are centres of free COSTMAP cells and a pair is kept only when the
 * planner joins it (robot: path no longer than twice the straight line, env.py:756-762; pedestrians get the
 * path's waypoints every 2 m, env.py:804); four rounds of candidates, the last one stays if none passes.
 * Finished arenas beyond cfg.regen_cap keep their map and play their next episode in place (the step has already
 * respawned them from the spawn table); counters[NAVSIM_COUNTER_REGEN_UNSERVED] counts them. */
size_t navsim_regen_workspace_bytes(const navsim_config* cfg);
/* navsim_regen off the step's critical path (round 3).  The world an arena receives at the end of an episode depends
 * on (cfg.seed, global arena index, episode number) only, so it can be generated AHEAD of time: keep a second, STAGED
 * navsim_state (own copies of every array navsim_regen writes, its episode[e] = live episode[e] + 1) and a staged
 * observation buffer; run the ordinary navsim_regen on the staged state for the arenas flagged in want[] (as its
 * io->done), on a side stream, while steps run.  After a step, navsim_regen_swap installs the staged world of every
 * finished arena (io->done[e] != 0; at most cfg.regen_cap, lowest indices first -- navsim_regen's own rule): it copies
 * the arena's rows of those arrays and of the observation from the staged state into the live one, marks the arena for
 * the next staging pass and sets stage->episode[e] = live episode + 1.  The live state is then exactly what navsim_regen would have left.
 * The caller orders the streams: a swap after the staging pass that served its arenas, the next staging pass after the
 * swap (nav_gym_amd/sim.py NavSim.enable_pregen).  Needs cfg.auto_reset = 1 (the step advances episode[e] at `done`).
 * A finished arena that is NOT installed by a call -- beyond regen_cap, or its staged world not ready (want[e] != 0) --
 * plays on in place like one beyond navsim_regen's cap and is staged again for its new episode number; with no such
 * surplus the live state after every call equals navsim_regen's bit for bit.
 * want [E], mark [E]: uint8 flags, zero-initialised by the caller with every arena staged (or all ones in want and one
 * navsim_regen_stage per regen_cap arenas first).  navsim_regen_swap only reads want and writes mark;
 * navsim_regen_stage (io->done must be `want`, io->obs the staged observation buffer) merges mark into want, runs
 * navsim_regen on the staged state and clears want for the arenas it served. */
int    navsim_regen_swap(const navsim_config* cfg, const navsim_state* live, const navsim_state* stage,
                         const navsim_step_io* io, const float* stage_obs, const uint8_t* want, uint8_t* mark,
                         const long long* ready, void* stream);
int    navsim_regen_stage(const navsim_config* cfg, const navsim_state* stage, const navsim_step_io* io, uint8_t* want,
                          uint8_t* mark, long long* ready, void* workspace, size_t workspace_bytes, void* stream);
/* navsim_regen_stage for a SHARE of the arenas (round 6): part p of n takes the marks of the 32-bit words w of mark[] with
 * w % n == p -- arenas in groups of four -- into ITS OWN want[] (one array per part; io->done = that array) and stages them.  Parts
 * own disjoint arenas: passes of different parts may run at the same time on different streams, each with its own workspace
 * (the launches of a staging pass for corridor maps with planned starts are latency-bound chains that leave the chip idle:
 * NavSim alternates two parts).  navsim_regen_stage(...) = part 0 of 1. */
int    navsim_regen_stage_part(const navsim_config* cfg, const navsim_state* stage, const navsim_step_io* io, uint8_t* want,
                               uint8_t* mark, long long* ready, void* workspace, size_t workspace_bytes, int32_t part,
                               int32_t n_parts, void* stream);
/* Round 5, the PIPELINED form (ready != NULL, cfg.regen_min_steps > 0): staging passes need not finish before the next swap.
 * ready [2 E] int64 (the second half is the passes' scratch; initialise [0, E) with the staged episode numbers once every arena
 * is staged): navsim_regen_stage records for every arena it served the episode number it staged; navsim_regen_swap installs a finished arena's staged world iff its episode lasted at least cfg.regen_min_steps
 * steps (live->done_steps) AND ready[e] equals the episode the arena now starts -- the first is a rule of the simulation (the
 * oracle's navsim_regen_cpu applies it too), the second a safety net that only fails when the caller queued its staging
 * passes too late (counters[NAVSIM_COUNTER_REGEN_LATE]); want[] is then not consulted.  mark [E rounded up to 4] uint8,
 * 4-byte aligned: set and consumed with 32-bit atomics, so swaps may run while a pass merges it.  The caller's order
 * (NavSim.enable_pregen(pipeline=P)): a staging pass every P steps on a side stream behind an event of that step; before the
 * swap of step k P, wait for the pass queued at step (k - 2) P; cfg.regen_min_steps >= 4 P. */
/* navsim_step + the pipelined navsim_regen_swap in ONE launch: an arena that finishes in this step, whose episode lasted
 * cfg.regen_min_steps steps and whose staged world is ready (ready[e] == the episode that starts), takes that world -- its own
 * workgroup copies the staged rows in place of the restart's second scan -- and asks for the next one (mark, stage->episode);
 * every other finished arena restarts in place exactly as navsim_step leaves it and asks for a world with its new episode
 * number.  Result = navsim_step followed by navsim_regen with regen_cap >= n_envs (every finished arena decides alone: the
 * call needs cfg.regen_cap >= cfg.n_envs; the staging passes' cap is the one of the config THEY are given).  Counters as
 * navsim_regen_swap.  Packed fields, pedestrians inside the step (ped_split 0 / 1); NAVSIM_E_UNSUPPORTED otherwise.
 * The caller queues the staging passes as for the pipelined swap (replace "swap of step" by "step"). */
/* NAVSIM_AUTORESET_NEXT_STEP with late = NULL and cfg.regen_min_steps = 0 (ABI 6): NO fallback call is needed -- an arena that is
 * reset by this call (io->reset_mask) and finds no world staged regenerates its own world inside the launch, its workgroup
 * running navsim_regen's device functions for that one arena in place of the step it does not take (rare, and slow for that
 * one workgroup; the result is navsim_regen's bit for bit).  Worlds of outdoor maps (cfg.regen_indoor_ratio = 0) without
 * cfg.regen_plan and without a costmap, at least 256 threads per arena, cfg.march_rule = NAVSIM_MARCH_F32 (the default);
 * NAVSIM_E_UNSUPPORTED otherwise (pass `late` then). */
/* late [E] uint8 or NULL -- the FALLBACK that needs no rule: the launch writes late[e] = 1 for every arena that finished,
 * is due a new world (by cfg.regen_min_steps, if set) and whose staged world was not ready, 0 for every other arena; the caller
 * follows the launch with navsim_regen(cfg', st, io' with io'->done = late) on the same stream (cfg' = cfg with a regen_cap that
 * sizes the workspace; with no arena late the call's launches find nothing to do).  The result is then navsim_step +
 * navsim_regen whatever the staging passes' timing -- also with cfg.regen_min_steps = 0, i.e. the reference's "a new map at
 * every reset()" unchanged; the passes only decide how many arenas take the fast path.  late = NULL needs
 * cfg.regen_min_steps >= 1 and the caller's order of passes and waits (above). */
int    navsim_step_install(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                           const navsim_state* stage, const float* stage_obs, uint8_t* mark, const long long* ready,
                           uint8_t* late, void* stream);
/* ... with navsim_replan(cfg, st, max_queries) of the PREVIOUS step's flags inside the same launch (navsim_step_replan's form and
 * conditions: costmaps of up to one word per thread of the arena's workgroup, else NAVSIM_E_UNSUPPORTED -- the caller then
 * runs navsim_replan behind navsim_step_install).  max_queries < 0: navsim_step_install. */
int    navsim_step_install_replan(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                                  const navsim_state* stage, const float* stage_obs, uint8_t* mark, const long long* ready,
                                  uint8_t* late, int32_t max_queries, void* stream);
/* NAVSIM_AUTORESET_NEXT_STEP (ABI 6): navsim_step_install[_replan] where an arena that finds no world staged is regenerated
 * BESIDE the next launch instead of behind this one.  An arena that finishes in this call learns at once whether the world of
 * the episode it will start is staged (ready[e]); if not, late_next[e] = 1 (0 for every other arena).  The next call receives
 * those flags as late_prev: it only zeroes the outputs of the arenas flagged there, while the caller's
 *     navsim_regen(cfg' = cfg with defer_reset_scan = 1 and a regen_cap of its own, st, io' with io'->done = late_prev)
 * runs on ANOTHER stream at the same time (both behind the call that wrote the flags; the caller joins the two streams
 * before its next call).  The arenas not flagged install their staged worlds at the front of the launch.  Same rollout as
 * navsim_step + navsim_regen keyed on io->reset_mask, whatever the staging passes' timing -- with no rule (cfg.regen_min_steps
 * = 0) and with nothing of the reset path on the steps' critical path.  late_next, late_prev: [E] uint8, two buffers the
 * caller alternates; max_queries < 0: no re-plan inside the launch. */
int    navsim_step_install_next(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                                const navsim_state* stage, const float* stage_obs, uint8_t* mark, const long long* ready,
                                uint8_t* late_next, const uint8_t* late_prev, int32_t max_queries, void* stream);
/* navsim_regen's helper stream.  Worlds of corridor maps with planned starts (cfg.regen_indoor_ratio > 0, cfg.regen_plan): the
 * distance transform of the new maps runs on a second stream between two events on `stream` (inside a hipGraph capture of
 * `stream` it joins and leaves the capture through them); environment NAVSIM_REGEN_FORK=0 keeps the call on `stream` alone.
 * navsim_regen_helper(s): the calling host thread's helper stream from now on (NULL / never called: one of the library's own,
 * created by navsim_prepare or the first such call).  Why a caller would choose: HIP spreads a process's streams over a few
 * hardware queues in creation order, and two streams on the same queue take turns -- NavSim times candidates against the
 * streams the helper is to run beside (nav_gym_amd/sim.py concurrent_stream).  A helper equal to the stream of a navsim_regen
 * call means "this call does not fork" (the per-step fallback of the pipelined reset path: its helper belongs to the passes). */
int    navsim_regen_helper(void* stream);
int    navsim_regen(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- reset path: costmap (env.py:312-332), pyastar2d.astar_path (env.py:343-354),
 *      path_to_waypoints (env.py:1261-1277) ---------------------------------------------------- */
/* cost [n, H/5, W/5] uint8 (1 = blocked): 5x nearest subsampling + 9x9 dilation (reflect-101 border). */
int navsim_costmap(const uint8_t* occ, int32_t n_maps, int32_t map_h, int32_t map_w, uint8_t* cost, void* stream);
/* n queries; query q plans on costmap map_index[q] (q when NULL).  Shortest 4-connected path between the
 * cells of start[q] and goal[q] (build-defined tie-break), cut into waypoints every
 * `interval` metres.  wp [n,max_wp,2], n_wp [n] (0 = no path), path_cells [n], path_len [n] (env.py:757-759);
 * the last three may be NULL.  The search runs in LDS (4 bytes per costmap cell: up to 200 x 200 cells,
 * i.e. 1000 x 1000 maps; larger costmaps return NAVSIM_E_UNSUPPORTED). */
int    navsim_plan(const uint8_t* cost, const int32_t* map_index, int32_t n_queries, int32_t cost_h, int32_t cost_w,
                   double cost_resolution, double origin_x, double origin_y, const double* start, const double* goal,
                   double interval, int32_t max_wp, double* wp, int32_t* n_wp, int32_t* path_cells, double* path_len,
                   void* stream);

/* env.py:667-680: every pedestrian within 0.5 m of its final waypoint gets a new goal -- a free costmap cell
 * more than cfg->ped_min_goal_dist away (up to 4 rounds of 16 draws) -- and the waypoints of the shortest
 * path to it every 2 m; it keeps its old waypoint when no round finds a path ("only if the human is not
 * adjacent to a wall").  At most max_queries pedestrians per call, in (arena, pedestrian) order; the rest
 * are served by a later call and counted in counters[NAVSIM_COUNTER_REPLAN_UNSERVED].  With st->ped_due present the
 * candidates are the pedestrians flagged there by the last navsim_step (the same set, found without a pass over the
 * state).  A pedestrian standing at
 * the end of a CUT route (st->ped_goal present and different from its last stored waypoint) is first planned to
 * that same goal; only if no path joins them does it draw a new goal like the others.
 * Needs st->costmap.  Call after navsim_step / navsim_regen on the same stream. */
size_t navsim_replan_workspace_bytes(const navsim_config* cfg, int32_t max_queries);
int    navsim_replan(const navsim_config* cfg, const navsim_state* st, int32_t max_queries, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- pedestrian control block (env.py:617-662) with the reference's HumanPolicy actor --------------
 * Weights of human_policy.py:24-30 in torch's own layouts (state_dict order). */
typedef struct navsim_policy_weights {
    const float* cv1_w;   /* [32,3,5]    act_fea_cv1.weight (Conv1d 3->32, k5, s2, p1) */
    const float* cv1_b;   /* [32] */
    const float* cv2_w;   /* [32,32,3]   act_fea_cv2.weight (Conv1d 32->32, k3, s2, p1) */
    const float* cv2_b;   /* [32] */
    const float* fc1_w;   /* [256,4096]  act_fc1.weight */
    const float* fc1_b;   /* [256] */
    const float* fc2_w;   /* [128,260]   act_fc2.weight */
    const float* fc2_b;   /* [128] */
    const float* a1_w;    /* [128]       actor1.weight */
    const float* a1_b;    /* [1] */
    const float* a2_w;    /* [128]       actor2.weight */
    const float* a2_b;    /* [1] */
} navsim_policy_weights;

/* For every live pedestrian: pop waypoints closer than 1 m (env.py:633-640), local goal in the body frame
 * (env.py:644-645), network input = its latest scan clipped to [0, 6], / 6 - 0.5, the same in all three
 * channels (env.py:629-630, 647), speed input = prev_actions; HumanPolicy actor forward
 * (human_policy.py:43-52); prev_actions <- clip(mean, [0,-1], [1,1]) (env.py:655-658);
 * ped_cmd <- prev_actions * v_pref (env.py:659-662), ready for navsim_step with NAVSIM_PED_EXTERNAL.
 * ped_scans [E,N,512] float32 is the output of navsim_ped_scans on the current state (cfg.ped_n_beams must
 * be 512); prev_actions [E,N,2] float32 in/out (zeros at reset, env.py:739); ped_cmd [E,N,2] float64 out.
 * Arithmetic: every dot product is a float32 fused-multiply-add chain in index order
 * starting from 0, bias added last -- what v_mfma_f32_32x32x2_f32 computes -- so device and oracle agree bit
 * for bit; against torch's kernels the mean differs by ~1e-6. */
size_t navsim_ped_policy_workspace_bytes(const navsim_config* cfg);
int    navsim_ped_policy(const navsim_config* cfg, const navsim_state* st, const navsim_policy_weights* w,
                         const float* ped_scans, float* prev_actions, double* ped_cmd, void* workspace,
                         size_t workspace_bytes, void* stream);
/* navsim_ped_policy for the pedestrians of the arenas [e0, e0 + n_e) only; same arrays, same workspace (calls on one workspace
 * must be ordered on one stream). */
int    navsim_ped_policy_part(const navsim_config* cfg, const navsim_state* st, const navsim_policy_weights* w,
                              const float* ped_scans, float* prev_actions, double* ped_cmd, void* workspace,
                              size_t workspace_bytes, int32_t e0, int32_t n_e, void* stream);
/* navsim_ped_scans + navsim_ped_policy in one pass over the pedestrians (round 4): every pedestrian's scan is taken from the
 * CURRENT state by the workgroup that convolves it (env.py:685-693 -> 629-630, 647 -> human_policy.py:38-42), stays in LDS and
 * never travels through HBM; the march of one pedestrian runs beside the convolutions of others.  scans_out [E,N,512] float32
 * or NULL: the clipped scans, exactly what navsim_ped_scans writes (rows of dead slots untouched).  prev_actions, ped_cmd,
 * workspace (navsim_ped_policy_workspace_bytes) as for navsim_ped_policy; results bit-identical to the two calls. */
int    navsim_ped_scan_policy(const navsim_config* cfg, const navsim_state* st, const navsim_policy_weights* w,
                              float* scans_out, float* prev_actions, double* ped_cmd, void* workspace,
                              size_t workspace_bytes, void* stream);

/* order[0..n) = the arenas sorted by descending cost (ties in unspecified order): longest-first launch order
 * for navsim_step (navsim_state.launch_order).  cost is what the step wrote to navsim_state.arena_cost. */
int navsim_launch_order(const uint32_t* cost, int32_t* order, int32_t n, void* stream);

/* navsim_step with that sort INSIDE the step's launch: one more workgroup, ahead of the arenas', sorts sort_cost [E] -- what an
 * EARLIER launch wrote to navsim_state.arena_cost -- into sort_order [E] while the arenas step (navsim_launch_order's rule:
 * 1024 buckets on [0, min(max, 4 mean + 1)], the costliest first, ties in unspecified order).  This launch itself writes
 * st->arena_cost and reads st->launch_order, so the caller keeps two buffers of each and alternates them: sort_order is the
 * launch_order of the launches that follow on the same stream.  Results are navsim_step's.
 * NAVSIM_E_ARG, before any launch: navsim_step's refusals; sort_cost or sort_order NULL, sort_cost == st->arena_cost,
 * sort_order == st->launch_order.  NAVSIM_E_UNSUPPORTED, nothing launched: a state with slot tables (st->map_slot), cfg->ped_split
 * == 2, or a step whose dynamic LDS is smaller than the sort's 4.2 KB (worlds without rect index rows and without pedestrians) --
 * the caller then sorts with navsim_launch_order and calls navsim_step. */
int navsim_step_sorted(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                       const uint32_t* sort_cost, int32_t* sort_order, void* stream);

/* ---- CrowdSim-v0: collision tests, goal test and reward / info selection of CrowdSim.step
 *      (nav_gym/src/crowd_sim/envs/crowd_sim.py:808-945, phase != 'test', border = None) -------------- */
typedef struct navsim_crowd_params {
    double time_step, discomfort_dist, map_size_m, map_resolution;
    double success_reward, collision_penalty, discomfort_penalty_factor, rotation_penalty_factor, timeout_penalty;
    double time_limit;
} navsim_crowd_params;
#define NAVSIM_CROWD_NOTHING 0
#define NAVSIM_CROWD_TIMEOUT 1
#define NAVSIM_CROWD_REACH_GOAL 2
#define NAVSIM_CROWD_COLLISION 3
#define NAVSIM_CROWD_COLLISION_OTHER 4
#define NAVSIM_CROWD_DANGER 5
/* Per env: closest approach of every agent to the robot over the step (point_to_segment_dist,
 * crowd_sim/envs/utils/utils.py:4-26, minus both radii: crowd_sim.py:808-826), the occupancy-grid windows
 * around the robot's next position (collision: half-width ceil(r / sqrt 2 / res) cells, crowd_sim.py:831-861;
 * discomfort: ceil((r + discomfort_dist) / res), crowd_sim.py:872-896), the goal test (crowd_sim.py:909-915)
 * and the reward / done / info cascade (crowd_sim.py:917-949).
 * free_map [E,G,G] uint8, 1 = free, indexed [x][y] like CrowdSim.map; robot [E,10] = px, py, next_px, next_py,
 * next_vx, next_vy, gx, gy, radius, action.r; agents [E,A,5] = px, py, vx, vy, radius; n_agents [E] or NULL
 * (= A); global_time [E].  Outputs reward [E], done [E], info [E] (NAVSIM_CROWD_*), min_dist [E] (Danger). */
int navsim_crowd_check(const navsim_crowd_params* p, int32_t n_envs, int32_t max_agents, int32_t grid,
                       const uint8_t* free_map, const double* robot, const double* agents, const int32_t* n_agents,
                       const double* global_time, double* reward, uint8_t* done, int32_t* info, double* min_dist,
                       void* stream);

/* ---- CrowdSim-v0 local maps (crowd_sim.py:999-1186) ------------------------------------------------ */
#define NAVSIM_CROWD_MAX_VERTS 8
typedef struct navsim_crowd_map_params {
    double angular_min, angular_max;    /* angular_map_min_angle / max_angle (config angle_min / angle_max x pi) */
    double angular_max_range;           /* angular_map_max_range */
    int32_t angular_dim;                /* angular_map_dim */
    int32_t normalize;                  /* get_local_map_angular(normalize=True) */
    double map_size_m, map_resolution, submap_size_m;     /* get_local_map */
} navsim_crowd_map_params;
/* get_local_map_angular (crowd_sim.py:1055-1102) with calculate_angular_map_distances (crowd_sim.py:999-1053): per
 * env the distance to the closest obstacle outline in each of angular_dim sectors of the robot frame, float64.
 * robot [E,4] = px, py, theta, radius; verts [E, max_obst, n_vert, 2] (n_vert <= NAVSIM_CROWD_MAX_VERTS, the
 * reference's obstacles have 4: crowd_sim.py:250-258); n_obst [E] or NULL (= max_obst); out [E, angular_dim]. */
int navsim_crowd_angular_map(const navsim_crowd_map_params* p, int32_t n_envs, int32_t max_obst, int32_t n_vert,
                             const double* robot, const double* verts, const int32_t* n_obst, double* out, void* stream);
/* get_local_map (crowd_sim.py:1104-1166): the binary submap of submap_size_m around the robot, rotated into its
 * heading (rotate_grid_around_center, crowd_sim.py:1168-1186; rotate = 0 skips the rotation) and thresholded at
 * 0.9.  free_map [E,G,G] uint8 (1 = free) indexed [x][y] like CrowdSim.map; robot as above; out [E,S,S] uint8 with
 * S = round(submap_size_m / map_resolution). */
int navsim_crowd_local_map(const navsim_crowd_map_params* p, int32_t n_envs, int32_t grid, const uint8_t* free_map,
                           const double* robot, int32_t rotate, uint8_t* out, void* stream);

/* ---- CrowdSim-v0 pedestrians: ORCA through rvo2 (crowd_sim/envs/policy/orca.py:85-135) and Agent.step
 *      (crowd_sim/envs/utils/agent.py:108-141) -------------------------------------------------------------- */
#define NAVSIM_ORCA_MAX_AGENTS 64      /* agents per query incl. agent 0 */
#define NAVSIM_ORCA_MAX_EDGES  128     /* obstacle edges per polygon set (max_obst * n_vert) */
typedef struct navsim_orca_params {
    float time_step;            /* CrowdSim.time_step (rvo2.PyRVOSimulator(time_step, ...)) */
    float neighbor_dist;        /* orca.py:62 10 */
    float time_horizon;         /* orca.py:64 5 */
    float time_horizon_obst;    /* orca.py:65 5 */
    int32_t max_neighbors;      /* orca.py:63 10 */
} navsim_orca_params;
/* What ORCA.predict does per pedestrian, for Q pedestrians at once: an RVO2 simulator holding agent 0 (the
 * pedestrian itself: position, velocity, radius + 0.01 + safety_space, max speed v_pref, preferred velocity toward
 * its goal) and the other agents it sees (preferred velocity 0), plus the static obstacle polygons; one doStep();
 * the new velocity of agent 0 and the ActionRot(v, r = atan2(vy, vx) - theta) made of it.  Only agent 0's
 * velocity is read back, so only it is computed.  rvo2's source is not in the reference tree: the RVO2 Library 2.0
 * algorithm is restated (oracle/navsim_ref.c says where it knowingly differs: no kd-trees); its half-plane conventions are
 * UNPINNED, its solve, neighbour list and obstacle safety are checked independently (below).
 * agents [Q, A, 6] float64 = px, py, vx, vy, radius, max_speed (A <= NAVSIM_ORCA_MAX_AGENTS); n_agents [Q] or NULL;
 * pref_vel [Q,2]; verts [S, O, V, 2] counter-clockwise polygons (O * V <= NAVSIM_ORCA_MAX_EDGES), n_obst [S] or
 * NULL, obst_set [Q] polygon set of each query or NULL (= set 0); theta [Q] or NULL; out_vel [Q,2]; out_action
 * [Q,2] or NULL.  float32 arithmetic like the library's.
 * What the answer is, apart from how RVO2 computes it: among the velocities within max_speed that satisfy the half-plane
 * of each of the max_neighbors nearest agents strictly inside neighbor_dist (ties by list order), the one nearest to the
 * preferred velocity; if there is none, a velocity within max_speed that minimises the largest penetration of an agent
 * half-plane, obstacle half-planes kept.  Against a float64 evaluation of that statement (tests/orca_f64.py) the velocity
 * holds to 2e-5 m/s, the largest penetration to 4e-5 and the speed to max_speed + 4e-3 when the program is infeasible and
 * no two half-plane directions have |det| < 0.01, and the disc swept for time_horizon_obst enters no polygon by more than
 * 3e-6 m.  NOT bounded: an infeasible program with nearly parallel half-planes.  float32 cancels in linearProgram1's
 * discriminant there, as in the library: speeds up to 1.37 m/s ABOVE max_speed and velocities 1.5 m/s from the float64
 * optimum were seen in crowds of 12-16 agents on 2-6 m.  Callers that need |v| <= max_speed clamp.
 * Degenerate inputs: a half-plane with NaN components (coincident agents with equal velocities) compares false everywhere
 * and is ignored. */
int navsim_crowd_orca(const navsim_orca_params* p, int32_t n_queries, int32_t max_agents, const double* agents,
                      const int32_t* n_agents, const double* pref_vel, int32_t max_obst, int32_t n_vert,
                      const double* verts, const int32_t* n_obst, const int32_t* obst_set, const double* theta,
                      double* out_vel, double* out_action, void* stream);
/* ---- NavGym-v0 pedestrians driven by ORCA (a build-defined model; rvo2 absent) ---------------------
 * navsim_ped_orca follows navsim_ped_policy's protocol: called in front of a navsim_step with NAVSIM_PED_EXTERNAL, it fills
 * ped_cmd from the simulator's own state.  For every live pedestrian i < n_peds[e] of every arena e, in float64 unless
 * stated otherwise and with nothing contracted into FMA:
 *  1. waypoint pop as the policy head and the step do it (sqrt(dx*dx+dy*dy) < 1.0 while head + 1 < n_waypoints); the new
 *     head is written to st->ped_wp_head.
 *  2. preferred velocity (orca.py:116-120): g = wp[head] - pos, s = sqrt(gx*gx + gy*gy), pref = s > 1 ? g / s : g.
 *  3. agent list: the pedestrian itself, the other live pedestrians of the arena in ascending index, then the robot if
 *     robot_visible.  Entries are (px, py, vx, vy, radius, max_speed): pedestrian velocities from ped_vel, pedestrian
 *     radius (ped_radius + 0.01) + safety_space, robot radius (robot_radius + 0.01) + safety_space, max_speed =
 *     ped_v_pref[e,i] for every entry; the robot's velocity is the one the social force sees,
 *     prev_action[e,0] * (cos, sin)(robot_pose[e,2]).  No obstacle polygons: static obstacles are NOT ORCA obstacles in
 *     this entry -- pedestrians follow routes planned on the 1 m-inflated costmap (navsim_ped_orca_walls below adds the
 *     arena's listed rectangles; NAVSIM_PED_SFM has a wall force).
 *  4. navsim_crowd_orca's algorithm on that query with theta = ped_pose[e,i,2]: inputs rounded to float32 where that
 *     function rounds them; neighbour selection, half-planes and linear programs in float32; ActionRot
 *     v = sqrt(vx*vx + vy*vy), r = atan2(vy, vx) - theta (orca.py:128-130).
 *  5. ped_cmd[e,i] = (v, r / cfg->time_step): Human.set_vel's theta + omega dt turns the pedestrian into its ORCA velocity
 *     and it moves by v dt along it.  Neither Human.set_vel nor the step clamps v: where navsim_crowd_orca exceeds
 *     max_speed (see there: infeasible, ill-conditioned programs in packed crowds) the pedestrian exceeds ped_v_pref.
 * Rows of slots >= n_peds[e] are left untouched.  Bit-identical to that composition of the oracle's functions.
 * NAVSIM_E_ARG (before any device call): NULL p or ped_cmd, cfg->ped_model != NAVSIM_PED_EXTERNAL,
 * max_peds + robot_visible > NAVSIM_ORCA_MAX_AGENTS, a non-positive radius / time_step / time_horizon, max_neighbors < 0. */
typedef struct navsim_ped_orca_params {
    navsim_orca_params orca;    /* time_step, neighbor_dist, time_horizon, time_horizon_obst (navsim_ped_orca_walls only), max_neighbors */
    double ped_radius, robot_radius, safety_space;
    int32_t robot_visible;      /* 1: the robot is the last agent of every pedestrian's list */
} navsim_ped_orca_params;
int navsim_ped_orca(const navsim_config* cfg, const navsim_state* st, const navsim_ped_orca_params* p,
                    double* ped_cmd /* [E,N,2] out */, void* stream);
/* navsim_ped_orca with the arena's LISTED rectangles as ORCA obstacles.  Steps 1, 2, 3 and 5 are navsim_ped_orca's; step 4 is
 * navsim_crowd_orca's algorithm on the same query WITH a polygon set, chosen per pedestrian:
 *  - the rectangle list of arena e: entries k = 0 .. 254 of the arena's st->rect_index row (the first 256 x 8 bytes: int16
 *    x0, y0, x1, y1, one distinct rectangle of occupied cells each), the row found through st->map_slot and
 *    cfg->shared_field as the step finds it.  Entries that are all zero are skipped wherever they stand -- so the lone cell
 *    (0,0) as a rectangle of its own is NOT an obstacle -- and so is an entry with x1 < x0 or y1 < y0 (no builder writes one).
 *    x is the index xy_to_ij returns first.
 *  - vertices in float64, rounded to float32 where navsim_crowd_orca rounds its verts: xa = origin_x + (double)x0 * resolution,
 *    xb = origin_x + (double)(x1 + 1) * resolution, ya / yb likewise with origin_y; counter-clockwise (xa,ya), (xb,ya),
 *    (xb,yb), (xa,yb).
 *  - selection, float32 with nothing contracted: range_sq = sqr(time_horizon_obst * max_speed + radius) (navsim_crowd_orca's
 *    obstacle range), dx = max(max(xa - px, px - xb), 0), dy likewise, d2 = dx*dx + dy*dy; in range when d2 < range_sq.  The
 *    max_rects nearest in-range rectangles are kept by Agent::insertAgentNeighbor's rule over ascending k: strict <, ties to
 *    the lower k, the range shrinks to the farthest kept rectangle once the list is full.
 *  - dropped[e,i] (or NULL) = in-range rectangles - kept ones: the cap is observable, no call fails because of it.
 *  - the polygon set of the query: the kept rectangles in ascending k, n_vert = 4; obstacle neighbour edges, the obstacle
 *    half-planes, the agent half-planes behind them, linearProgram2, linearProgram3 with the obstacle half-planes kept are
 *    navsim_crowd_orca's.  (A point outside an axis-aligned rectangle is strictly outside at most two of its edges: at most
 *    2 max_rects obstacle edges and half-planes per pedestrian.)
 * What is an obstacle: the LISTED rectangles and nothing else.  On worlds from navsim_regen with outdoor maps these are the
 * border ring and every box; on other maps the rectangles of the valid tile records (navsim_build_rects) -- a subset of the
 * occupied cells, never a free cell; occupied cells no record names are not seen.  With the default time_horizon_obst = 5
 * the range is about 5 m, more rectangles are in range than kept and dropped is often non-zero: the NEAREST are kept.
 * max_rects = 0: navsim_ped_orca bit for bit (no rectangle is read, rect_index may be NULL, dropped = 0 for live pedestrians).
 * Bit-identical to that composition (tests/ped_orca_walls_spec.py).  Checked in float64 (tests/orca_f64.py): with
 * time_horizon_obst 0.5 and 2 the disc swept for time_horizon_obst along the answer enters no kept rectangle by more than
 * 3e-6 m where it starts clear by 1 mm and nothing was dropped (every max_rects).  NOT bounded: time_horizon_obst = 5 with
 * ten rectangles of a 6 m map in range -- 2 of 90 queries of a 33-pedestrian arena were sent into a box (the centre's path
 * 0.05 m from its corner within the horizon), and other scenes of the kind show the same: a box more than 1.2 m away gets no
 * half-plane, as in navsim_crowd_orca on the same polygons.  Prefer time_horizon_obst <= 2.
 * NAVSIM_E_ARG: navsim_ped_orca's refusals; max_rects < 0 or > NAVSIM_PED_ORCA_MAX_RECTS; max_rects > 0 with
 * st->rect_index == NULL, time_horizon_obst <= 0, cfg->resolution <= 0, cfg->map_h or map_w < 1 (the row cannot be found or
 * turned into metres), or st->map_slot together with cfg->shared_field (which navsim_step refuses too).  NAVSIM_E_UNSUPPORTED, before any launch: the lists of one wavefront --
 * 4 (5 G (N + 1) + (10 L + 16 max_rects) G N) bytes, G = 64 / N arenas (1 above 32), L = min(max_neighbors, N - 1 +
 * robot_visible) -- exceed a CU's 160 KB of LDS. */
#define NAVSIM_PED_ORCA_MAX_RECTS 32   /* 4 x 32 = NAVSIM_ORCA_MAX_EDGES: navsim_crowd_orca can always express the query */
int navsim_ped_orca_walls(const navsim_config* cfg, const navsim_state* st, const navsim_ped_orca_params* p,
                          int32_t max_rects, double* ped_cmd /* [E,N,2] out */, int32_t* dropped /* [E,N] out or NULL */,
                          void* stream);
/* Agent.step with an ActionRot (agent.py:108-141): theta' = theta + r; p += (cos, sin)(theta') * v * dt;
 * vel = v * (cos, sin)(theta'); theta = theta' mod 2 pi.  pose [n,3] in/out, action [n,2], vel [n,2] or NULL. */
int navsim_crowd_agent_step(double* pose, const double* action, double* vel, int32_t n, double time_step, void* stream);

/* navsim_replan + navsim_step in ONE launch (ABI 5): the pedestrians the PREVIOUS step flagged in st->ped_due_prev are
 * re-planned (exactly as navsim_replan(cfg, st, max_queries) would: same candidates, same order, same cap and counters)
 * and then every arena is stepped (exactly as navsim_step would).  The arena with a waiting pedestrian is re-planned by its
 * own workgroup right before that workgroup steps it, and those workgroups open the launch, so the searches -- a chain of
 * dependent breadth-first levels for ~2 % of the arenas -- run beside the step of all the others instead of behind it
 * (round 4) or on a second stream (navsim_step_part).  Needs st->costmap, st->ped_due / ped_due_prev (two buffers the
 * caller alternates, as for navsim_step_part).  A rollout  step_replan, step_replan, ...  equals  step, replan, step,
 * replan, ...  shifted by one re-plan: the first call finds no flags, a final navsim_replan leaves the same state. */
int navsim_step_replan(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io, int32_t max_queries,
                       void* stream);

/* Everything a later navsim_step / navsim_reset_obs / navsim_regen / navsim_replan with this configuration would set ONCE per
 * kernel (dynamic LDS above 64 KB needs hipFuncSetAttribute) is set now; nothing is launched.  Call it before capturing those
 * calls in a hipGraph (nav_gym_amd/sim.py NavSim.enable_graphs): attribute calls do not belong inside a capture.  io: the
 * buffers a reset would use (checked like navsim_reset_obs checks them). */
int navsim_prepare(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io);

/* First observation after reset() (env.py:822-831): scan at the current robot pose, stack filled
 * with copies, prev_pose = pose, vel = 0; sets prev_pose/prev_action/n_hist.  `mask` [E] uint8 or
 * NULL selects which envs are (re)initialised; others keep obs_prev -> obs copied through. */
int navsim_reset_obs(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                     const uint8_t* mask, void* stream);

/* reset() of SOME arenas, part one (env.py:730-746; ABI 6): every arena with mask[e] != 0 takes the next start / goal pair of
 * its spawn table and the next episode number, its step counter returns to 0 (and done_steps[e], when present, records the
 * steps of the episode that is abandoned) -- what the step does at `done` under auto-reset.  Follow it with
 * navsim_reset_obs(mask) (same map: first observations) or navsim_regen with io->done = mask (a new world per arena).
 * Needs the spawn tables. */
int navsim_restart(const navsim_config* cfg, const navsim_state* st, const uint8_t* mask, void* stream);

/* reset() of SOME arenas on a simulator with staged worlds (navsim_regen_stage; stage, stage_obs, mark, ready as for
 * navsim_step_install), in ONE launch: a workgroup of 256 threads per arena.  io: what navsim_reset_obs takes (obs_prev, obs,
 * the goal arrays).
 *   mask[e] == 0  the arena keeps its state; its row is copied obs_prev -> obs (as navsim_reset_obs does); late[e] = 0.
 *   mask[e] != 0  first what navsim_restart does: done_steps[e] = steps[e], episode[e] += 1, steps[e] = 0, the next start /
 *                 goal pair.  Then ready[e] is read (acquire, device scope).  If it equals the new episode[e], the arena's
 *                 workgroup installs the staged world exactly as the step does for an arena that finishes: the slot-table
 *                 exchange (or the map copy without slot tables), the small rows, the staged first observation, the goal
 *                 arrays, ped_due[e] = 0; then it requests the world after this one (barrier, fence, number, flag).
 *                 late[e] = 0, counted in counters[NAVSIM_COUNTER_REGEN_SERVED].
 *                 Otherwise late[e] = 1, counted in counters[NAVSIM_COUNTER_REGEN_LATE]; what is staged carries a stale
 *                 number, so the arena is marked for staging again with episode[e] + 1.  Its world and its row are left to the
 *                 caller: navsim_regen with io->done = late (and cfg.regen_min_steps = 0).
 * cfg.regen_min_steps is not consulted: a reset asks for a new world whatever the length of the abandoned episode.
 * The staged world of arena e is the world of episode[e] + 1, a function of (seed, global arena, episode number) only, and a
 * masked reset starts exactly that episode.  So, followed by navsim_regen with io->done = late, the live state and the rows
 * equal  navsim_restart(mask) + navsim_reset_obs(mask) + navsim_regen with io->done = mask  -- whatever the staging passes'
 * timing (a pass may run beside the launch: the ready / mark protocol is the step's).
 * NAVSIM_E_ARG: stage, stage_obs, mark, ready, mask, late or st->done_steps NULL; mark not 4-byte aligned; the two states differ
 * in their optional buffers or slot tables; cfg->auto_reset == NAVSIM_AUTORESET_NONE.  NAVSIM_E_UNSUPPORTED: a field that is not
 * packed (NAVSIM_FIELD_U16T), cfg->defer_reset_scan.  n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_reset_install(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                         const navsim_state* stage, const float* stage_obs, uint8_t* mark, const long long* ready,
                         const uint8_t* mask, uint8_t* late, void* stream);

/* ---- episode statistics: what gymnasium's RecordEpisodeStatistics keeps, on the device, one launch behind the step ----------
 * Caller-owned device arrays, all [E].  The first five are the accumulators of the episode in progress; the ep_* six are
 * what the latest navsim_episode_stats_update published for the arenas that FINISHED in the step it followed (rows where
 * io->done != 0; the other rows are stale).  A caller that wants the published rows to outlive the next update alternates
 * two sets of ep_* buffers (nav_gym_amd/sim.py does, with the step's own output pairs). */
typedef struct navsim_episode_stats {
    /* episode in progress */
    double*  ret;                   /* sum of the rewards of its steps */
    int32_t* length;                /* steps */
    double*  path_length;           /* metres travelled, from the observation tails */
    double*  min_clearance;         /* min over steps and beams of scan - scan_threshold, metres; +inf before the first step */
    int32_t* discomfort_steps;      /* steps with a beam inside the discomfort zone and none inside the crash zone */
    /* episode that the latest update finished */
    double*  ep_return;
    int32_t* ep_length;
    double*  ep_path_length;
    double*  ep_min_clearance;
    int32_t* ep_discomfort_steps;
    uint8_t* ep_outcome;            /* NAVSIM_EPISODE_* bits */
    unsigned long long* totals;     /* [NAVSIM_N_EPISODE_TOTALS] running totals over finished episodes; may be NULL */
} navsim_episode_stats;

#define NAVSIM_EPISODE_SUCCESS     1   /* io->is_success != 0 in the episode's last step */
#define NAVSIM_EPISODE_CRASH       2   /* io->is_crash != 0 */
#define NAVSIM_EPISODE_TIME_LIMIT  4   /* io->truncated given and set (cfg.max_episode_steps) */

#define NAVSIM_N_EPISODE_TOTALS    5
#define NAVSIM_EPISODE_TOTAL_EPISODES     0   /* finished episodes */
#define NAVSIM_EPISODE_TOTAL_SUCCESSES    1
#define NAVSIM_EPISODE_TOTAL_CRASHES      2
#define NAVSIM_EPISODE_TOTAL_TIME_LIMITS  3
#define NAVSIM_EPISODE_TOTAL_STEPS        4   /* steps of the finished episodes (the sum of their ep_length) */

/* Call it right after navsim_step (and whatever follows the step: navsim_regen, navsim_replan) on the same stream, with the io
 * of that step.  One launch: a wavefront per arena, four arenas per workgroup.
 * Reads io->obs, final_obs, reward, done, is_success, is_crash, truncated (may be NULL), reset_mask, and of the state ONLY
 * st->scan_threshold and st->scan_discomfort.  It never reads a pose: after a same-step restart the state already belongs
 * to the next episode, and the observation's tail carries what is needed.  Per arena e, with S = n_scan_stack, B = n_beams:
 *  1. cfg->auto_reset == NAVSIM_AUTORESET_NEXT_STEP and io->reset_mask[e] != 0: nothing of arena e is touched.  That call of
 *     the step RESET the arena; it returned reward 0, done 0 for it, which is no step of any episode.
 *  2. row = io->final_obs[e] if cfg->auto_reset == NAVSIM_AUTORESET_SAME_STEP and io->done[e], else io->obs[e]: the LAST
 *     observation of the step, what the reference's step() returns (env.py:700-728).  scan = row[(S-1) B : S B], the newest
 *     scan of the stack (_stack_scan, env.py:257-279; older slots are not read); tail = row[S B :] = prev_xy, xy, vel, yaw
 *     (env.py:455).
 *  3. length += 1; ret = ret + io->reward[e].
 *  4. dx = (double)tail[2] - (double)tail[0]; dy = (double)tail[3] - (double)tail[1];
 *     path_length = path_length + sqrt(dx * dx + dy * dy).  float64, in this order, every operation rounded on its own (no
 *     fused multiply-add: DESIGN.md section 4).  After a crash the row is the re-scan at the REVERTED pose (env.py:700-717),
 *     so the increment of a crash step is whatever that row's tail says -- the statistic follows the observations.
 *  5. min_clearance = min(min_clearance, min over k of (double)scan[k] - (double)scan_threshold[k]).
 *  6. crash_row = any k: scan[k] < scan_threshold[k]; discomfort_steps += (any k: scan[k] < scan_discomfort[k]) and not
 *     crash_row (env.py:543-547; float32 comparisons like the reference's).
 *  7. io->done[e] != 0: ep_outcome[e] = (is_success[e] != 0) | (is_crash[e] != 0) << 1 | (truncated && truncated[e]) << 2; the
 *     five accumulators go to ep_*[e]; totals, when given, receive integer atomic adds (episodes + 1, the outcome's counts,
 *     steps + length: integer sums, the same whatever the order); the accumulators return to (0, 0, 0, +inf, 0).
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, io or s NULL; any of the eleven arrays of s (totals aside),
 * io->obs, reward, done, is_success, is_crash, st->scan_threshold or st->scan_discomfort NULL; SAME_STEP without
 * io->final_obs; NEXT_STEP without io->reset_mask; n_envs < 0, n_beams < 1, n_scan_stack < 1.  NAVSIM_E_UNSUPPORTED: more than
 * 8192 beams (the two threshold tables are staged in 64 KB of LDS).  n_envs == 0: NAVSIM_OK, nothing is launched.
 * NAVSIM_AUTORESET_NONE: nothing restarts by itself, and an arena that is stepped on past its `done` may keep that flag set
 * (the reference's step() does the same); every such call would be published as an episode of one step and counted.  The
 * caller resets finished arenas before their next step (navsim_restart + navsim_reset_obs, with navsim_episode_stats_clear)
 * for the rows and totals to mean episodes. */
int navsim_episode_stats_update(const navsim_config* cfg, const navsim_state* st, const navsim_step_io* io,
                                const navsim_episode_stats* s, void* stream);
/* The accumulators of the arenas with mask[e] != 0 (mask NULL: of all arenas) return to (0, 0, 0, +inf, 0): what a reset() of
 * those arenas needs.  ep_* and totals are not touched.  NAVSIM_E_ARG: cfg or s NULL, one of the eleven arrays NULL. */
int navsim_episode_stats_clear(const navsim_config* cfg, const navsim_episode_stats* s, const uint8_t* mask, void* stream);

/* ---- observed pedestrians: the K nearest pedestrians the robot has in line of sight, in its frame, from one launch ------------
 * What the SARL / CADRL / attention family of crowd-navigation policies takes as input: per arena a list of observed humans --
 * position and velocity in the robot's frame, sorted by distance, an entry only for a human the robot can actually see.
 * BUILD-DEFINED, all of it: the reference's NavGym-v0 has no such observation (env.py:455-461 returns the lidar stack and a
 * 7-float tail).  In particular: the line of sight starts at the scan's INTEGER origin cell (env.py:386, 419) while d comes from
 * the float64 pose -- the two can be up to a cell apart; only one or three rays are cast per pedestrian, so partial occlusion
 * between them is not seen; other pedestrians and the robot's own body do not occlude. */
typedef struct navsim_ped_observe_params {
    double  ped_radius;     /* metres, >= 0 */
    double  sensor_range;   /* metres, finite, >= 0: a pedestrian is in range iff d - ped_radius <= sensor_range */
    int32_t max_obs;        /* K, 1 .. NAVSIM_MAX_PEDS: rows kept per arena */
    int32_t rays;           /* 1 or 3: lines of sight tried per pedestrian */
    int32_t occlusion;      /* 0: every pedestrian in range (and in the field of view) counts as seen; no march */
    int32_t fov;            /* 1: the relative bearing must lie in [cfg.angle_min, cfg.angle_last] */
} navsim_ped_observe_params;

typedef struct navsim_ped_observation {
    float*   state;    /* [E,K,5] x, y, vx, vy in the robot's frame, d */
    int32_t* index;    /* [E,K]   pedestrian index of the row, -1 = unused row */
    int32_t* count;    /* [E]     pedestrians SEEN (may exceed K: the cap is observable) */
    uint8_t* visible;  /* [E,N]   1 = pedestrian i is seen; may be NULL */
} navsim_ped_observation;

/* One launch (a wavefront per arena, four arenas per workgroup) that reads st->robot_pose, n_peds, ped_pose, ped_vel and the
 * distance field of the arena's map slot (cfg.shared_field, st->map_slot, st->field_overflow; both field formats), and writes
 * EVERY element of `out`.  Call it behind the step (and whatever follows it: navsim_regen, navsim_replan) on the same stream.
 * Per arena e, everything float64 in exactly this order, every operation rounded on its own (no fused multiply-add: DESIGN.md
 * section 4); nv:: are the functions of navmath.hpp / navmath_ref.h; N = cfg.max_peds, K = p->max_obs:
 *  1. skip && skip[e]: count = 0, every row of state 0, every index -1, visible 0.  The arena is done.
 *  2. n = min(n_peds[e], N); (rx, ry, th) = robot_pose[e]; c = nv::cos(th), s = nv::sin(th);
 *     (i0, j0) = xy_to_ij_f32((float)rx, (float)ry): the integer cell the robot's own scan starts from (env.py:386, 419).
 *  3. pedestrian i < n: ax = px_i - rx, ay = py_i - ry, d = sqrt(ax*ax + ay*ay); x = c*ax + s*ay, y = c*ay - s*ax; with
 *     ped_vel, vxr = c*vx + s*vy, vyr = c*vy - s*vx.  in_range = (d - ped_radius <= sensor_range).
 *     in_fov = !fov || (cfg.angle_min <= b && b <= cfg.angle_last), b = nv::atan2(y, x).
 *  4. line of sight: seen = 1 when !occlusion or d <= ped_radius.  Otherwise ux = ax/d, uy = ay/d, and ray k = 0 .. rays-1
 *     with the offsets o = (0, +ped_radius, -ped_radius) -- the centre, then the two silhouette points -- is cast at
 *     tx = ax - o_k*uy, ty = ay + o_k*ux: heading = (float)nv::atan2(ty, tx), (dx, dy) = beam_dir(heading) (navsim_cast_static's),
 *     r = the restatement of range_libc's calc_range that navsim_cast_static runs, on the field of the arena's map slot, from
 *     ((float)i0, (float)j0) along (dx, dy) with max_range = (float)((int64)H*W) and cfg.march_rule -- the general form with its
 *     bounds test: a ray that leaves the map returns max_range.  r_m = (double)(r * (float)cfg.resolution), the float32 product
 *     of env.py:426.  reach = sqrt(tx*tx + ty*ty) - (k == 0 ? ped_radius : 0).  Ray k is clear iff r_m >= reach; seen = any
 *     ray clear.  (The kernel stops a ray at floor(reach / resolution) + 4 cells -- at most floor((sensor_range + 2 ped_radius) /
 *     resolution) + 4 for a pedestrian in range -- where every outcome is `clear`; kernels_ped_observe.hpp writes the bound out;
 *     the result is the one of H*W.)
 *  5. visible[e,i] = in_range && in_fov && seen; entries i >= n are 0.  count[e] = the number of set entries.
 *  6. the seen pedestrians in ascending (d, i) order -- equal d: the lower index first -- give the first min(count, K) rows:
 *     state[e,row] = ((float)x, (float)y, (float)vxr, (float)vyr, (float)d), index[e,row] = i.  Every further row is 0 / -1.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p or out NULL; out->state, index or count NULL; st->robot_pose,
 * n_peds, ped_pose, ped_vel or field NULL; cfg.ped_model == NAVSIM_PED_NONE; max_obs outside 1 .. NAVSIM_MAX_PEDS; rays not 1
 * or 3; ped_radius or sensor_range negative or not finite; n_envs < 0; max_peds outside 1 .. NAVSIM_MAX_PEDS; map_h or map_w
 * < 1; a march_rule that is none of NAVSIM_MARCH_*; st->map_slot with cfg.shared_field.  NAVSIM_E_UNSUPPORTED: a field_format
 * that is neither NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T.  n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_ped_observe(const navsim_config* cfg, const navsim_state* st, const navsim_ped_observe_params* p,
                       const uint8_t* skip, const navsim_ped_observation* out, void* stream);

/* ---- goal path: a distance-to-goal field per arena, and from it the robot's path distance and a steering sub-goal ---------------
 * What a policy, a reward shaper, a curriculum or an evaluation ("success weighted by path length") reads where the straight line
 * to the goal (info['distance']) points through walls.  BUILD-DEFINED, all of it: the reference plans the spawn path on its
 * costmap and throws it away (env.py:366-383); it has no field and no sub-goal.  Everything below is integer arithmetic or
 * float64 with every operation rounded on its own (no fused multiply-add: DESIGN.md section 4).
 *
 * THE NAVIGATION GRID of an arena.  Hc = map_h / 5, Wc = map_w / 5 (integer division): the costmap's cells.  Nav cell (ic, jc),
 * 0 <= ic < Wc along x (the field's column), 0 <= jc < Hc along y (the field's row), is SAMPLED at map cell (5 ic + 2, 5 jc + 2):
 * d = the float32 distance, in cells, that the field of the arena's map slot holds there (cfg.shared_field, st->map_slot,
 * st->field_overflow; identical in NAVSIM_FIELD_F32 and NAVSIM_FIELD_U16T, the overflow plane included).  With
 * hard = (float)(hard_clearance / resolution) and clear = (float)(clearance / resolution), float32 comparisons:
 *   d < hard: IMPASSABLE;   hard <= d < clear: in the BAND, multiplier m = band_cost;   otherwise CLEAR, m = 1.
 * Cells outside the grid are impassable.  hard_clearance >= 3 resolution is required: the sample lies at most 2.83 cells from every
 * cell of its 5 x 5 block, so every nav cell whose block holds an occupied cell is impassable -- a wall one cell thick does not leak.
 * The nav cell OF A POSITION (x, y): (i, j) = xy_to_ij_f32((float)x, (float)y), the scan's origin cell (env.py:386, 419);
 * (ic, jc) = (min(i / 5, Wc - 1), min(j / 5, Hc - 1)).
 *
 * THE FIELD.  dist [Hc, Wc] uint16 per arena (element jc Wc + ic), in map cells: a straight hop weighs 5, a diagonal hop 7;
 * 0xFFFF = impassable, unreachable, or farther than 65534.  The GOAL CELL is the nav cell of st->robot_goal[e]; it has
 * dist = 0 whatever its class.  A neighbour n of a cell is ADMISSIBLE when it lies in the grid and is passable (not impassable)
 * or the goal cell, and -- for a diagonal hop -- the two cells orthogonally adjacent to both are passable or the goal cell as
 * well (no corner is cut).  Every other passable cell c holds
 *     dist[c] = min(0xFFFF, min over admissible neighbours n of dist[n] + w(direction) m(c)),
 * an impassable cell that is not the goal cell holds 0xFFFF.  With positive weights these equations have exactly one solution, the
 * cost of the cheapest path saturated at 0xFFFF, so the field does not depend on the order in which cells are relaxed.
 *
 * NEIGHBOUR ORDER k = 0 .. 7, (d ic, d jc): (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (+1,-1) (-1,+1) (-1,-1); w = 5 for k < 4, else 7. */
typedef struct navsim_goal_path_params {
    double  hard_clearance;   /* metres, finite, >= 3 cfg.resolution */
    double  clearance;        /* metres, finite, >= hard_clearance */
    double  lookahead;        /* metres, finite, >= 0: how far down the field the sub-goal lies */
    int32_t band_cost;        /* 1 .. 16: the multiplier of a hop that leaves a band cell */
} navsim_goal_path_params;

typedef struct navsim_goal_field {
    uint16_t* dist;                  /* [E,Hc,Wc] */
    int64_t*  key;                   /* [E,3] (episode, bits of gx, bits of gy) the arena's field was built for; the caller
                                        initialises key[e,0] = -1: never built */
    unsigned long long* rebuilds;    /* [1] fields rebuilt so far (atomic adds); may be NULL */
} navsim_goal_field;

typedef struct navsim_goal_path_out {
    float*   distance;   /* [E]   metres */
    float*   subgoal;    /* [E,2] the target in the robot's frame, metres */
    uint8_t* status;     /* [E]   0 = skipped, else NAVSIM_GOAL_PATH_* */
} navsim_goal_path_out;

#define NAVSIM_GOAL_PATH_OK                 1   /* the robot stands on the field; distance is a path length */
#define NAVSIM_GOAL_PATH_REACHED_GOAL_CELL  2   /* or'ed to OK: the walk ended on the goal cell, the sub-goal IS the goal */
#define NAVSIM_GOAL_PATH_OFF_FIELD          4   /* the robot's nav cell holds 0xFFFF: straight-line values */

/* Bytes of navsim_goal_field.dist: n_envs (map_h / 5) (map_w / 5) uint16.  0: cfg NULL, n_envs < 0, map_h / 5 < 1 or map_w / 5 < 1. */
size_t navsim_goal_field_bytes(const navsim_config* cfg);

/* TWO launches, whatever the number of arenas that rebuild (kernels_goal_path.hpp): the first tests every arena's key and
 * rebuilds the stale fields, one 1024-thread workgroup per field with the grid in LDS; the second answers the query of every
 * arena, eight lanes an arena, without LDS.  No device-to-host copy, nothing that blocks; every loop in both kernels has a
 * stated bound.  Call it behind the step (and whatever follows it: navsim_regen, navsim_replan) on the same stream.  It reads
 * st->robot_pose, robot_goal, episode and the distance field, and writes EVERY element of `out`.  Per arena e:
 *  1. skip && skip[e]: distance = 0, subgoal = (0, 0), status = 0.  Nothing of the arena is rebuilt or read; its key stays.
 *  2. rebuild: iff (rebuild && rebuild[e]) or key[e] != (st->episode[e], the 64 bits of gx, the 64 bits of gy) the arena's
 *     field is rebuilt as above from its map and (gx, gy) = robot_goal[e]; key[e] is recorded and *rebuilds += 1.
 *     Every in-launch restart advances episode[e] (the step's restart from the spawn table, navsim_step_install*, navsim_regen
 *     behind the step -- it serves arenas the step restarted --, navsim_regen_swap, navsim_reset_install, navsim_restart), so the
 *     key follows them; a caller that changes a map or a goal WITHOUT a new episode number (a reset of every arena that starts
 *     the numbers again, a state loaded from a snapshot) passes rebuild for those arenas.
 *  3. (rx, ry, th) = robot_pose[e]; the robot's nav cell r as above.  dist[r] == 0xFFFF: status = OFF_FIELD, target = the goal
 *     (gx, gy), rem = 0; continue at 6.
 *  4. the walk: cur = r, walked = 0, L = lookahead_cells = (int)min(floor(lookahead / resolution), 1048576.0).  At most
 *     min(L / 5, Hc Wc) times: stop if cur is the goal cell; among the admissible neighbours n_k of cur take the one with the
 *     least (dist[n_k] + w_k, k) -- ties go to the lower k of the neighbour order; stop if there is none (which a field built by
 *     step 2 never shows) or if walked + w_k > L; else cur = n_k, walked += w_k.  On a field of step 2 dist falls at every hop
 *     (dist[n_k] <= dist[cur] - 5 m(cur) + 2), so the walk needs no more than L / 5 hops and never returns to a cell.
 *  5. the target: cur is the goal cell: (gx, gy) itself, rem = 0, status = OK | REACHED_GOAL_CELL.  Otherwise the centre of cur,
 *     (origin_x + ((double)(5 ic) + 2.5) * resolution, origin_y + ((double)(5 jc) + 2.5) * resolution), rem = dist[cur], status = OK.
 *  6. dx = tx - rx, dy = ty - ry; distance = (float)(sqrt(dx*dx + dy*dy) + (double)rem * resolution);
 *     c = nv::cos(th), s = nv::sin(th); subgoal = ((float)(c*dx + s*dy), (float)(c*dy - s*dx)).
 *  7. consequence: distance is the length in metres (5 / 7 chamfer metric: between 1 % below and 8 % above the Euclidean length
 *     between two cells) of the cheapest path where that path keeps `clearance` from the walls; it OVERSTATES it by (band_cost - 1) times
 *     the part that runs inside the band; it equals the straight-line distance, bit for bit what step 3 would give, once the goal
 *     cell lies within the look-ahead.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p, field or out NULL; field->dist or key, out->distance, subgoal or
 * status NULL (rebuilds may be NULL); st->robot_pose, robot_goal, episode or field NULL; a parameter that is not finite;
 * hard_clearance < 3 resolution; clearance < hard_clearance; band_cost outside 1 .. 16; lookahead < 0; n_envs < 0; map_h / 5 < 1
 * or map_w / 5 < 1; st->map_slot with cfg.shared_field.  NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32
 * nor NAVSIM_FIELD_U16T; a grid whose 3 (Hc + 2) (Wc + 2) bytes do not fit the LDS of one workgroup (160 KB less 8 KB: 200 x 200
 * nav cells, the reference's 1000 x 1000 maps, take 122.4 KB).  n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_goal_path(const navsim_config* cfg, const navsim_state* st, const navsim_goal_path_params* p,
                     const uint8_t* rebuild, const uint8_t* skip, const navsim_goal_field* field,
                     const navsim_goal_path_out* out, void* stream);

/* ---- local planner: a dynamic-window action per arena from one launch ------------------------------------------------------------
 * A classical baseline controller on the batch (a number to beat, an expert for demonstrations, a per-candidate cost surface, a
 * check that an arena is solvable): every arena forms a window of reachable twists around the twist its last step integrated,
 * rolls each candidate out with the step's own kinematics, tests a disc model of the robot's body against the arena's distance
 * field and against pedestrians moved at constant velocity, scores the admissible candidates and returns the best as an action.
 * BUILD-DEFINED, all of it: the reference has ORCA as a robot policy of its other simulator only, NavGym-v0 has no controller. */
#define NAVSIM_DWA_MAX_DISCS 4
typedef struct navsim_dwa_params {
    double  acc_lin, acc_rot;          /* >= 0: the window is prev twist +- acc * cfg.time_step */
    double  body_radius;               /* >= 0 */
    double  body_offset[NAVSIM_DWA_MAX_DISCS];  /* disc centres on the body's x axis, metres from the pose origin */
    double  ped_radius, margin, clearance_cap;  /* >= 0 */
    double  w_progress, w_heading, w_clearance, w_speed;   /* finite */
    int32_t n_discs;                   /* 1 .. 4 */
    int32_t n_v, n_w;                  /* 1 .. 16, 1 .. 32: C = n_v n_w candidates, index c = iv n_w + iw */
    int32_t horizon;                   /* T, 1 .. 32 steps of cfg.time_step */
    int32_t use_peds;                  /* 0: pedestrians ignored (always so with NAVSIM_PED_NONE) */
} navsim_dwa_params;

#define NAVSIM_DWA_OK      1   /* the chosen candidate is admissible */
#define NAVSIM_DWA_BLOCKED 2   /* no candidate is admissible: the chosen one violates the margin last */

typedef struct navsim_dwa_out {
    double*  twist;      /* [E,2] chosen (v, omega) */
    double*  action;     /* [E,2] the same in cfg.action_kind's form (WHEELS: wl = (v - omega track / 2) / r, wr = (v + omega track / 2) / r) */
    float*   clearance;  /* [E]   the chosen candidate's minclr (below), metres */
    int32_t* best;       /* [E]   chosen candidate index */
    uint8_t* status;     /* [E]   0 skipped, NAVSIM_DWA_OK 1, NAVSIM_DWA_BLOCKED 2 */
    double*  scores;     /* [E,C] or NULL: score of every candidate, -inf where inadmissible */
    int32_t* first_hit;  /* [E,C] or NULL: 0 = admissible, else the step k of the first violation */
} navsim_dwa_out;

/* ONE launch (a workgroup per arena, a lane per candidate; kernels_dwa.hpp), no device-to-host copy, nothing that blocks.  Call it
 * behind the step (and whatever follows it: navsim_regen, navsim_replan, navsim_goal_path -- whose out->subgoal is this call's
 * `subgoal`) on the same stream.  It reads st->robot_pose, robot_goal, prev_action, the distance field of the arena's map slot
 * (cfg.shared_field, st->map_slot, st->field_overflow; both field formats) and, with pedestrians, n_peds, ped_pose and ped_vel; it
 * writes EVERY element of `out`.  Everything is float64 in exactly this order, every operation rounded on its own (no fused
 * multiply-add: DESIGN.md section 4); nv:: are the functions of navmath.hpp / navsim_device.hpp (navmath_ref.h); dt = cfg.time_step,
 * N = cfg.max_peds, T = p->horizon, C = n_v n_w.  Per arena e:
 *  1. skip && skip[e]: twist, action, clearance and best are 0, status is 0, the arena's rows of scores / first_hit are 0.
 *     Nothing of the arena is read.
 *  2. the window.  (v0, w0) = st->prev_action[e]: the twist the last step integrated.  The step stores it in TWIST form whatever
 *     cfg.action_kind is -- after the wheel conversion, cfg.clamp_action and cfg.min_turning_radius (include/navsim.h
 *     NAVSIM_ACTION_WHEELS: "the twist after conversion and clamp is what the step integrates"), (0, 0) at the start of an episode
 *     -- so nothing is converted back.
 *     vlo = max(linvel_lo, v0 - acc_lin * dt), vhi = min(linvel_hi, v0 + acc_lin * dt); if vlo > vhi both become
 *     min(max(v0, linvel_lo), linvel_hi).  wlo, whi alike from w0, acc_rot and rotvel_lo, rotvel_hi.
 *     v_iv = n_v == 1 ? vhi : vlo + (vhi - vlo) * ((double)iv / (double)(n_v - 1)), iv = 0 .. n_v - 1;
 *     w_iw = n_w == 1 ? whi : wlo + (whi - wlo) * ((double)iw / (double)(n_w - 1)), iw = 0 .. n_w - 1.
 *     Candidate c = iv n_w + iw is the twist (v_iv, w_iw).
 *  3. the target.  (rx, ry, th) = robot_pose[e].  subgoal == NULL: (tx, ty) = robot_goal[e].  Otherwise, with
 *     (s, c) = nv::sincos(th) and (sx, sy) = subgoal[e] widened to float64: tx = rx + (c*sx - s*sy), ty = ry + (s*sx + c*sy).
 *     dx = tx - rx, dy = ty - ry, d0 = sqrt(dx*dx + dy*dy).
 *  4. the rollout of candidate c.  p = robot_pose[e], minclr = clearance_cap, hit = 0.  For k = 1 .. T:
 *     nv::set_vel(p, v, w, dt, cfg.axle_offset, nullptr) (the step's integration, env.py:664), then (sk, ck) = nv::sincos(p[2]).
 *     For disc j < n_discs: cx = p[0] + body_offset[j] * ck, cy = p[1] + body_offset[j] * sk.
 *       static clearance: (i, j) = nv::xy_to_ij(cx, cy) (batch_xy_to_ij on float64 inputs, env.py:1228-1253), then
 *       i = min(i, map_w - 1), j = min(j, map_h - 1) -- xy_to_ij clips x by map_h and y by map_w, which differ on a map that is
 *       not square --; cs = (double)field.at(i, j) * resolution - body_radius, field.at = the float32 distance in cells the
 *       field of the arena's map slot holds for column i, row j.
 *       pedestrian clearance, when use_peds and cfg.ped_model != NAVSIM_PED_NONE, for every pedestrian q < min(n_peds[e], N):
 *       tk = (double)k * dt, ex = (ped_pose[e,q,0] + ped_vel[e,q,0] * tk) - cx, ey = (ped_pose[e,q,1] + ped_vel[e,q,1] * tk) - cy,
 *       cp = sqrt(ex*ex + ey*ey) - (ped_radius + body_radius).
 *     clr_k = the least of all cs and cp of step k.  clr_k < margin: hit = k and the rollout stops.  Otherwise
 *     minclr = min(minclr, clr_k).
 *  5. the score of an admissible candidate (hit == 0).  With p the pose after step T and (sT, cT) = nv::sincos(p[2]):
 *     gx = tx - p[0], gy = ty - p[1], dT = sqrt(gx*gx + gy*gy), align = dT > 0 ? (cT*gx + sT*gy) / dT : 1,
 *     score = ((w_progress * (d0 - dT) + w_heading * align) + w_clearance * minclr) + w_speed * v.
 *  6. the choice.  The admissible candidate with the greatest score wins, ties go to the lowest c: status = NAVSIM_DWA_OK.  No
 *     candidate admissible: the one with the greatest hit wins, ties to the lowest c: status = NAVSIM_DWA_BLOCKED.
 *     twist = its (v, w); action = twist under NAVSIM_ACTION_TWIST, ((v - w * wheel_track / 2) / wheel_radius,
 *     (v + w * wheel_track / 2) / wheel_radius) under NAVSIM_ACTION_WHEELS; clearance = (float)minclr -- of a blocked candidate
 *     the least clearance of the steps before its hit --; best = c.
 *  7. scores[e,c] = the score, -inf where hit != 0; first_hit[e,c] = hit -- of every candidate, when the arrays are given.
 * (The kernel takes each step's minima over float32 field values and over squared distances and converts once: sqrt, the product
 * with resolution and the subtraction of a constant are monotone and correctly rounded, so the results are the rule's bit for bit.)
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p or out NULL; out->twist, action, clearance, best or status NULL
 * (scores and first_hit may be NULL); st->robot_pose, robot_goal, prev_action or field NULL; st->n_peds, ped_pose or ped_vel NULL
 * with use_peds set and a pedestrian model on (then also max_peds outside 1 .. NAVSIM_MAX_PEDS); a parameter that is not finite;
 * acc_lin, acc_rot, body_radius, ped_radius, margin or clearance_cap negative; n_discs outside 1 .. 4, n_v outside 1 .. 16, n_w
 * outside 1 .. 32, horizon outside 1 .. 32; n_envs < 0; map_h or map_w < 1; resolution or time_step not finite or not positive;
 * an action_kind that is none of NAVSIM_ACTION_*, NAVSIM_ACTION_WHEELS with a wheel_radius that is not positive; st->map_slot with
 * cfg.shared_field.  NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T.
 * n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_dwa(const navsim_config* cfg, const navsim_state* st, const navsim_dwa_params* p,
               const float* subgoal /* [E,2] robot frame, or NULL */, const uint8_t* skip,
               const navsim_dwa_out* out, void* stream);

/* ---- egocentric local map: wall and pedestrian grids per arena in the robot's frame, one launch -------------------------------------
 * What a CNN policy over a local costmap, a DRL-VO style pedestrian "kinematic map" or the local-map half of the reference's
 * SOADRL networks (crowd_nav/policy/network_om.py) reads: a G x G picture around the robot, rotated with it, of the clearance to
 * the walls, the clearance to the nearest pedestrian and the velocity of the pedestrian that covers a cell.  BUILD-DEFINED, all
 * of it (navsim_crowd_local_map serves only the other simulator's binary CrowdSim.map). */
#define NAVSIM_LOCAL_MAP_MAX 128
typedef struct navsim_local_map_params {
    double  cell;        /* metres per grid cell, finite, > 0 */
    double  ahead;       /* metres the window's centre lies ahead of the pose origin on the body's x axis, finite */
    double  cap;         /* metres, finite, > 0: clearances saturate here */
    double  ped_radius;  /* metres, finite, >= 0 */
    int32_t size;        /* G, 1 .. NAVSIM_LOCAL_MAP_MAX (128) */
    int32_t channels;    /* C: 1 walls; 2 + pedestrian clearance; 4 + the covering pedestrian's velocity */
} navsim_local_map_params;

/* ONE launch (arena x strip of cells, four cells and one 16-byte store per lane and channel where G % 4 == 0;
 * kernels_local_map.hpp), no device-to-host copy, nothing that blocks, no allocation.  Call it behind the step (and whatever
 * follows it: navsim_regen, navsim_replan; navsim_ped_observe when its `visible` array is this call's) on the same stream.  It
 * reads st->robot_pose, the distance field of the arena's map slot (cfg.shared_field, st->map_slot, st->field_overflow; both field
 * formats) and, with channels > 1, n_peds and ped_pose (channels == 4: ped_vel); it writes EVERY element of out [E,C,G,G] float32,
 * out[e, ch, r, q].  Everything is float64 in exactly this order, every operation rounded on its own (no fused multiply-add:
 * DESIGN.md section 4); nv:: are the functions of navmath.hpp / navsim_device.hpp (navmath_ref.h); G = p->size, C = p->channels,
 * N = cfg.max_peds; min / max as written: min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b.  Per arena e:
 *  1. skip && skip[e]: every element of the arena's block out[e] is 0.  Nothing of the arena is read.
 *  2. the pose.  (rx, ry, th) = robot_pose[e], (s, c) = nv::sincos(th).
 *  3. the centre of cell (r, q), r counting FORWARD along the body's x axis and q to the LEFT along its y axis:
 *     u = (((double)r + 0.5) - (double)G * 0.5) * cell + ahead,  v = (((double)q + 0.5) - (double)G * 0.5) * cell,
 *     wx = rx + (c*u - s*v),  wy = ry + (s*u + c*v).
 *  4. channel 0, the wall clearance.  fi = (float)((wx - origin_x) / resolution), fj = (float)((wy - origin_y) / resolution):
 *     the float32 quotients of nv::xy_to_ij, before its clipping.  The cell is INSIDE iff 0 <= fi && fi < (float)map_w &&
 *     0 <= fj && fj < (float)map_h -- the field has map_w columns for i and map_h rows for j, the addressing of navsim_dwa step 4
 *     (which clamps i by map_w and j by map_h).  On a map that is not square this DELIBERATELY differs from xy_to_ij's own
 *     clipping, which clips x by map_h and y by map_w (env.py:1244-1247): a picture of the map shows the map that is stored.
 *     Inside: (i, j) = ((int)fi, (int)fj), value = (float)min((double)field.at(i, j) * resolution, cap), field.at = the float32
 *     distance in cells the field of the arena's map slot holds for column i, row j.  Outside: 0 -- the world ends in a wall.
 *  5. channel 1 (C >= 2), the pedestrian clearance.  Of the pedestrians i < min(n_peds[e], N) -- with `visible` given only those
 *     with visible[e*N + i] != 0 --: ex = ped_pose[e,i,0] - wx, ey = ped_pose[e,i,1] - wy, d2 = ex*ex + ey*ey; the NEAREST one has
 *     the least (d2, i).  No pedestrian: value = (float)cap.  Otherwise value = (float)min(max(sqrt(d2) - ped_radius, 0), cap).
 *  6. channels 2 and 3 (C == 4), the velocity.  Where the nearest pedestrian covers the cell, sqrt(d2) <= ped_radius, its velocity
 *     (vx, vy) = ped_vel[e,i] in the robot's frame: (float)(c*vx + s*vy) and (float)(c*vy - s*vx).  Elsewhere both are 0.
 * (The kernel finds the nearest pedestrian over squared distances and takes one sqrt: the rule's own order.)
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p or out NULL; st->robot_pose or st->field NULL; channels none of 1,
 * 2, 4; size outside 1 .. NAVSIM_LOCAL_MAP_MAX; cell or cap not finite or not positive; ahead not finite; ped_radius not finite or
 * negative; channels > 1 with cfg.ped_model == NAVSIM_PED_NONE, with st->n_peds, ped_pose or ped_vel NULL or with max_peds outside
 * 1 .. NAVSIM_MAX_PEDS; st->map_slot with cfg.shared_field; n_envs < 0; map_h or map_w < 1; resolution not finite or not positive;
 * origin_x or origin_y not finite.  NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T.
 * n_envs == 0: NAVSIM_OK, nothing is launched.  `visible` is not read with channels == 1. */
int navsim_local_map(const navsim_config* cfg, const navsim_state* st, const navsim_local_map_params* p,
                     const uint8_t* visible /* [E,N] or NULL */, const uint8_t* skip /* [E] or NULL */,
                     float* out /* [E,C,G,G] */, void* stream);

/* ---- scan ground truth: the robot's scan without noise, and per beam what it fell on, from one launch ---------------------------
 * What a 2D-lidar person / leg detector (the DROW / DR-SPAAM family) or a lidar tracker trains on, what a policy that masks or
 * weights pedestrian returns reads, and what a scan denoiser takes as its target: the step's observation has walls, pedestrian
 * bodies, pedestrian legs and (optionally) noise min-merged into one range per beam and keeps no record of which won.
 * BUILD-DEFINED, all of it: the reference returns the merged scan alone (env.py:385-441).  The arithmetic is the one of
 * robot_scan / gather_prims (oracle/navsim_ref.c:557-631), which restate env.py:385-435. */
#define NAVSIM_BEAM_NONE     0   /* no return: the clipped range equals range_max (the beams that never receive noise) */
#define NAVSIM_BEAM_WALL     1   /* the static map */
#define NAVSIM_BEAM_PED_BODY 2   /* a side of a pedestrian's footprint rectangle */
#define NAVSIM_BEAM_PED_LEG  3   /* a leg disc of a pedestrian with legs (cfg.lidar_legs) */
typedef struct navsim_scan_labels_out {
    float*   range;   /* [E,B] the robot's scan of the current state without noise: clipped to [0, range_max] */
    uint8_t* label;   /* [E,B] NAVSIM_BEAM_NONE 0 | _WALL 1 | _PED_BODY 2 | _PED_LEG 3 */
    int8_t*  index;   /* [E,B] pedestrian index for labels 2 and 3, else -1 */
    int32_t* hits;    /* [E,N] beams labelled with pedestrian i; entries i >= n are 0; may be NULL */
} navsim_scan_labels_out;

/* ONE launch (a workgroup per arena; kernels_scan_labels.hpp), no device-to-host copy, nothing that blocks, no allocation.  Call
 * it behind the step (and whatever follows it: navsim_regen, navsim_replan) on the same stream.  It reads st->robot_pose, the
 * distance field of the arena's map slot (cfg.shared_field, st->map_slot, st->field_overflow, st->rect_table; both field formats)
 * and, with a pedestrian model, n_peds, ped_pose, ped_dist and ped_has_legs; it writes EVERY element of `out`.  float32 unless
 * stated, every operation rounded on its own (no fused multiply-add: DESIGN.md section 4); B = cfg.n_beams, N = cfg.max_peds.
 * Per arena e:
 *  1. skip && skip[e]: every range 0, every label 0, every index -1, every hits entry 0.  Nothing of the arena is read.
 *  2. n = min(n_peds[e], N), or 0 with NAVSIM_PED_NONE.  The lidar pose (lx, ly, lth) is the float32 cast of robot_pose[e]
 *     (env.py:386); the origin cell (i0, j0) = xy_to_ij_f32(lx, ly) (env.py:419).  Beam k's heading is
 *     (float)(linspace_k(k) + (double)lth), its direction beam_dir(heading): the values the step uses.
 *  3. candidate 0, the static ray: the restatement of range_libc's calc_range that navsim_cast_static runs, on the field of the
 *     arena's map slot, from ((float)i0, (float)j0) along the beam, with cfg.march_rule and max_range = (float)((int64)H*W),
 *     times (float)cfg.resolution (env.py:425-426).
 *  4. candidates 1, 2, ... in gather_prims' order: first, for i = 0 .. n-1 ascending, the four sides v -> (v+1) mod 4 of every
 *     pedestrian that is NOT (ped_has_legs[e,i] and cfg.lidar_legs) -- its corners the float64 rotation and translation of the
 *     human footprint (+-0.22, +-0.19) by ped_pose[e,i], rounded to float32 --; then, for i ascending, the right and then the
 *     left disc of every pedestrian that is: leg_centres on the float32 casts of ped_pose[e,i] and ped_dist[e,i], radius 0.03.
 *  5. r starts as candidate 0's value.  Each further candidate, in order, replaces r iff its seg_merge / circle_merge accepts
 *     (t >= 0 and, for a side, 0 <= u <= 1) and t < r, strictly.  The WINNER is the last candidate that lowered r, candidate 0
 *     if none did -- which is the first candidate in order whose value equals the final r.
 *  6. r is clipped to [0, range_max] (env.py:435): range[e,k] = r.  label = NAVSIM_BEAM_NONE iff r == (float)range_max; else
 *     _WALL, _PED_BODY or _PED_LEG by the winner's kind.  index = the winner's pedestrian for _PED_BODY and _PED_LEG, else -1.
 *  7. hits[e,i] = the number of beams k with index[e,k] == i (0 for i >= n).
 * PROPERTY: with cfg.add_scan_noise == 0, range[e] equals the newest scan slot -- the last B floats ahead of the 7-float tail --
 * of the observation row the step (or navsim_reset_obs) wrote for the same state, bit for bit.  With noise on the two differ
 * by the noise alone, and only where label != NAVSIM_BEAM_NONE.
 * How the kernel meets the sequential rule: its primitives lie in step 4's order; `range` comes from the step's own merge
 * (merge_prims_culled_core: an atomic minimum per beam, in whatever order) after the step's own march (stopped at
 * floor(range_max / resolution) + 4 cells and culled beyond range_max, neither of which changes a clipped range); a second pass
 * then takes, per beam, the least candidate number whose t EQUALS the merged range, candidate 0 first -- the winner of step 5.
 * Equality is by value: candidates of +0.0f and -0.0f on one beam (a lidar origin exactly on two primitives' lines) tie, the
 * earlier one wins as in step 5, and the sign of that zero in `range` is the one the step's merge leaves in the observation.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st or out NULL; out->range, label or index NULL; st->robot_pose or
 * st->field NULL; with a pedestrian model st->n_peds, ped_pose, ped_dist or ped_has_legs NULL; n_envs < 0; n_beams < 1; map_h or
 * map_w < 1; max_peds outside 0 .. NAVSIM_MAX_PEDS (outside 1 .. with a pedestrian model); a march_rule that is none of
 * NAVSIM_MARCH_*; st->map_slot with cfg.shared_field.  NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32 nor
 * NAVSIM_FIELD_U16T; st->rect_table with a float32 field or a map above 1024 cells a side; with a pedestrian model a field of view
 * angle_last - angle_min above 2 pi (the culled merge, as in navsim_step); beams x pedestrians beyond one compute unit's LDS
 * (16 bytes per beam + 120 per pedestrian slot against 160 KB).  n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_scan_labels(const navsim_config* cfg, const navsim_state* st, const uint8_t* skip /* [E] or NULL */,
                       const navsim_scan_labels_out* out, void* stream);

/* ---- action lookahead: what navsim_step would return for each of K candidate actions of an arena, from one launch --------------
 * What a safety shield, an action mask, a one-step Q-target or a "try before you commit" planner asks: if this arena took
 * action a now, what would the step return?  Without this entry the answer costs a copy of the whole state, a step and a
 * restore per candidate.  navsim_dwa does not give it: its disc model differs from the scan-based crash test by a cell or two,
 * its pedestrians move at constant velocity, and it returns one action, not the outcomes of the caller's own.
 * BUILD-DEFINED as an entry; every value is the step's own arithmetic (env.py:591-728 as DESIGN.md section 6 restates it). */
#define NAVSIM_LOOKAHEAD_MAX 64
typedef struct navsim_lookahead_params {
    int32_t n_actions;   /* K, 1 .. NAVSIM_LOOKAHEAD_MAX */
    double  range;       /* R: the scans' cap in metres (rule 5) */
} navsim_lookahead_params;

typedef struct navsim_lookahead_out {
    double*  reward;      /* [E,K] */
    uint8_t* done;        /* [E,K] success | crash | time limit */
    float*   is_success;  /* [E,K] */
    float*   is_crash;    /* [E,K] */
    uint8_t* discomfort;  /* [E,K] */
    double*  distance;    /* [E,K] */
    float*   margin;      /* [E,K] */
    double*  pose;        /* [E,K,3] pose the step would scan from (before any crash revert) */
    uint8_t* status;      /* [E] 0 skipped, 1 evaluated */
} navsim_lookahead_out;

/* ONE launch (a workgroup per arena; kernels_lookahead.hpp), no device-to-host copy, nothing that blocks, no allocation, and it
 * WRITES NOTHING BUT `out`: the state is read-only.  Call it wherever navsim_step could be called on the same stream.
 * actions [E,K,2] is in cfg.action_kind's form.  ped_cmd [E,N,2] stands for st->ped_cmd under NAVSIM_PED_EXTERNAL (NULL: st->ped_cmd
 * itself; ignored with the other models).  float32 / float64 as in the step, every operation rounded on its own; B = cfg.n_beams,
 * N = cfg.max_peds, K = p->n_actions, R = p->range.  Per arena e:
 *  1. skip && skip[e]: status[e] = 0 and every other element of the arena's rows 0.  Nothing of the arena is read.  Else status 1.
 *  2. The pedestrians at t + 1 are what the fused step computes, exactly, under NAVSIM_PED_SFM and NAVSIM_PED_EXTERNAL, for
 *     n = min(n_peds[e], N) pedestrians (0 with NAVSIM_PED_NONE): the waypoint pop (env.py:633-642) from ped_wp_head; the social
 *     force with the robot at robot_pose[e] -- the pose of time t -- moving at prev_action[e][0], or
 *     Human.set_vel on the pedestrian's command; then the leg odometry (env.py:237-255) with ped_prev_yaw.  Only the new pose
 *     and the new ped_dist of a pedestrian are kept.  The new goal at a final waypoint, ped_wp_head, ped_due and everything else
 *     the step stores for a pedestrian change neither this step's poses nor its scan: they are not computed and not written.
 *  3. Candidate k: (a0, a1) = actions[e,k] goes through the step's phase 0 in its order -- under NAVSIM_ACTION_WHEELS
 *     (wheel_radius (l + r) / 2, wheel_radius (r - l) / wheel_track); cfg.clamp_action; cfg.min_turning_radius (env.py:595-600);
 *     KetiRobot.set_vel with cfg.axle_offset from robot_pose[e] (env.py:664).  The result is pose[e,k].  The lidar pose is its
 *     float32 cast (env.py:386), the origin cell xy_to_ij_f32 of that (env.py:419).
 *  4. The candidate's scan is rules 2 - 6 of navsim_scan_labels (range only) with two changes: the pedestrians are those of rule
 *     2 here, seen from the candidate's lidar pose; and R stands for range_max in the march limit (floor(R / resolution) + 4
 *     cells), in the primitive cull and in the clip to [0, R].  There is no noise.
 *  5. R must satisfy max_k scan_discomfort[k] + 0.1 <= R <= range_max.  The thresholds live on the device only, so this entry
 *     checks 0 < R <= range_max (NAVSIM_E_ARG otherwise) and the LOWER bound is the caller's to keep: NavSim.enable_lookahead
 *     refuses an R below it (ValueError) and its default is the smallest multiple of 0.25 m that satisfies it.
 *     Why the cap changes no outcome: a march stopped at floor(R / resolution) + 4 cells and a cull beyond R change no range
 *     clipped to R (the step's argument for range_max, kernels_field.hpp march_limit), so a beam's capped value r' is
 *     min(r, R) of its uncapped value r.  Every threshold lies below R - 0.1, so r' < threshold iff r < threshold: the flags
 *     are the uncapped scan's.  A beam with r' = R has a discomfort ratio (R - thr) / ((dthr - thr) + 1e-6) above 1, its
 *     uncapped ratio is larger still, and a beam below its discomfort threshold has a ratio below 1: whenever the ratio's minimum
 *     is used (discomfort without crash) it is taken on a beam below R, where r' = r.  So the minimum is the uncapped scan's.
 *  6. Outcomes of candidate k, r_k its clipped ranges: is_crash = any r_k < scan_threshold[k]; discomfort = any r_k <
 *     scan_discomfort[k], and not crash; rmin = the minimum of nv::discomfort_ratio over all beams when discomfort (else
 *     unused), as the step's phase 3; (reward, success, crash, distance) = the reference's reward (env.py:464-589) of
 *     (prev_pose[e], pose[e,k], vel = prev_action[e], robot_goal[e], crash, discomfort, rmin) -- its velocity terms use the
 *     PREVIOUS action (env.py:453) and are the same for every candidate; done = success or crash or, with
 *     cfg.max_episode_steps > 0, steps[e] + 1 >= max_episode_steps; margin = min over beams of r_k - scan_threshold[k] in
 *     float32: is_crash holds iff margin < 0.  margin depends on R (a beam clipped to R contributes R - threshold).
 *  7. PROPERTY, with cfg.add_scan_noise == 0 or a noise standard deviation of 0: reward, done, is_success, is_crash and distance
 *     of candidate k equal, bit for bit, what navsim_step with io.action[e] = actions[e,k] writes for arena e from the same
 *     state.  With noise on they are the noise-free outcome.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p, actions or out NULL; any of out's nine arrays NULL; n_actions
 * outside 1 .. NAVSIM_LOOKAHEAD_MAX; R not finite, not positive or above range_max; st->robot_pose, robot_goal, prev_action,
 * prev_pose, steps, field, scan_threshold or scan_discomfort NULL; a ped_model that is none of NAVSIM_PED_*; with a pedestrian
 * model st->n_peds, ped_pose, ped_vel, ped_prev_yaw, ped_dist or ped_has_legs NULL; with NAVSIM_PED_SFM ped_v_pref,
 * ped_waypoints, ped_n_waypoints or ped_wp_head NULL or max_waypoints < 1; with NAVSIM_PED_EXTERNAL both ped_cmd and st->ped_cmd
 * NULL; n_envs < 0; n_beams < 1; map_h or map_w < 1; max_peds outside 0 .. NAVSIM_MAX_PEDS (outside 1 .. with a pedestrian
 * model); a march_rule that is none of NAVSIM_MARCH_*; resolution or time_step not positive and finite; an action_kind that is
 * none of NAVSIM_ACTION_*, NAVSIM_ACTION_WHEELS with a wheel_radius that is not positive; st->map_slot with cfg.shared_field.
 * NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T; st->rect_table with a float32
 * field or a map above 1024 cells a side; with a pedestrian model a field of view angle_last - angle_min above 2 pi (the culled
 * merge, as in navsim_step); LDS beyond one compute unit's 160 KB -- 12 bytes per beam, 56 per candidate and, with a pedestrian
 * model, 144 per pedestrian slot + 32 and 16 (N (N - 1) / 2 + N) for the social force's pair table.
 * n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_lookahead(const navsim_config* cfg, const navsim_state* st, const navsim_lookahead_params* p,
                     const double* actions /* [E,K,2] */, const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */,
                     const uint8_t* skip /* [E] or NULL */, const navsim_lookahead_out* out, void* stream);

/* ---- lookahead observations: the whole return of navsim_step for each of K candidate actions of an arena, from one launch ---------
 * navsim_lookahead answers "what would the step return" for the scalars.  A one-step target r + gamma V(obs'), a full-action
 * backup, a learned value at the leaves of a search or a safety critic on the successor also need obs', the observation, and
 * with scan noise on they need the outcome the step will really compute: its crash and discomfort tests run on the NOISY
 * ranges.  The noise is counter-based -- its key is (seed, global arena, episode, step count, beam) -- so a launch that only
 * reads the state can reproduce the very draw the step is going to make.  Without this entry the answer costs a copy of the
 * whole state, a step and a restore per candidate.
 * BUILD-DEFINED as an entry; every value is the step's own arithmetic (env.py:591-728 as DESIGN.md section 6 restates it). */
#define NAVSIM_LOOKOBS_NOISE_OFF  0   /* no noise: the nine shared outputs are navsim_lookahead's at R = range_max */
#define NAVSIM_LOOKOBS_NOISE_STEP 1   /* the draw navsim_step itself would make (nothing is added unless cfg.add_scan_noise) */
typedef struct navsim_lookahead_obs_params {
    int32_t n_actions;   /* K, 1 .. NAVSIM_LOOKAHEAD_MAX */
    int32_t noise;       /* NAVSIM_LOOKOBS_NOISE_* */
} navsim_lookahead_obs_params;

typedef struct navsim_lookahead_obs_out {
    double*  reward;      /* [E,K] */
    uint8_t* done;        /* [E,K] success | crash | time limit */
    float*   is_success;  /* [E,K] */
    float*   is_crash;    /* [E,K] */
    uint8_t* discomfort;  /* [E,K] */
    double*  distance;    /* [E,K] */
    float*   margin;      /* [E,K] */
    double*  pose;        /* [E,K,3] pose the step would scan from (before any crash revert) */
    uint8_t* status;      /* [E] 0 skipped, 1 evaluated */
    float*   scan;        /* [E,K,B] the newest slot of the row: the candidate's scan, or the re-scan after its crash */
    float*   tail;        /* [E,K,7] the row's tail */
    float*   goals;       /* [E,K,4] achieved_goal (2), desired_goal (2) */
    uint8_t* truncated;   /* [E,K] what io.truncated would hold */
    float*   obs;         /* [E,K,S*B+7] the full row, or NULL: not written */
} navsim_lookahead_obs_out;

/* ONE launch (a workgroup per arena; kernels_lookahead_obs.hpp), no device-to-host copy, nothing that blocks, no allocation, and
 * it WRITES NOTHING BUT `out`: the state is read-only.  actions, ped_cmd and skip as navsim_lookahead's.  obs_prev [E,S*B+7] is the
 * observation the previous step or reset returned (what io.obs_prev of the step would be).  B = cfg.n_beams, S = cfg.n_scan_stack,
 * D = S*B + 7, K = p->n_actions.  Per arena e, what navsim_step under NAVSIM_AUTORESET_NONE would return for each candidate:
 *  1. skip && skip[e]: status[e] = 0 and every other element of the arena's rows 0 (obs included).  Nothing of the arena is
 *     read.  Else status 1.
 *  2. The pedestrians at t + 1: navsim_lookahead's rule 2, once per arena, shared by all candidates and by rule 6's re-scan.
 *  3. Candidate k's pose[e,k], lidar pose and origin cell: navsim_lookahead's rule 3 (the step's phase 0).
 *  4. Scan A of candidate k: navsim_lookahead's rule 4 at R = range_max -- the march limit, the cull and the clip to
 *     [0, range_max] are the step's own.  Then the noise (env.py:437-440): with p->noise == NAVSIM_LOOKOBS_NOISE_STEP,
 *     cfg.add_scan_noise and std = scan_noise_std[e] > 0, a beam b whose clipped range is not range_max becomes
 *     r + std * gauss_noise(noise_stream(seed, env_index_base + e, step_key), b) in float32 (product, then sum), step_key =
 *     episode[e] * 2^32 + (steps[e] + 1) * 2: the key and the draw of the step that would run now.  The noisy value is not
 *     clipped again.  With NAVSIM_LOOKOBS_NOISE_OFF nothing is added.
 *  5. Outcomes of candidate k on those ranges r_k, as the step's phases 3 and 4: is_crash = any r_k < scan_threshold;
 *     discomfort = any r_k < scan_discomfort, and not crash; rmin = the minimum of nv::discomfort_ratio over all beams when
 *     discomfort; (reward, success, crash, distance) = the reference's reward of (prev_pose[e], pose[e,k], vel =
 *     prev_action[e], robot_goal[e], crash, discomfort, rmin); with cfg.max_episode_steps = T > 0, truncated = not (success or
 *     crash) and steps[e] + 1 >= T, else 0; done = success or crash or truncated; margin = min over beams of r_k -
 *     scan_threshold in float32 (navsim_lookahead's rule 6 on these ranges: is_crash holds iff margin < 0).
 *  6. Crash revert (env.py:707-723): a candidate with is_crash takes the re-scan as its scan -- from prev_pose[e] (its float32
 *     cast the lidar pose), the pedestrians of rule 2, clipped as rule 4 and with rule 4's noise under the key step_key + 1.  The
 *     re-scan does not depend on the candidate: it is computed at most once per arena, only if some candidate crashed, and
 *     copied to every crashing candidate.  Its flags are dropped, as the step drops them.  The row pose of such a candidate is
 *     (prev_pose[e][0], prev_pose[e][1], prev_pose[e][2]); of every other candidate pose[e,k].
 *  7. tail[e,k] = float32 of (prev_pose[e][0], prev_pose[e][1], row pose x, row pose y, prev_action[e][0], prev_action[e][1],
 *     wrap_pi(row pose yaw)); goals[e,k] = float32 of (row pose x, row pose y, robot_goal[e][0], robot_goal[e][1]): the step's
 *     phase 6 for a row that is not the first of an episode.
 *  8. obs[e,k] (only if out->obs): slot S - 1 (elements (S-1) B .. S B - 1) is scan[e,k]; slot j < S - 1 is slot j + 1 of
 *     obs_prev[e] where S - 1 - j <= n_hist[e], else scan[e,k] (env.py:257-279, the step's stack fill and shift); the last 7
 *     elements are tail[e,k].
 *  9. PROPERTY with NAVSIM_LOOKOBS_NOISE_STEP, noise on or off: obs / goals, reward, done, truncated, is_success, is_crash and
 *     distance of candidate k equal, bit for bit, what navsim_step under NAVSIM_AUTORESET_NONE with io.action[e] = actions[e,k]
 *     and io.obs_prev = obs_prev writes for arena e from the same state.  Under NAVSIM_AUTORESET_SAME_STEP a candidate with done
 *     set equals io.final_obs / io.final_goals, every other candidate io.obs and the goals.  The first observation of a
 *     restarted episode is not modelled.  With NAVSIM_LOOKOBS_NOISE_OFF the nine shared outputs equal navsim_lookahead's at
 *     R = range_max.  Observations for H > 1 steps: navsim_rollout_obs.
 * NAVSIM_E_ARG, before anything touches the device: everything navsim_lookahead refuses with NAVSIM_E_ARG (there is no R); a
 * noise that is neither constant; out->scan, tail, goals or truncated NULL; n_scan_stack < 1; out->obs with n_scan_stack > 1 and
 * obs_prev or st->n_hist NULL; with NAVSIM_LOOKOBS_NOISE_STEP and cfg.add_scan_noise, st->scan_noise_std or st->episode NULL.
 * NAVSIM_E_UNSUPPORTED: as navsim_lookahead (the LDS is the same: 12 bytes per beam, 56 per candidate, the pedestrians' share).
 * n_envs == 0: NAVSIM_OK, nothing is launched. */
int navsim_lookahead_obs(const navsim_config* cfg, const navsim_state* st, const navsim_lookahead_obs_params* p,
                         const double* actions /* [E,K,2] */, const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */,
                         const float* obs_prev /* [E,S*B+7] or NULL */, const uint8_t* skip /* [E] or NULL */,
                         const navsim_lookahead_obs_out* out, void* stream);

/* ---- action-sequence rollout: what the next H navsim_step calls would return for each of K action sequences of an arena ---------
 * The question behind a sampling-based model-predictive controller (random shooting, MPPI, CEM), an n-step return target or a
 * multi-step shield: if this arena executed the actions a_0 .. a_{H-1}, what would the next H steps return?  Without this entry
 * the answer costs a copy of the whole state, H steps of EVERY arena and a restore per sequence.  navsim_lookahead answers it for
 * one step; navsim_dwa looks ahead with a model of its own (two discs, pedestrians at constant velocity) and returns one action.
 * BUILD-DEFINED as an entry; every value is the step's own arithmetic (env.py:591-728 as DESIGN.md section 6 restates it). */
#define NAVSIM_ROLLOUT_MAX_K 256
#define NAVSIM_ROLLOUT_MAX_H 32
typedef struct navsim_rollout_params {
    int32_t n_seq;       /* K, 1 .. NAVSIM_ROLLOUT_MAX_K */
    int32_t horizon;     /* H, 1 .. NAVSIM_ROLLOUT_MAX_H */
    double  range;       /* R: the scans' cap in metres, as navsim_lookahead's (its rule 5) */
    double  gamma;       /* discount of `ret`, 0 .. 1 */
} navsim_rollout_params;

typedef struct navsim_rollout_out {
    double*  reward;           /* [E,K,H]   the step's reward at step h; 0 behind the sequence's last evaluated step */
    double*  pose;             /* [E,K,H,3] the pose the step scans from at step h (before any crash revert); 0 behind the end */
    double*  ret;              /* [E,K]     g = 1, ret = 0; for h < length: ret = ret + g * reward[h]; g = g * gamma  (no fma) */
    int32_t* length;           /* [E,K]     steps evaluated: index of the first done step + 1, else H */
    uint8_t* outcome;          /* [E,K]     of the last evaluated step: bit 0 success, bit 1 crash, bit 2 time limit (episode_stats' bits) */
    int32_t* discomfort_steps; /* [E,K]     evaluated steps with discomfort and no crash */
    float*   min_margin;       /* [E,K]     min over evaluated steps of the lookahead's margin */
    double*  distance;         /* [E,K]     the step's distance at the last evaluated step */
    int32_t* exact_steps;      /* [E,K]     see rule 8 */
    uint8_t* status;           /* [E]       0 skipped, 1 evaluated */
} navsim_rollout_out;

/* ONE launch (a workgroup per arena and sequence; kernels_rollout.hpp), no device-to-host copy, nothing that blocks, no
 * allocation, and it WRITES NOTHING BUT `out`: the state is read-only.  Call it wherever navsim_step could be called on the same
 * stream.  actions [E,K,H,2] is in cfg.action_kind's form.  ped_cmd [E,N,2] stands for st->ped_cmd under NAVSIM_PED_EXTERNAL
 * (NULL: st->ped_cmd itself; ignored with the other models).  float32 / float64 as in the step, every operation rounded on its
 * own; B = cfg.n_beams, N = cfg.max_peds, K = p->n_seq, H = p->horizon, R = p->range.  Per arena e and sequence k, for
 * h = 0 .. H-1:
 *  1. Step h = 0 is exactly rules 2 - 6 of navsim_lookahead with candidate action actions[e,k,0]: pose[e,k,0] is its pose,
 *     reward[e,k,0] its reward, the step's margin its margin, and so on.
 *  2. The carry.  What the fused step stores for its next call (kernels_step.hpp phase 6 and ped_finish) is carried from step h
 *     to step h + 1: the robot's pose (the pose the step scanned from: a step that is carried over did not crash); prev_pose =
 *     that pose (its xy is all the reward reads); prev_action = the action of step h as the step stores it -- after wheels to
 *     twist, cfg.clamp_action and cfg.min_turning_radius; steps + 1; and per pedestrian its pose, its velocity, ped_prev_yaw =
 *     wrap_pi(new yaw), ped_dist after the leg odometry, and ped_wp_head after the waypoint pop.
 *  3. Steps h >= 1 repeat rules 2 - 6 of navsim_lookahead on the carried values with action actions[e,k,h]: the waypoint pop
 *     starts at the carried head; the social force sees the carried robot pose moving at the carried prev_action[0]; the leg
 *     odometry uses the carried ped_prev_yaw and ped_dist; the reward's velocity terms use the carried prev_action and its
 *     progress term the carried prev_pose; the time limit tests the carried steps + 1 against cfg.max_episode_steps.
 *  4. A sequence ends at its first done step -- success, crash, or the time limit (bit 2 of outcome: set only without success
 *     and crash, as io.truncated).  length[e,k] = that step's index + 1, or H.  Nothing behind it is evaluated: reward and pose
 *     rows h >= length are 0; the crash revert and any restart are not modelled.  ret, discomfort_steps and min_margin run over
 *     the evaluated steps, outcome and distance are the last evaluated step's.  skip && skip[e]: status[e] = 0 and every other
 *     element of the arena's rows 0, nothing of the arena is read; else status 1.
 *  5. No scan noise, as in the lookahead: with noise on the values are the noise-free outcome (navsim_rollout_obs draws each
 *     future step's own noise and returns the observation rows as well).
 *  6. NAVSIM_PED_EXTERNAL: the commands of the call are held for all H steps.  NAVSIM_PED_NONE: no pedestrians.
 *  7. What the rollout leaves out: the real step gives a pedestrian that comes within 0.5 m of its LAST waypoint a new goal and
 *     a new route (env.py:666-680: a draw from the spawn table inside the step, or st->ped_due and the navsim_replan launch).  The
 *     rollout draws nothing and plans nothing: that pedestrian keeps heading for its last waypoint.
 *  8. Exactness.  exact_steps[e,k] is the number of leading steps for which every carried value is what the real step sequence
 *     would hold.  The step raises ped_due for pedestrian i (ped_finish) iff, with (x, y) its pose AFTER this step's move and
 *     (wx, wy) = ped_waypoints[e,i,ped_n_waypoints[e,i] - 1], sqrt((x - wx)^2 + (y - wy)^2) < 0.5 in float64, every operation
 *     rounded on its own.  The rollout evaluates the same predicate on its carried pedestrians under NAVSIM_PED_SFM (with the
 *     other models no waypoint is read and the predicate is never true): exact_steps = H unless it holds for some pedestrian at
 *     an evaluated step h; then exact_steps = h + 1 for the first such h -- the new route takes effect from the next step on.
 * R: rule 5 of navsim_lookahead, unchanged (max_k scan_discomfort[k] + 0.1 <= R <= range_max; this entry checks 0 < R <=
 * range_max, NavSim.enable_rollout the lower bound).  margin depends on R, nothing else does.
 * PROPERTY, with cfg.add_scan_noise == 0 or a noise standard deviation of 0: for every h < min(length, exact_steps),
 * reward[e,k,h] and pose[e,k,h], and -- when the last evaluated step length - 1 is < exact_steps -- outcome and distance, equal
 * bit for bit what H consecutive navsim_step calls with io.action[e] = actions[e,k,h] write for arena e from the same state
 * (pose: st->robot_pose behind a step that did not crash), the re-plan launches running between them as the caller's step path
 * runs them.  With H = 1 every output equals navsim_lookahead's for the same actions, R and state: reward, pose, distance;
 * outcome = is_success | is_crash << 1 | (done and neither) << 2; discomfort_steps = discomfort; min_margin = margin;
 * length = exact_steps = 1; ret = reward.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p, actions or out NULL; any of out's ten arrays NULL; n_seq outside
 * 1 .. NAVSIM_ROLLOUT_MAX_K; horizon outside 1 .. NAVSIM_ROLLOUT_MAX_H; R not finite, not positive or above range_max; gamma
 * outside 0 .. 1 (NaN included); st->robot_pose, robot_goal, prev_action, prev_pose, steps, field, scan_threshold or
 * scan_discomfort NULL; a ped_model that is none of NAVSIM_PED_*; with a pedestrian model st->n_peds, ped_pose, ped_vel,
 * ped_prev_yaw, ped_dist or ped_has_legs NULL; with NAVSIM_PED_SFM ped_v_pref, ped_waypoints, ped_n_waypoints or ped_wp_head
 * NULL or max_waypoints outside 1 .. NAVSIM_MAX_WAYPOINTS; with NAVSIM_PED_EXTERNAL both ped_cmd and st->ped_cmd NULL;
 * n_envs < 0; n_beams < 1; map_h or map_w < 1; max_peds outside 0 .. NAVSIM_MAX_PEDS (outside 1 .. with a pedestrian model); a
 * march_rule that is none of NAVSIM_MARCH_*; resolution or time_step not positive and finite; an action_kind that is none of
 * NAVSIM_ACTION_*, NAVSIM_ACTION_WHEELS with a wheel_radius that is not positive; st->map_slot with cfg.shared_field.
 * NAVSIM_E_UNSUPPORTED: a field_format that is neither NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T; st->rect_table with a float32
 * field or a map above 1024 cells a side; with a pedestrian model a field of view angle_last - angle_min above 2 pi (the culled
 * merge, as in navsim_step); LDS beyond one compute unit's 160 KB -- per workgroup 12 bytes per beam and, with a pedestrian
 * model, 144 per pedestrian slot + 32 and 16 (N (N - 1) / 2 + N) for the social force's pair table (18.8 KB at 1081 beams and 20
 * pedestrians); n_envs x n_seq above 2^31 - 1 workgroups.  n_envs == 0: NAVSIM_OK, nothing is launched.
 * Cost, measured on an MI355X (profiles/r23_rollout/summary.txt; 4096 arenas x 1081 beams, R = 1.75 m, kernel times from a
 * kernel trace): linear in K H -- one sequence-step of the whole batch takes 37.6 - 39.7 us without pedestrians and 76.5 - 79.3 us
 * with twenty an arena, about half of the step kernel's time for one real step of the same arenas (80.6 / 145.8 us); (K, H) =
 * (16, 8) is 5.08 / 10.15 ms, (64, 16) 38.5 / 78.3 ms: x 1.44 - 1.53 resp. x 2.39 - 2.76 of H navsim_lookahead launches at the same K.
 * Out of scope: pedestrians driven by navsim_ped_orca or navsim_ped_policy (their commands come from launches of their own);
 * re-plans inside the horizon (rules 7 and 8); anything behind an episode's end (rule 4).  Noise-aware outcomes and the
 * observations of the H steps: navsim_rollout_obs. */
int navsim_rollout(const navsim_config* cfg, const navsim_state* st, const navsim_rollout_params* p,
                   const double* actions /* [E,K,H,2] */, const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */,
                   const uint8_t* skip /* [E] or NULL */, const navsim_rollout_out* out, void* stream);

/* ---- MPPI local planner: sampled plans, navsim_rollout and the importance-weighted update, all on the device ------------------
 * A sampling-based model-predictive controller on the batch: every arena keeps a plan of H actions, perturbs it K times with
 * time-correlated Gaussian noise, evaluates the K sequences with the step's own arithmetic (navsim_rollout), weights them by
 * exp(-cost / lambda) and takes the weighted mean as its new plan.  BUILD-DEFINED, all of it: the reference has no controller. */
typedef struct navsim_mppi_params {
    int32_t n_samples;       /* K, 1 .. NAVSIM_ROLLOUT_MAX_K */
    int32_t horizon;         /* H, 1 .. NAVSIM_ROLLOUT_MAX_H */
    int32_t iterations;      /* 1 .. 8 */
    int32_t stop_sample;     /* 0 / 1: sequence 1 is the all-zero action (needs 0 inside the box) */
    int32_t select;          /* 0: out->action is the new plan's first action; 1: the best sequence's first action */
    int32_t pad_;
    double  range, gamma;    /* navsim_rollout_params' */
    double  sigma[2];        /* >= 0: standard deviation of the perturbation per action component */
    double  lo[2], hi[2];    /* lo <= hi: the action box, in cfg.action_kind's form */
    double  init_action[2];  /* inside the box: what a fresh plan holds */
    double  beta, alpha;     /* beta in [0, 1): the noise's AR(1) coefficient; alpha = sqrt(1 - beta * beta), computed by the caller */
    double  lambda;          /* > 0: the temperature */
    double  w_goal, w_crash, off_field_cost;   /* >= 0 */
} navsim_mppi_params;

typedef struct navsim_mppi_ws {     /* caller-allocated, persists between calls */
    double*  plan;           /* [E,H,2] */
    int64_t* plan_key;       /* [E,2] (episode, steps) the plan was made for; the caller initialises plan_key[e,0] = -1 */
    double*  actions;        /* [E,K,H,2] the sampled sequences of the last iteration */
    navsim_rollout_out roll; /* all ten arrays: navsim_rollout's outputs for `actions` */
    double*  cost;           /* [E,K] */
} navsim_mppi_ws;

typedef struct navsim_mppi_out {
    double*  action;         /* [E,2] in cfg.action_kind's form: feed it to the next navsim_step */
    int32_t* best;           /* [E]   the best sequence (rule 7) */
    double*  cost_best;      /* [E]   its cost */
    double*  ess;            /* [E]   effective sample size S^2 / Q, 1 .. K */
    uint8_t* status;         /* [E]   0 skipped, NAVSIM_MPPI_OK 1, NAVSIM_MPPI_ALL_CRASH 2 */
} navsim_mppi_out;

#define NAVSIM_MPPI_OK        1
#define NAVSIM_MPPI_ALL_CRASH 2   /* every sequence crashed inside the horizon */

/* 3 x iterations launches (sample, navsim_rollout's own, update; kernels_mppi.hpp), no device-to-host copy, nothing that blocks, no
 * allocation; the state is only read and nothing but `ws` and `out` is written.  Call it wherever navsim_rollout could be called,
 * on the same stream.  `field` (with `gp`, the parameters it was built with) is the goal field the caller's navsim_goal_path
 * built for THIS state: it is only read, its keys are not looked at -- a stale field is the caller's business; NULL: the
 * straight-line distance.  ped_cmd and skip are navsim_rollout's.  Float64, every operation rounded on its own, no fused
 * multiply-add; B, N and the state as in navsim_rollout; genv = cfg.env_index_base + e.  Per arena e:
 *  1. skip && skip[e]: every element of out's row is 0 (status 0); the arena's rows of ws->actions, ws->cost and ws->roll are 0
 *     (ws->roll as navsim_rollout leaves a skipped arena); nothing of the arena is read; ws->plan and ws->plan_key stay untouched.
 *  2. Warm start, once per call.  (ep, s) = (st->episode[e], st->steps[e]).  plan_key[e] == (ep, s): the plan stays.
 *     plan_key[e] == (ep, s - 1): plan[h] = plan[h+1] for h < H-1, plan[H-1] stays.  Otherwise plan[h] = init_action for all h.
 *     Then plan_key[e] = (ep, s).  (A restart, a reset of some arenas, an installed world, a missed step: all show in the two
 *     counters, no host logic decides.)
 *  3. For it = 0 .. iterations-1 do 4 - 8.
 *  4. Sample.  key = ((uint64)ep << 32) + ((uint64)s << 3) + it.  For sequence k: stream_k = nv::hash4(cfg.seed ^ key, genv, key,
 *     0x6D707069 + ((uint64)k << 32));  g(k,h,c) = (double)nv::gauss_noise(stream_k, 2h + c);  eps(k,0,c) = g(k,0,c),
 *     eps(k,h,c) = beta * eps(k,h-1,c) + alpha * g(k,h,c);
 *     actions[e,k,h,c] = min(max(plan[h,c] + sigma[c] * eps(k,h,c), lo[c]), hi[c]).
 *     Two exceptions: k = 0 is the plan itself, min(max(plan[h,c], lo[c]), hi[c]); with stop_sample and K >= 2, k = 1 is
 *     min(max(0, lo[c]), hi[c]) throughout.  The draw depends on (seed, genv, ep, s, it, k, h, c) alone.
 *  5. navsim_rollout's launch on ws->actions into ws->roll, with (K, H, range, gamma), ped_cmd and skip.
 *  6. Cost.  L = length[e,k], crash_k = outcome[e,k] & 2, (x, y) = pose[e,k,L-1,0..1].  Without field: D_k = distance[e,k].
 *     With field: D_k = (double) of the float32 distance that rules 3 - 6 of navsim_goal_path give for a robot standing at
 *     (x, y) on arena e's field with gp's look-ahead and hard clearance; where that rule's status is OFF_FIELD,
 *     D_k = D_k + off_field_cost.  J_k = w_goal * D_k - ret[e,k]; if (crash_k) J_k = J_k + w_crash; cost[e,k] = J_k.
 *  7. jmin = the least J_k, scanning k upward.  best = the least (crash_k != 0, J_k, k) lexicographically: a sequence that did
 *     not crash whenever there is one.  w_k = nv::exp_neg(-((J_k - jmin) / lambda)).  S = 0; for k = 0 .. K-1: S = S + w_k.
 *     Q = 0; Q = Q + w_k * w_k likewise.  For every (h, c): m = 0; for k upward: m = m + w_k * actions[e,k,h,c];
 *     plan[h,c] = min(max(m / S, lo[c]), hi[c]).  (S >= 1: the sequence at jmin has weight exactly 1.)
 *  8. Outputs, of the LAST iteration: action = plan[0] (select 0) or actions[e,best,0] (select 1); cost_best = J_best;
 *     ess = S * S / Q; status = NAVSIM_MPPI_OK, or NAVSIM_MPPI_ALL_CRASH when every sequence crashed.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p, ws or out NULL; any array of ws (its ten rollout arrays
 * included) or of out NULL; n_samples, horizon or iterations outside their ranges; stop_sample or select outside 0 / 1; a sigma
 * that is negative or not finite; lo, hi or init_action not finite, lo > hi, init_action outside the box; stop_sample with 0
 * outside the box; beta outside [0, 1); alpha further than 1e-12 from sqrt(1 - beta^2); lambda not positive and finite; w_goal,
 * w_crash or off_field_cost negative or not finite (NaN fails every one of these); field without gp, field->dist NULL, gp's
 * hard_clearance or lookahead not finite, hard_clearance < 3 resolution, lookahead < 0, map_h / 5 < 1 or map_w / 5 < 1;
 * st->episode NULL.  Everything navsim_rollout refuses for (n_samples, horizon, range, gamma), ws->actions and ws->roll is refused
 * with navsim_rollout's code (its pedestrian models too: navsim_ped_orca / navsim_ped_policy worlds are out of scope for its
 * reason).  n_envs == 0: NAVSIM_OK, nothing is launched.
 * Cost, measured on an MI355X (profiles/r24_mppi/summary.txt; 4096 arenas x 1081 beams, goal field on): the sample kernel 21 - 24 us
 * and the update kernel 49 - 90 us a launch (K = 32 / 64; rule 7's sums are sequential in k by specification), 0.03 - 0.22 % of an
 * iteration beside navsim_rollout's launch: (K, H) = (32, 24) 28.9 ms without pedestrians and 59.2 ms with twenty an arena,
 * (64, 16) 38.6 / 78.6 ms.
 * Out of scope: covariance adaptation (CEM), noise-aware outcomes, pedestrians driven by navsim_ped_orca or navsim_ped_policy. */
int navsim_mppi(const navsim_config* cfg, const navsim_state* st, const navsim_mppi_params* p,
                const navsim_goal_field* field /* or NULL */, const navsim_goal_path_params* gp /* with field */,
                const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */, const uint8_t* skip /* [E] or NULL */,
                const navsim_mppi_ws* ws, const navsim_mppi_out* out, void* stream);

/* ---- pedestrian forecast: where the pedestrians of an arena will be after each of the next H navsim_step calls, one launch ------
 * What a prediction-aware crowd-navigation policy observes (the pedestrians' future trajectories: pred_method 'truth' or
 * 'const_vel' of the CrowdNav++ / intention-aware family), what a trajectory predictor is trained on and compared with (the
 * simulator's own futures; the constant-velocity baseline), and what a risk signal reads (each pedestrian's predicted closest
 * approach).  Without this entry a future costs a copy of the whole state, H steps of every arena and a restore; navsim_rollout
 * carries exactly these pedestrians forward, one copy per sequence, and throws them away -- beside a scan per step that a
 * forecast does not need.  BUILD-DEFINED as an entry; every value under NAVSIM_FORECAST_TRUE is the step's own arithmetic. */
#define NAVSIM_FORECAST_MAX_H 32          /* = NAVSIM_ROLLOUT_MAX_H: a plan of navsim_mppi fits */
#define NAVSIM_FORECAST_HOLD      0       /* robot: the state's prev_action, repeated */
#define NAVSIM_FORECAST_STOP      1       /* robot: the zero twist */
#define NAVSIM_FORECAST_ACTIONS   2       /* robot: `actions` [E,H,2] in cfg.action_kind's form */
#define NAVSIM_FORECAST_TRUE      0       /* model: the configured pedestrian model (social force, or external commands held) */
#define NAVSIM_FORECAST_CONST_VEL 1       /* model: every pedestrian keeps its velocity */
typedef struct navsim_ped_forecast_params {
    int32_t horizon;     /* H, 1 .. NAVSIM_FORECAST_MAX_H */
    int32_t robot;       /* NAVSIM_FORECAST_HOLD / STOP / ACTIONS: what the robot is assumed to do over the horizon */
    int32_t model;       /* NAVSIM_FORECAST_TRUE / CONST_VEL */
    int32_t pad_;
} navsim_ped_forecast_params;

typedef struct navsim_ped_forecast_out {    /* time-major: at step h the N slots of an arena are N adjacent rows */
    double*  pose;         /* [E,H,N,3] pedestrian i after forecast step h */
    double*  vel;          /* [E,H,N,2] its velocity */
    float*   rel;          /* [E,H,N,2] its position in the robot's CURRENT frame (the pose at time t): rule 6 */
    double*  robot_pose;   /* [E,H,3]   the robot pose assumed after step h */
    double*  min_dist;     /* [E,N]     least centre distance between robot_pose[h] and pose[h,i] over the horizon; +inf for an unused slot */
    int32_t* min_step;     /* [E,N]     the first h that attains min_dist; -1 for an unused slot */
    int32_t* exact_steps;  /* [E]       see rule 5 */
    uint8_t* status;       /* [E]       0 skipped, 1 forecast */
} navsim_ped_forecast_out;

/* ONE launch (a wavefront per arena, a lane per pedestrian, the horizon loop inside; kernels_ped_forecast.hpp), no device-to-host
 * copy, nothing that blocks, no allocation, and it WRITES NOTHING BUT `out`: the state is read-only.  Call it wherever navsim_step
 * could be called on the same stream.  actions [E,H,2] is in cfg.action_kind's form (read under NAVSIM_FORECAST_ACTIONS only).
 * ped_cmd [E,N,2] stands for st->ped_cmd under NAVSIM_PED_EXTERNAL with NAVSIM_FORECAST_TRUE (NULL: st->ped_cmd itself; ignored
 * otherwise).  Float64, every operation rounded on its own, no fused multiply-add; N = cfg.max_peds, H = p->horizon,
 * n = min(n_peds[e], N), dt = cfg.time_step.  Per arena e:
 *  1. skip && skip[e]: status[e] = 0 and EVERY other element of the arena's rows is 0 (min_dist and min_step too).  Nothing of
 *     the arena is read.  Else status 1.
 *  2. The robot, for h = 0 .. H-1, from p = robot_pose[e] and prev_v = prev_action[e][0]: the action (a0, a1) of step h is
 *     prev_action[e] (HOLD), (0, 0) (STOP) or actions[e,h] (ACTIONS).  It goes through the step's phase 0, operation for
 *     operation as navsim_rollout's rule 3 (navsim_lookahead's rule 3): under ACTIONS with NAVSIM_ACTION_WHEELS
 *     (wheel_radius (l + r) / 2, wheel_radius (r - l) / wheel_track) -- HOLD and STOP are twists already and skip only this
 *     conversion --; cfg.clamp_action; cfg.min_turning_radius (env.py:595-600); KetiRobot.set_vel with cfg.axle_offset from p
 *     (env.py:664).  The result is robot_pose[e,h] and the next p; prev_v = a0 as the step would store it (after clamp and
 *     turning radius).  The robot's crash, its crash revert, the episode's end and a restart are NOT modelled.
 *     Clamp and turning radius are idempotent on a prev_action the step stored, so HOLD equals ACTIONS with that twist under
 *     NAVSIM_ACTION_TWIST: a clamped value lies inside its interval and stays; with lim = |a1| min_turning_radius computed from
 *     the same a1, the stored a0 satisfies a0 >= lim (a0 >= 0) or a0 <= -lim (a0 < 0), so the rule selects a0 again or a lim
 *     equal to it; and where the radius rule pushed a0 out of [linvel_lo, linvel_hi], a0 IS lim: the clamp pulls it in and the
 *     radius rule returns the same lim.
 *  3. NAVSIM_FORECAST_TRUE, step h, for the n pedestrians, over the step's own functions (kernels_step.hpp):
 *       1. pop waypoints from the carried head (ped_pop_waypoints; NAVSIM_PED_SFM);
 *       2. stage the agents of time t + h: the carried pedestrians, and the robot at its carried pose p with speed prev_v along
 *          its heading -- (p.x, p.y, prev_v cos p.th, prev_v sin p.th), exactly as ped_stage_wave does;
 *       3. compute the pair terms (ped_pair_term);
 *       4. ped_sfm_step towards the waypoint at the head, or under NAVSIM_PED_EXTERNAL nv::set_vel on the pedestrian's command
 *          of the call, held for the whole horizon (navsim_rollout's rule 6);
 *       5. the robot moves by rule 2 on this step's action.
 *     Carried per pedestrian: pose, velocity, waypoint head; for the robot: pose and prev_action as the step would store it.
 *     pose[e,h,i] / vel[e,h,i] are the pedestrian's after step 4.  Leg odometry, ped_prev_yaw and the scan are not needed and
 *     not computed; nothing is drawn and nothing is planned.
 *  4. NAVSIM_FORECAST_CONST_VEL: with (x, y, yaw) = ped_pose[e,i] and (vx, vy) = ped_vel[e,i],
 *     pose[e,h,i] = (x + vx * ((double)(h + 1) * dt), y + vy * ((double)(h + 1) * dt), yaw), vel[e,h,i] = (vx, vy).  It reads
 *     only ped_pose / ped_vel and is valid with every pedestrian model.  The robot still moves by rule 2, and rules 6 and 7
 *     use that pose.  exact_steps = 0.
 *  5. Exactness (navsim_rollout's rule 8).  exact_steps[e] is the number of leading steps that are the step's own.  The step
 *     raises ped_due for pedestrian i (ped_finish) iff, with (x, y) its pose AFTER this step's move and (wx, wy) =
 *     ped_waypoints[e,i,ped_n_waypoints[e,i] - 1], sqrt((x - wx)^2 + (y - wy)^2) < 0.5 in float64, every operation rounded on
 *     its own: the real step then gives the pedestrian a new goal and a new route (env.py:666-680).  Under NAVSIM_PED_SFM
 *     exact_steps = H unless the predicate holds for some pedestrian at a step h; then exact_steps = h + 1 for the first such
 *     h -- the new route takes effect from the next step on -- and the forecast GOES ON without the re-plan: that pedestrian
 *     keeps heading for its last waypoint, and all H rows are filled.  Always H under NAVSIM_PED_EXTERNAL.
 *  6. rel[e,h,i], navsim_ped_observe's frame convention (its rule 3) with the robot pose of time t, (rx, ry, th) =
 *     robot_pose[e] of the state: c = nv::cos(th), s = nv::sin(th); ax = pose[e,h,i].x - rx, ay = pose[e,h,i].y - ry;
 *     rel = ((float)(c*ax + s*ay), (float)(c*ay - s*ax)): float64 in this order, rounded once.
 *  7. d_h = sqrt(dx*dx + dy*dy) with dx = pose[e,h,i].x - robot_pose[e,h].x, dy likewise.  min_dist[e,i] = the least d_h,
 *     min_step[e,i] = the first h that attains it (d_h < the minimum so far, starting from +inf).
 *  8. Slots i >= n: every row 0, min_dist = +inf, min_step = -1.
 * PROPERTY: under NAVSIM_FORECAST_TRUE with NAVSIM_FORECAST_ACTIONS, for every h below both exact_steps[e] and the first step
 * at which the arena's episode ends, pose[e,h,:n], vel[e,h,:n] and robot_pose[e,h] equal bit for bit st->ped_pose, st->ped_vel
 * and st->robot_pose after h + 1 consecutive navsim_step calls with io.action[e] = actions[e,h] from the same state, the
 * re-plan launches running between them as the caller's step path runs them.  Scan noise plays no part.  The rows of a
 * horizon H are the leading rows of every longer horizon.
 * NAVSIM_E_ARG, before anything touches the device: cfg, st, p or out NULL; any of out's eight arrays NULL; horizon outside
 * 1 .. NAVSIM_FORECAST_MAX_H; a robot that is none of HOLD / STOP / ACTIONS, a model that is none of TRUE / CONST_VEL;
 * NAVSIM_FORECAST_ACTIONS without actions; cfg.ped_model == NAVSIM_PED_NONE or none of NAVSIM_PED_*; max_peds outside
 * 1 .. NAVSIM_MAX_PEDS; st->robot_pose, prev_action, n_peds, ped_pose or ped_vel NULL; under NAVSIM_FORECAST_TRUE with
 * NAVSIM_PED_SFM st->field, ped_v_pref, ped_waypoints, ped_n_waypoints or ped_wp_head NULL or max_waypoints outside
 * 1 .. NAVSIM_MAX_WAYPOINTS, with NAVSIM_PED_EXTERNAL both ped_cmd and st->ped_cmd NULL; n_envs < 0; map_h or map_w < 1;
 * resolution or time_step not positive and finite; an action_kind that is none of NAVSIM_ACTION_*, NAVSIM_ACTION_WHEELS with a
 * wheel_radius that is not positive; st->map_slot with cfg.shared_field.  NAVSIM_E_UNSUPPORTED: a field_format that is neither
 * NAVSIM_FIELD_F32 nor NAVSIM_FIELD_U16T; st->rect_table with a float32 field or a map above 1024 cells a side (the field-format
 * cases navsim_rollout refuses).  n_envs == 0: NAVSIM_OK, nothing is launched.
 * Cost, measured on an MI355X (profiles/r25_ped_forecast/summary.txt; 4096 arenas x 20 pedestrians, kernel times from a kernel
 * trace, the step kernel at 145.4 us in the same trace): linear in H -- 25.4 - 26.6 us a forecast step under NAVSIM_FORECAST_TRUE
 * (H = 8 / 16 / 32: 213 / 419 / 814 us), 2.4 - 3.0 us under NAVSIM_FORECAST_CONST_VEL (23.8 / 41.0 / 75.7 us).
 * Out of scope: pedestrians driven by navsim_ped_orca or navsim_ped_policy under NAVSIM_FORECAST_TRUE (their commands come
 * from launches of their own: the caller passes the commands it wants held, or asks for NAVSIM_FORECAST_CONST_VEL); re-plans
 * inside the horizon (rule 5); the robot's crash and anything behind an episode's end (rule 2). */
int navsim_ped_forecast(const navsim_config* cfg, const navsim_state* st, const navsim_ped_forecast_params* p,
                        const double* actions /* [E,H,2] or NULL */, const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */,
                        const uint8_t* skip /* [E] or NULL */, const navsim_ped_forecast_out* out, void* stream);

/* ---- rollout observations: the whole return of the next H navsim_step calls for each of K action sequences of an arena -----------
 * navsim_rollout carries an arena through H steps and returns scalars, under a short cap and without scan noise;
 * navsim_lookahead_obs returns everything the step returns, with the step's own noise draw, for one step.  This entry does both:
 * the observation row, the goals, the reward and the outcome of every step of every sequence, with the noise the h-th future
 * step will draw -- the obs of an n-step or model-value-expansion target sum gamma^h r_h + gamma^H V(obs_H), of a learned value
 * at the leaves of a depth-H search, of terminal-value MPC, of multi-step model-based augmentation with the simulator as the
 * model.  Without it each costs a copy of the whole state, H steps of EVERY arena and a restore per sequence.
 * BUILD-DEFINED as an entry; every value is the step's own arithmetic (env.py:591-728 as DESIGN.md section 6 restates it). */
typedef struct navsim_rollout_obs_params {
    int32_t n_seq;       /* K, 1 .. NAVSIM_ROLLOUT_MAX_K */
    int32_t horizon;     /* H, 1 .. NAVSIM_ROLLOUT_MAX_H */
    int32_t noise;       /* NAVSIM_LOOKOBS_NOISE_OFF / NAVSIM_LOOKOBS_NOISE_STEP */
    double  gamma;       /* discount of `ret`, 0 .. 1 */
} navsim_rollout_obs_params;

typedef struct navsim_rollout_obs_out {
    /* navsim_rollout_out's ten arrays, same shapes and meanings (min_margin: the lookahead observations' margin, i.e. on the
       noisy full-range ranges) */
    double*  reward;           /* [E,K,H] */
    double*  pose;             /* [E,K,H,3] */
    double*  ret;              /* [E,K] */
    int32_t* length;           /* [E,K] */
    uint8_t* outcome;          /* [E,K] */
    int32_t* discomfort_steps; /* [E,K] */
    float*   min_margin;       /* [E,K] */
    double*  distance;         /* [E,K] */
    int32_t* exact_steps;      /* [E,K] */
    uint8_t* status;           /* [E] */
    float*   obs_last;         /* [E,K,S*B+7]   the row of the sequence's last evaluated step */
    float*   goals_last;       /* [E,K,4]       achieved_goal (2), desired_goal (2) of that step */
    float*   obs_all;          /* [E,K,H,S*B+7] the row of every step, or NULL: not written */
    float*   goals_all;        /* [E,K,H,4]     or NULL (both or neither) */
} navsim_rollout_obs_out;

/* ONE launch (a workgroup per arena and sequence; kernels_rollout_obs.hpp), no device-to-host copy, nothing that blocks, no
 * allocation, and it WRITES NOTHING BUT `out`: the state is read-only.  actions, ped_cmd and skip as navsim_rollout's, obs_prev
 * as navsim_lookahead_obs's.  B = cfg.n_beams, S = cfg.n_scan_stack, D = S*B + 7, K = p->n_seq, H = p->horizon.  Per arena e and
 * sequence k, for h = 0 .. H-1:
 *  1. Carry, end, external commands, what is left out, exactness and skip are navsim_rollout's rules 2, 3, 4, 6, 7 and 8
 *     unchanged: a sequence ends at its first done step; length, outcome, exact_steps, ret, discomfort_steps, distance and
 *     status keep their definitions.  Rows h >= length are 0, in obs_all and goals_all too; a skipped arena's rows are all 0,
 *     obs_last and goals_last included.
 *  2. Scan of step h: navsim_lookahead_obs's rule 4 from the carried state -- the march limit, the cull and the clip of
 *     range_max -- with the noise key step_key_h = episode[e] * 2^32 + (steps[e] + 1 + h) * 2, the draw the h-th future step
 *     will make.  Crash, discomfort, ratio, reward, time limit and margin come from those ranges: navsim_lookahead_obs's rule 5
 *     with the carried prev_pose, prev_action and steps.  min_margin is the minimum of that margin over the evaluated steps.
 *  3. A step h that crashes ends the sequence, and its row takes the reference's re-scan (navsim_lookahead_obs's rule 6): from
 *     the carried prev_pose -- for h = 0 prev_pose[e], for h >= 1 (pose[e,k,h-1] x, y, wrap_pi of its yaw), what the step's
 *     phase 6 stores -- with the sequence's OWN pedestrians at t + h + 1 and the key step_key_h + 1.  It is computed per
 *     sequence: sequences share no pedestrians beyond h = 0.  The row pose of that step is the carried prev_pose;
 *     pose[e,k,h] stays the pose the step scanned from, as in navsim_rollout.
 *  4. Row h [D]: the newest slot S - 1 is the scan of rule 2 or 3; slot j < S - 1 is slot j + 1 of the previous row where
 *     S - 1 - j <= n_hist_h, else the newest scan.  The previous row is the sequence's own row h - 1, obs_prev[e] for h = 0.
 *     n_hist_0 = st->n_hist[e], n_hist_{h+1} = min(n_hist_h + 1, S - 1) (the step's phase 6).  Tail and goals are
 *     navsim_lookahead_obs's rule 7 on the carried values: the carried prev_pose xy, the row pose xy, the carried prev_action,
 *     wrap_pi(row pose yaw); goals = (row pose xy, robot_goal[e]).  obs_last / goals_last are row length - 1; obs_all /
 *     goals_all, when given, hold every row.
 *  5. PROPERTY with NAVSIM_LOOKOBS_NOISE_STEP, noise on or off: for every h < min(length, exact_steps), reward, pose, row h and
 *     goals h equal, bit for bit, what the h-th of H consecutive navsim_step calls under NAVSIM_AUTORESET_NONE writes for arena
 *     e from the same state, with io.action[e] = actions[e,k,h] and io.obs_prev the previous call's io.obs (obs_prev for the
 *     first); outcome, distance, obs_last and goals_last do too when length - 1 < exact_steps.  Under
 *     NAVSIM_AUTORESET_SAME_STEP a done row equals io.final_obs / io.final_goals.  With NAVSIM_LOOKOBS_NOISE_OFF the ten shared
 *     outputs equal navsim_rollout's at R = range_max.  With H = 1, under either noise setting, every output equals
 *     navsim_lookahead_obs's: obs_last its obs, goals_last its goals, the scalars as navsim_rollout's PROPERTY maps them.
 * NAVSIM_E_ARG, before anything touches the device: everything navsim_rollout refuses with NAVSIM_E_ARG (there is no R); a
 * noise that is neither constant; out->obs_last or goals_last NULL; exactly one of out->obs_all / goals_all NULL;
 * n_scan_stack < 1; n_scan_stack > 1 with obs_prev or st->n_hist NULL; with NAVSIM_LOOKOBS_NOISE_STEP and cfg.add_scan_noise,
 * st->scan_noise_std or st->episode NULL.  NAVSIM_E_UNSUPPORTED: as navsim_rollout, the dynamic LDS being the same (12 bytes per
 * beam and the pedestrians' share: the older scans of a row are read back from the rows the same threads stored, not kept in
 * LDS); 1.6 KB of static LDS.  n_envs == 0: NAVSIM_OK, nothing is launched.
 * Cost: profiles/r27_rollout_obs/summary.txt (README, "Rollout observations").
 * Out of scope: pedestrians driven by navsim_ped_orca or navsim_ped_policy; re-plans inside the horizon; the first observation
 * of a restarted episode; using this launch inside navsim_mppi. */
int navsim_rollout_obs(const navsim_config* cfg, const navsim_state* st, const navsim_rollout_obs_params* p,
                       const double* actions /* [E,K,H,2] */, const double* ped_cmd /* [E,N,2] or NULL: st->ped_cmd */,
                       const float* obs_prev /* [E,S*B+7] or NULL */, const uint8_t* skip /* [E] or NULL */,
                       const navsim_rollout_obs_out* out, void* stream);

/* Name of the fused step kernel as rocprofv3 reports it (bench.py / profiles). */
const char* navsim_step_kernel_name(void);

/* ---- test hooks (used by tests/ only) ---------------------------------------------------- */
size_t navsim_sizeof_config(void);
size_t navsim_sizeof_state(void);
size_t navsim_sizeof_step_io(void);
/* deterministic device math of DESIGN.md section 4: fn 0 sin, 1 cos, 2 atan2(x, x2), 3 exp(x<=0),
 * 4 angle_correction (utils.py:5-9), 5 python-float % 2pi, 6 the packed field's sqrtf on integers, 11 / 12 the
 * march step of sqrtf(x) under NAVSIM_MARCH_F64 in its float64 form / in its float32-only form (7-10: diagnostics), 13 the
 * beam-table direction against the full evaluation, 14 the social-force pair term's antisymmetry (0 = f(i,j) == -f(j,i) bitwise),
 * 17 the scan noise's Gaussian of beam i of the stream whose low / high 32-bit words are x[i] / x2[i].
 * x, x2, out are device float64 [n]. */
int navsim_debug_math(int32_t fn, const double* x, const double* x2, double* out, int32_t n, void* stream);
/* batch_xy_to_ij (env.py:1228-1253) exactly as the scan evaluates it: xy [n,2] float64 in, ij [n,2] int32 out;
 * as_f32 = 1 rounds the inputs to float32 first and divides in float32 (the lidar origin, env.py:386, 419). */
int navsim_debug_xy_to_ij(const navsim_config* cfg, const double* xy, int32_t as_f32, int32_t* ij, int32_t n, void* stream);
/* navsim_goal_path's rebuilds, from now on and on this thread, record the relaxation sweeps each took: sweeps [E] device int32,
 * entry e written when arena e's field is rebuilt; NULL (the default) turns the record off.  The library keeps the POINTER: the
 * array must stay allocated (and hold the cfg.n_envs of every later call) until the hook is set to NULL again -- set it to NULL
 * before freeing the array.  Always NAVSIM_OK. */
int navsim_debug_goal_path_sweeps(int32_t* sweeps);

/* The spawn loops' acceptance rules (env.py:366-383, 748-762, 786-793) on SUPPLIED candidates -- the very device
 * functions navsim_regen's samplers call -- so that tests can compare them with the decisions the reference's own
 * _sample_start_goal_path / reset() took on the same candidates (tests/golden/golden_reset.npz).
 * cost [Hc,Wc] uint8 costmap (nonzero = blocked); kind [n]: 0 = the robot's pair, 1 = a pedestrian's; start, goal
 * [n,2] metres; robot [n,2] the robot's xy for kind 1 (may be NULL); wp_scratch [n, cfg.max_waypoints, 2].
 * code [n]: 0 kept, 1 start closer than cfg.ped_min_robot_dist to the robot, 2 goal distance outside its interval
 * (robot: cfg.min_goal_dist < d < cfg.max_goal_dist; pedestrian: d > cfg.ped_min_goal_dist), 3 no path, 4 (robot)
 * path_distance > 2 |goal - start|. */
int navsim_debug_spawn_decisions(const navsim_config* cfg, const uint8_t* cost, int32_t Hc, int32_t Wc, int32_t n,
                                 const int32_t* kind, const double* start, const double* goal, const double* robot,
                                 double* wp_scratch, int32_t* code, void* stream);

/* ---- measurement hooks (used by profiles/ only; nothing of the hot path calls them) ---------- */
/* Scattered-read microbenchmark behind DESIGN.md section 6's "a scattered 4-byte read costs a 128-byte fill"
 * (profiles/gather_granularity.py): n_threads lanes each read `iters` pseudo-random words of x[n_words];
 * mode selects the access width / stride pattern; out[n_threads] keeps the loads alive. */
int navsim_debug_gather(const float* x, uint64_t n_words, int32_t mode, int32_t iters, int32_t n_threads,
                        float* out, void* stream);
/* Phase time stamps of the fused step (profiles/_r01_tools/stamp_phases.py, profiles/_diag/tail_profile.py):
 * device buffer of 8 x n_envs uint64 receiving s_memtime / s_memrealtime at the phase boundaries of every arena's
 * workgroup; NULL disables.  Only a library built with -DNAVSIM_STAMPS records anything; the shipped build
 * compiles no stamp into the kernel and returns NAVSIM_E_UNSUPPORTED. */
int navsim_debug_set_stamps(unsigned long long* buf);
/* Self-test of the way the step kernels read their arguments (round 6: kernels_step.hpp NAVSIM_KERNARGS -- references into the
 * kernarg segment laid out as a struct of the kernel's leading parameters, instead of the by-value copies): one launch whose
 * parameters carry byte patterns compares every byte of the views with the copies.  NAVSIM_OK when they agree;
 * NAVSIM_E_UNSUPPORTED when a toolchain lays kernel arguments out differently (build with -DNAVSIM_KARG_VIEW=0 then). */
int navsim_debug_kernarg_layout(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NAVSIM_H */
