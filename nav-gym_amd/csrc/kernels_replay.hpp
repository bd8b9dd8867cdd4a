// kernels_replay.hpp -- the pieces of navsim_step that the read-only kernels re-enact, each stated ONCE: lookahead_kernel,
// lookahead_obs_kernel, rollout_kernel, rollout_obs_kernel and (twist and carried pedestrian only) ped_forecast_kernel call them.
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace, in front of
// kernels_lookahead.hpp; NOT part of navsim_step_inst.hip: the step keeps its own copies in kernels_step.hpp).
//
// Every piece is held to the step bit for bit (-ffp-contract=off; the order of the float32 / float64 operations is the contract),
// so a change of the step's side is made here and nowhere else in those kernels:
//   replay_twist      the step's phase 0 on an action (kernels_step.hpp, "phase 0": wheels to twist, clamp_action,
//                     min_turning_radius; env.py:595-600) -- navsim_lookahead's rule 3, navsim_rollout's rule 3
//   ScanPose          scan_pose_step: KetiRobot.set_vel through nv::set_vel_with on the four sincos values (env.py:664), then
//                     scan_pose_set: the float32 lidar pose (env.py:386), its sincos for the beam table, the integer origin cell
//                     (env.py:419) -- the step's phase 0 / phase 2 head; the crash re-scans use scan_pose_set alone
//   replay_prims      the pedestrians' lidar primitives in the ORACLE's order (env.py:392-414, gather_prims: the sides of the
//                     pedestrians without legs by ascending pedestrian, then the leg discs) -- navsim_scan_labels' rule 4.
//                     scan_labels_kernel keeps its own copy, which also records owners: with this function two of its eleven
//                     forms need 102 scalar registers for 99 and lose their eighth wave (profiles/r28_replay)
//   replay_march      the static ray of every beam, 64 adjacent beams at a time handed out by an LDS counter: probe_round /
//                     ray_result, scan_labels_kernel's march (navsim_lookahead's rule 4); replay_merge: the step's
//                     merge_prims_culled_core behind it; replay_scan: cull, march and merge of a whole workgroup
//   replay_verdict    crash / discomfort over the beams, the margin, the discomfort ratio's minimum when the step would compute it
//                     (env.py:563-569, the step's phase 3) -- navsim_lookahead's rule 6
//   replay_reward     nv::reward_scalar and the time limit (the step's phase 4)
//   CarriedPed        what a pedestrian carries from step to step (ped_finish's stores), loaded from the state
//   replay_lds_bytes / replay_lds_carve   the dynamic LDS of one workgroup
// The march and the verdict take a POINTER to their LDS counter / vote word and never arm it: the lookahead pair arms all K of
// them in its part A, the rollout pair re-arms one on thread 64 every step.

__host__ __device__ inline size_t lookahead_align16(size_t n) { return (n + 15) & ~(size_t)15; }

__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = (o < v) ? o : v;
    }
    return v;
}

// a value that is the same on every lane, moved to scalar registers
__device__ __forceinline__ float uniform_f32(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// ---- dynamic LDS of one workgroup: per beam dir (8 B) and rng (4 B); `own` bytes of the kernel's own (the lookahead's 56 B per
// candidate; the rollout has none); with a pedestrian model PedShared (144 B per pedestrian slot + 32: the agents at time t, the
// primitives, their beam intervals) and the social force's pair table (16 B x (N (N - 1) / 2 + N)).  1081 beams, 20 pedestrians,
// K = 9 candidates: 12.7 + 0.5 + 2.9 + 3.4 KB.
inline size_t replay_lds_bytes(const navsim_config* c, size_t own) {
    size_t n = lookahead_align16((size_t)c->n_beams * (sizeof(float2) + sizeof(float))) + lookahead_align16(own);
    if (c->ped_model != NAVSIM_PED_NONE) n += lookahead_align16(ped_lds_bytes(c->max_peds)) + ped_pair_bytes(c->max_peds);
    return n;
}
struct ReplayLds {
    float2* dir;             // [B] beam directions of the scan in flight
    float* rng;              // [B] its ranges
    char* own;               // the kernel's own bytes
    PedShared ps;            // with a pedestrian model
    double2* pair;
    Prims pr;                // ps's primitives
};
__device__ __forceinline__ ReplayLds replay_lds_carve(char* dyn, const navsim_config& c, size_t own) {
    const int N = c.max_peds, B = c.n_beams;
    ReplayLds l = {};
    l.dir = (float2*)dyn;
    l.rng = (float*)(dyn + sizeof(float2) * (size_t)B);
    l.own = dyn + lookahead_align16((size_t)B * (sizeof(float2) + sizeof(float)));
    char* behind = l.own + lookahead_align16(own);
    if (c.ped_model != NAVSIM_PED_NONE) {
        l.ps = ped_lds_carve(behind, N);
        l.pair = (double2*)(behind + lookahead_align16(ped_lds_bytes(N)));
    }
    l.pr = {l.ps.seg, l.ps.disc, l.ps.info};
    return l;
}

// ---- the step's phase 0 on an action.  raw: as the caller hands it in (wheel speeds under NAVSIM_ACTION_WHEELS); otherwise a
// twist already.  Out: the twist as the step stores it in prev_action.
__device__ __forceinline__ void replay_twist(const navsim_config& c, bool raw, double& a0, double& a1) {
    if (raw && c.action_kind == NAVSIM_ACTION_WHEELS) {
        const double wl = a0, wr = a1;
        a0 = c.wheel_radius * (wl + wr) * 0.5;
        a1 = c.wheel_radius * (wr - wl) / c.wheel_track;
    }
    if (c.clamp_action) {
        a0 = a0 < c.linvel_lo ? c.linvel_lo : (a0 > c.linvel_hi ? c.linvel_hi : a0);
        a1 = a1 < c.rotvel_lo ? c.rotvel_lo : (a1 > c.rotvel_hi ? c.rotvel_hi : a1);
    }
    if (c.min_turning_radius > 0.0) {                                                // env.py:595-600
        const double lim = fabs(a1) * c.min_turning_radius;
        if (a0 >= 0.0) a0 = (a0 > lim) ? a0 : lim;
        else           a0 = (a0 < -lim) ? a0 : -lim;
    }
}

// ---- the pose a scan starts from.  A lane that computes one for the others fills a ScanPose of its own and stores it whole:
// what it needs again (the pose for its output row) then comes from registers, not back from LDS
struct ScanPose {
    double p[3];             // the robot's pose
    double cT, sT;           // cos / sin of (double)(float)p[2] for the beam-table fast path
    int i0, j0;              // integer ray origin (env.py:419)
};
__device__ __forceinline__ void scan_pose_set(ScanPose& sp, const navsim_config& c, double x, double y, double th) {
    sp.p[0] = x; sp.p[1] = y; sp.p[2] = th;
    const float lth = (float)th;                                                     // env.py:386
    double sT, cT;
    nv::sincos((double)lth, sT, cT);
    sp.cT = cT; sp.sT = sT;
    int i0, j0;
    nv::xy_to_ij_f32((float)x, (float)y, c, i0, j0);                                 // env.py:419
    sp.i0 = i0; sp.j0 = j0;
}
// from the pose rp of time t and the twist of replay_twist: the pose the step scans from
__device__ __forceinline__ void scan_pose_step(ScanPose& sp, const navsim_config& c, const double* rp, double a0, double a1) {
    const double dt = c.time_step;
    const double th_old = rp[2];
    const double th = th_old + a1 * dt;                                              // set_vel's intermediate heading
    double s0, c0, s1, c1;
    nv::sincos(th_old, s0, c0);
    nv::sincos(th, s1, c1);
    double p[3] = {rp[0], rp[1], th_old};                                            // env.py:664
    nv::set_vel_with(p, a0, a1, dt, c.axle_offset, s0, c0, s1, c1, nullptr);
    scan_pose_set(sp, c, p[0], p[1], p[2]);
}

// ---- the pedestrians' lidar primitives, on the lanes of wavefront 0 (pedestrian i on lane tid = i; every lane calls).  pp: the
// pedestrian's pose, dist: its leg odometry (read only where legged).  Returns the arena's counts and this lane's first slot --
// in disc[] where legged, in seg[] otherwise.
struct PrimSlot { int nseg, ndisc, first; };
__device__ __forceinline__ PrimSlot replay_prims(int n, int tid, bool is_ped, bool legged, const double* pp, const double* dist,
                                                 float (*seg)[4], float (*disc)[2]) {
    const lanemask_t lm = mask_of(legged);
    const int legs_all = __popcll(lm), legs_below = __popcll(lm & ((1ull << tid) - 1ull));
    const PrimSlot r = {4 * (n - legs_all), 2 * legs_all, legged ? 2 * legs_below : 4 * (tid - legs_below)};
    if (is_ped) {                                                                    // env.py:392-414
        const int q = r.first;
        if (legged) {
            float cc[4];
            nv::leg_centres((float)pp[0], (float)pp[1], (float)pp[2], (float)dist[0], (float)dist[1], (float)dist[2], cc);
            disc[q][0] = cc[0]; disc[q][1] = cc[1];
            disc[q + 1][0] = cc[2]; disc[q + 1][1] = cc[3];
        } else {
            const double fpx[4] = {0.22, -0.22, -0.22, 0.22};   // human.py:5-10
            const double fpy[4] = {0.19, 0.19, -0.19, -0.19};
            double s, cs;
            nv::sincos(pp[2], s, cs);
            float vx[4], vy[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                vx[v] = (float)((cs * fpx[v] - s * fpy[v]) + pp[0]);
                vy[v] = (float)((s * fpx[v] + cs * fpy[v]) + pp[1]);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int w = (v + 1) & 3;
                seg[q + v][0] = vx[v]; seg[q + v][1] = vy[v]; seg[q + v][2] = vx[w]; seg[q + v][3] = vy[w];
            }
        }
    }
    return r;
}

// ---- the static ray of every beam into rng[] (metres, not clipped), 64 adjacent beams at a time, handed out as wavefronts
// finish.  Every thread of the workgroup calls it; `counter` is an LDS word that is 0 when the first wavefront arrives.  lth is
// (float)sp.p[2]; the origin cell is made a scalar here so that it holds no vector register through the march.
template <typename Field, int RULE, bool RECT>
__device__ __forceinline__ void replay_march(const navsim_config& c, const navsim_state& st, const Field& field, const char* rects,
                                             const ScanPose& sp, float lth, double step, float max_range, int* counter,
                                             float2* dir, float* rng) {
    const int B = c.n_beams, H = c.map_h, W = c.map_w, lane = (int)threadIdx.x & 63;
    const int i0 = __builtin_amdgcn_readfirstlane(sp.i0), j0 = __builtin_amdgcn_readfirstlane(sp.j0);
    const float x0 = (float)i0, y0 = (float)j0, res = (float)c.resolution;
    const double cT = sp.cT, sT = sp.sT;
    const bool int_range = int_range_ok(H, W);
    const unsigned tpr = (unsigned)((W + 7) >> kRectShift);
    for (;;) {
        int chunk = 0;
        if (lane == 0) chunk = atomicAdd(counter, 1);
        chunk = __builtin_amdgcn_readfirstlane(chunk);
        if (chunk * 64 >= B) break;
        const int k = chunk * 64 + lane;
        if (k < B) {
            float dx, dy;
            beam_dir_k(c, st.beam_table, k, step, (double)lth, cT, sT, dx, dy);
            dir[k] = make_float2(dx, dy);
            float t = 0.0f;
            lanemask_t active = mask_of(true), hit = 0;
            while (active != 0)
                probe_round<Field, RULE, RECT>(field, rects, tpr, x0, y0, dx, dy, (unsigned)W, (unsigned)H, max_range, t, active, hit);
            rng[k] = ray_result<RULE>(hit, int_range, i0, j0, x0, y0, dx, dy, t, max_range) * res;
        }
    }
}
// behind the march's barrier: the pedestrians' primitives lower rng[]
template <int BLOCK>
__device__ __forceinline__ void replay_merge(int B, int nseg, int ndisc, float lx, float ly, double step, const Prims pr,
                                             const float2* dir, float* rng) {
    if (nseg + ndisc) {
        merge_prims_culled_core<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng);
        __syncthreads();
    }
}
// one scan of the whole workgroup from a lidar pose: cull, march, merge
template <int BLOCK, typename Field, int RULE, bool RECT>
__device__ __forceinline__ void replay_scan(const navsim_config& c, const navsim_state& st, const Field& field, const char* rects,
                                            const Prims pr, int nseg, int ndisc, const ScanPose& sp, double step, float rcull,
                                            float max_range, int* counter, float2* dir, float* rng) {
    const float lx = (float)sp.p[0], ly = (float)sp.p[1], lth = (float)sp.p[2];      // env.py:386
    if (nseg + ndisc) prim_in_range<BLOCK>(nseg + ndisc, nseg, lx, ly, rcull, pr, (float)step, (float)(c.angle_min + (double)lth));
    replay_march<Field, RULE, RECT>(c, st, field, rects, sp, lth, step, max_range, counter, dir, rng);
    __syncthreads();
    replay_merge<BLOCK>(c.n_beams, nseg, ndisc, lx, ly, step, pr, dir, rng);
}

// ---- the verdict over the beams.  Each thread brings what its own pass over the beams found (cr, dc: a beam under the crash /
// discomfort threshold; mg: its smallest margin); rng[] holds the ranges that pass judged -- CLIP: not yet clipped to [0, rcap]
// (the capped pair), otherwise as they stand (the observation pair: clipped and noisy).  *vote is 0 on entry; wave_margin /
// wave_ratio are BLOCK / 64 LDS words each that nobody else touches until the workgroup's next barrier but one (the lookahead
// pair alternates two sets).  One barrier, two with a ratio.  margin and rmin are thread 0's.
struct BeamVerdict { int crash, discomfort; float margin; double rmin; };
template <int BLOCK, bool CLIP>
__device__ __forceinline__ BeamVerdict replay_verdict(int B, int cr, int dc, float mg, int* vote, float* wave_margin, double* wave_ratio,
                                                      const float* rng, const float* thr, const float* dthr, float rcap) {
    constexpr int WAVES = BLOCK / 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mg = wave_min_f32(mg);
    int v = (int)(mask_of(cr != 0) != 0) | ((int)(mask_of(dc != 0) != 0) << 1);
    if (lane == 0) {
        if (v != 0) atomicOr(vote, v);
        wave_margin[wave] = mg;
    }
    __syncthreads();
    v = __builtin_amdgcn_readfirstlane(*vote);
    BeamVerdict r = {v & 1, (v >> 1) & 1, 0.0f, 1.0e300};
    const bool ratio = r.discomfort && !r.crash;
    if (ratio) {                                                                     // env.py:563-569, as the step's phase 3
        double rmin = 1.0e300;
        for (int k = tid; k < B; k += BLOCK) {
            float x = rng[k];
            if (CLIP) {
                x = x < 0.0f ? 0.0f : x;
                x = x > rcap ? rcap : x;
            }
            const double q = nv::discomfort_ratio((double)x, thr[k], dthr[k]);
            rmin = q < rmin ? q : rmin;
        }
        rmin = wave_min_f64(rmin);
        if (lane == 0) wave_ratio[wave] = rmin;
        __syncthreads();
        r.rmin = rmin;
    }
    if (tid == 0) {
        float margin = wave_margin[0];
        for (int w = 1; w < WAVES; ++w) margin = wave_margin[w] < margin ? wave_margin[w] : margin;
        r.margin = margin;
        if (ratio)
            for (int w = 1; w < WAVES; ++w) r.rmin = wave_ratio[w] < r.rmin ? wave_ratio[w] : r.rmin;
    }
    return r;
}

// ---- reward and end of the episode (thread 0).  vel: the PREVIOUS action (env.py:453); steps_now: the step count behind this
// step's increment (env.py:592).  truncated: the time limit ended an episode that neither succeeded nor crashed (phase 4).
struct StepVerdict { nv::RewardOut o; int done, truncated; };
__device__ __forceinline__ StepVerdict replay_reward(const navsim_config& c, const double* prev_xy, const double* pose, const double* vel,
                                                     const double* goal, const BeamVerdict& v, long long steps_now) {
    // (loaded in one round in front of the call: the callers hand in LDS and global memory, and thread 0 is alone here)
    const double a[2] = {prev_xy[0], prev_xy[1]}, b[2] = {pose[0], pose[1]}, w[2] = {vel[0], vel[1]}, g[2] = {goal[0], goal[1]};
    StepVerdict r;
    r.o = nv::reward_scalar(c, a, b, w, g, v.crash != 0, v.discomfort != 0, v.rmin);
    r.truncated = !r.o.done && c.max_episode_steps > 0 && steps_now >= (long long)c.max_episode_steps;
    r.done = r.o.done || r.truncated;
    return r;
}

// ---- what a pedestrian carries from step to step inside a horizon: pedestrian i in the registers of lane i of wavefront 0.
// n_waypoints, v_pref, has_legs and the waypoints do not change inside a horizon (nothing is drawn or planned).
struct CarriedPed {
    double pp[3] = {0.0, 0.0, 0.0}, pvel[2] = {0.0, 0.0};    // ped_pose, ped_vel
    double dist[3] = {0.0, 0.0, 0.0}, yaw = 0.0;             // ped_dist, ped_prev_yaw (LIDAR)
    bool legged = false;                                     // two leg discs for the lidar, not four sides (LIDAR)
    double vpref = 0.0;                                      // social force: v_pref, the waypoints and the head
    const double* wp = nullptr;
    int head = 0, nw = 1;
    const double* cmd = nullptr;                             // held: the command of the whole horizon
};
// pedestrian pq of the state (a live one).  LIDAR: also what the lidar's primitives need (a caller without a scan passes false
// and never reads those members -- nor the state's arrays behind them).  sfm / held: the social force moves it / a held command
// does (cmd_arg in place of st.ped_cmd where given); neither: it keeps its velocity.
template <bool LIDAR>
__device__ __forceinline__ void carried_ped_load(CarriedPed& p, const navsim_config& c, const navsim_state& st, size_t pq, bool sfm,
                                                 bool held, const double* cmd_arg) {
    p.pp[0] = st.ped_pose[pq * 3]; p.pp[1] = st.ped_pose[pq * 3 + 1]; p.pp[2] = st.ped_pose[pq * 3 + 2];
    p.pvel[0] = st.ped_vel[pq * 2]; p.pvel[1] = st.ped_vel[pq * 2 + 1];
    if (LIDAR) {
        p.dist[0] = st.ped_dist[pq * 3]; p.dist[1] = st.ped_dist[pq * 3 + 1]; p.dist[2] = st.ped_dist[pq * 3 + 2];
        p.yaw = st.ped_prev_yaw[pq];
        p.legged = st.ped_has_legs[pq] && c.lidar_legs;
    }
    if (sfm) {
        p.wp = st.ped_waypoints + (pq * c.max_waypoints) * 2;
        p.nw = st.ped_n_waypoints[pq];
        p.nw = p.nw < 1 ? 1 : (p.nw > c.max_waypoints ? c.max_waypoints : p.nw);     // (a state the step accepts holds 1 .. max_waypoints)
        p.head = st.ped_wp_head[pq];
        p.head = p.head < 0 ? 0 : (p.head > p.nw - 1 ? p.nw - 1 : p.head);
        p.vpref = st.ped_v_pref[pq];
    } else if (held) {
        p.cmd = (cmd_arg ? cmd_arg : st.ped_cmd) + pq * 2;
    }
}
