// kernels_rollout.hpp -- action-sequence rollout (include/navsim.h navsim_rollout): what the next H navsim_step calls would return
// if an arena executed the action sequence a_0 .. a_{H-1}, for K sequences per arena, from the current state, which is only read.
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace, behind kernels_replay.hpp, whose
// pieces -- twist, scan pose, primitives, march, verdict, reward, carried pedestrian, LDS layout -- it calls).
//
// One workgroup of kRolloutBlock threads per (arena, sequence): a grid of E x K, sequence k of arena e on workgroup e K + k (the
// sequences of an arena are neighbours in the grid and read the same map).  From the second step on nothing is shared between
// sequences -- the social force sees the robot's pose and speed, so every sequence has its own pedestrians -- and a sequence ends
// where its episode ends, so there is nothing to share a workgroup for.  What navsim_step stores for its next call is CARRIED:
//   the robot (RollShared, static LDS): pose, prev_pose's xy, prev_action (after wheels-to-twist, clamp and turning radius: the
//     value kernels_step.hpp phase 6 stores), the step count;
//   pedestrian i on lane i of wavefront 0, in registers for the whole horizon: pose, velocity, ped_prev_yaw, ped_dist, the
//     waypoint head (ped_finish's stores).  n_waypoints, v_pref, has_legs and the waypoints themselves do not change inside the
//     horizon (rule 7: nothing is drawn or planned).
// A step h, seven barriers with pedestrians under the social force, four without pedestrians (+ 1 with a discomfort ratio);
// (1) - (4) are rollout_advance below, shared with rollout_obs_kernel:
//   (1) wavefront 0: waypoint pop from the carried head, the agents of time t staged in LDS (ped_stage_wave's body on the carried
//       values); thread 64 (wavefront 1, lane 0): the step's phase 0 on actions[e,k,h] from the carried pose (replay_twist,
//       scan_pose_step) -- the new pose, its float32 lidar pose, sincos and origin cell.  Barrier.
//   (2) social force only: the n (n - 1) / 2 + n pair terms over ALL 256 threads (ped_pair_term: each term lands in its own slot,
//       whoever computes it) -- 210 terms at 20 pedestrians are one round instead of wavefront 0's four.  Barrier.
//   (3) wavefront 0: ped_sfm_step (or nv::set_vel on the held command), the re-plan predicate, nv::leg_odometry, the lidar's
//       primitives in the oracle's order and prim_in_range<64> on its own lanes, as the fused step's wavefront 0; then it joins
//   (4) all wavefronts: the capped scan, 64 adjacent beams at a time handed out by an LDS counter (probe_round / ray_result under
//       march_limit(H, W, R, res), lookahead_kernel's part B).  Barrier; merge_prims_culled_core; barrier.
//   (5) flags and margin (one pass, a vote through LDS; barrier), the ratio's minimum when the step would compute it (barrier),
//       thread 0's nv::reward_scalar, the outputs of step h, the carry for step h + 1 and `stop`.  Barrier; all leave together.
// Rows behind the sequence's last evaluated step are zeroed by the whole workgroup at the end.
//
// Dynamic LDS (rollout_lds_bytes): 12 B per beam (dir 8, rng 4), with a pedestrian model PedShared (144 B per pedestrian slot +
// 32) and the pair table (16 B x (N (N - 1) / 2 + N)) -- the lookahead's without its 56 B per candidate: 12.7 + 2.9 + 3.4 KB at
// 1081 beams and 20 pedestrians.  Static LDS: RollShared + the wavefronts' minima.
//
// Arguments: the kernel reads cfg, state and RolloutArgs in place in the kernarg segment (NAVSIM_KERNARGS, kernels_step.hpp):
// most of their fields are live across the horizon loop.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms: 168 VGPRs in every one, 106 SGPRs, 125 - 132
// SGPRs spilled to VGPR lanes, no VGPR spill, scratch 0 bytes per lane, occupancy 3 waves per SIMD (three workgroups a compute
// unit; LDS would allow eight), 208 bytes of static LDS.  lookahead_kernel, with the same device functions outside any loop,
// needs 74: the registers are this kernel's open item, and where they go is NOT found.  Three forms were compiled and not taken:
// a bound of 128 registers for a fourth wave (__launch_bounds__(256, 4)) spills 34 - 35 VGPRs, 116 bytes of scratch per lane;
// the carried pedestrians and thread 0's sums in LDS instead of registers (76 bytes a pedestrian slot) still need 158; that form
// with cfg / state / arguments re-read inside every step through a pointer the compiler cannot see through (nothing of them
// hoisted out of the horizon loop) 154.  So neither the carry nor hoisted configuration values hold the registers.
// Measured: profiles/r23_rollout/summary.txt (README, "Action-sequence rollout").

struct RolloutArgs {
    navsim_rollout_out out;
    const double* actions;
    const double* ped_cmd;
    const uint8_t* skip;
    int K, H;
    double range, gamma;
};
struct RolloutKernargs { navsim_config c; navsim_state st; RolloutArgs a; };

constexpr int kRolloutBlock = 256;

struct RollShared {
    // carried from step to step (rule 2)
    double rp[3];            // the robot's pose at time t
    double prev_xy[2];       // prev_pose's xy
    double prev_act[2];      // prev_action
    long long steps;         // steps
    // step h
    ScanPose sp;             // the pose the step scans from (rule 3 of the lookahead)
    double act[2];           // the action as the step stores it
    int next_chunk;          // next 64-beam chunk to hand to a wavefront
    int vote;                // crash (bit 0) and discomfort (bit 1) ORed over the wavefronts
    int nseg, ndisc;         // the lidar's primitives of this step
    int stop;                // the sequence ended at this step
    int length;              // steps evaluated so far
};

// Dynamic LDS of one (arena, sequence): replay_lds_bytes with nothing of the kernel's own
inline size_t rollout_lds_bytes(const navsim_config* c) { return replay_lds_bytes(c, 0); }

// the carried robot at h = 0: the state's (one thread)
__device__ __forceinline__ void rollout_carry_load(RollShared& sh, const navsim_state& st, int e) {
    const double* rp_g = st.robot_pose + 3 * (size_t)e;
    sh.rp[0] = rp_g[0]; sh.rp[1] = rp_g[1]; sh.rp[2] = rp_g[2];
    sh.prev_xy[0] = st.prev_pose[3 * (size_t)e]; sh.prev_xy[1] = st.prev_pose[3 * (size_t)e + 1];
    sh.prev_act[0] = st.prev_action[2 * (size_t)e]; sh.prev_act[1] = st.prev_action[2 * (size_t)e + 1];
    sh.steps = (long long)st.steps[e];
    sh.nseg = 0; sh.ndisc = 0; sh.stop = 0; sh.length = 0;
}

// Steps (1) - (4) of step h, for rollout_kernel and rollout_obs_kernel: from the carry (sh, and pedestrian i in cp on lane i of
// wavefront 0) to the merged, unclipped scan of the pose sh.sp in l.rng, with the carried pedestrians moved to t + h + 1.  action:
// actions[e,k,h]; pose_out: pose[e,k,h]; keep_pose / keep_act: where thread 64 also leaves the pose and the stored action of
// step h (rollout_obs_kernel's tail reads them; nullptr: nowhere); exact: rule 8's count (wave-uniform on wavefront 0; thread 0
// reports it).  Ends behind the merge's barrier.
template <int BLOCK, typename Field, int RULE, bool RECT>
__device__ __forceinline__ void rollout_advance(const navsim_config& c, const navsim_state& st, const Field& field, const char* rects,
                                                const ReplayLds& l, RollShared& sh, CarriedPed& cp, int n, bool is_ped,
                                                const double* action, double* pose_out, double* keep_pose, double* keep_act, int h,
                                                int HZ, int& exact, double step, float rcull, float max_range) {
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool sfm = c.ped_model == NAVSIM_PED_SFM;
    const double dt = c.time_step;
    const PedShared& ps = l.ps;
    // ---- (1) wavefront 0: waypoint pop and staging (ped_stage_wave on the carried values)
    if (wave == 0 && n > 0 && sfm) {
        if (is_ped) {
            cp.head = ped_pop_waypoints(cp.wp, cp.head, cp.nw, cp.pp);
            ps.ax[tid] = cp.pp[0]; ps.ay[tid] = cp.pp[1]; ps.avx[tid] = cp.pvel[0]; ps.avy[tid] = cp.pvel[1];
        }
        if (tid == 0) {
            double s, cs;
            nv::sincos(sh.rp[2], s, cs);
            const double prev_v = sh.prev_act[0];
            ps.ax[n] = sh.rp[0]; ps.ay[n] = sh.rp[1];
            ps.avx[n] = prev_v * cs; ps.avy[n] = prev_v * s;
        }
    }
    // ---- (1) thread 64: the step's phase 0 on actions[e,k,h], operation for operation
    if (tid == 64) {
        double a0 = action[0], a1 = action[1];
        replay_twist(c, true, a0, a1);
        ScanPose sp;
        scan_pose_step(sp, c, sh.rp, a0, a1);
        sh.sp = sp;
        sh.act[0] = a0; sh.act[1] = a1;
        sh.next_chunk = 0; sh.vote = 0;
        pose_out[0] = sp.p[0]; pose_out[1] = sp.p[1]; pose_out[2] = sp.p[2];
        if (keep_pose) {
            keep_pose[0] = sp.p[0]; keep_pose[1] = sp.p[1]; keep_pose[2] = sp.p[2];
            keep_act[0] = a0; keep_act[1] = a1;
        }
    }
    __syncthreads();
    // ---- (2) the pair terms, shared out over the workgroup
    if (sfm && n > 0) {
        const int n_terms = n * (n - 1) / 2 + n;
        for (int t = tid; t < n_terms; t += BLOCK) ped_pair_term(c, ps, l.pair, n, t);
        __syncthreads();
    }
    const float lx = (float)sh.sp.p[0], ly = (float)sh.sp.p[1], lth = (float)sh.sp.p[2];          // env.py:386
    // ---- (3) wavefront 0: the pedestrians at t + h + 1 and what the lidar sees of them
    if (wave == 0 && n > 0) {
        bool due = false;
        if (is_ped) {
            if (sfm) {
                ped_sfm_step(c, field, ps, l.pair, n, tid, cp.vpref, cp.wp + 2 * cp.head, dt, cp.pp, cp.pvel);
                // the step's predicate for ped_due (ped_finish): the post-move distance to the LAST waypoint under 0.5 m
                const double ddx = cp.pp[0] - cp.wp[2 * (cp.nw - 1)], ddy = cp.pp[1] - cp.wp[2 * (cp.nw - 1) + 1];
                due = sqrt(ddx * ddx + ddy * ddy) < 0.5;                             // (nw >= 1: carried_ped_load)
            } else {
                nv::set_vel(cp.pp, cp.cmd[0], cp.cmd[1], dt, 0.0, cp.pvel);          // env.py:662
            }
            nv::leg_odometry(cp.pp, cp.pvel, cp.yaw, dt, cp.dist);
            cp.yaw = nv::wrap_pi(cp.pp[2]);
        }
        if (mask_of(due) != 0 && exact == HZ) exact = h + 1;                         // rule 8 (wave-uniform; thread 0 reports it)
        const PrimSlot slot = replay_prims(n, tid, is_ped, cp.legged, cp.pp, cp.dist, ps.seg, ps.disc);
        if (tid == 0) { sh.nseg = slot.nseg; sh.ndisc = slot.ndisc; }
        wave_lds_sync();
        prim_in_range<64>(slot.nseg + slot.ndisc, slot.nseg, lx, ly, rcull, l.pr, (float)step, (float)(c.angle_min + (double)lth));
    }
    // ---- (4) the static ray of every beam under the cap, 64 adjacent beams at a time, handed out as wavefronts finish
    replay_march<Field, RULE, RECT>(c, st, field, rects, sh.sp, lth, step, max_range, &sh.next_chunk, l.dir, l.rng);
    __syncthreads();
    replay_merge<BLOCK>(c.n_beams, sh.nseg, sh.ndisc, lx, ly, step, l.pr, l.dir, l.rng);
}

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kRolloutBlock) void rollout_kernel(navsim_config c_, navsim_state st_, RolloutArgs a_) {
    NAVSIM_KERNARGS(RolloutKernargs, c_, st_, a_);
    const navsim_config& c = ka.c; const navsim_state& st = ka.st; const RolloutArgs& a = ka.a;
    constexpr int BLOCK = kRolloutBlock, WAVES = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ RollShared sh;
    __shared__ double wave_ratio[WAVES];
    __shared__ float wave_margin[WAVES];
    const int K = a.K, HZ = a.H;
    const int e = (int)(blockIdx.x / (unsigned)K), kseq = (int)(blockIdx.x % (unsigned)K);
    const int tid = threadIdx.x, wave = tid >> 6;
    const int N = c.max_peds, B = c.n_beams, H = c.map_h, W = c.map_w;
    const size_t sq = (size_t)e * K + kseq;                      // row of [E,K]
    const size_t row = sq * (size_t)HZ;                          // first row of [E,K,H]
    if (a.skip && a.skip[e]) {                                                       // rule 4: a skipped arena
        for (int h = tid; h < HZ; h += BLOCK) {
            a.out.reward[row + h] = 0.0;
            a.out.pose[3 * (row + h)] = 0.0; a.out.pose[3 * (row + h) + 1] = 0.0; a.out.pose[3 * (row + h) + 2] = 0.0;
        }
        if (tid == 0) {
            a.out.ret[sq] = 0.0; a.out.length[sq] = 0; a.out.outcome[sq] = 0; a.out.discomfort_steps[sq] = 0;
            a.out.min_margin[sq] = 0.0f; a.out.distance[sq] = 0.0; a.out.exact_steps[sq] = 0;
            if (kseq == 0) a.out.status[e] = 0;
        }
        return;
    }
    const ReplayLds l = replay_lds_carve(dyn, c, 0);
    float* const rng = l.rng;

    int n = 0;
    if (c.ped_model != NAVSIM_PED_NONE) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);

    // ---- the carried values at h = 0: the state's.  Wavefront 0: pedestrian i on lane i (N <= 64); rule 6: a command is held
    const bool is_ped = wave == 0 && tid < n;
    CarriedPed cp;
    if (is_ped) carried_ped_load<true>(cp, c, st, (size_t)e * N + tid, c.ped_model == NAVSIM_PED_SFM, true, a.ped_cmd);
    if (tid == 64) {
        rollout_carry_load(sh, st, e);
        if (kseq == 0) a.out.status[e] = 1;
    }
    __syncthreads();

    const double step = nv::linspace_step(c);
    const float rcap = (float)a.range;
    const float rcull = prim_cull_range(a.range);
    const float max_range = march_limit(H, W, a.range, c.resolution);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const float* thr = st.scan_threshold;
    const float* dthr = st.scan_discomfort;
    const double goal[2] = {st.robot_goal[2 * (size_t)e], st.robot_goal[2 * (size_t)e + 1]};

    // thread 0: what the sequence accumulates
    double ret = 0.0, g = 1.0, distance = 0.0;
    float min_margin = INFINITY;
    int dsteps = 0, exact = HZ, outcome = 0;

    for (int h = 0; h < HZ; ++h) {
        // ---- (1) - (4): the scan of step h
        rollout_advance<BLOCK, Field, RULE, RECT>(c, st, field, rects, l, sh, cp, n, is_ped, a.actions + 2 * (row + h),
                                                  a.out.pose + 3 * (row + h), nullptr, nullptr, h, HZ, exact, step, rcull, max_range);
        // ---- (5) flags and margin (rule 6 of the lookahead)
        int cr = 0, dc = 0;
        float mg = INFINITY;
        for (int k = tid; k < B; k += BLOCK) {
            float r = rng[k];
            r = r < 0.0f ? 0.0f : r;                                                 // env.py:435, with R for range_max
            r = r > rcap ? rcap : r;
            const float thr_k = thr[k];
            cr |= (r < thr_k);
            dc |= (r < dthr[k]);
            const float m = r - thr_k;
            mg = m < mg ? m : mg;
        }
        const BeamVerdict v = replay_verdict<BLOCK, true>(B, cr, dc, mg, &sh.vote, wave_margin, wave_ratio, rng, thr, dthr, rcap);
        if (tid == 0) {
            const long long steps_now = sh.steps + 1;                                // env.py:592
            const StepVerdict r = replay_reward(c, sh.prev_xy, sh.sp.p, sh.prev_act, goal, v, steps_now);
            a.out.reward[row + h] = r.o.reward;
            ret = ret + g * r.o.reward;
            g = g * a.gamma;
            min_margin = v.margin < min_margin ? v.margin : min_margin;
            dsteps += (v.discomfort && !v.crash) ? 1 : 0;
            distance = r.o.distance;
            outcome = (r.o.success != 0.0f ? 1 : 0) | (r.o.crash != 0.0f ? 2 : 0) | (r.truncated ? 4 : 0);
            // the carry (rule 2): what phase 6 of the step stores when the episode goes on
            sh.rp[0] = sh.sp.p[0]; sh.rp[1] = sh.sp.p[1]; sh.rp[2] = sh.sp.p[2];
            sh.prev_xy[0] = sh.sp.p[0]; sh.prev_xy[1] = sh.sp.p[1];
            sh.prev_act[0] = sh.act[0]; sh.prev_act[1] = sh.act[1];
            sh.steps = steps_now;
            sh.length = h + 1;
            sh.stop = r.done;
        }
        __syncthreads();
        if (sh.stop) break;                                                          // rule 4: nothing behind a done step
    }
    const int length = sh.length;
    for (int h = length + tid; h < HZ; h += BLOCK) {
        a.out.reward[row + h] = 0.0;
        a.out.pose[3 * (row + h)] = 0.0; a.out.pose[3 * (row + h) + 1] = 0.0; a.out.pose[3 * (row + h) + 2] = 0.0;
    }
    if (tid == 0) {
        a.out.ret[sq] = ret;
        a.out.length[sq] = length;
        a.out.outcome[sq] = (uint8_t)outcome;
        a.out.discomfort_steps[sq] = dsteps;
        a.out.min_margin[sq] = min_margin;
        a.out.distance[sq] = distance;
        a.out.exact_steps[sq] = exact;
    }
}
