// kernels_lookahead.hpp -- action lookahead (include/navsim.h navsim_lookahead): what navsim_step would return for each of K
// candidate actions of an arena, from the current state, which is only read.  Part of the single translation unit
// navsim_kernels.hip (included inside its anonymous namespace, behind kernels_replay.hpp, which states the replayed pieces of the
// step -- twist, scan pose, primitives, march, verdict, LDS layout -- once for this kernel and its three relatives).
//
// One workgroup of kLookaheadBlock threads per arena, in two parts.
//
// (A) once per arena, two wavefronts side by side (lookahead_part_a, shared with lookahead_obs_kernel):
//   wavefront 0 -- the pedestrians at t + 1, pedestrian i on lane i, with the step's own functions in the step's order
//     (ped_stage_wave: waypoint pop and staging; ped_pair_term; ped_sfm_step, or nv::set_vel on the command; nv::leg_odometry),
//     so the same float64 values.  Nothing of it reads the robot's NEW pose (the social force sees the pose of time t: DESIGN.md
//     section 6, phase 0), so it is shared by all candidates.  The new pose and odometry never leave the lane's registers: the
//     lane turns them into the lidar's primitives (replay_prims: WORLD coordinates -- they do not depend on the candidate
//     either) in LDS, each pedestrian at its place in the oracle's order.
//   wavefront 1 -- the K candidate poses, candidate k on lane k (K <= 64): replay_twist on actions[e,k], then scan_pose_step.  A
//     lane's float64 work costs the wavefront the same whether one lane or 64 are live: K poses cost what one does.  56 bytes
//     per candidate in LDS (LookCand).
// (B) per candidate, the whole workgroup: replay_scan under march_limit(H, W, R, res) (cull -- it depends on the lidar pose --,
//   march, merge), then the flags and the margin (one pass over the beams, replay_verdict's vote through LDS), the discomfort
//   ratio's minimum when the step would compute it (discomfort without crash: a second pass), and thread 0's nv::reward_scalar.
//   Three barriers per candidate, four with pedestrians in the arena, five with a ratio.  What changes from one candidate to the
//   next in LDS -- chunk counter and vote (in LookCand, armed in part A), the per-wavefront minima (two sets, by the candidate's
//   parity) -- is never re-armed between barriers.
//
// The march is scan_labels_kernel's: probe_round from t = 0 in the pedestrian scans' form (RECT: the tile's record from global
// memory), the step's floats (tests/test_gpu_scan_labels.py holds that form to the step's observation bit for bit).  R replaces
// range_max in the march limit, the cull and the clip; include/navsim.h states why no flag and no minimum ratio changes.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms: 74 VGPRs, 106 SGPRs, occupancy 6 waves per SIMD,
// scratch 0 bytes per lane, no VGPR spill; 104 - 135 SGPRs spilled to VGPR lanes (the configuration and the state arrive as
// kernel arguments and most of their fields are live across the candidate loop), 112 bytes of static LDS; the dynamic LDS is
// lookahead_lds_bytes below.  Thread 0's nv::reward_scalar block is written out here, not replay_reward as in the three
// relatives: with the shared function the compiler needs 72 vector registers, which is a seventh wave -- a change of occupancy
// that a change of its own should take and measure (profiles/r28_replay/summary.txt).
//
// Measured (profiles/r22_lookahead/summary.txt, 4096 arenas x 1081 beams, R = 1.75 m): K = 9 takes 327.9 us with 20 pedestrians
// an arena and 255.3 us with none -- x 2.23 resp. x 3.12 of the whole step kernel in the same trace; K = 64 1787 / 1602 us.  A
// candidate costs 25 - 36 us under a cap of 39 cells and 103 - 122 us under range_max's 504: the cap shortens the march, not the
// candidate's fixed work -- every beam's float64 direction (beam_dir_k), the first probes' dependent record loads from global
// memory (the step probes an LDS copy), the barriers.  Not tried: directions by rotating those of the arena's first candidate,
// candidates split over wavefronts (12 bytes a beam per wavefront), the LDS index form of the march.

struct LookaheadArgs {
    navsim_lookahead_out out;
    const double* actions;
    const double* ped_cmd;
    const uint8_t* skip;
    int K;
    double range;
};

constexpr int kLookaheadBlock = 256;

struct LookCand {
    ScanPose sp;             // the pose the step would scan from (rule 3)
    int next_chunk;          // next 64-beam chunk to hand to a wavefront
    int vote;                // crash (bit 0) and discomfort (bit 1) ORed over the wavefronts
};
static_assert(sizeof(LookCand) == 56, "include/navsim.h states 56 bytes per candidate");

// Dynamic LDS of one arena: replay_lds_bytes with 56 B per candidate
inline size_t lookahead_lds_bytes(const navsim_config* c, int K) { return replay_lds_bytes(c, (size_t)K * sizeof(LookCand)); }

// Part A of lookahead_kernel and lookahead_obs_kernel: wavefront 0 leaves the primitives of the n pedestrians at t + 1 in l.ps
// and their counts in prim_count[0 .. 1] (which thread 0 has zeroed); wavefront 1 leaves the K candidates armed in cand[] and
// their poses in pose_out[K][3].  actions: the arena's K actions; the caller's barrier follows.
template <typename Field>
__device__ __forceinline__ void lookahead_part_a(const navsim_config& c, const navsim_state& st, const Field& field, int e, int n, int K,
                                                 const ReplayLds& l, LookCand* cand, int* prim_count, const double* actions,
                                                 const double* ped_cmd, double* pose_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = c.max_peds;
    const double dt = c.time_step;
    const double* rp_g = st.robot_pose + 3 * (size_t)e;
    const double* pa_g = st.prev_action + 2 * (size_t)e;
    // ---- wavefront 0: the pedestrians at t + 1 and what the lidar sees of them (N <= 64: one lane per pedestrian)
    if (wave == 0 && n > 0) {
        const PedShared& ps = l.ps;
        const bool is_ped = tid < n;
        const size_t pq = (size_t)e * N + (is_ped ? tid : 0);
        double pp[3] = {0.0, 0.0, 0.0}, pvel[2] = {0.0, 0.0};
        if (is_ped) {
            pp[0] = st.ped_pose[pq * 3]; pp[1] = st.ped_pose[pq * 3 + 1]; pp[2] = st.ped_pose[pq * 3 + 2];
            pvel[0] = st.ped_vel[pq * 2]; pvel[1] = st.ped_vel[pq * 2 + 1];
        }
        if (c.ped_model == NAVSIM_PED_SFM) {
            int nw = 1;
            const int head = ped_stage_wave(c, st, n, tid, is_ped, pq, rp_g, pa_g[0], ps, pp, pvel, nw);
            wave_lds_sync();
            const int n_terms = n * (n - 1) / 2 + n;
            for (int t = tid; t < n_terms; t += 64) ped_pair_term(c, ps, l.pair, n, t);
            wave_lds_sync();
            const double* wp = st.ped_waypoints + (pq * c.max_waypoints) * 2;
            if (is_ped) ped_sfm_step(c, field, ps, l.pair, n, tid, st.ped_v_pref[pq], wp + 2 * head, dt, pp, pvel);
        } else if (is_ped) {
            const double* cmd = (ped_cmd ? ped_cmd : st.ped_cmd) + pq * 2;
            nv::set_vel(pp, cmd[0], cmd[1], dt, 0.0, pvel);                          // env.py:662
        }
        double dist[3] = {0.0, 0.0, 0.0};
        if (is_ped) {
            dist[0] = st.ped_dist[pq * 3]; dist[1] = st.ped_dist[pq * 3 + 1]; dist[2] = st.ped_dist[pq * 3 + 2];
            nv::leg_odometry(pp, pvel, st.ped_prev_yaw[pq], dt, dist);
        }
        const bool legged = is_ped && st.ped_has_legs[pq] && c.lidar_legs;
        const PrimSlot slot = replay_prims(n, tid, is_ped, legged, pp, dist, ps.seg, ps.disc);
        if (tid == 0) { prim_count[0] = slot.nseg; prim_count[1] = slot.ndisc; }
    }
    // ---- wavefront 1: the candidates' poses (rule 3; the step's phase 0, operation for operation)
    if (wave == 1 && lane < K) {
        double a0 = actions[2 * lane], a1 = actions[2 * lane + 1];
        replay_twist(c, true, a0, a1);
        LookCand cd;
        scan_pose_step(cd.sp, c, rp_g, a0, a1);
        cd.next_chunk = 0; cd.vote = 0;
        cand[lane] = cd;
        pose_out[3 * lane] = cd.sp.p[0]; pose_out[3 * lane + 1] = cd.sp.p[1]; pose_out[3 * lane + 2] = cd.sp.p[2];
    }
}

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kLookaheadBlock) void lookahead_kernel(navsim_config c, navsim_state st, LookaheadArgs a) {
    constexpr int BLOCK = kLookaheadBlock, WAVES = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ double wave_ratio[2][WAVES];
    __shared__ float wave_margin[2][WAVES];
    __shared__ int prim_count[2];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int N = c.max_peds, B = c.n_beams, H = c.map_h, W = c.map_w, K = a.K;
    const size_t row = (size_t)e * K;
    if (a.skip && a.skip[e]) {                                                       // rule 1
        for (int k = tid; k < K; k += BLOCK) {
            a.out.reward[row + k] = 0.0; a.out.done[row + k] = 0; a.out.is_success[row + k] = 0.0f; a.out.is_crash[row + k] = 0.0f;
            a.out.discomfort[row + k] = 0; a.out.distance[row + k] = 0.0; a.out.margin[row + k] = 0.0f;
            a.out.pose[3 * (row + k)] = 0.0; a.out.pose[3 * (row + k) + 1] = 0.0; a.out.pose[3 * (row + k) + 2] = 0.0;
        }
        if (tid == 0) a.out.status[e] = 0;
        return;
    }
    const ReplayLds l = replay_lds_carve(dyn, c, (size_t)K * sizeof(LookCand));
    LookCand* cand = (LookCand*)l.own;
    float* const rng = l.rng;

    int n = 0;                                                                       // rule 2
    if (c.ped_model != NAVSIM_PED_NONE) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const double* pa_g = st.prev_action + 2 * (size_t)e;
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);
    if (tid == 0) { prim_count[0] = 0; prim_count[1] = 0; a.out.status[e] = 1; }

    lookahead_part_a(c, st, field, e, n, K, l, cand, prim_count, a.actions + 2 * row, a.ped_cmd, a.out.pose + 3 * row);
    __syncthreads();
    const int nseg = prim_count[0], ndisc = prim_count[1];

    // ---- part B: the candidates, one behind the other
    const double step = nv::linspace_step(c);
    const float rcap = (float)a.range;
    const float rcull = prim_cull_range(a.range);
    const float max_range = march_limit(H, W, a.range, c.resolution);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const float* thr = st.scan_threshold;
    const float* dthr = st.scan_discomfort;
    const double* pv_g = st.prev_pose + 3 * (size_t)e;
    const double* goal_g = st.robot_goal + 2 * (size_t)e;
    for (int q = 0; q < K; ++q) {
        LookCand& cd = cand[q];
        const int par = q & 1;
        // rule 4: the scan under the cap (info[]: its last readers, candidate q - 1's merge, lie in front of that candidate's
        // vote barrier)
        replay_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, l.pr, nseg, ndisc, cd.sp, step, rcull, max_range, &cd.next_chunk,
                                              l.dir, rng);
        // rule 6: flags and margin
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
        const BeamVerdict v = replay_verdict<BLOCK, true>(B, cr, dc, mg, &cd.vote, wave_margin[par], wave_ratio[par], rng, thr, dthr, rcap);
        if (tid == 0) {                                                              // (replay_reward, written out: see "Resources")
            const double prev_xy[2] = {pv_g[0], pv_g[1]};
            const double pose[2] = {cd.sp.p[0], cd.sp.p[1]};
            const double vel[2] = {pa_g[0], pa_g[1]};                                // env.py:453: the PREVIOUS action
            const double goal[2] = {goal_g[0], goal_g[1]};
            const nv::RewardOut o = nv::reward_scalar(c, prev_xy, pose, vel, goal, v.crash != 0, v.discomfort != 0, v.rmin);
            int done = o.done;
            if (c.max_episode_steps > 0 && (int)(st.steps[e] + 1) >= c.max_episode_steps) done = 1;
            a.out.reward[row + q] = o.reward;
            a.out.done[row + q] = (uint8_t)done;
            a.out.is_success[row + q] = o.success;
            a.out.is_crash[row + q] = o.crash;
            a.out.discomfort[row + q] = (uint8_t)(v.discomfort && !v.crash);
            a.out.distance[row + q] = o.distance;
            a.out.margin[row + q] = v.margin;
        }
    }
}
