// kernels_lookahead.hpp -- action lookahead (include/navsim.h navsim_lookahead): what navsim_step would return for each of K
// candidate actions of an arena, from the current state, which is only read.  Part of the single translation unit
// navsim_kernels.hip (included inside its anonymous namespace; not a standalone header).
//
// One workgroup of kLookaheadBlock threads per arena, in two parts.
//
// (A) once per arena, two wavefronts side by side:
//   wavefront 0 -- the pedestrians at t + 1, pedestrian i on lane i, with the step's own functions in the step's order
//     (ped_stage_wave: waypoint pop and staging; ped_pair_term; ped_sfm_step, or nv::set_vel on the command; nv::leg_odometry),
//     so the same float64 values.  Nothing of it reads the robot's NEW pose (the social force sees the pose of time t: DESIGN.md
//     section 6, phase 0), so it is shared by all candidates.  The new pose and odometry never leave the lane's registers: the
//     lane turns them into the lidar's primitives (four sides or two leg discs, WORLD coordinates -- they do not depend on the
//     candidate either) in LDS, each pedestrian at its place in the oracle's order (a ballot, as kernels_scan_labels.hpp).
//   wavefront 1 -- the K candidate poses, candidate k on lane k (K <= 64): the step's phase 0 on actions[e,k] (wheels to twist,
//     clamp_action, min_turning_radius, KetiRobot.set_vel through nv::set_vel_with), then the float32 lidar pose, its sincos
//     and the integer origin cell.  A lane's float64 work costs the wavefront the same whether one lane or 64 are live: K
//     poses cost what one does.  56 bytes per candidate in LDS (LookCand).
// (B) per candidate, the whole workgroup: prim_in_range (the cull depends on the lidar pose), the beams in 64-beam chunks
//   through probe_round / ray_result under march_limit(H, W, R, res), merge_prims_culled_core, then the flags and the margin
//   (one pass over the beams, one vote through LDS), the discomfort ratio's minimum when the step would compute it (discomfort
//   without crash: a second pass), and thread 0's nv::reward_scalar.  Three barriers per candidate, four with pedestrians in
//   the arena, five with a ratio.  What changes from one candidate to the next in LDS -- chunk counter and vote (in LookCand,
//   armed in part A), the per-wavefront minima (two sets, by the candidate's parity) -- is never re-armed between barriers.
//
// The march is scan_labels_kernel's: probe_round from t = 0 in the pedestrian scans' form (RECT: the tile's record from global
// memory), the step's floats (tests/test_gpu_scan_labels.py holds that form to the step's observation bit for bit).  R replaces
// range_max in the march limit, the cull and the clip; include/navsim.h states why no flag and no minimum ratio changes.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms: 78 - 79 VGPRs, 106 SGPRs, occupancy 6 waves per
// SIMD, scratch 0 bytes per lane, no VGPR spill; 103 - 154 SGPRs spilled to VGPR lanes (the configuration and the state arrive
// as kernel arguments and most of their fields are live across the candidate loop), 112 bytes of static LDS; the dynamic LDS
// is lookahead_lds_bytes below.
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
    double rp[3];            // the pose the step would scan from (rule 3)
    double cT, sT;           // cos / sin of (double)(float)rp[2] for the beam-table fast path
    int i0, j0;              // integer ray origin (env.py:419)
    int next_chunk;          // next 64-beam chunk to hand to a wavefront
    int vote;                // crash (bit 0) and discomfort (bit 1) ORed over the wavefronts
};
static_assert(sizeof(LookCand) == 56, "include/navsim.h states 56 bytes per candidate");

__host__ __device__ inline size_t lookahead_align16(size_t n) { return (n + 15) & ~(size_t)15; }
// Dynamic LDS of one arena, in the order lookahead_kernel carves it: per beam dir (8 B) and rng (4 B); 56 B per candidate; with a
// pedestrian model PedShared (144 B per pedestrian slot + 32: the agents at time t, the primitives, their beam intervals) and the
// social force's pair table (16 B x (N (N - 1) / 2 + N)).  1081 beams, 20 pedestrians, K = 9: 12.7 + 0.5 + 2.9 + 3.4 KB.
inline size_t lookahead_lds_bytes(const navsim_config* c, int K) {
    size_t n = lookahead_align16((size_t)c->n_beams * (sizeof(float2) + sizeof(float))) + lookahead_align16((size_t)K * sizeof(LookCand));
    if (c->ped_model != NAVSIM_PED_NONE) n += lookahead_align16(ped_lds_bytes(c->max_peds)) + ped_pair_bytes(c->max_peds);
    return n;
}

__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = (o < v) ? o : v;
    }
    return v;
}

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kLookaheadBlock) void lookahead_kernel(navsim_config c, navsim_state st, LookaheadArgs a) {
    constexpr int BLOCK = kLookaheadBlock, WAVES = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ double wave_ratio[2][WAVES];
    __shared__ float wave_margin[2][WAVES];
    __shared__ int prim_count[2];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    float2* dir = (float2*)dyn;
    float* rng = (float*)(dyn + sizeof(float2) * (size_t)B);
    char* behind = dyn + lookahead_align16((size_t)B * (sizeof(float2) + sizeof(float)));
    LookCand* cand = (LookCand*)behind;
    behind += lookahead_align16((size_t)K * sizeof(LookCand));
    const bool ped_model = c.ped_model != NAVSIM_PED_NONE;
    PedShared ps = {};
    double2* pair = nullptr;
    if (ped_model) {
        ps = ped_lds_carve(behind, N);
        pair = (double2*)(behind + lookahead_align16(ped_lds_bytes(N)));
    }
    const Prims pr = {ps.seg, ps.disc, ps.info};

    int n = 0;                                                                       // rule 2
    if (ped_model) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const double dt = c.time_step;
    const double* rp_g = st.robot_pose + 3 * (size_t)e;
    const double* pa_g = st.prev_action + 2 * (size_t)e;
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);
    if (tid == 0) { prim_count[0] = 0; prim_count[1] = 0; a.out.status[e] = 1; }

    // ---- part A, wavefront 0: the pedestrians at t + 1 and what the lidar sees of them (N <= 64: one lane per pedestrian)
    if (wave == 0 && n > 0) {
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
            for (int t = tid; t < n_terms; t += 64) ped_pair_term(c, ps, pair, n, t);
            wave_lds_sync();
            const double* wp = st.ped_waypoints + (pq * c.max_waypoints) * 2;
            if (is_ped) ped_sfm_step(c, field, ps, pair, n, tid, st.ped_v_pref[pq], wp + 2 * head, dt, pp, pvel);
        } else if (is_ped) {
            const double* cmd = (a.ped_cmd ? a.ped_cmd : st.ped_cmd) + pq * 2;
            nv::set_vel(pp, cmd[0], cmd[1], dt, 0.0, pvel);                          // env.py:662
        }
        double dist[3] = {0.0, 0.0, 0.0};
        if (is_ped) {
            dist[0] = st.ped_dist[pq * 3]; dist[1] = st.ped_dist[pq * 3 + 1]; dist[2] = st.ped_dist[pq * 3 + 2];
            nv::leg_odometry(pp, pvel, st.ped_prev_yaw[pq], dt, dist);
        }
        const bool legged = is_ped && st.ped_has_legs[pq] && c.lidar_legs;
        const lanemask_t lm = mask_of(legged);
        const int legs_all = __popcll(lm), legs_below = __popcll(lm & ((1ull << tid) - 1ull));
        const int nseg_w = 4 * (n - legs_all);
        if (tid == 0) { prim_count[0] = nseg_w; prim_count[1] = 2 * legs_all; }
        if (is_ped) {                                                                // env.py:392-414
            if (legged) {
                float cc[4];
                nv::leg_centres((float)pp[0], (float)pp[1], (float)pp[2], (float)dist[0], (float)dist[1], (float)dist[2], cc);
                const int q = 2 * legs_below;
                ps.disc[q][0] = cc[0]; ps.disc[q][1] = cc[1];
                ps.disc[q + 1][0] = cc[2]; ps.disc[q + 1][1] = cc[3];
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
                const int q = 4 * (tid - legs_below);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int w = (v + 1) & 3;
                    ps.seg[q + v][0] = vx[v]; ps.seg[q + v][1] = vy[v]; ps.seg[q + v][2] = vx[w]; ps.seg[q + v][3] = vy[w];
                }
            }
        }
    }
    // ---- part A, wavefront 1: the candidates' poses (rule 3; the step's phase 0, operation for operation)
    if (wave == 1 && lane < K) {
        double a0 = a.actions[2 * (row + lane)], a1 = a.actions[2 * (row + lane) + 1];
        if (c.action_kind == NAVSIM_ACTION_WHEELS) {
            const double wl = a0, wr = a1;
            a0 = c.wheel_radius * (wl + wr) * 0.5;
            a1 = c.wheel_radius * (wr - wl) / c.wheel_track;
        }
        if (c.clamp_action) {
            a0 = a0 < c.linvel_lo ? c.linvel_lo : (a0 > c.linvel_hi ? c.linvel_hi : a0);
            a1 = a1 < c.rotvel_lo ? c.rotvel_lo : (a1 > c.rotvel_hi ? c.rotvel_hi : a1);
        }
        if (c.min_turning_radius > 0.0) {                                            // env.py:595-600
            const double lim = fabs(a1) * c.min_turning_radius;
            if (a0 >= 0.0) a0 = (a0 > lim) ? a0 : lim;
            else           a0 = (a0 < -lim) ? a0 : -lim;
        }
        const double th_old = rp_g[2];
        const double th = th_old + a1 * dt;                                          // set_vel's intermediate heading
        double s0, c0, s1, c1;
        nv::sincos(th_old, s0, c0);
        nv::sincos(th, s1, c1);
        double p[3] = {rp_g[0], rp_g[1], th_old};                                    // env.py:664
        nv::set_vel_with(p, a0, a1, dt, c.axle_offset, s0, c0, s1, c1, nullptr);
        LookCand& cd = cand[lane];
        cd.rp[0] = p[0]; cd.rp[1] = p[1]; cd.rp[2] = p[2];
        const float lth = (float)p[2];                                               // env.py:386
        double sT, cT;
        nv::sincos((double)lth, sT, cT);
        cd.cT = cT; cd.sT = sT;
        int i0, j0;
        nv::xy_to_ij_f32((float)p[0], (float)p[1], c, i0, j0);                       // env.py:419
        cd.i0 = i0; cd.j0 = j0;
        cd.next_chunk = 0; cd.vote = 0;
        a.out.pose[3 * (row + lane)] = p[0]; a.out.pose[3 * (row + lane) + 1] = p[1]; a.out.pose[3 * (row + lane) + 2] = p[2];
    }
    __syncthreads();
    const int nseg = prim_count[0], ndisc = prim_count[1], nprim = nseg + ndisc;

    // ---- part B: the candidates, one behind the other
    const double step = nv::linspace_step(c);
    const float rcap = (float)a.range;
    const float rcull = prim_cull_range(a.range);
    const float max_range = march_limit(H, W, a.range, c.resolution);
    const float res = (float)c.resolution;
    const bool int_range = int_range_ok(H, W);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const unsigned tpr = (unsigned)((W + 7) >> kRectShift);
    const float* thr = st.scan_threshold;
    const float* dthr = st.scan_discomfort;
    const double* pv_g = st.prev_pose + 3 * (size_t)e;
    const double* goal_g = st.robot_goal + 2 * (size_t)e;
    for (int q = 0; q < K; ++q) {
        LookCand& cd = cand[q];
        const int par = q & 1;
        const float lx = (float)cd.rp[0], ly = (float)cd.rp[1], lth = (float)cd.rp[2];          // env.py:386
        const int i0 = __builtin_amdgcn_readfirstlane(cd.i0), j0 = __builtin_amdgcn_readfirstlane(cd.j0);
        const float x0 = (float)i0, y0 = (float)j0;
        const double cT = cd.cT, sT = cd.sT;
        // (info[]: its last readers, candidate q - 1's merge, lie in front of that candidate's vote barrier)
        if (nprim) prim_in_range<BLOCK>(nprim, nseg, lx, ly, rcull, pr, (float)step, (float)(c.angle_min + (double)lth));
        // rule 4: the static ray of every beam under the cap, 64 adjacent beams at a time, handed out as wavefronts finish
        for (;;) {
            int chunk = 0;
            if (lane == 0) chunk = atomicAdd(&cd.next_chunk, 1);
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
        __syncthreads();
        if (nprim) {
            merge_prims_culled_core<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng);
            __syncthreads();
        }
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
        mg = wave_min_f32(mg);
        int v = (int)(mask_of(cr != 0) != 0) | ((int)(mask_of(dc != 0) != 0) << 1);
        if (lane == 0) {
            if (v != 0) atomicOr(&cd.vote, v);
            wave_margin[par][wave] = mg;
        }
        __syncthreads();
        v = __builtin_amdgcn_readfirstlane(cd.vote);
        const int crash = v & 1, discomfort = (v >> 1) & 1;
        double rmin = 1.0e300;
        if (discomfort && !crash) {                                                  // env.py:563-569, as the step's phase 3
            for (int k = tid; k < B; k += BLOCK) {
                float r = rng[k];
                r = r < 0.0f ? 0.0f : r;
                r = r > rcap ? rcap : r;
                const double ratio = nv::discomfort_ratio((double)r, thr[k], dthr[k]);
                rmin = ratio < rmin ? ratio : rmin;
            }
            rmin = wave_min_f64(rmin);
            if (lane == 0) wave_ratio[par][wave] = rmin;
            __syncthreads();
        }
        if (tid == 0) {
            float margin = wave_margin[par][0];
            for (int w = 1; w < WAVES; ++w) margin = wave_margin[par][w] < margin ? wave_margin[par][w] : margin;
            if (discomfort && !crash)
                for (int w = 1; w < WAVES; ++w) rmin = wave_ratio[par][w] < rmin ? wave_ratio[par][w] : rmin;
            const double prev_xy[2] = {pv_g[0], pv_g[1]};
            const double pose[2] = {cd.rp[0], cd.rp[1]};
            const double vel[2] = {pa_g[0], pa_g[1]};                                // env.py:453: the PREVIOUS action
            const double goal[2] = {goal_g[0], goal_g[1]};
            const nv::RewardOut o = nv::reward_scalar(c, prev_xy, pose, vel, goal, crash != 0, discomfort != 0, rmin);
            int done = o.done;
            if (c.max_episode_steps > 0 && (int)(st.steps[e] + 1) >= c.max_episode_steps) done = 1;
            a.out.reward[row + q] = o.reward;
            a.out.done[row + q] = (uint8_t)done;
            a.out.is_success[row + q] = o.success;
            a.out.is_crash[row + q] = o.crash;
            a.out.discomfort[row + q] = (uint8_t)(discomfort && !crash);
            a.out.distance[row + q] = o.distance;
            a.out.margin[row + q] = margin;
        }
    }
}
