// kernels_lookahead_obs.hpp -- lookahead observations (include/navsim.h navsim_lookahead_obs): the WHOLE return of navsim_step for
// each of K candidate actions of an arena -- observation row, goals, reward, done, truncated, flags -- from the current state,
// which is only read, with the scan noise the step itself would draw.  Part of the single translation unit navsim_kernels.hip
// (included inside its anonymous namespace, behind kernels_lookahead.hpp, whose LookCand, LDS layout and wave_min_f32 it uses).
//
// lookahead_kernel's shape: one workgroup of kLookaheadBlock threads per arena; part A (pedestrians at t + 1 on wavefront 0,
// the K candidate poses on wavefront 1) is that kernel's, line for line; part B runs the candidates one behind the other with
// dir / rng in LDS, at the step's own march limit (range_max).  What is new here:
//   the finish pass -- ONE pass over the beams per candidate reads the merged range from LDS, clips it, adds the step's noise
//     (the stream of step_key = episode << 32 | (steps + 1) * 2: the draw the step would make), takes the flags and the margin
//     from the NOISY value as the step does, keeps it in LDS for the discomfort ratio and stores it to the candidate's scan row:
//     beam tid + i * 256 by thread tid, so every store instruction of a wavefront covers 256 adjacent bytes.  Before the vote
//     is known: a candidate that turns out to crash has its scan row overwritten below, by the same threads;
//   tail and goals -- behind the loop, all candidates at once, candidate k on lane k of wavefront 1 (the votes stay in LookCand).
//     Inside the loop, on thread 0 beside the reward, the float64 atan2 of wrap_pi was the kernel's register high-water mark:
//     102 vector registers, 4 waves per SIMD, and the launch took x 1.45 - 1.50 of navsim_lookahead's at range_max (K = 9 on the
//     c2-shaped world: 1457 us against 974 us) -- the march is bound by the latency of its dependent loads, i.e. by occupancy;
//   the crash re-scan -- at most once per arena, behind the candidate loop, only if a candidate crashed: from prev_pose, the
//     same pedestrians, the noise key step_key + 1; each thread copies its beams into the scan row of every crashing candidate
//     straight from the register;
//   the full rows [S*B + 7] -- only when the caller gave out.obs, last: every thread reads back the beams of the scan rows it
//     stored itself and writes the newest slot, the slots the stack fill takes (S - 1 - j > n_hist) and the shifted slots of
//     obs_prev.  With the row pointers live through the candidate loop the kernel held 83 vector registers (5 waves).
// Barriers per candidate: lookahead_kernel's (three, four with pedestrians, five with a ratio); the re-scan adds two or three
// per arena.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms under __launch_bounds__(256, 6): 79 - 80 VGPRs,
// 106 SGPRs, occupancy 6 waves per SIMD, scratch 0 bytes per lane, no VGPR spill; 170 - 212 SGPRs spilled to VGPR lanes
// (lookahead_kernel: 103 - 154), 112 bytes of static LDS; the dynamic LDS is lookahead_lds_bytes (12 bytes a beam, 56 a
// candidate, the pedestrians' share).
// Without the second bound the compiler settles on 81 vector registers, one above what six waves allow.
// Measured: profiles/r26_lookahead_obs/summary.txt.
// Not tried: a grid over (arena, group of candidates), directions by rotation, the LDS index form of the march.

struct LookObsArgs {
    navsim_lookahead_obs_out out;
    const double* actions;
    const double* ped_cmd;
    const float* obs_prev;
    const uint8_t* skip;
    int K;
    int noise;                // 1: the step's draw (host: NAVSIM_LOOKOBS_NOISE_STEP and cfg.add_scan_noise), 0: none
};

// One scan from a lidar pose into rng[] (metres, merged with the pedestrians' primitives, NOT clipped): rule 4's march.  Every
// thread of the workgroup calls it; `counter` is an LDS word that is 0 on entry and that nobody else touches.
template <int BLOCK, typename Field, int RULE, bool RECT>
__device__ __forceinline__ void lookobs_scan(const navsim_config& c, const navsim_state& st, const Field& field, const char* rects,
                                             const Prims pr, int nseg, int ndisc, float lx, float ly, float lth, int i0, int j0,
                                             double cT, double sT, double step, float rcull, float max_range, int* counter,
                                             float2* dir, float* rng) {
    const int B = c.n_beams, H = c.map_h, W = c.map_w, lane = (int)threadIdx.x & 63;
    const int nprim = nseg + ndisc;
    const float x0 = (float)i0, y0 = (float)j0, res = (float)c.resolution;
    const bool int_range = int_range_ok(H, W);
    const unsigned tpr = (unsigned)((W + 7) >> kRectShift);
    if (nprim) prim_in_range<BLOCK>(nprim, nseg, lx, ly, rcull, pr, (float)step, (float)(c.angle_min + (double)lth));
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
    __syncthreads();
    if (nprim) {
        merge_prims_culled_core<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng);
        __syncthreads();
    }
}

// a value that is the same on every lane, moved to scalar registers
__device__ __forceinline__ float uniform_f32(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// env.py:435-440 on one merged range: the clip, then the step's noise on a beam that is not at range_max
__device__ __forceinline__ float lookobs_finish(float r, float rmax, bool noise_on, float noise_std, uint64_t nkey, int k) {
    r = r < 0.0f ? 0.0f : r;
    r = r > rmax ? rmax : r;
    if (noise_on && r != rmax) r = r + noise_std * nv::gauss_noise(nkey, (uint32_t)k);
    return r;
}

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kLookaheadBlock, 6) void lookahead_obs_kernel(navsim_config c, navsim_state st, LookObsArgs a) {
    constexpr int BLOCK = kLookaheadBlock, WAVES = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ double wave_ratio[2][WAVES];
    __shared__ float wave_margin[2][WAVES];
    __shared__ int prim_count[2];
    __shared__ int rescan_chunk;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = c.max_peds, B = c.n_beams, S = c.n_scan_stack, H = c.map_h, W = c.map_w, K = a.K;
    const size_t D = (size_t)S * B + 7;
    const size_t row = (size_t)e * K;
    if (a.skip && a.skip[e]) {                                                       // rule 1
        for (int k = tid; k < K; k += BLOCK) {
            a.out.reward[row + k] = 0.0; a.out.done[row + k] = 0; a.out.is_success[row + k] = 0.0f; a.out.is_crash[row + k] = 0.0f;
            a.out.discomfort[row + k] = 0; a.out.distance[row + k] = 0.0; a.out.margin[row + k] = 0.0f; a.out.truncated[row + k] = 0;
            a.out.pose[3 * (row + k)] = 0.0; a.out.pose[3 * (row + k) + 1] = 0.0; a.out.pose[3 * (row + k) + 2] = 0.0;
        }
        for (size_t k = tid; k < (size_t)K * B; k += BLOCK) a.out.scan[row * B + k] = 0.0f;
        for (int k = tid; k < K * 7; k += BLOCK) a.out.tail[row * 7 + k] = 0.0f;
        for (int k = tid; k < K * 4; k += BLOCK) a.out.goals[row * 4 + k] = 0.0f;
        if (a.out.obs)
            for (size_t k = tid; k < (size_t)K * D; k += BLOCK) a.out.obs[row * D + k] = 0.0f;
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
    if (tid == 0) { prim_count[0] = 0; prim_count[1] = 0; rescan_chunk = 0; a.out.status[e] = 1; }

    // ---- part A, wavefront 0: the pedestrians at t + 1 and what the lidar sees of them (lookahead_kernel's, line for line)
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
    const int nseg = prim_count[0], ndisc = prim_count[1];

    // ---- part B: the candidates, one behind the other
    const double step = nv::linspace_step(c);
    const float rmax = (float)c.range_max;
    const float rcull = prim_cull_range(c.range_max);
    const float max_range = march_limit(H, W, c.range_max, c.resolution);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const float* thr = st.scan_threshold;
    const float* dthr = st.scan_discomfort;
    const double* pv_g = st.prev_pose + 3 * (size_t)e;
    const double* goal_g = st.robot_goal + 2 * (size_t)e;
    // rule 4's noise: the step's key and the global arena index (kernels_step.hpp, where sh.step_key is formed).  One value per
    // arena each: made scalars here, so that none of them holds a vector register through the march
    const float noise_std = a.noise ? uniform_f32(st.scan_noise_std[e]) : 0.0f;
    const bool noise_on = noise_std > 0.0f;
    const uint64_t genv = (uint64_t)(c.env_index_base + e);
    auto noise_key = [&](unsigned long long add) -> uint64_t {
        if (!noise_on) return 0;
        const unsigned long long key = (unsigned long long)st.episode[e] * 0x100000000ULL + (unsigned long long)(st.steps[e] + 1) * 2ULL + add;
        return uniform_u64(nv::noise_stream(c.seed, genv, key));
    };
    const uint64_t nkey = noise_key(0);
    for (int q = 0; q < K; ++q) {
        LookCand& cd = cand[q];
        const int par = q & 1;
        const float lx = (float)cd.rp[0], ly = (float)cd.rp[1], lth = (float)cd.rp[2];          // env.py:386
        const int i0 = __builtin_amdgcn_readfirstlane(cd.i0), j0 = __builtin_amdgcn_readfirstlane(cd.j0);
        // (info[] and rng[]: their last readers of candidate q - 1 lie in front of that candidate's vote or ratio barrier)
        lookobs_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, pr, nseg, ndisc, lx, ly, lth, i0, j0, cd.cT, cd.sT, step, rcull,
                                               max_range, &cd.next_chunk, dir, rng);
        // rules 4 - 5: clip, noise, flags and margin in one pass; the scan row from the same register
        float* const scan_q = a.out.scan + (row + q) * B;
        int cr = 0, dc = 0;
        float mg = INFINITY;
        for (int k = tid; k < B; k += BLOCK) {
            const float r = lookobs_finish(rng[k], rmax, noise_on, noise_std, nkey, k);
            const float thr_k = thr[k];
            cr |= (r < thr_k);
            dc |= (r < dthr[k]);
            const float m = r - thr_k;
            mg = m < mg ? m : mg;
            rng[k] = r;                                                              // (for the ratio: read back by this thread)
            scan_q[k] = r;
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
                const double ratio = nv::discomfort_ratio((double)rng[k], thr[k], dthr[k]);
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
            int done = o.done, trunc = 0;
            if (c.max_episode_steps > 0) {                                           // the step's phase 4
                trunc = !o.done && (int)(st.steps[e] + 1) >= c.max_episode_steps;
                if (trunc) done = 1;
            }
            a.out.reward[row + q] = o.reward;
            a.out.done[row + q] = (uint8_t)done;
            a.out.truncated[row + q] = (uint8_t)trunc;
            a.out.is_success[row + q] = o.success;
            a.out.is_crash[row + q] = o.crash;
            a.out.discomfort[row + q] = (uint8_t)(discomfort && !crash);
            a.out.distance[row + q] = o.distance;
            a.out.margin[row + q] = margin;
        }
    }

    // ---- rules 6 - 7: the row's pose (reverted behind a crash, env.py:707-717), tail and goals as phase 6 writes them -- all
    // candidates at once, candidate k on lane k of wavefront 1 (K wrap_pi cost what one does; inside the loop, on thread 0,
    // its float64 atan2 was the kernel's register high-water mark).  The votes stay in LookCand: the last candidate's were
    // complete at its vote barrier, and nobody writes them afterwards; is_crash is the vote's bit 0 (nv::reward_scalar).
    if (wave == 1 && lane < K) {
        const LookCand& cd = cand[lane];
        const bool crashed = (cd.vote & 1) != 0;
        const double tx = crashed ? pv_g[0] : cd.rp[0], ty = crashed ? pv_g[1] : cd.rp[1];
        const double yaw = nv::wrap_pi(crashed ? pv_g[2] : cd.rp[2]);                // env.py:454
        float t7[7];
        t7[0] = (float)pv_g[0]; t7[1] = (float)pv_g[1];                              // env.py:449-452
        t7[2] = (float)tx; t7[3] = (float)ty;
        t7[4] = (float)pa_g[0]; t7[5] = (float)pa_g[1];
        t7[6] = (float)yaw;
        float* tail = a.out.tail + 7 * (row + lane);
#pragma unroll
        for (int i = 0; i < 7; ++i) tail[i] = t7[i];
        if (a.out.obs) {
            float* const obs_t = a.out.obs + (row + lane) * D + (size_t)S * B;
#pragma unroll
            for (int i = 0; i < 7; ++i) obs_t[i] = t7[i];
        }
        float* gl = a.out.goals + 4 * (row + lane);
        gl[0] = (float)tx; gl[1] = (float)ty; gl[2] = (float)goal_g[0]; gl[3] = (float)goal_g[1];
    }

    // ---- rule 6: the crash re-scan, once per arena and only if a candidate crashed
    int any = 0;
    for (int q = 0; q < K; ++q) any |= cand[q].vote;
    if (__builtin_amdgcn_readfirstlane(any) & 1) {
        const float lx = (float)pv_g[0], ly = (float)pv_g[1], lth = (float)pv_g[2];
        int i0, j0;
        nv::xy_to_ij_f32(lx, ly, c, i0, j0);
        i0 = __builtin_amdgcn_readfirstlane(i0); j0 = __builtin_amdgcn_readfirstlane(j0);
        double sT, cT;
        nv::sincos((double)lth, sT, cT);
        lookobs_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, pr, nseg, ndisc, lx, ly, lth, i0, j0, cT, sT, step, rcull, max_range,
                                               &rescan_chunk, dir, rng);
        const uint64_t nkey2 = noise_key(1);                                         // the re-scan's key: step_key + 1
        for (int k = tid; k < B; k += BLOCK) {
            const float r = lookobs_finish(rng[k], rmax, noise_on, noise_std, nkey2, k);
            for (int q = 0; q < K; ++q)
                if (__builtin_amdgcn_readfirstlane(cand[q].vote) & 1) a.out.scan[(row + q) * B + k] = r;
        }
    }

    // ---- rule 8: the full rows, from the scan rows as they now stand.  Thread tid reads back the beams tid + i * 256 it stored
    // itself (a thread sees its own stores: no fence, no barrier), so the candidate loop carries no row pointers -- with them it
    // held 83 vector registers, 5 waves per SIMD.  Slot j < S - 1 takes the scan where S - 1 - j > n_hist, i.e. the first n_fill
    // slots; the others are obs_prev's slots j + 1 (the host refuses out.obs without obs_prev / n_hist when S > 1).
    if (a.out.obs) {
        const float* const prev_e = S > 1 ? a.obs_prev + (size_t)e * D : nullptr;
        int n_fill = 0;
        if (S > 1) { n_fill = S - 1 - st.n_hist[e]; n_fill = n_fill < 0 ? 0 : (n_fill > S - 1 ? S - 1 : n_fill); }
        n_fill = __builtin_amdgcn_readfirstlane(n_fill);
        for (int q = 0; q < K; ++q) {
            const float* const scan_q = a.out.scan + (row + q) * B;
            float* const obs_q = a.out.obs + (row + q) * D;
            for (int k = tid; k < B; k += BLOCK) {
                const float r = scan_q[k];
                obs_q[(size_t)(S - 1) * B + k] = r;
                for (int j = 0; j < n_fill; ++j) obs_q[(size_t)j * B + k] = r;
                for (int j = n_fill; j < S - 1; ++j) obs_q[(size_t)j * B + k] = prev_e[(size_t)(j + 1) * B + k];   // env.py:267-274
            }
        }
    }
}
