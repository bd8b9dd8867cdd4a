// kernels_lookahead_obs.hpp -- lookahead observations (include/navsim.h navsim_lookahead_obs): the WHOLE return of navsim_step for
// each of K candidate actions of an arena -- observation row, goals, reward, done, truncated, flags -- from the current state,
// which is only read, with the scan noise the step itself would draw.  Part of the single translation unit navsim_kernels.hip
// (included inside its anonymous namespace, behind kernels_lookahead.hpp, whose LookCand and lookahead_part_a it uses; the replayed
// pieces of the step -- scan, verdict, reward, LDS layout -- are kernels_replay.hpp's).
//
// lookahead_kernel's shape: one workgroup of kLookaheadBlock threads per arena; part A (pedestrians at t + 1 on wavefront 0,
// the K candidate poses on wavefront 1) is that kernel's lookahead_part_a; part B runs the candidates one behind the other with
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
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms under __launch_bounds__(256, 6): 76 - 78 VGPRs,
// 106 SGPRs, occupancy 6 waves per SIMD, scratch 0 bytes per lane, no VGPR spill; 186 - 214 SGPRs spilled to VGPR lanes
// (lookahead_kernel: 104 - 135), 112 bytes of static LDS; the dynamic LDS is lookahead_lds_bytes (12 bytes a beam, 56 a
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
    const ReplayLds l = replay_lds_carve(dyn, c, (size_t)K * sizeof(LookCand));
    LookCand* cand = (LookCand*)l.own;
    float* const rng = l.rng;

    int n = 0;                                                                       // rule 2
    if (c.ped_model != NAVSIM_PED_NONE) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const double* pa_g = st.prev_action + 2 * (size_t)e;
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);
    if (tid == 0) { prim_count[0] = 0; prim_count[1] = 0; rescan_chunk = 0; a.out.status[e] = 1; }

    lookahead_part_a(c, st, field, e, n, K, l, cand, prim_count, a.actions + 2 * row, a.ped_cmd, a.out.pose + 3 * row);
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
        // (info[] and rng[]: their last readers of candidate q - 1 lie in front of that candidate's vote or ratio barrier)
        replay_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, l.pr, nseg, ndisc, cd.sp, step, rcull, max_range, &cd.next_chunk,
                                              l.dir, rng);
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
        const BeamVerdict v = replay_verdict<BLOCK, false>(B, cr, dc, mg, &cd.vote, wave_margin[par], wave_ratio[par], rng, thr, dthr, rmax);
        if (tid == 0) {
            const StepVerdict r = replay_reward(c, pv_g, cd.sp.p, pa_g, goal_g, v, (long long)(int)(st.steps[e] + 1));
            a.out.reward[row + q] = r.o.reward;
            a.out.done[row + q] = (uint8_t)r.done;
            a.out.truncated[row + q] = (uint8_t)r.truncated;
            a.out.is_success[row + q] = r.o.success;
            a.out.is_crash[row + q] = r.o.crash;
            a.out.discomfort[row + q] = (uint8_t)(v.discomfort && !v.crash);
            a.out.distance[row + q] = r.o.distance;
            a.out.margin[row + q] = v.margin;
        }
    }

    // ---- rules 6 - 7: the row's pose (reverted behind a crash, env.py:707-717), tail and goals as phase 6 writes them -- all
    // candidates at once, candidate k on lane k of wavefront 1 (K wrap_pi cost what one does; inside the loop, on thread 0,
    // its float64 atan2 was the kernel's register high-water mark).  The votes stay in LookCand: the last candidate's were
    // complete at its vote barrier, and nobody writes them afterwards; is_crash is the vote's bit 0 (nv::reward_scalar).
    if (wave == 1 && lane < K) {
        const LookCand& cd = cand[lane];
        const bool crashed = (cd.vote & 1) != 0;
        const double tx = crashed ? pv_g[0] : cd.sp.p[0], ty = crashed ? pv_g[1] : cd.sp.p[1];
        const double yaw = nv::wrap_pi(crashed ? pv_g[2] : cd.sp.p[2]);              // env.py:454
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
        ScanPose sp;                                                                 // (registers: every thread computes it)
        scan_pose_set(sp, c, pv_g[0], pv_g[1], pv_g[2]);
        replay_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, l.pr, nseg, ndisc, sp, step, rcull, max_range, &rescan_chunk, l.dir, rng);
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
