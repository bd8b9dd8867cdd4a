// kernels_rollout_obs.hpp -- rollout observations (include/navsim.h navsim_rollout_obs): the WHOLE return of the next H navsim_step
// calls -- observation row, goals, reward, pose, outcome -- if an arena executed the action sequence a_0 .. a_{H-1}, for K sequences
// per arena, from the current state, which is only read, with the scan noise each of those steps would draw.  Part of the single
// translation unit navsim_kernels.hip (included inside its anonymous namespace, behind kernels_lookahead_obs.hpp and
// kernels_rollout.hpp: lookobs_finish, RollShared's carry and rollout_advance are theirs; the re-scan, the verdict and the reward are
// kernels_replay.hpp's).
//
// rollout_kernel's shape: one workgroup of kRolloutBlock threads per (arena, sequence), the carry of its header (the robot in
// static LDS, pedestrian i in the registers of lane i of wavefront 0), its steps (1) - (4) through rollout_advance at the step's own
// march limit (range_max).  What is new here:
//   the finish pass -- ONE pass over the beams per step reads the merged range from LDS, clips it, adds the noise of the h-th
//     future step (the stream of step_key_h = episode << 32 | (steps + 1 + h) * 2; steps and episode are the state's: no carried
//     value enters the key but h), takes the flags and the margin from the NOISY value as the step does, keeps it in LDS for the
//     discomfort ratio and writes the step's row: the newest slot, the slots the stack fill takes and the shifted older slots;
//   WHERE THE S - 1 OLDER SCANS LIVE -- in global memory, in the rows the same threads stored: thread tid owns the beams
//     tid + i * 256 of every slot of every row of its sequence, so it reads back what it wrote itself (a thread sees its own
//     stores: no fence, no barrier) and the kernel needs no LDS ring (4 (S - 1) bytes a beam would be 13 KB at 1081 beams and a
//     stack of 4, as much again as dir / rng).  The working row is obs_last[e,k]: step h shifts it IN PLACE -- slot j takes the
//     thread's own slot j + 1, j ascending, each slot read before it is written -- from obs_prev[e] at h = 0.  With obs_all every
//     element is also stored to row h of it; that row is never read back.  When the loop ends, obs_last holds the row of the
//     last evaluated step with nothing copied;
//   the crash re-scan -- BEHIND the horizon loop, at most once per sequence: a crash ends the sequence, so the pedestrians of
//     t + h + 1 still stand in LDS when the loop is left.  replay_scan from the carried prev_pose, the key step_key_h + 1; each
//     thread overwrites its beams of the newest slot and of the filled slots, in obs_last and in row h of obs_all;
//   tail and goals -- behind the loop, all steps at once, step h on lane h of wavefront 1, from the poses and actions the loop
//     left in static LDS (5 doubles a step), as lookahead_obs_kernel does for its candidates: the float64 atan2 of wrap_pi stays
//     out of the loop.  The carried prev_pose yaw, wrap_pi(pose yaw) (kernels_step.hpp phase 6), is needed only there and for
//     the re-scan's lidar pose.
// Barriers per step: rollout_kernel's.  The re-scan adds four or five per sequence.
//
// Dynamic LDS (rollout_lds_bytes): rollout_kernel's, 12 B per beam and the pedestrians' share.  Static LDS: RollObsShared
// (1.5 KB) + the wavefronts' minima.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms under __launch_bounds__(256, 3): 167 VGPRs in
// every one, 106 SGPRs, 144 - 166 SGPRs spilled to VGPR lanes, 2 VGPRs spilled, scratch 12 bytes per lane, occupancy 3 waves per
// SIMD (rollout_kernel's), 1488 bytes of static LDS.  Without the second bound (NAVSIM_ROLLOUT_OBS_WAVES=2) the compiler settles
// on 170 VGPRs, two above what three waves allow: no VGPR spill, scratch 0, 146 - 157 spilled SGPRs, occupancy 2.  rollout_kernel
// holds 168.  Both forms were measured, alternating in one call (profiles/r27_rollout_obs/summary.txt): (K, H) = (16, 8) on
// the c3-shaped world takes 22.4 ms bounded against 30.9 ms unbounded -- the march is bound by the latency of its dependent
// loads, the time follows the resident waves, and the two spilled registers do not show.  Where the spill sits was not looked up.
// Tried and not taken: tail and goals on thread 0 inside the loop (lookahead_obs_kernel's first form; its float64 atan2 was
// that kernel's register high-water mark) was not built at all -- the loop only records 5 doubles a step.  Not tried: an LDS
// ring for the older scans, directions by rotation, a bound of four waves (rollout_kernel's spilled 34 VGPRs there).
#ifndef NAVSIM_ROLLOUT_OBS_WAVES
#define NAVSIM_ROLLOUT_OBS_WAVES 3
#endif

struct RolloutObsArgs {
    navsim_rollout_obs_out out;
    const double* actions;
    const double* ped_cmd;
    const float* obs_prev;
    const uint8_t* skip;
    int K, H;
    int noise;                // 1: each step's own draw (host: NAVSIM_LOOKOBS_NOISE_STEP and cfg.add_scan_noise), 0: none
    double gamma;
};
struct RolloutObsKernargs { navsim_config c; navsim_state st; RolloutObsArgs a; };

struct RollObsShared {
    RollShared r;                                    // rollout_kernel's carry and per-step values
    double hp[NAVSIM_ROLLOUT_MAX_H][3];              // pose[e,k,h] as the loop computed it
    double hact[NAVSIM_ROLLOUT_MAX_H][2];            // the action of step h as the step stores it
    int crashed;                                     // the last evaluated step crashed
};

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kRolloutBlock, NAVSIM_ROLLOUT_OBS_WAVES) void rollout_obs_kernel(navsim_config c_, navsim_state st_, RolloutObsArgs a_) {
    NAVSIM_KERNARGS(RolloutObsKernargs, c_, st_, a_);
    const navsim_config& c = ka.c; const navsim_state& st = ka.st; const RolloutObsArgs& a = ka.a;
    constexpr int BLOCK = kRolloutBlock, WAVES = BLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ RollObsShared so;
    __shared__ double wave_ratio[WAVES];
    __shared__ float wave_margin[WAVES];
    RollShared& sh = so.r;
    const int K = a.K, HZ = a.H;
    const int e = (int)(blockIdx.x / (unsigned)K), kseq = (int)(blockIdx.x % (unsigned)K);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = c.max_peds, B = c.n_beams, S = c.n_scan_stack, H = c.map_h, W = c.map_w;
    const size_t D = (size_t)S * B + 7;
    const size_t sq = (size_t)e * K + kseq;                      // row of [E,K]
    const size_t row = sq * (size_t)HZ;                          // first row of [E,K,H]
    float* const last = a.out.obs_last + sq * D;
    if (a.skip && a.skip[e]) {                                                       // rule 1: a skipped arena
        for (int h = tid; h < HZ; h += BLOCK) {
            a.out.reward[row + h] = 0.0;
            a.out.pose[3 * (row + h)] = 0.0; a.out.pose[3 * (row + h) + 1] = 0.0; a.out.pose[3 * (row + h) + 2] = 0.0;
        }
        for (size_t i = tid; i < D; i += BLOCK) last[i] = 0.0f;
        if (a.out.obs_all) {
            for (size_t i = tid; i < (size_t)HZ * D; i += BLOCK) a.out.obs_all[row * D + i] = 0.0f;
            for (int i = tid; i < HZ * 4; i += BLOCK) a.out.goals_all[row * 4 + i] = 0.0f;
        }
        if (tid < 4) a.out.goals_last[4 * sq + tid] = 0.0f;
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

    // ---- the carried values at h = 0: the state's (rollout_kernel's)
    const bool is_ped = wave == 0 && tid < n;
    CarriedPed cp;
    if (is_ped) carried_ped_load<true>(cp, c, st, (size_t)e * N + tid, c.ped_model == NAVSIM_PED_SFM, true, a.ped_cmd);
    if (tid == 64) {
        rollout_carry_load(sh, st, e);
        so.crashed = 0;
        if (kseq == 0) a.out.status[e] = 1;
    }
    __syncthreads();

    const double step = nv::linspace_step(c);
    const float rmax = (float)c.range_max;
    const float rcull = prim_cull_range(c.range_max);
    const float max_range = march_limit(H, W, c.range_max, c.resolution);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const float* thr = st.scan_threshold;
    const float* dthr = st.scan_discomfort;
    const double goal[2] = {st.robot_goal[2 * (size_t)e], st.robot_goal[2 * (size_t)e + 1]};
    // rule 2's noise: one value per arena each, made scalars (lookahead_obs_kernel's)
    const float noise_std = a.noise ? uniform_f32(st.scan_noise_std[e]) : 0.0f;
    const bool noise_on = noise_std > 0.0f;
    const uint64_t genv = (uint64_t)(c.env_index_base + e);
    auto noise_key = [&](int h, unsigned long long add) -> uint64_t {                // the stream of step_key_h + add
        if (!noise_on) return 0;
        const unsigned long long key = (unsigned long long)st.episode[e] * 0x100000000ULL +
                                       (unsigned long long)(st.steps[e] + 1 + h) * 2ULL + add;
        return uniform_u64(nv::noise_stream(c.seed, genv, key));
    };
    // rule 4's stack: n_hist as the step's phase 6 carries it; the first n_fill slots of a row take its newest scan
    int n_hist = 0;
    if (S > 1) { n_hist = st.n_hist[e]; n_hist = n_hist < 0 ? 0 : (n_hist > S - 1 ? S - 1 : n_hist); }
    n_hist = __builtin_amdgcn_readfirstlane(n_hist);
    const float* const prev_e = S > 1 ? a.obs_prev + (size_t)e * D : nullptr;

    // thread 0: what the sequence accumulates
    double ret = 0.0, g = 1.0, distance = 0.0;
    float min_margin = INFINITY;
    int dsteps = 0, exact = HZ, outcome = 0;

    for (int h = 0; h < HZ; ++h) {
        // ---- (1) - (4): the scan of step h (rollout_kernel's rollout_advance); thread 64 keeps the pose and the action for the tail
        rollout_advance<BLOCK, Field, RULE, RECT>(c, st, field, rects, l, sh, cp, n, is_ped, a.actions + 2 * (row + h),
                                                  a.out.pose + 3 * (row + h), so.hp[h], so.hact[h], h, HZ, exact, step, rcull, max_range);
        // ---- (5) rules 2 and 4: clip, noise, flags and margin in one pass; the row of step h from the same register
        const uint64_t nkey = noise_key(h, 0);
        const int n_fill = S - 1 - n_hist;                                       // (0 .. S - 1: n_hist lies in 0 .. S - 1)
        const float* const src = h == 0 ? prev_e : last;
        float* const all_h = a.out.obs_all ? a.out.obs_all + (row + h) * D : nullptr;
        int cr = 0, dc = 0;
        float mg = INFINITY;
        for (int k = tid; k < B; k += BLOCK) {
            const float r = lookobs_finish(rng[k], rmax, noise_on, noise_std, nkey, k);
            const float thr_k = thr[k];
            cr |= (r < thr_k);
            dc |= (r < dthr[k]);
            const float m = r - thr_k;
            mg = m < mg ? m : mg;
            rng[k] = r;                                                          // (for the ratio: read back by this thread)
            for (int j = 0; j < S - 1; ++j) {                                    // env.py:257-279; in place: slot j + 1 is read first
                const float v = j < n_fill ? r : src[(size_t)(j + 1) * B + k];
                last[(size_t)j * B + k] = v;
                if (all_h) all_h[(size_t)j * B + k] = v;
            }
            last[(size_t)(S - 1) * B + k] = r;
            if (all_h) all_h[(size_t)(S - 1) * B + k] = r;
        }
        const BeamVerdict v = replay_verdict<BLOCK, false>(B, cr, dc, mg, &sh.vote, wave_margin, wave_ratio, rng, thr, dthr, rmax);
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
            // the carry (navsim_rollout's rule 2): what phase 6 of the step stores when the episode goes on
            sh.rp[0] = sh.sp.p[0]; sh.rp[1] = sh.sp.p[1]; sh.rp[2] = sh.sp.p[2];
            sh.prev_xy[0] = sh.sp.p[0]; sh.prev_xy[1] = sh.sp.p[1];
            sh.prev_act[0] = sh.act[0]; sh.prev_act[1] = sh.act[1];
            sh.steps = steps_now;
            sh.length = h + 1;
            sh.stop = r.done;
            so.crashed = r.o.crash != 0.0f;
        }
        __syncthreads();
        if (sh.stop) break;                                                          // nothing behind a done step
        n_hist = n_hist + 1 < S - 1 ? n_hist + 1 : S - 1;                            // phase 6 of the step
    }
    // (n_hist is now the last evaluated step's: the loop was left in front of its update, or length == HZ and it is unused)
    const int length = sh.length;
    const int hl = length - 1;                                                       // the last evaluated step
    const bool crashed = so.crashed != 0;
    const double* pv_g = st.prev_pose + 3 * (size_t)e;
    const double* pa_g = st.prev_action + 2 * (size_t)e;

    // ---- rules 3 and 4: row pose, tail and goals of every evaluated step at once, step h on lane h of wavefront 1.  prev_pose
    // and prev_action of step h are what step h - 1 left: its pose with the yaw wrapped, its action
    if (wave == 1 && lane < length) {
        const int h = lane, hm = h > 0 ? h - 1 : 0;
        const double px = h > 0 ? so.hp[hm][0] : pv_g[0], py = h > 0 ? so.hp[hm][1] : pv_g[1];
        const double pth_w = nv::wrap_pi(so.hp[hm][2]);
        const double pth = h > 0 ? pth_w : pv_g[2];
        const double pa0 = h > 0 ? so.hact[hm][0] : pa_g[0], pa1 = h > 0 ? so.hact[hm][1] : pa_g[1];
        const bool rev = crashed && h == hl;                                         // env.py:707-717
        const double tx = rev ? px : so.hp[h][0], ty = rev ? py : so.hp[h][1];
        const double yaw = nv::wrap_pi(rev ? pth : so.hp[h][2]);                     // env.py:454
        float t7[7];
        t7[0] = (float)px; t7[1] = (float)py;                                        // env.py:449-452
        t7[2] = (float)tx; t7[3] = (float)ty;
        t7[4] = (float)pa0; t7[5] = (float)pa1;
        t7[6] = (float)yaw;
        const float g4[4] = {(float)tx, (float)ty, (float)goal[0], (float)goal[1]};
        if (a.out.obs_all) {
            float* const tail = a.out.obs_all + (row + h) * D + (size_t)S * B;
#pragma unroll
            for (int i = 0; i < 7; ++i) tail[i] = t7[i];
            float* const gl = a.out.goals_all + 4 * (row + h);
#pragma unroll
            for (int i = 0; i < 4; ++i) gl[i] = g4[i];
        }
        if (h == hl) {
            float* const tail = last + (size_t)S * B;
#pragma unroll
            for (int i = 0; i < 7; ++i) tail[i] = t7[i];
            float* const gl = a.out.goals_last + 4 * sq;
#pragma unroll
            for (int i = 0; i < 4; ++i) gl[i] = g4[i];
        }
        if (rev) {                                                                   // the re-scan's lidar pose: the carried prev_pose
            scan_pose_set(sh.sp, c, px, py, pth);
            sh.next_chunk = 0;
        }
    }

    // ---- rule 3: the crash re-scan, from the carried prev_pose, the sequence's own pedestrians of t + hl + 1 (still in LDS)
    if (crashed) {
        __syncthreads();
        replay_scan<BLOCK, Field, RULE, RECT>(c, st, field, rects, l.pr, sh.nseg, sh.ndisc, sh.sp, step, rcull, max_range, &sh.next_chunk,
                                              l.dir, rng);
        const uint64_t nkey2 = noise_key(hl, 1);                                     // the re-scan's key: step_key_h + 1
        const int n_fill = S - 1 - n_hist;
        float* const all_h = a.out.obs_all ? a.out.obs_all + (row + hl) * D : nullptr;
        for (int k = tid; k < B; k += BLOCK) {
            const float r = lookobs_finish(rng[k], rmax, noise_on, noise_std, nkey2, k);
            for (int j = 0; j < n_fill; ++j) {
                last[(size_t)j * B + k] = r;
                if (all_h) all_h[(size_t)j * B + k] = r;
            }
            last[(size_t)(S - 1) * B + k] = r;
            if (all_h) all_h[(size_t)(S - 1) * B + k] = r;
        }
    }

    // ---- rows behind the sequence's last evaluated step
    for (int h = length + tid; h < HZ; h += BLOCK) {
        a.out.reward[row + h] = 0.0;
        a.out.pose[3 * (row + h)] = 0.0; a.out.pose[3 * (row + h) + 1] = 0.0; a.out.pose[3 * (row + h) + 2] = 0.0;
    }
    if (a.out.obs_all) {
        for (size_t i = (size_t)length * D + tid; i < (size_t)HZ * D; i += BLOCK) a.out.obs_all[row * D + i] = 0.0f;
        for (int i = length * 4 + tid; i < HZ * 4; i += BLOCK) a.out.goals_all[row * 4 + i] = 0.0f;
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
