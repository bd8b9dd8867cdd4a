// kernels_rollout.hpp -- action-sequence rollout (include/navsim.h navsim_rollout): what the next H navsim_step calls would return
// if an arena executed the action sequence a_0 .. a_{H-1}, for K sequences per arena, from the current state, which is only read.
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace; not a standalone header).
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
// A step h, seven barriers with pedestrians under the social force, four without pedestrians (+ 1 with a discomfort ratio):
//   (1) wavefront 0: waypoint pop from the carried head, the agents of time t staged in LDS (ped_stage_wave's body on the carried
//       values); thread 64 (wavefront 1, lane 0): the step's phase 0 on actions[e,k,h] from the carried pose, operation for
//       operation as lookahead_kernel's part A -- the new pose, its float32 lidar pose, sincos and origin cell.  Barrier.
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
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the eleven forms: 164 VGPRs in every one, 106 SGPRs, 117 - 132
// SGPRs spilled to VGPR lanes, no VGPR spill, scratch 0 bytes per lane, occupancy 3 waves per SIMD (three workgroups a compute
// unit; LDS would allow eight), 208 bytes of static LDS.  lookahead_kernel, with the same device functions outside any loop,
// needs 78: the registers are this kernel's open item, and where they go is NOT found.  Three forms were compiled and not taken:
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
    double np[3];            // the pose the step scans from (rule 3 of the lookahead)
    double act[2];           // the action as the step stores it
    double cT, sT;           // cos / sin of (double)(float)np[2] for the beam-table fast path
    int i0, j0;              // integer ray origin (env.py:419)
    int next_chunk;          // next 64-beam chunk to hand to a wavefront
    int vote;                // crash (bit 0) and discomfort (bit 1) ORed over the wavefronts
    int nseg, ndisc;         // the lidar's primitives of this step
    int stop;                // the sequence ended at this step
    int length;              // steps evaluated so far
};

// Dynamic LDS of one (arena, sequence), in the order rollout_kernel carves it
inline size_t rollout_lds_bytes(const navsim_config* c) {
    size_t n = lookahead_align16((size_t)c->n_beams * (sizeof(float2) + sizeof(float)));
    if (c->ped_model != NAVSIM_PED_NONE) n += lookahead_align16(ped_lds_bytes(c->max_peds)) + ped_pair_bytes(c->max_peds);
    return n;
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    float2* dir = (float2*)dyn;
    float* rng = (float*)(dyn + sizeof(float2) * (size_t)B);
    char* behind = dyn + lookahead_align16((size_t)B * (sizeof(float2) + sizeof(float)));
    const bool ped_model = c.ped_model != NAVSIM_PED_NONE;
    const bool sfm = c.ped_model == NAVSIM_PED_SFM;
    PedShared ps = {};
    double2* pair = nullptr;
    if (ped_model) {
        ps = ped_lds_carve(behind, N);
        pair = (double2*)(behind + lookahead_align16(ped_lds_bytes(N)));
    }
    const Prims pr = {ps.seg, ps.disc, ps.info};

    int n = 0;
    if (ped_model) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const double dt = c.time_step;
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);

    // ---- the carried values at h = 0: the state's
    // wavefront 0: pedestrian i on lane i (N <= 64)
    const bool is_ped = wave == 0 && tid < n;
    const size_t pq = (size_t)e * N + (is_ped ? tid : 0);
    double pp[3] = {0.0, 0.0, 0.0}, pvel[2] = {0.0, 0.0}, pdist[3] = {0.0, 0.0, 0.0}, pyaw = 0.0, vpref = 0.0;
    int head = 0, nw = 1;
    bool legged = false;
    const double* wp = nullptr;
    const double* cmd = nullptr;
    if (is_ped) {
        pp[0] = st.ped_pose[pq * 3]; pp[1] = st.ped_pose[pq * 3 + 1]; pp[2] = st.ped_pose[pq * 3 + 2];
        pvel[0] = st.ped_vel[pq * 2]; pvel[1] = st.ped_vel[pq * 2 + 1];
        pdist[0] = st.ped_dist[pq * 3]; pdist[1] = st.ped_dist[pq * 3 + 1]; pdist[2] = st.ped_dist[pq * 3 + 2];
        pyaw = st.ped_prev_yaw[pq];
        legged = st.ped_has_legs[pq] && c.lidar_legs;
        if (sfm) {
            wp = st.ped_waypoints + (pq * c.max_waypoints) * 2;
            nw = st.ped_n_waypoints[pq];
            nw = nw < 1 ? 1 : (nw > c.max_waypoints ? c.max_waypoints : nw);         // (a state the step accepts holds 1 .. max_waypoints)
            head = st.ped_wp_head[pq];
            head = head < 0 ? 0 : (head > nw - 1 ? nw - 1 : head);
            vpref = st.ped_v_pref[pq];
        } else {
            cmd = (a.ped_cmd ? a.ped_cmd : st.ped_cmd) + pq * 2;                     // rule 6: held for the whole horizon
        }
    }
    if (tid == 64) {
        const double* rp_g = st.robot_pose + 3 * (size_t)e;
        sh.rp[0] = rp_g[0]; sh.rp[1] = rp_g[1]; sh.rp[2] = rp_g[2];
        sh.prev_xy[0] = st.prev_pose[3 * (size_t)e]; sh.prev_xy[1] = st.prev_pose[3 * (size_t)e + 1];
        sh.prev_act[0] = st.prev_action[2 * (size_t)e]; sh.prev_act[1] = st.prev_action[2 * (size_t)e + 1];
        sh.steps = (long long)st.steps[e];
        sh.nseg = 0; sh.ndisc = 0; sh.stop = 0; sh.length = 0;
        if (kseq == 0) a.out.status[e] = 1;
    }
    __syncthreads();

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
    const double goal[2] = {st.robot_goal[2 * (size_t)e], st.robot_goal[2 * (size_t)e + 1]};
    const int n_terms = n * (n - 1) / 2 + n;

    // thread 0: what the sequence accumulates
    double ret = 0.0, g = 1.0, distance = 0.0;
    float min_margin = INFINITY;
    int dsteps = 0, exact = HZ, outcome = 0;

    for (int h = 0; h < HZ; ++h) {
        // ---- (1) wavefront 0: waypoint pop and staging (ped_stage_wave on the carried values)
        if (wave == 0 && n > 0 && sfm) {
            if (is_ped) {
                head = ped_pop_waypoints(wp, head, nw, pp);
                ps.ax[tid] = pp[0]; ps.ay[tid] = pp[1]; ps.avx[tid] = pvel[0]; ps.avy[tid] = pvel[1];
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
            double a0 = a.actions[2 * (row + h)], a1 = a.actions[2 * (row + h) + 1];
            if (c.action_kind == NAVSIM_ACTION_WHEELS) {
                const double wl = a0, wr = a1;
                a0 = c.wheel_radius * (wl + wr) * 0.5;
                a1 = c.wheel_radius * (wr - wl) / c.wheel_track;
            }
            if (c.clamp_action) {
                a0 = a0 < c.linvel_lo ? c.linvel_lo : (a0 > c.linvel_hi ? c.linvel_hi : a0);
                a1 = a1 < c.rotvel_lo ? c.rotvel_lo : (a1 > c.rotvel_hi ? c.rotvel_hi : a1);
            }
            if (c.min_turning_radius > 0.0) {                                        // env.py:595-600
                const double lim = fabs(a1) * c.min_turning_radius;
                if (a0 >= 0.0) a0 = (a0 > lim) ? a0 : lim;
                else           a0 = (a0 < -lim) ? a0 : -lim;
            }
            const double th_old = sh.rp[2];
            const double th = th_old + a1 * dt;                                      // set_vel's intermediate heading
            double s0, c0, s1, c1;
            nv::sincos(th_old, s0, c0);
            nv::sincos(th, s1, c1);
            double p[3] = {sh.rp[0], sh.rp[1], th_old};                              // env.py:664
            nv::set_vel_with(p, a0, a1, dt, c.axle_offset, s0, c0, s1, c1, nullptr);
            sh.np[0] = p[0]; sh.np[1] = p[1]; sh.np[2] = p[2];
            sh.act[0] = a0; sh.act[1] = a1;
            const float lth = (float)p[2];                                           // env.py:386
            double sT, cT;
            nv::sincos((double)lth, sT, cT);
            sh.cT = cT; sh.sT = sT;
            int i0, j0;
            nv::xy_to_ij_f32((float)p[0], (float)p[1], c, i0, j0);                   // env.py:419
            sh.i0 = i0; sh.j0 = j0;
            sh.next_chunk = 0; sh.vote = 0;
            a.out.pose[3 * (row + h)] = p[0]; a.out.pose[3 * (row + h) + 1] = p[1]; a.out.pose[3 * (row + h) + 2] = p[2];
        }
        __syncthreads();
        // ---- (2) the pair terms, shared out over the workgroup
        if (sfm && n > 0) {
            for (int t = tid; t < n_terms; t += BLOCK) ped_pair_term(c, ps, pair, n, t);
            __syncthreads();
        }
        const float lx = (float)sh.np[0], ly = (float)sh.np[1], lth = (float)sh.np[2];            // env.py:386
        // ---- (3) wavefront 0: the pedestrians at t + 1 and what the lidar sees of them
        if (wave == 0 && n > 0) {
            bool due = false;
            if (is_ped) {
                if (sfm) {
                    ped_sfm_step(c, field, ps, pair, n, tid, vpref, wp + 2 * head, dt, pp, pvel);
                    // the step's predicate for ped_due (ped_finish): the post-move distance to the LAST waypoint under 0.5 m
                    const double ddx = pp[0] - wp[2 * (nw - 1)], ddy = pp[1] - wp[2 * (nw - 1) + 1];
                    due = sqrt(ddx * ddx + ddy * ddy) < 0.5;                         // (nw >= 1: checked where the pedestrian is loaded)
                } else {
                    nv::set_vel(pp, cmd[0], cmd[1], dt, 0.0, pvel);                  // env.py:662
                }
                nv::leg_odometry(pp, pvel, pyaw, dt, pdist);
                pyaw = nv::wrap_pi(pp[2]);
            }
            if (mask_of(due) != 0 && exact == HZ) exact = h + 1;                     // rule 8 (wave-uniform; thread 0 reports it)
            const lanemask_t lm = mask_of(legged);
            const int legs_all = __popcll(lm), legs_below = __popcll(lm & ((1ull << tid) - 1ull));
            const int nseg_w = 4 * (n - legs_all);
            if (tid == 0) { sh.nseg = nseg_w; sh.ndisc = 2 * legs_all; }
            if (is_ped) {                                                            // env.py:392-414
                if (legged) {
                    float cc[4];
                    nv::leg_centres((float)pp[0], (float)pp[1], (float)pp[2], (float)pdist[0], (float)pdist[1], (float)pdist[2], cc);
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
            wave_lds_sync();
            prim_in_range<64>(nseg_w + 2 * legs_all, nseg_w, lx, ly, rcull, pr, (float)step, (float)(c.angle_min + (double)lth));
        }
        // ---- (4) the static ray of every beam under the cap, 64 adjacent beams at a time, handed out as wavefronts finish
        {
            const int i0 = __builtin_amdgcn_readfirstlane(sh.i0), j0 = __builtin_amdgcn_readfirstlane(sh.j0);
            const float x0 = (float)i0, y0 = (float)j0;
            const double cT = sh.cT, sT = sh.sT;
            for (;;) {
                int chunk = 0;
                if (lane == 0) chunk = atomicAdd(&sh.next_chunk, 1);
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
        __syncthreads();
        {
            const int nseg = sh.nseg, ndisc = sh.ndisc;
            if (nseg + ndisc) {
                merge_prims_culled_core<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng);
                __syncthreads();
            }
        }
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
        mg = wave_min_f32(mg);
        int v = (int)(mask_of(cr != 0) != 0) | ((int)(mask_of(dc != 0) != 0) << 1);
        if (lane == 0) {
            if (v != 0) atomicOr(&sh.vote, v);
            wave_margin[wave] = mg;
        }
        __syncthreads();
        v = __builtin_amdgcn_readfirstlane(sh.vote);
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
            if (lane == 0) wave_ratio[wave] = rmin;
            __syncthreads();
        }
        if (tid == 0) {
            float margin = wave_margin[0];
            for (int w = 1; w < WAVES; ++w) margin = wave_margin[w] < margin ? wave_margin[w] : margin;
            if (discomfort && !crash)
                for (int w = 1; w < WAVES; ++w) rmin = wave_ratio[w] < rmin ? wave_ratio[w] : rmin;
            const double prev_xy[2] = {sh.prev_xy[0], sh.prev_xy[1]};
            const double pose[2] = {sh.np[0], sh.np[1]};
            const double vel[2] = {sh.prev_act[0], sh.prev_act[1]};                  // env.py:453: the PREVIOUS action
            const nv::RewardOut o = nv::reward_scalar(c, prev_xy, pose, vel, goal, crash != 0, discomfort != 0, rmin);
            const long long steps_now = sh.steps + 1;                                // env.py:592
            const int limit = !o.done && c.max_episode_steps > 0 && steps_now >= (long long)c.max_episode_steps;
            const int done = o.done || limit;
            a.out.reward[row + h] = o.reward;
            ret = ret + g * o.reward;
            g = g * a.gamma;
            min_margin = margin < min_margin ? margin : min_margin;
            dsteps += (discomfort && !crash) ? 1 : 0;
            distance = o.distance;
            outcome = (o.success != 0.0f ? 1 : 0) | (o.crash != 0.0f ? 2 : 0) | (limit ? 4 : 0);
            // the carry (rule 2): what phase 6 of the step stores when the episode goes on
            sh.rp[0] = sh.np[0]; sh.rp[1] = sh.np[1]; sh.rp[2] = sh.np[2];
            sh.prev_xy[0] = sh.np[0]; sh.prev_xy[1] = sh.np[1];
            sh.prev_act[0] = sh.act[0]; sh.prev_act[1] = sh.act[1];
            sh.steps = steps_now;
            sh.length = h + 1;
            sh.stop = done;
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
