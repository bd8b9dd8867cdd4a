// kernels_mppi.hpp -- MPPI local planner (include/navsim.h navsim_mppi): per arena a plan of H actions, K perturbed copies of it,
// their outcomes from navsim_rollout's own launch, and the importance-weighted mean as the new plan.
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace; not a standalone header): the
// goal-field walk is kernels_goal_path.hpp's goal_walk / goal_distance, the launch between the two kernels kernels_rollout.hpp's.
//
// Per iteration THREE launches: mppi_sample_kernel, rollout_kernel (launch_rollout, unchanged), mppi_update_kernel.
//   mppi_sample_kernel: a workgroup per arena, a thread per (k, c) -- 2 K threads rounded up to wavefronts, at most 512.  In the
//     call's first iteration thread 0 compares plan_key with (episode, steps) and records it (rule 2); the first 2 H threads
//     apply the decision through LDS (read, barrier, write: the shift moves the plan in place).  Every thread then walks h --
//     the AR(1) chain is serial in h -- and stores its component of actions[e,k,h]: the two threads of a sequence fill 16
//     consecutive bytes per h, a sequence's rows are contiguous.  The plan is read from LDS.
//   mppi_update_kernel: a workgroup of 256 threads per arena.
//     cost: without a goal field a lane per k.  With one, EIGHT lanes per k (goal_walk's shape: lane j of a group looks at
//       neighbour j), 32 sequences per pass, K / 32 passes; a walk is at most lookahead_cells / 5 hops of uint16 loads.
//     thread 0 scans J for jmin and best (K <= 256 values in LDS, in k's order); a lane per k writes the weights to LDS;
//     a lane per (h, c) -- at most 64, wavefront 0 -- runs the k loop for m and S in the stated order and stores the plan;
//     thread 64 (wavefront 1) runs S and Q beside them and writes the arena's row of `out`.
//   The sums are sequential in k BY SPECIFICATION (rule 7): 256 dependent float64 adds per lane at K = 256, beside a rollout
//   launch of milliseconds.
// Arguments: ONE block of its own (MppiArgs: the call's structs and what the kernels read of cfg and the state), as
// goal_field_kernel has it -- navsim_config / navsim_state do not ride in the kernarg segment.  No atomics.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): mppi_sample_kernel 26 VGPRs, 52 SGPRs, 520 bytes of static LDS, 8 waves
// per SIMD; mppi_update_kernel (FieldF32 / FieldU16T / FieldU16TN) 44 / 46 / 44 VGPRs, 103 / 105 / 103 SGPRs, 5136 bytes of static
// LDS, 7 waves per SIMD; no spill and no scratch in either.
// Measured (profiles/r24_mppi/summary.txt; 4096 arenas x 1081 beams): sample 21 - 24 us, update 49 - 90 us at K = 32 / 64 beside a
// rollout launch of 28.9 - 78.6 ms -- 0.03 - 0.22 % of a call's kernel time.
#pragma once

struct MppiArgs {
    navsim_mppi_params p;
    navsim_mppi_ws ws;
    navsim_mppi_out out;
    const uint8_t* skip;
    // navsim_state's
    const int64_t* episode; const int64_t* steps; const double* robot_goal;
    const void* field; const float* overflow; const int32_t* map_slot;
    const uint16_t* goal_dist;           // navsim_goal_field.dist, or NULL: the straight-line distance
    // navsim_config's
    uint64_t seed;
    double origin_x, origin_y, resolution;
    int env_index_base, map_h, map_w, shared_field;
    // the goal path's
    float hard;                          // cells: (float)(hard_clearance / resolution)
    int lookahead_cells, Hc, Wc;
    int it, last;                        // the iteration of this launch; 1: the call's last iteration (rule 8)
};

constexpr int kMppiUpdateBlock = 256;    // >= NAVSIM_ROLLOUT_MAX_K: a lane per k
constexpr int kMppiSampleMax = 2 * NAVSIM_ROLLOUT_MAX_K;

__device__ __forceinline__ double mppi_clamp(double v, double lo, double hi) {       // min(max(v, lo), hi)
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

__global__ __launch_bounds__(kMppiSampleMax) void mppi_sample_kernel(MppiArgs a) {
    __shared__ double s_plan[2 * NAVSIM_ROLLOUT_MAX_H];
    __shared__ int s_mode;
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int K = a.p.n_samples, H = a.p.horizon, n = 2 * H;
    double* actions = a.ws.actions + (size_t)e * K * n;
    if (a.skip && a.skip[e]) {                                                       // rule 1
        if (a.it == 0)
            for (int i = tid; i < K * n; i += (int)blockDim.x) actions[i] = 0.0;
        return;
    }
    double* plan = a.ws.plan + (size_t)e * n;
    const int64_t ep = a.episode[e], s = a.steps[e];
    if (a.it == 0) {                                                                 // rule 2
        if (tid == 0) {
            int64_t* key = a.ws.plan_key + 2 * (size_t)e;
            const int64_t k0 = key[0], k1 = key[1];
            s_mode = (k0 == ep && k1 == s) ? 0 : ((k0 == ep && k1 == s - 1) ? 1 : 2);
            key[0] = ep; key[1] = s;
        }
        __syncthreads();
        const int mode = s_mode;
        if (tid < n) {
            const int src = (mode == 1 && tid + 2 < n) ? tid + 2 : tid;
            s_plan[tid] = mode == 2 ? ((tid & 1) ? a.p.init_action[1] : a.p.init_action[0]) : plan[src];
        }
        __syncthreads();
        if (tid < n && mode != 0) plan[tid] = s_plan[tid];
    } else {
        if (tid < n) s_plan[tid] = plan[tid];
        __syncthreads();
    }
    if (tid >= 2 * K) return;
    // ---- rule 4: sequence k, component c
    const int k = tid >> 1, c = tid & 1;
    const double lo = c ? a.p.lo[1] : a.p.lo[0], hi = c ? a.p.hi[1] : a.p.hi[0], sigma = c ? a.p.sigma[1] : a.p.sigma[0];
    const double beta = a.p.beta, alpha = a.p.alpha;
    const bool plain = k == 0, stop = a.p.stop_sample != 0 && K >= 2 && k == 1;
    const uint64_t genv = (uint64_t)(a.env_index_base + e);
    const uint64_t key = ((uint64_t)ep << 32) + ((uint64_t)s << 3) + (uint64_t)a.it;
    const uint64_t stream = nv::hash4(a.seed ^ key, genv, key, 0x6D707069ULL + ((uint64_t)k << 32));
    double* row = actions + (size_t)k * n + c;
    double eps = 0.0;
    for (int h = 0; h < H; ++h) {
        double v;
        if (stop) {
            v = 0.0;
        } else if (plain) {
            v = s_plan[2 * h + c];
        } else {
            const double g = (double)nv::gauss_noise(stream, (uint32_t)(2 * h + c));
            eps = h == 0 ? g : beta * eps + alpha * g;
            v = s_plan[2 * h + c] + sigma * eps;
        }
        row[2 * h] = mppi_clamp(v, lo, hi);
    }
}

template <typename Field>
__global__ __launch_bounds__(kMppiUpdateBlock) void mppi_update_kernel(MppiArgs a) {
    __shared__ double s_J[kMppiUpdateBlock], s_w[kMppiUpdateBlock];
    __shared__ int s_crash[kMppiUpdateBlock];
    __shared__ double s_jmin;
    __shared__ int s_best, s_all;
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    const int K = a.p.n_samples, H = a.p.horizon, n = 2 * H;
    const size_t sq0 = (size_t)e * K;
    if (a.skip && a.skip[e]) {                                                       // rule 1
        for (int k = tid; k < K; k += kMppiUpdateBlock) a.ws.cost[sq0 + k] = 0.0;
        if (tid == 0) {
            a.out.action[2 * (size_t)e] = 0.0; a.out.action[2 * (size_t)e + 1] = 0.0;
            a.out.best[e] = 0; a.out.cost_best[e] = 0.0; a.out.ess[e] = 0.0; a.out.status[e] = 0;
        }
        return;
    }
    const navsim_rollout_out& r = a.ws.roll;
    // ---- rule 6: J_k into LDS and ws->cost
    auto finish = [&](int k, double D) {
        const int crash = (r.outcome[sq0 + k] & 2) != 0;
        double J = a.p.w_goal * D - r.ret[sq0 + k];
        if (crash) J = J + a.p.w_crash;
        a.ws.cost[sq0 + k] = J;
        s_J[k] = J; s_crash[k] = crash;
    };
    if (a.goal_dist) {
        const int Hc = a.Hc, Wc = a.Wc;
        const int ms = a.shared_field ? 0 : (a.map_slot ? a.map_slot[e] : e);       // map_slot_of
        const Field field(a.field, a.overflow, ms, a.map_h, a.map_w);
        const uint16_t* dist = a.goal_dist + (size_t)e * Hc * Wc;
        const double gx = a.robot_goal[2 * (size_t)e], gy = a.robot_goal[2 * (size_t)e + 1];
        const float ox = (float)a.origin_x, oy = (float)a.origin_y, res = (float)a.resolution;
        for (int base = 0; base < K; base += kMppiUpdateBlock / 8) {               // workgroup-uniform
            const int k = base + (tid >> 3);
            const bool active = k < K;
            double x = 0.0, y = 0.0;
            if (active) {
                int L = r.length[sq0 + k];
                L = L < 1 ? 1 : (L > H ? H : L);                                     // (the rollout writes 1 .. H)
                const double* pose = r.pose + 3 * ((sq0 + k) * (size_t)H + (size_t)(L - 1));
                x = pose[0]; y = pose[1];
            }
            int ci, cj, gi, gj;
            unsigned dcur;
            bool off;
            goal_walk(field, dist, Hc, Wc, a.hard, a.lookahead_cells, ox, oy, res, a.map_h, a.map_w, lane, active, x, y, gx, gy,
                      ci, cj, gi, gj, dcur, off);
            if (active && (tid & 7) == 0) {
                const bool reached = !off && ci == gi && cj == gj;
                double dx, dy;
                double D = (double)goal_distance(a.origin_x, a.origin_y, a.resolution, off, reached, ci, cj, dcur, x, y, gx, gy, dx, dy);
                if (off) D = D + a.p.off_field_cost;
                finish(k, D);
            }
        }
    } else {
        for (int k = tid; k < K; k += kMppiUpdateBlock) finish(k, r.distance[sq0 + k]);
    }
    __syncthreads();
    // ---- rule 7: jmin and best, in k's order
    if (tid == 0) {
        double jmin = s_J[0], bj = s_J[0];
        int best = 0, bc = s_crash[0], all = s_crash[0];
        for (int k = 1; k < K; ++k) {
            const double J = s_J[k];
            const int cr = s_crash[k];
            if (J < jmin) jmin = J;
            if (cr < bc || (cr == bc && J < bj)) { best = k; bc = cr; bj = J; }
            all &= cr;
        }
        s_jmin = jmin; s_best = best; s_all = all;
    }
    __syncthreads();
    if (tid < K) s_w[tid] = nv::exp_neg(-((s_J[tid] - s_jmin) / a.p.lambda));
    __syncthreads();
    const double* actions = a.ws.actions + sq0 * (size_t)n;
    if (tid < n) {                                                                   // a lane per (h, c)
        const int c = tid & 1;
        double m = 0.0, S = 0.0;
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const double w = s_w[k];
            S = S + w;
            m = m + w * actions[(size_t)k * n + tid];
        }
        const double v = mppi_clamp(m / S, c ? a.p.lo[1] : a.p.lo[0], c ? a.p.hi[1] : a.p.hi[0]);
        a.ws.plan[(size_t)e * n + tid] = v;
        if (a.last && a.p.select == 0 && tid < 2) a.out.action[2 * (size_t)e + tid] = v;
    }
    if (tid == 64 && a.last) {                                                       // rule 8
        double S = 0.0, Q = 0.0;
        for (int k = 0; k < K; ++k) {
            const double w = s_w[k];
            S = S + w;
            Q = Q + w * w;
        }
        const int best = s_best;
        if (a.p.select != 0) {
            a.out.action[2 * (size_t)e] = actions[(size_t)best * n];
            a.out.action[2 * (size_t)e + 1] = actions[(size_t)best * n + 1];
        }
        a.out.best[e] = best;
        a.out.cost_best[e] = s_J[best];
        a.out.ess[e] = S * S / Q;
        a.out.status[e] = (uint8_t)(s_all ? NAVSIM_MPPI_ALL_CRASH : NAVSIM_MPPI_OK);
    }
}
