// kernels_dwa.hpp -- local planner (include/navsim.h navsim_dwa): a dynamic-window action per arena -- a window of reachable
// twists, each rolled out with the step's kinematics against the distance field and the pedestrians, the best one returned --
// one launch that reads the state the step left.
// Not a standalone header: a section of navsim_kernels.hip (kernels_field.hpp's fields and map_slot_of).
#pragma once

// ============================================================================================
// One workgroup per arena, a lane per candidate: 64 ceil(C / 64) threads, C = n_v n_w <= 512.
//   A  the workgroup writes the pedestrians' positions of the steps k = 1 .. T to LDS once, thread-strided over (k, pedestrian):
//      pose + vel * ((double)k * dt), the rule's own operations.  Dynamic LDS, T x max_peds x 16 bytes (at most 32 x 64 x 16 =
//      32 KB; none without pedestrians).  One barrier.
//   B  lane c rolls candidate c out: nv::set_vel_with per step, Field::at of every disc's cell straight from global memory (a
//      candidate's discs touch neighbouring cells, a workgroup's candidates fan out from one pose: the lines are shared in L2),
//      the pedestrians of step k by broadcast LDS reads (every lane reads the same address).  The loop over k is wave-uniform and
//      leaves as soon as no candidate of the wavefront is still rolling.
//   C  one reduction over the key (class, value, -c): class 1 = admissible with value = score, class 0 = inadmissible with value =
//      hit; six xor-shuffles inside a wavefront, then the wavefronts' winners through LDS (at most eight) and one barrier; the
//      lane that holds the winner writes the arena's row.
// Less work than the rule's wording, same bits:
//   - sincos(p[2]) after step k is set_vel's own sincos of the old heading in step k + 1 (same argument): evaluated once, two
//     sincos per step instead of three;
//   - a step's static clearance is taken as the minimum over the discs' float32 field values and converted once, its pedestrian
//     clearance as the minimum over squared distances with one sqrt: the widening, the product with resolution > 0, sqrt and the
//     subtraction of a constant are monotone and correctly rounded, so min commutes with them;
//   - the window, the target and d0 are arena-uniform and computed by every lane alike (no LDS round trip).
// The cell of a disc is clamped into the map on both axes (navsim.h step 4): no read leaves the arena's field whatever the pose.
// No private arrays (the pose is three named doubles; set_vel_with's p[3] is taken apart by the compiler), no scratch.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950), FieldF32 / FieldU16T / FieldU16TN alike: 61 VGPRs, 106 SGPRs, no
// scratch, no VGPR spill, 3 / 13 / 5 SGPRs spilled to vector-register lanes (navsim_config and navsim_state ride in scalar
// registers, as in ped_observe_kernel), 128 bytes of static LDS (the wavefronts' winners) + the pedestrians, 7 waves per SIMD.
// ============================================================================================
constexpr int kDwaMaxWaves = 8;          // 16 x 32 candidates

struct DwaArgs {
    navsim_dwa_params p;
    navsim_dwa_out out;
    const float* subgoal;
    const uint8_t* skip;
    int use_peds;                        // p.use_peds && cfg.ped_model != NAVSIM_PED_NONE
};

// is key a (cls, val, c) better than key b?  class first, then the value, then the LOWER candidate index
__device__ __forceinline__ bool dwa_better(int cls_a, double val_a, int c_a, int cls_b, double val_b, int c_b) {
    if (cls_a != cls_b) return cls_a > cls_b;
    if (val_a != val_b) return val_a > val_b;
    return c_a < c_b;
}

template <typename Field>
__global__ __launch_bounds__(64 * kDwaMaxWaves) void dwa_kernel(navsim_config c, navsim_state st, DwaArgs a) {
    extern __shared__ __align__(16) unsigned char dwa_lds[];
    __shared__ double s_val[kDwaMaxWaves];
    __shared__ int s_cls[kDwaMaxWaves], s_idx[kDwaMaxWaves];
    double2* s_ped = (double2*)dwa_lds;                           // [T, N]: the pedestrians' positions at step k
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = (int)(blockDim.x >> 6);
    const int e = blockIdx.x;
    const int n_v = a.p.n_v, n_w = a.p.n_w, C = n_v * n_w, T = a.p.horizon, N = c.max_peds;
    const size_t ee = (size_t)e;
    double* scores = a.out.scores ? a.out.scores + ee * C : nullptr;
    int32_t* first_hit = a.out.first_hit ? a.out.first_hit + ee * C : nullptr;
    if (a.skip && a.skip[e] != 0) {                               // step 1 (workgroup-uniform: ahead of every barrier)
        if (tid < C) {
            if (scores) scores[tid] = 0.0;
            if (first_hit) first_hit[tid] = 0;
        }
        if (tid == 0) {
            a.out.twist[2 * ee] = 0.0; a.out.twist[2 * ee + 1] = 0.0;
            a.out.action[2 * ee] = 0.0; a.out.action[2 * ee + 1] = 0.0;
            a.out.clearance[e] = 0.0f; a.out.best[e] = 0; a.out.status[e] = 0;
        }
        return;
    }
    const double dt = c.time_step;
    // ---- A: the pedestrians of every step
    int n = 0;
    if (a.use_peds) {
        n = st.n_peds[e];
        n = n > N ? N : (n < 0 ? 0 : n);
        int k = tid / N, q = tid - k * N;                         // slot tid, tid + blockDim, ... of [T, N]: (k, q) carried along
        const int dk = (int)blockDim.x / N, dq = (int)blockDim.x - dk * N;
#pragma unroll 1
        for (int slot = tid; slot < T * N; slot += blockDim.x) {
            if (q < n) {
                const size_t g = ee * N + q;
                const double tk = (double)(k + 1) * dt;
                const double px = st.ped_pose[3 * g] + st.ped_vel[2 * g] * tk;
                const double py = st.ped_pose[3 * g + 1] + st.ped_vel[2 * g + 1] * tk;
                s_ped[slot] = make_double2(px, py);
            }
            k += dk; q += dq;
            if (q >= N) { q -= N; k += 1; }
        }
        __syncthreads();
    }
    // ---- steps 2 and 3: the window and the target (arena-uniform)
    const double v0 = st.prev_action[2 * ee], w0 = st.prev_action[2 * ee + 1];
    double vlo = v0 - a.p.acc_lin * dt, vhi = v0 + a.p.acc_lin * dt;
    vlo = vlo > c.linvel_lo ? vlo : c.linvel_lo;
    vhi = vhi < c.linvel_hi ? vhi : c.linvel_hi;
    if (vlo > vhi) {
        const double m = v0 > c.linvel_lo ? v0 : c.linvel_lo;
        vlo = vhi = m < c.linvel_hi ? m : c.linvel_hi;
    }
    double wlo = w0 - a.p.acc_rot * dt, whi = w0 + a.p.acc_rot * dt;
    wlo = wlo > c.rotvel_lo ? wlo : c.rotvel_lo;
    whi = whi < c.rotvel_hi ? whi : c.rotvel_hi;
    if (wlo > whi) {
        const double m = w0 > c.rotvel_lo ? w0 : c.rotvel_lo;
        wlo = whi = m < c.rotvel_hi ? m : c.rotvel_hi;
    }
    const double rx = st.robot_pose[3 * ee], ry = st.robot_pose[3 * ee + 1], th = st.robot_pose[3 * ee + 2];
    double sk, ck;                                                // sincos of the current heading, carried from step to step
    nv::sincos(th, sk, ck);
    double tx = st.robot_goal[2 * ee], ty = st.robot_goal[2 * ee + 1];
    if (a.subgoal) {
        const double sx = (double)a.subgoal[2 * ee], sy = (double)a.subgoal[2 * ee + 1];
        tx = rx + (ck * sx - sk * sy);
        ty = ry + (sk * sx + ck * sy);
    }
    const double dx0 = tx - rx, dy0 = ty - ry;
    const double d0 = sqrt(dx0 * dx0 + dy0 * dy0);
    // ---- B, step 4: candidate c on thread c
    const bool mine = tid < C;
    const int cc = mine ? tid : 0;
    const int iv = cc / n_w, iw = cc - iv * n_w;
    const double v = n_v == 1 ? vhi : vlo + (vhi - vlo) * ((double)iv / (double)(n_v - 1));
    const double w = n_w == 1 ? whi : wlo + (whi - wlo) * ((double)iw / (double)(n_w - 1));
    const Field field(st.field, st.field_overflow, map_slot_of(c, st, e), c.map_h, c.map_w);
    const int n_discs = a.p.n_discs;
    const double pr_sum = a.p.ped_radius + a.p.body_radius;
    double px = rx, py = ry, pth = th;
    double minclr = a.p.clearance_cap;
    int hit = 0;
    bool rolling = mine;
#pragma unroll 1
    for (int k = 1; k <= T; ++k) {                                // wave-uniform
        if (__ballot(rolling) == 0ull) break;
        if (rolling) {
            double s1, c1;
            nv::sincos(pth + w * dt, s1, c1);                     // set_vel's intermediate heading
            double p[3] = {px, py, pth};
            nv::set_vel_with(p, v, w, dt, c.axle_offset, sk, ck, s1, c1, nullptr);
            px = p[0]; py = p[1]; pth = p[2];
            nv::sincos(pth, sk, ck);
            float fmin = 0.0f;
            double d2min = 0.0;
            bool have_ped = false;
            const double2* peds = s_ped + (size_t)(k - 1) * N;
#pragma unroll 1
            for (int j = 0; j < n_discs; ++j) {
                const double off = a.p.body_offset[j];
                const double cx = px + off * ck, cy = py + off * sk;
                int ci, cj;
                nv::xy_to_ij(cx, cy, c, ci, cj);
                ci = ci < c.map_w - 1 ? ci : c.map_w - 1;
                cj = cj < c.map_h - 1 ? cj : c.map_h - 1;
                const float f = field.at(ci, cj);
                fmin = (j == 0 || f < fmin) ? f : fmin;
#pragma unroll 1
                for (int q = 0; q < n; ++q) {
                    const double2 pq = peds[q];
                    const double ex = pq.x - cx, ey = pq.y - cy;
                    const double d2 = ex * ex + ey * ey;
                    d2min = (!have_ped || d2 < d2min) ? d2 : d2min;
                    have_ped = true;
                }
            }
            double clr = (double)fmin * c.resolution - a.p.body_radius;
            if (have_ped) {
                const double cp = sqrt(d2min) - pr_sum;
                clr = cp < clr ? cp : clr;
            }
            if (clr < a.p.margin) { hit = k; rolling = false; }
            else minclr = clr < minclr ? clr : minclr;
        }
    }
    // ---- step 5: the score
    double score = 0.0;
    if (mine && hit == 0) {
        const double gx = tx - px, gy = ty - py;
        const double dT = sqrt(gx * gx + gy * gy);
        const double align = dT > 0.0 ? (ck * gx + sk * gy) / dT : 1.0;
        score = ((a.p.w_progress * (d0 - dT) + a.p.w_heading * align) + a.p.w_clearance * minclr) + a.p.w_speed * v;
    }
    if (mine) {                                                   // step 7
        if (scores) scores[tid] = hit == 0 ? score : -__builtin_inf();
        if (first_hit) first_hit[tid] = hit;
    }
    // ---- C, step 6: the greatest (class, value, -c)
    int cls = mine ? (hit == 0 ? 1 : 0) : -1;
    double val = hit == 0 ? score : (double)hit;
    int idx = tid;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o_cls = __shfl_xor(cls, m), o_idx = __shfl_xor(idx, m);
        const double o_val = __shfl_xor(val, m);
        if (dwa_better(o_cls, o_val, o_idx, cls, val, idx)) { cls = o_cls; val = o_val; idx = o_idx; }
    }
    if (n_waves > 1) {                                            // workgroup-uniform
        if (lane == 0) { s_cls[wave] = cls; s_val[wave] = val; s_idx[wave] = idx; }
        __syncthreads();
        cls = s_cls[0]; val = s_val[0]; idx = s_idx[0];
        for (int q = 1; q < n_waves; ++q) {
            const int o_cls = s_cls[q], o_idx = s_idx[q];
            const double o_val = s_val[q];
            if (dwa_better(o_cls, o_val, o_idx, cls, val, idx)) { cls = o_cls; val = o_val; idx = o_idx; }
        }
    }
    if (tid == idx) {                                             // the winner holds its own twist and clearance
        a.out.twist[2 * ee] = v; a.out.twist[2 * ee + 1] = w;
        double a0 = v, a1 = w;
        if (c.action_kind == NAVSIM_ACTION_WHEELS) {
            a0 = (v - w * c.wheel_track / 2.0) / c.wheel_radius;
            a1 = (v + w * c.wheel_track / 2.0) / c.wheel_radius;
        }
        a.out.action[2 * ee] = a0; a.out.action[2 * ee + 1] = a1;
        a.out.clearance[e] = (float)minclr;
        a.out.best[e] = idx;
        a.out.status[e] = (uint8_t)(cls == 1 ? NAVSIM_DWA_OK : NAVSIM_DWA_BLOCKED);
    }
}
