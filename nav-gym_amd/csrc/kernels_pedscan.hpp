// kernels_pedscan.hpp -- pedestrian scans, beam table, device-math test hook, gather microbenchmark.
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace;
// not a standalone header).

// ============================================================================================
// env.py:685-693: the 512-beam half-plane scan of every pedestrian (what the reference feeds to
// HumanPolicy).  One workgroup per (pedestrian, arena): rectangles of the other agents in LDS,
// march from the pedestrian's integer cell, bearing-culled polygon merge, clip to 6 m.
// ============================================================================================
// The scan of pedestrian i of arena e (n live pedestrians) by its BLOCK-thread workgroup, into rng[0 .. PB) of the
// dynamic LDS region `dyn` (ped_scan_lds_bytes below: float2 dir[PB], float rng[PB], then the rectangle sides of the other agents and
// their beam-index intervals (prim_in_range), sized by cfg.max_peds): merged, NOT yet clipped.  Ends with a barrier.
// tab (optional): cos / sin of the robot-frame beam angles -- the beam direction by beam_dir_fast (one float64 angle
// addition whose float32 rounding is proven per beam), else the full sincos; identical results.
struct PedScanShared { double cT, sT; int nseg, i0, j0; float lx, ly, lth; };
// Host side of that region, in the order of the four pointers ped_scan_core derives: dir (8 B per beam) and rng (4 B per
// beam), rounded up to 16 B; seg, four sides x 16 B, and info_s, four intervals x 8 B, per other agent (the others + the robot).
inline size_t ped_scan_lds_bytes(const navsim_config* c) {
    const size_t beams = (size_t)c->ped_n_beams * (sizeof(float2) + sizeof(float));
    return ((beams + 15) & ~(size_t)15) + (size_t)(c->max_peds + 1) * (4 * 16 + 4 * 8);
}
template <typename Field, int BLOCK, int RULE, bool RECT>
__device__ __forceinline__ void ped_scan_core(const navsim_config& c, const navsim_state& st, int e, int i, int n,
                                                const double* __restrict__ tab, char* dyn, PedScanShared& ss) {
    int& nseg_s = ss.nseg; int& i0_s = ss.i0; int& j0_s = ss.j0;
    float& lx_s = ss.lx; float& ly_s = ss.ly; float& lth_s = ss.lth;
    double& cT_s = ss.cT; double& sT_s = ss.sT;
    const int tid = threadIdx.x;
    const int N = c.max_peds, PB = c.ped_n_beams, H = c.map_h, W = c.map_w;
    float2* dir = (float2*)dyn;
    float* rng = (float*)(dyn + sizeof(float2) * (size_t)PB);
    float (*seg)[4] = (float(*)[4])(dyn + ((12 * (size_t)PB + 15) & ~(size_t)15));
    float* info_s = (float*)(seg + 4 * (N + 1));
    if (tid == 0) {
        nseg_s = 0;
        const double* pp = st.ped_pose + ((size_t)e * N + i) * 3;
        lx_s = (float)pp[0]; ly_s = (float)pp[1]; lth_s = (float)pp[2];              // env.py:386
        nv::xy_to_ij_f32(lx_s, ly_s, c, i0_s, j0_s);                                 // env.py:419
        if (tab) { double sn, cs; nv::sincos((double)lth_s, sn, cs); cT_s = cs; sT_s = sn; }
    }
    __syncthreads();
    if (tid <= n && tid != i) {                                                      // env.py:404-414
        const int a = tid;
        const double* pose = (a < n) ? st.ped_pose + ((size_t)e * N + a) * 3 : st.robot_pose + 3 * (size_t)e;
        const double hfx[4] = {0.22, -0.22, -0.22, 0.22}, hfy[4] = {0.19, 0.19, -0.19, -0.19};   // human.py:5-10
        double s, cs;
        nv::sincos(pose[2], s, cs);
        float vx[4], vy[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            double x = (a < n) ? hfx[v] : c.robot_seen_footprint[2 * v];
            double y = (a < n) ? hfy[v] : c.robot_seen_footprint[2 * v + 1];
            vx[v] = (float)((cs * x - s * y) + pose[0]);
            vy[v] = (float)((s * x + cs * y) + pose[1]);
        }
        int q = atomicAdd(&nseg_s, 4);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            int w = (v + 1) & 3;
            seg[q + v][0] = vx[v]; seg[q + v][1] = vy[v]; seg[q + v][2] = vx[w]; seg[q + v][3] = vy[w];
        }
    }
    __syncthreads();                                                                 // seg[] and nseg_s: written by threads <= n, read by all
    const Prims pr = {seg, nullptr, info_s};
    const double step = (PB > 1) ? (c.ped_angle_last - c.ped_angle_min) / (double)(PB - 1) : 0.0;
    const float rmax = (float)c.ped_range_max;
    // which sides can matter, for which beams: needs only the sides and the lidar pose, so it runs before the march and
    // the barrier behind the march publishes info_s
    prim_in_range<BLOCK>(nseg_s, nseg_s, lx_s, ly_s, rmax * 1.0001f + 0.01f, pr, (float)step,
                         (float)(c.ped_angle_min + (double)lth_s));
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4)
                             : nullptr;
    const unsigned tpr = (unsigned)((W + 7) >> kRectShift);
    const float max_range = march_limit(H, W, c.ped_range_max, c.resolution);
    const float res = (float)c.resolution;
    const float x0 = (float)i0_s, y0 = (float)j0_s;
    const double lth = (double)lth_s;
    for (int k = tid; k < PB; k += block_threads<BLOCK>()) {
        const double lin = ped_beam_angle(c, k);
        float heading = (float)(lin + lth);
        float dx, dy;
        bool fast = false;
        if (tab) {
            const double2 cs = ((const double2*)tab)[k];
            fast = beam_dir_fast(lin, lth, cs.x, cs.y, cT_s, sT_s, heading, dx, dy);
        }
        if (!fast) nv::beam_dir(heading, dx, dy);
#ifdef NAVSIM_DIAG_PED_CHEAP_DIR   // diagnostic build only (wrong directions): what does the exact direction cost?
        dx = __cosf(heading); dy = __sinf(heading);
#endif
        dir[k] = make_float2(dx, dy);
        float t = 0.0f;
        lanemask_t active = mask_of(true), hit = 0;
        while (active != 0)
            probe_round<Field, RULE, RECT>(field, rects, tpr, x0, y0, dx, dy, (unsigned)W, (unsigned)H, max_range, t, active, hit);
        rng[k] = ray_result<RULE>(hit, int_range_ok(H, W), i0_s, j0_s, x0, y0, dx, dy, t, max_range) * res;
    }
    __syncthreads();
    merge_prims_culled_core<BLOCK>(PB, lx_s, ly_s, (float)step, nseg_s, 0, pr, dir, rng);
    __syncthreads();
}

template <typename Field, int BLOCK, int RULE, bool RECT>
__global__ __launch_bounds__(BLOCK) void ped_scan_kernel(navsim_config c, navsim_state st, float* __restrict__ out, int e0) {
    // the compiled maximum of 64 pedestrians cost 6 KB per workgroup and, with 512 beams, two of the CU's 16 workgroups:
    // the region is sized by cfg.max_peds
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int e = e0 + (int)blockIdx.y, i = blockIdx.x, tid = threadIdx.x;      // (e0: navsim_ped_scans_part)
    const int N = c.max_peds, PB = c.ped_n_beams;
    int n = st.n_peds[e];
    n = n > N ? N : n;
    if (i >= n) return;
    __shared__ PedScanShared ss;
    ped_scan_core<Field, BLOCK, RULE, RECT>(c, st, e, i, n, nullptr, dyn, ss);
    const float* rng = (const float*)(dyn + sizeof(float2) * (size_t)PB);
    const float rmax = (float)c.ped_range_max;
    float* row = out + ((size_t)e * N + i) * PB;
    for (int k = tid; k < PB; k += BLOCK) {
        float r = rng[k];
        r = r < 0.0f ? 0.0f : r;
        r = r > rmax ? rmax : r;
        row[k] = r;
    }
}

// env.py:685-693 + 629-630, 647 + human_policy.py:38-42 in ONE workgroup per pedestrian (round 4, verdict item 7): the scan
// stays in LDS, is clipped and scaled in place and feeds conv1 / conv2; the latency-bound march of one workgroup runs beside
// the FMA-bound convolutions of its CU's other workgroups.  The scan's LDS region is reused by conv1's output.  scans_out
// (optional): the clipped scan rows [E, N, 512], what navsim_ped_scans writes.  A dead slot writes nothing (its features
// stay whatever the scratch held: policy_head_kernel never reads a dead slot's result).  Same functions, same order as
// ped_scan_kernel -> policy_features_kernel: bit-identical.
template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(256) void ped_scan_features_kernel(navsim_config c, navsim_state st, int p0, int n_ped,
                                                                const double* __restrict__ tab, float* __restrict__ scans_out,
                                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                                const float* __restrict__ w2t, const float* __restrict__ b2,
                                                                float* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];      // max(scan region, o1[kConvCh][258])
    __shared__ float x[520];
    const int tid = threadIdx.x, p = blockIdx.x;
    if (p >= n_ped) return;
    const int N = c.max_peds;
    const size_t q = (size_t)p0 + p;
    const int e = (int)(q / N), i = (int)(q - (size_t)e * N);
    int n = st.n_peds[e];
    n = n > N ? N : n;
    if (i >= n) return;
    __shared__ PedScanShared ss;
    // BLOCK = 0 (threads read from the launch): the 256-thread instantiation of the scan crashes this compiler's inliner
    ped_scan_core<Field, 0, RULE, RECT>(c, st, e, i, n, tab, dyn, ss);
    const float* rng = (const float*)(dyn + sizeof(float2) * 512);
    const float rmax = (float)c.ped_range_max;
    float* row = scans_out ? scans_out + q * 512 : nullptr;
    for (int k = tid; k < 512; k += 256) {
        float r = rng[k];
        r = r < 0.0f ? 0.0f : r;
        r = r > rmax ? rmax : r;
        if (row) row[k] = r;
        x[1 + k] = policy_input(r);
    }
    __syncthreads();                                                // rng is dead: conv1 writes over it
    policy_conv(x, (float(*)[258])dyn, w1, b1, w2t, b2, feat + (size_t)p * kPolFeat);
}

// ============================================================================================
// CrowdSim-v0 (crowd_sim.py:808-949; oracle navsim_crowd_check_cpu): one wavefront per env.  Lanes take the
// agents (closest approach over the step, wave min / any) and then the cells of the two occupancy-grid
// windows around the robot's next position; lane 0 runs the reward / info cascade.  float64, Python order.
// ============================================================================================
__device__ __forceinline__ double crowd_p2s(double x1, double y1, double x2, double y2, double x3, double y3) {
    double px = x2 - x1, py = y2 - y1;                          // crowd_sim/envs/utils/utils.py:4-26
    if (px == 0.0 && py == 0.0) { double a = x3 - x1, b = y3 - y1; return sqrt(a * a + b * b); }
    double u = ((x3 - x1) * px + (y3 - y1) * py) / (px * px + py * py);
    if (u > 1.0) u = 1.0; else if (u < 0.0) u = 0.0;
    double x = x1 + u * px, y = y1 + u * py;
    double a = x - x3, b = y - y3;
    return sqrt(a * a + b * b);
}

__device__ __forceinline__ bool crowd_window_hits(const uint8_t* __restrict__ m, int G, int n_cells, int ix, int iy,
                                                  int half, int lane) {
    int sx = ix - half, ex = sx + half * 2, sy = iy - half, ey = sy + half * 2;   // crowd_sim.py:843-861
    sx = sx < 0 ? 0 : sx; ex = ex > n_cells ? n_cells : ex;
    sy = sy < 0 ? 0 : sy; ey = ey > n_cells ? n_cells : ey;
    bool hit = false;
    if (ex > sx && ey > sy) {
        const int w = ey - sy, cells = (ex - sx) * w;
        for (int k = lane; k < cells; k += 64) {
            int x = sx + k / w, y = sy + k % w;
            if (x < G && y < G && !m[(size_t)x * G + y]) hit = true;
        }
    }
    return __ballot(hit) != 0;
}

__global__ __launch_bounds__(64) void crowd_check_kernel(navsim_crowd_params p, int max_agents, int grid,
                                                         const uint8_t* __restrict__ free_map,
                                                         const double* __restrict__ robot,
                                                         const double* __restrict__ agents,
                                                         const int32_t* __restrict__ n_agents,
                                                         const double* __restrict__ global_time,
                                                         double* __restrict__ reward, uint8_t* __restrict__ done,
                                                         int32_t* __restrict__ info, double* __restrict__ min_dist) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const double* r = robot + (size_t)e * 10;
    const double radius = r[8];
    int na = n_agents ? n_agents[e] : max_agents;
    na = na > max_agents ? max_agents : na;
    double dmin = INFINITY;
    bool coll = false;
    for (int a = lane; a < na; a += 64) {                           // crowd_sim.py:808-826
        const double* g = agents + ((size_t)e * max_agents + a) * 5;
        double px = g[0] - r[0], py = g[1] - r[1];
        double vx = g[2] - r[4], vy = g[3] - r[5];
        double ex = px + vx * p.time_step, ey = py + vy * p.time_step;
        double closest = crowd_p2s(px, py, ex, ey, 0.0, 0.0) - g[4] - radius;
        if (closest < 0.0) coll = true;
        else if (closest < dmin) dmin = closest;
    }
    for (int off = 32; off > 0; off >>= 1) {                        // exact: min of float64 values
        double o = __shfl_xor(dmin, off);
        dmin = o < dmin ? o : dmin;
    }
    bool collision = __ballot(coll) != 0;
    const int n_cells = (int)__builtin_rint(p.map_size_m / p.map_resolution);
    const uint8_t* m = free_map + (size_t)e * grid * grid;
    const int ix = (int)__builtin_rint((r[2] + p.map_size_m / 2.0) / p.map_resolution);   // int(round(.)): half to even
    const int iy = (int)__builtin_rint((r[3] + p.map_size_m / 2.0) / p.map_resolution);
    const int half = (int)ceil(radius / sqrt(2.0) / p.map_resolution);
    if (crowd_window_hits(m, grid, n_cells, ix, iy, half, lane)) collision = true;
    const int half2 = (int)ceil((radius + p.discomfort_dist) / p.map_resolution);
    const bool close_to_obstacle = crowd_window_hits(m, grid, n_cells, ix, iy, half2, lane);
    if (lane != 0) return;
    double gx = r[2] - r[6], gy = r[3] - r[7];
    const bool reaching_goal = sqrt(gx * gx + gy * gy) < radius;
    double rew, md = INFINITY;
    int dn, code;
    if (global_time[e] >= p.time_limit) { rew = p.timeout_penalty; dn = 1; code = NAVSIM_CROWD_TIMEOUT; }
    else if (reaching_goal) { rew = p.success_reward; dn = 1; code = NAVSIM_CROWD_REACH_GOAL; }
    else if (collision) { rew = p.collision_penalty; dn = 1; code = NAVSIM_CROWD_COLLISION; }
    else if (close_to_obstacle) { rew = -p.discomfort_penalty_factor * p.time_step * 0.1; dn = 0; code = NAVSIM_CROWD_DANGER; md = 0.1; }
    else if (dmin < p.discomfort_dist) { rew = (dmin - p.discomfort_dist) * p.discomfort_penalty_factor * p.time_step; dn = 0; code = NAVSIM_CROWD_DANGER; md = dmin; }
    else if (fabs(r[9]) > 0.0) { rew = fabs(r[9]) * p.rotation_penalty_factor; dn = 0; code = NAVSIM_CROWD_NOTHING; }
    else { rew = 0.0; dn = 0; code = NAVSIM_CROWD_NOTHING; }
    reward[e] = rew; done[e] = (uint8_t)dn; info[e] = code;
    if (min_dist) min_dist[e] = md;
}

__global__ __launch_bounds__(256) void beam_table_kernel(navsim_config c, double* __restrict__ tab) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c.n_beams) return;
    double s, cs;
    nv::sincos(nv::linspace_k(c, k, nv::linspace_step(c)), s, cs);
    tab[2 * k] = cs;
    tab[2 * k + 1] = s;
}

// test hook: the deterministic math on device
__global__ void math_kernel(int fn, const double* x, const double* x2, double* out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    switch (fn) {
        case 0: nv::sincos(x[i], s, c); out[i] = s; break;
        case 1: nv::sincos(x[i], s, c); out[i] = c; break;
        case 2: out[i] = nv::atan2_(x[i], x2 ? x2[i] : 1.0); break;
        case 3: out[i] = nv::exp_neg(x[i]); break;
        case 4: out[i] = nv::wrap_pi(x[i]); break;
        case 5: out[i] = nv::mod_2pi(x[i]); break;
        case 6: out[i] = (double)nv::sqrt_small_int((float)x[i]); break;
        case 7: out[i] = (double)__builtin_amdgcn_sqrtf((float)x[i]); break;        // raw v_sqrt_f32 (diagnostic)
        case 8: out[i] = (double)sqrtf((float)x[i]); break;                          // compiler's IEEE sqrtf
        case 9: {                                                                     // rsq + one residual step (diagnostic)
            const float xf = (float)x[i];
            const float y = __builtin_amdgcn_rsqf(xf);
            float sq = xf * y;
            const float r = __builtin_fmaf(-sq, sq, xf);
            sq = __builtin_fmaf(r * 0.5f, y, sq);
            out[i] = (double)(xf == 0.0f ? 0.0f : sq);
            break;
        }
        case 11: out[i] = (double)march_step<NAVSIM_MARCH_F64>(nv::sqrt_small_int((float)x[i])); break;
        case 12: out[i] = (double)march_step<kMarchF64Exact32>(nv::sqrt_small_int((float)x[i])); break;
        case 10: {                                                                    // v_sqrt + one residual step via rcp-free half
            const float xf = (float)x[i];
            float sq = __builtin_amdgcn_sqrtf(xf);
            const float y = __builtin_amdgcn_rsqf(xf);
            const float r = __builtin_fmaf(-sq, sq, xf);
            sq = __builtin_fmaf(r * 0.5f, y, sq);
            out[i] = (double)(xf == 0.0f ? 0.0f : sq);
            break;
        }
        case 13: {
            // the beam-table fast path against the full evaluation: x = robot heading (rounded to float32 as
            // env.py:386 does), x2 = robot-frame beam angle.  0: proven and equal, 1: not proven (the scan would
            // evaluate beam_dir), 2: proven but DIFFERENT (must never happen)
            const double lth = (double)(float)x[i], lin = x2 ? x2[i] : 0.0;
            double st, ct, sT, cT;
            nv::sincos(lin, st, ct);
            nv::sincos(lth, sT, cT);
            float heading, dx, dy, rx, ry;
            const bool fast = beam_dir_fast(lin, lth, ct, st, cT, sT, heading, dx, dy);
            nv::beam_dir(heading, rx, ry);
            out[i] = !fast ? 1.0 : ((__float_as_uint(dx) == __float_as_uint(rx) && __float_as_uint(dy) == __float_as_uint(ry)) ? 0.0 : 2.0);
            break;
        }
        case 15: {
            // the scan's integer hit range (kernels_step.hpp ray_result) against the float32 sqrtf form it replaced, for the
            // offset (ix, iy) = (i % 2895 - 1447, i / 2895 - 1447) of a hit cell from the origin: every offset a map of at most
            // kIntRangeMaxSide cells a side can produce.  out = 0 when bit-identical, else 1
            const int ix = i % 2895 - 1447, iy = i / 2895 - 1447;
            const float xd = (float)ix, yd = (float)iy;
            out[i] = (__float_as_uint(hit_range_int(ix, iy)) == __float_as_uint(sqrtf(xd * xd + yd * yd))) ? 0.0 : 1.0;
            break;
        }
        case 16: {
            // gauss_noise's two float32 pieces against the forms they replaced (navsim_device.hpp), for m = i in [0, 2^24):
            // logf of u1 = (m + 1) 2^-24 by nv::log_normal against the compiler's __logf, and the angle m * (6.28318530718f * 2^-24)
            // against 6.28318530718f * (m * 2^-24).  out = 0 when both are bit-identical, else 1
            const float u1 = ((float)(unsigned)i + 1.0f) * (1.0f / 16777216.0f), u2 = (float)(unsigned)i * (1.0f / 16777216.0f);
            const bool log_eq = __float_as_uint(nv::log_normal(u1)) == __float_as_uint(__logf(u1));
            const bool ang_eq = __float_as_uint((float)(unsigned)i * (6.28318530718f / 16777216.0f)) == __float_as_uint(6.28318530718f * u2);
            out[i] = (log_eq && ang_eq) ? 0.0 : 1.0;
            break;
        }
        case 14: {
            // sfm_pair's antisymmetry, on which the fused step's half pair table rests (ped_pair_term stores the term of an
            // unordered pedestrian pair once and ped_sfm_step SUBTRACTS it for the second reader): the force on j from i must
            // be minus the force on i from j BIT FOR BIT.  x[i] seeds two agents (positions within a few metres, velocities
            // below 1.5 m/s, some coincident or at rest); out = 0 when both components are exact negatives, else 1.
            // A future anisotropic or field-of-view term breaks this loudly here instead of silently for the partner j < i.
            navsim_config c = {};
            c.sfm_lambda = 2.0; c.sfm_gamma = 0.35; c.sfm_n = 2.0; c.sfm_n_prime = 3.0;
            uint64_t h = nv::mix64((uint64_t)__double_as_longlong(x[i]) + 0x9E3779B97F4A7C15ULL * (uint64_t)(i + 1));
            auto u = [&]() { h = nv::mix64(h + 0x632BE59BD9B4E019ULL); return (double)(h >> 11) * (1.0 / 9007199254740992.0); };
            double xi = 10.0 + 6.0 * u(), yi = 10.0 + 6.0 * u(), xj = 10.0 + 6.0 * u(), yj = 10.0 + 6.0 * u();
            double vxi = 3.0 * u() - 1.5, vyi = 3.0 * u() - 1.5, vxj = 3.0 * u() - 1.5, vyj = 3.0 * u() - 1.5;
            const double pick = u();
            if (pick < 0.02) { xj = xi; yj = yi; }                          // coincident agents
            else if (pick < 0.06) { vxi = vyi = vxj = vyj = 0.0; }          // both at rest
            else if (pick < 0.10) { vxj = vxi; vyj = vyi; }                 // equal velocities
            double fx, fy, gx, gy;
            sfm_pair(c, xi, yi, vxi, vyi, xj, yj, vxj, vyj, fx, fy);
            sfm_pair(c, xj, yj, vxj, vyj, xi, yi, vxi, vyi, gx, gy);
            // by VALUE: a skipped pair is (+0, +0) in both orders, and the reader's `sum -= +0` equals the oracle's
            // `sum += +0` (the running sum starts at +0 and never becomes -0); every other value is equal iff bit-equal
            const bool ok = fx == -gx && fy == -gy;
            out[i] = ok ? 0.0 : 1.0;
            break;
        }
        case 17: {
            // nv::gauss_noise alone (tests/scan_noise_f64.py is its float64 model): the stream's low word in x, its high word
            // in x2 (absent: 0), both whole numbers below 2^32; the beam is the element's index
            const uint64_t lo = (uint64_t)(uint32_t)x[i], hi = x2 ? (uint64_t)(uint32_t)x2[i] : 0ull;
            out[i] = (double)nv::gauss_noise(lo | (hi << 32), (uint32_t)i);
            break;
        }
        default: out[i] = 0.0;
    }
}

__global__ __launch_bounds__(256) void xy_to_ij_kernel(navsim_config c, const double* __restrict__ xy, int as_f32,
                                                       int32_t* __restrict__ ij, int n) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int i, j;
    if (as_f32) nv::xy_to_ij_f32((float)xy[2 * t], (float)xy[2 * t + 1], c, i, j);
    else        nv::xy_to_ij(xy[2 * t], xy[2 * t + 1], c, i, j);
    ij[2 * t] = i; ij[2 * t + 1] = j;
}

// microbenchmark (profiles/gather_granularity.py): random 4-byte gathers over a large buffer.
// mode 0: one load per thread; 1: + the neighbour in the same 64-B sector; 2: + the word 64 B away
// in the same 128-B line; 3: + a second independent random word.
__global__ __launch_bounds__(256) void gather_probe_kernel(const float* __restrict__ x, uint64_t n_words,
                                                           int mode, int iters, uint64_t seed,
                                                           float* __restrict__ out) {
    uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float acc = 0.0f;
    for (int it = 0; it < iters; ++it) {
        uint64_t h = nv::mix64(seed + gid * 0x9E3779B97F4A7C15ULL + (uint64_t)it);
        uint64_t i = h % n_words;
        acc += x[i];
        if (mode == 1) acc += x[i ^ 1];
        if (mode == 2) acc += x[i ^ 16];
        if (mode == 3) acc += x[nv::mix64(h) % n_words];
    }
    out[gid] = acc;
}

thread_local hipError_t g_last_hip_error = hipSuccess;
inline int launch_status() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return NAVSIM_OK;
    g_last_hip_error = e;
    return NAVSIM_E_LAUNCH;
}
