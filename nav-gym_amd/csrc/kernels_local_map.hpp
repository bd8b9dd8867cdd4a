// kernels_local_map.hpp -- egocentric local map (include/navsim.h navsim_local_map): per arena a G x G grid in the robot's frame
// with the wall clearance, the clearance to the nearest pedestrian and that pedestrian's velocity -- one launch that reads the
// state the step left.
// Not a standalone header: a section of navsim_kernels.hip (kernels_field.hpp's fields and map_slot_of).
#pragma once

// ============================================================================================
// A two-dimensional grid, arena x strip: blockIdx.x is the arena, blockIdx.y a strip of consecutive cells of its grid in
// row-major (r, q) order -- whole rows wherever the row length divides the strip.  A thread owns VEC neighbouring cells of one
// row: VEC = 4 where G % 4 == 0 and `out` is 16-byte aligned (the four cells are one float4 store per channel, 1 KiB per
// wave-instruction on the contiguous q axis), VEC = 1 for every other G (a dword per lane, still contiguous).  The workgroup is
// as large as the arena's items need, 64 .. 256 threads: G = 16 is ONE wavefront per arena, G = 128 is sixteen workgroups of four
// that spread over the compute units.
//   A  the first wavefront stages the arena's pedestrians in LDS once per workgroup, a lane per pedestrian: the count and the
//      visible mask applied by a ballot that COMPACTS the survivors in ascending index (so the first of equal squared
//      distances in the list is the rule's lowest i), the position in the world frame -- the rule takes ex = px - wx there, a
//      rotated position would round differently -- and the velocity already rotated into the robot's frame and narrowed.  One
//      barrier; none with one channel.
//   B  a thread forms its cells' centres (the row's u, c*u and s*u once), reads the field cell of each straight from global
//      memory (a window is a few hundred cells across: the lines stay in L2) and walks the staged pedestrians with broadcast LDS
//      reads, the four cells side by side.
//   C  one store per channel.  The writes are the cost: 4096 arenas x 4 channels x 64 x 64 cells are 268 MB a call.
// Less work than the rule's wording, same bits: the minimum is taken over squared distances and sqrt once (the rule itself
// orders by d2; sqrt, the subtraction of ped_radius and the clamps are monotone and correctly rounded, so the least d2 also has
// the least clearance), and WHICH pedestrian holds it is looked up only in covered cells, the only ones that show it (step 6);
// a cell reads ONE field value, so the wall channel has no minimum to commute with.
// No atomics, no scratch, no inline assembly; the per-cell arrays have constant extents and live in registers.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 7.
// ============================================================================================
constexpr int kLocalMapBlock = 256;

struct LocalMapArgs {
    navsim_local_map_params p;
    const uint8_t* visible;
    const uint8_t* skip;
    float* out;
};

struct LocalMapLds {
    double x[NAVSIM_MAX_PEDS], y[NAVSIM_MAX_PEDS];      // world frame
    float vx[NAVSIM_MAX_PEDS], vy[NAVSIM_MAX_PEDS];     // robot frame
    int n;
};

template <int VEC>
__device__ __forceinline__ void local_map_store(float* o, const float (&v)[VEC]);
template <>
__device__ __forceinline__ void local_map_store<1>(float* o, const float (&v)[1]) { o[0] = v[0]; }
template <>
__device__ __forceinline__ void local_map_store<4>(float* o, const float (&v)[4]) {
    *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
}

template <typename Field, int VEC>
__global__ __launch_bounds__(kLocalMapBlock) void local_map_kernel(navsim_config c, navsim_state st, LocalMapArgs a) {
    __shared__ LocalMapLds s;
    const int tid = threadIdx.x, e = blockIdx.x;
    const int G = a.p.size, C = a.p.channels, cells = G * G, N = c.max_peds;
    const int cell0 = (int)(blockIdx.y * blockDim.x + tid) * VEC;      // < 2 * 128 * 128
    const bool mine = cell0 < cells;
    const size_t ee = (size_t)e;
    float* out = a.out + ee * C * cells + cell0;
    if (a.skip && a.skip[e] != 0) {                               // step 1 (workgroup-uniform: ahead of the barrier)
        if (mine) {
            float zero[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) zero[k] = 0.0f;
            for (int ch = 0; ch < C; ++ch) local_map_store<VEC>(out + (size_t)ch * cells, zero);
        }
        return;
    }
    // ---- step 2: the pose (arena-uniform, every thread alike)
    const double rx = st.robot_pose[3 * ee], ry = st.robot_pose[3 * ee + 1], th = st.robot_pose[3 * ee + 2];
    double sn, cs;
    nv::sincos(th, sn, cs);
    // ---- A: the pedestrians that count, compacted in ascending index
    int n = 0;
    if (C > 1) {                                                  // (workgroup-uniform)
        if (tid < 64) {                                           // (the first wavefront, whole)
            int cnt = st.n_peds[e];
            cnt = cnt > N ? N : cnt;
            bool ok = tid < cnt;
            if (ok && a.visible) ok = a.visible[ee * N + tid] != 0;
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int slot = __popcll(m & ((1ull << tid) - 1ull));
                const size_t g = ee * N + tid;
                s.x[slot] = st.ped_pose[3 * g];
                s.y[slot] = st.ped_pose[3 * g + 1];
                if (C == 4) {
                    const double vx = st.ped_vel[2 * g], vy = st.ped_vel[2 * g + 1];
                    s.vx[slot] = (float)(cs * vx + sn * vy);
                    s.vy[slot] = (float)(cs * vy - sn * vx);
                }
            }
            if (tid == 0) s.n = __popcll(m);
        }
        __syncthreads();
        n = s.n;
    }
    if (!mine) return;
    // ---- B, step 3: the cells' centres
    const int r = cell0 / G, q0 = cell0 - r * G;                  // VEC = 4: G % 4 == 0, the four cells share the row
    const double cell = a.p.cell, half = (double)G * 0.5, cap = a.p.cap;
    const double u = (((double)r + 0.5) - half) * cell + a.p.ahead;
    const double cu = cs * u, su = sn * u;
    double wx[VEC], wy[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const double v = (((double)(q0 + k) + 0.5) - half) * cell;
        wx[k] = rx + (cu - sn * v);
        wy[k] = ry + (su + cs * v);
    }
    // ---- step 4: the wall clearance
    const Field field(st.field, st.field_overflow, map_slot_of(c, st, e), c.map_h, c.map_w);
    const float fw = (float)c.map_w, fh = (float)c.map_h;
    float val[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float fi = (float)((wx[k] - c.origin_x) / c.resolution);    // nv::xy_to_ij's quotients, before its clipping
        const float fj = (float)((wy[k] - c.origin_y) / c.resolution);
        float w = 0.0f;                                           // outside: the world ends in a wall
        if (fi >= 0.0f && fi < fw && fj >= 0.0f && fj < fh) {     // column i < map_w, row j < map_h: no read leaves the field
            const double d = (double)field.at((int)fi, (int)fj) * c.resolution;
            w = (float)(d < cap ? d : cap);
        }
        val[k] = w;
    }
    local_map_store<VEC>(out, val);
    if (C == 1) return;
    // ---- step 5: the nearest pedestrian.  The loop keeps the least d2 alone -- six float64 operations a pedestrian and cell; the
    // index that goes with it is only needed where the pedestrian covers the cell (below)
    double d2m[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) d2m[k] = __builtin_inf();
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const double px = s.x[i], py = s.y[i];                    // broadcast reads
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const double ex = px - wx[k], ey = py - wy[k];
            d2m[k] = __builtin_fmin(d2m[k], ex * ex + ey * ey);
        }
    }
    const double pr = a.p.ped_radius;
    bool covered[VEC], any = false;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const double dist = sqrt(d2m[k]);
        double x = dist - pr;
        x = x > 0.0 ? x : 0.0;
        x = x < cap ? x : cap;
        val[k] = n > 0 ? (float)x : (float)cap;
        covered[k] = n > 0 && dist <= pr;
        any = any || covered[k];
    }
    local_map_store<VEC>(out + (size_t)cells, val);
    if (C != 4) return;
    // ---- step 6: the covering pedestrian's velocity.  Few cells are covered: only their lanes walk the list again, downwards, so
    // that of equal squared distances (the same operations on the same operands: the same bits as above) the lowest index stays
    int im[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) im[k] = 0;
    if (any) {
#pragma unroll 1
        for (int i = n - 1; i >= 0; --i) {
            const double px = s.x[i], py = s.y[i];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double ex = px - wx[k], ey = py - wy[k];
                im[k] = (ex * ex + ey * ey == d2m[k]) ? i : im[k];
            }
        }
    }
    float v2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        val[k] = covered[k] ? s.vx[im[k]] : 0.0f;
        v2[k] = covered[k] ? s.vy[im[k]] : 0.0f;
    }
    local_map_store<VEC>(out + (size_t)2 * cells, val);
    local_map_store<VEC>(out + (size_t)3 * cells, v2);
}
