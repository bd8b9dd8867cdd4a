// kernels_goal_path.hpp -- goal path (include/navsim.h navsim_goal_path): per arena a distance-to-goal field on the 5 x 5-cell
// navigation grid and, read from it, the path distance and a steering sub-goal of the robot -- two launches that read the state
// the step left.
// Not a standalone header: a section of navsim_kernels.hip (kernels_field.hpp's fields and map_slot_of).
#pragma once

// ============================================================================================
// TWO launches per call, whatever the number of arenas that rebuild:
//   1  goal_field_kernel: G = min(E, compute units x workgroups that fit a unit) workgroups of 1024 threads (never fewer than
//      E / 1024).  Workgroup b owns the arenas b, b + G, b + 2 G, ...: its threads test those arenas' keys IN PARALLEL (one arena
//      per thread, the stale ones appended to a list in LDS), so a call that rebuilds nothing costs each workgroup one round of
//      loads and two barriers.  Every listed arena is then rebuilt by the whole workgroup, the grid in LDS:
//        a  classify: thread-strided over the cells of the padded grid, Field::at at the cell's sample -> one byte per cell (0
//           impassable, else the cell's multiplier m; bit 7 marks the goal cell).  The grid carries a one-cell impassable border,
//           so no neighbour access tests a bound.  A thread carries the (row, column) of its cell from one cell to the next:
//           the kernel divides four times, before its loops.
//        b  relax, pull-style: a thread owns one contiguous strip of the (padded) grid in raster order and is the only writer of
//           its cells; a cell takes min over its admissible neighbours of dist[n] + w m, saturated.  Neighbour values may be stale
//           -- they only ever fall, so a stale one is merely too large -- and inside its own strip a thread sees its own writes
//           at once (Gauss-Seidel along the strip).  The raster direction of the strips alternates between sweeps.  A sweep in
//           which no thread changed a cell read nothing but final values: the fixed point, which is the specification's
//           (navsim.h: the equations have one solution).  The "changed" flag is one of THREE LDS words used in turn -- sweep s
//           raises word s mod 3, the barrier, everyone reads it, thread 0 clears word (s + 2) mod 3, which nobody touches again
//           before the next barrier -- so a sweep costs ONE barrier.  Bound: Hc Wc sweeps (a value crosses at least one cell per
//           sweep), never reached.
//           The strip length is 2 x an odd number of cells: the threads of a wavefront then read words an odd number of banks
//           apart -- conflict-free over the 32 lanes a ds_read_u16 serves per cycle.
//        c  copy the interior to field.dist (consecutive threads, consecutive cells: coalesced), record the key, count the rebuild.
//      LDS: 3 bytes per padded cell -- 122.4 KB at 200 x 200 nav cells (1000 x 1000 maps), one workgroup per compute unit there; 31 KB
//      at 100 x 100, two.  Only these G workgroups ever hold that LDS: the arenas that merely look up are served by launch 2, which
//      has none at all.
//   2  goal_query_kernel: EIGHT lanes per arena -- lane k = neighbour k -- eight arenas per wavefront, four wavefronts per
//      workgroup, no LDS and no workgroup barrier.  Per hop each lane loads its neighbour's dist and the field at that
//      neighbour's sample in parallel; one ballot gives every group the passability of its eight neighbours (the no-corner-cutting
//      test of a diagonal reads two bits of it), three xor-shuffles the minimum of (dist + w, k).  The hop loop is wave-uniform
//      with the bound min(lookahead_cells / 5, Hc Wc) and leaves as soon as no group of the wavefront walks.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950), FieldF32 / FieldU16T / FieldU16TN:
//   goal_field_kernel  VGPRs 49 / 47 / 47, SGPRs 92 / 99 / 92, no scratch, no VGPR and no SGPR spill, 4112 bytes of static LDS (the
//                      list) + the grid; 8 waves per SIMD by registers -- the LDS and the 1024-thread workgroup set the occupancy.
//                      The launch reads its OWN argument block (GoalFieldArgs: what it needs of cfg, the state and the call) and
//                      its loops are flat and never unrolled: with navsim_config / navsim_state as parameters, loops nested per row
//                      and column and the compiler's unrolling, the loop-invariant scalars did not fit 102 SGPRs (4 - 17 spilled
//                      to vector-register lanes).
//   goal_query_kernel  VGPRs 45 / 48 / 46, SGPRs 46 / 47 / 45, no scratch, no spill, no LDS, 8 waves per SIMD (its walk is the device
//                      function goal_walk, which kernels_mppi.hpp's update kernel calls too).
// ============================================================================================
constexpr int kGoalBlock = 1024;         // threads of a rebuilding workgroup
constexpr int kGoalWaves = 4;            // wavefronts per workgroup of the query
constexpr unsigned kGoalInf = 0xFFFFu;

struct GoalPathArgs {
    navsim_goal_field field;
    navsim_goal_path_out out;
    const uint8_t* skip;
    float hard;                          // cells: (float)(hard_clearance / resolution)
    int lookahead_cells;
    int Hc, Wc;
};

// the nav cell of a position: the scan-origin cell / 5, clipped into the grid (ic along x = the field's column, jc its row)
// (ox, oy, res = (float)cfg.origin_x, (float)cfg.origin_y, (float)cfg.resolution: nv::xy_to_ij_f32 on its operands)
__device__ __forceinline__ void goal_nav_cell(float x, float y, float ox, float oy, float res, int map_h, int map_w, int Hc, int Wc,
                                              int& ic, int& jc) {
    int i, j;
    nv::xy_to_ij_f32(x, y, ox, oy, res, map_h, map_w, i, j);
    ic = i / 5; jc = j / 5;
    ic = ic < Wc ? ic : Wc - 1;
    jc = jc < Hc ? jc : Hc - 1;
}

// one relaxation of padded cell p (Wp = padded row length); true if the cell fell
__device__ __forceinline__ bool goal_relax(uint16_t* dist, const uint8_t* cls, int p, int Wp, int goal_p) {
    const unsigned k = cls[p];
    if (k == 0u || p == goal_p) return false;
    const unsigned m = k & 0x1Fu;
    const unsigned up = dist[p - Wp], dn = dist[p + Wp], lf = dist[p - 1], rt = dist[p + 1];
    const unsigned o1 = up < dn ? up : dn, o2 = lf < rt ? lf : rt;
    unsigned best = (o1 < o2 ? o1 : o2) + 5u * m;        // an impassable neighbour holds 0xFFFF: it cannot lower anything
    const bool cu = cls[p - Wp] != 0, cd = cls[p + Wp] != 0, cl = cls[p - 1] != 0, cr = cls[p + 1] != 0;
    // (all four diagonals are read, then selected: no branch around a load)
    const unsigned r0 = dist[p - Wp - 1], r1 = dist[p - Wp + 1], r2 = dist[p + Wp - 1], r3 = dist[p + Wp + 1];
    const unsigned d0 = (cu & cl) ? r0 : kGoalInf, d1 = (cu & cr) ? r1 : kGoalInf;
    const unsigned d2 = (cd & cl) ? r2 : kGoalInf, d3 = (cd & cr) ? r3 : kGoalInf;
    const unsigned e1 = d0 < d1 ? d0 : d1, e2 = d2 < d3 ? d2 : d3;
    const unsigned diag = (e1 < e2 ? e1 : e2) + 7u * m;
    best = best < diag ? best : diag;
    best = best < kGoalInf ? best : kGoalInf;
    if (best < dist[p]) { dist[p] = (uint16_t)best; return true; }
    return false;
}

// what launch 1 reads of cfg, the state and the call -- nothing else rides in its scalar registers
struct GoalFieldArgs {
    const void* field; const float* overflow; const int32_t* map_slot;   // navsim_state's
    const double* robot_goal; const int64_t* episode;
    navsim_goal_field out;
    const uint8_t* rebuild; const uint8_t* skip;
    int32_t* sweeps;
    float ox, oy, res;                   // (float)cfg.origin_x, origin_y, resolution: xy_to_ij_f32's operands
    float hard, clear;
    int band_cost, n_envs, map_h, map_w, shared_field, Hc, Wc;
};

template <typename Field>
__global__ __launch_bounds__(kGoalBlock) void goal_field_kernel(GoalFieldArgs a) {
    extern __shared__ __align__(16) unsigned char goal_lds[];
    __shared__ int s_list[kGoalBlock];
    __shared__ int s_count;
    __shared__ int s_flag[3];
    const int tid = threadIdx.x, E = a.n_envs, G = gridDim.x;
    const int Hc = a.Hc, Wc = a.Wc, Wp = Wc + 2, cells = (Hc + 2) * Wp, inner = Hc * Wc;
    uint16_t* dist = (uint16_t*)goal_lds;                                // [Hc + 2, Wp]
    uint8_t* cls = goal_lds + (((size_t)cells * 2 + 15) & ~(size_t)15);  // [Hc + 2, Wp]
    // the strip of this thread: 2 x odd cells (above)
    const int per = (cells + kGoalBlock - 1) / kGoalBlock;
    const int strip = 2 * (((per + 1) / 2) | 1);
    const int p_lo = tid * strip < cells ? tid * strip : cells;
    const int p_hi = p_lo + strip < cells ? p_lo + strip : cells;
    // (row, column) of this thread's first cell and of a step of 1024 cells, in the padded grid and in the interior: the only
    // divisions of the kernel
    const int pr0 = tid / Wp, pq0 = tid - pr0 * Wp, pdr = kGoalBlock / Wp, pdq = kGoalBlock - pdr * Wp;
    const int ir0 = tid / Wc, iq0 = tid - ir0 * Wc, idr = kGoalBlock / Wc, idq = kGoalBlock - idr * Wc;
    const int n_mine = (E - (int)blockIdx.x + G - 1) / G;                // arenas blockIdx.x, + G, + 2 G, ...
    // ---- the stale arenas of this workgroup, tested in parallel (the host launches G >= E / 1024 workgroups: n_mine <= 1024)
    if (tid == 0) s_count = 0;
    __syncthreads();
    {
        const bool mine = tid < n_mine;
        const int e = mine ? (int)blockIdx.x + tid * G : (int)blockIdx.x;
        const int64_t* key = a.out.key + 3 * (size_t)e;
        const bool skipped = a.skip ? a.skip[e] != 0 : false;
        const bool forced = a.rebuild ? a.rebuild[e] != 0 : false;
        const bool stale = key[0] != a.episode[e] || key[1] != (int64_t)__double_as_longlong(a.robot_goal[2 * (size_t)e]) ||
                           key[2] != (int64_t)__double_as_longlong(a.robot_goal[2 * (size_t)e + 1]);
        if (mine && !skipped && (stale || forced)) s_list[atomicAdd(&s_count, 1)] = e;
    }
    __syncthreads();
    {
        const int n_list = s_count;                                      // <= 1024
#pragma unroll 1
        for (int q = 0; q < n_list; ++q) {
            const int e = s_list[q];
            const double gx = a.robot_goal[2 * (size_t)e], gy = a.robot_goal[2 * (size_t)e + 1];
            int gi, gj;
            goal_nav_cell((float)gx, (float)gy, a.ox, a.oy, a.res, a.map_h, a.map_w, Hc, Wc, gi, gj);
            const int goal_p = (gj + 1) * Wp + gi + 1;
            // ---- a: classify -- every cell of the padded grid is written: a wavefront per row, a lane per column (no division)
            if (tid < 3) s_flag[tid] = 0;
            {
                const int ms = a.shared_field ? 0 : (a.map_slot ? a.map_slot[e] : e);      // map_slot_of
                const Field field(a.field, a.overflow, ms, a.map_h, a.map_w);
                int r = pr0, q2 = pq0;                                   // padded cell p = tid, tid + 1024, ...: (row, column) carried along
#pragma unroll 1
                for (int p = tid; p < cells; p += kGoalBlock) {
                    {
                        // nav cell (q2 - 1, r - 1), sampled at 5 (q2 - 1) + 2; a border cell reads its interior neighbour's
                        // sample and is impassable whatever that says: no branch around the read
                        const int qi = q2 < 1 ? 1 : (q2 > Wc ? Wc : q2), ri = r < 1 ? 1 : (r > Hc ? Hc : r);
                        const float d = field.at(5 * qi - 3, 5 * ri - 3);
                        unsigned k = d < a.hard ? 0u : (d < a.clear ? (unsigned)a.band_cost : 1u);
                        k = (qi == q2 && ri == r) ? k : 0u;
                        cls[p] = (uint8_t)(p == goal_p ? (k | 0x80u) : k);
                        dist[p] = (uint16_t)(p == goal_p ? 0u : kGoalInf);
                    }
                    r += pdr; q2 += pdq;
                    if (q2 >= Wp) { q2 -= Wp; r += 1; }
                }
            }
            __syncthreads();
            // ---- b: relax
            int sweeps = 0, slot = 0;
#pragma unroll 1
            for (int sweep = 0; sweep < inner; ++sweep) {                // bound Hc Wc
                bool changed = false;
                const int step = (sweep & 1) ? -1 : 1;                   // the strip forwards, then backwards
                int p = step > 0 ? p_lo : p_hi - 1;
#pragma unroll 1
                for (int n = p_hi - p_lo; n > 0; --n, p += step) changed |= goal_relax(dist, cls, p, Wp, goal_p);
                if (changed) s_flag[slot] = 1;
                __syncthreads();
                const int any = s_flag[slot];
                const int clear_slot = slot == 0 ? 2 : slot - 1;         // (slot + 2) mod 3
                if (tid == 0) s_flag[clear_slot] = 0;
                slot = slot == 2 ? 0 : slot + 1;
                sweeps = sweep + 1;
                if (!any) break;                                         // workgroup-uniform
            }
            // ---- c: the interior, the key, the counters
            uint16_t* out = a.out.dist + (size_t)e * inner;
            {
                int p = (ir0 + 1) * Wp + iq0 + 1, q2 = iq0;              // interior cell L = tid, tid + 1024, ...: its padded index carried along
#pragma unroll 1
                for (int L = tid; L < inner; L += kGoalBlock) {
                    out[L] = dist[p];
                    p += idr * Wp + idq; q2 += idq;
                    if (q2 >= Wc) { q2 -= Wc; p += 2; }                  // the next row: past its two border cells
                }
            }
            if (tid == 0) {
                int64_t* key = a.out.key + 3 * (size_t)e;
                key[0] = a.episode[e];
                key[1] = (int64_t)__double_as_longlong(gx);
                key[2] = (int64_t)__double_as_longlong(gy);
                if (a.out.rebuilds) atomicAdd(a.out.rebuilds, 1ull);
                if (a.sweeps) a.sweeps[e] = sweeps;
            }
            __syncthreads();                                             // the grid is free for the next arena
        }
    }
}

// Steps 3 - 5 of navsim_goal_path for a robot at (rx, ry) on the field `dist` whose goal is (gx, gy): EIGHT lanes per walker --
// lane k of a group = neighbour k -- and every lane of the wavefront calls it (ballots and shuffles; the hop loop is
// wave-uniform).  `active`: this group has a walker.  All eight lanes of a group return the same values: the walk's last cell
// (ci, cj), the goal's cell (gi, gj), dcur = dist[cur] and `off` (step 3).  goal_query_kernel and mppi_update_kernel
// (kernels_mppi.hpp) call it.
template <typename Field>
__device__ __forceinline__ void goal_walk(const Field& field, const uint16_t* dist, int Hc, int Wc, float hard, int lookahead_cells,
                                          float ox, float oy, float res, int map_h, int map_w, int lane, bool active,
                                          double rx, double ry, double gx, double gy,
                                          int& ci, int& cj, int& gi, int& gj, unsigned& dcur, bool& off) {
    const int k = lane & 7;
    // neighbour k of the fixed order: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (+1,-1) (-1,+1) (-1,-1)
    const int di = k < 2 ? 1 - 2 * k : (k < 4 ? 0 : (k < 6 ? 1 : -1));
    const int dj = k < 2 ? 0 : (k < 4 ? 5 - 2 * k : ((k & 1) ? -1 : 1));
    const unsigned w = k < 4 ? 5u : 7u;
    const unsigned need_bits = k < 4 ? 0u : ((di > 0 ? 1u : 2u) | (dj > 0 ? 4u : 8u));      // a diagonal's two orthogonal cells
    ci = 0; cj = 0; gi = 0; gj = 0;
    dcur = kGoalInf;
    if (active) {                                                        // step 2
        goal_nav_cell((float)gx, (float)gy, ox, oy, res, map_h, map_w, Hc, Wc, gi, gj);
        goal_nav_cell((float)rx, (float)ry, ox, oy, res, map_h, map_w, Hc, Wc, ci, cj);
        dcur = dist[cj * Wc + ci];
    }
    off = active && dcur == kGoalInf;                                    // step 3
    bool walking = active && !off;
    int walked = 0;
    const int by_look = lookahead_cells / 5, by_grid = Hc * Wc;
    const int max_hops = by_look < by_grid ? by_look : by_grid;
    for (int hop = 0; hop < max_hops; ++hop) {                           // step 4; wave-uniform
        walking = walking && !(ci == gi && cj == gj);
        if (__ballot(walking) == 0ull) break;
        const int ni = ci + di, nj = cj + dj;
        unsigned dn = kGoalInf;
        bool pass = false;
        if (walking && ni >= 0 && ni < Wc && nj >= 0 && nj < Hc) {
            dn = dist[nj * Wc + ni];
            pass = (ni == gi && nj == gj) || !(field.at(5 * ni + 2, 5 * nj + 2) < hard);
        }
        const unsigned bits = (unsigned)(__ballot(pass) >> (lane & 56)) & 0xFFu;      // the eight neighbours of this walker
        const bool adm = pass && (bits & need_bits) == need_bits;
        int key = adm ? (int)((dn + w) * 8u + (unsigned)k) : 0x7FFFFFFF;
        int o = __shfl_xor(key, 1); key = o < key ? o : key;
        o = __shfl_xor(key, 2); key = o < key ? o : key;
        o = __shfl_xor(key, 4); key = o < key ? o : key;
        if (walking) {
            const int kk = key & 7, ww = kk < 4 ? 5 : 7;
            if (key == 0x7FFFFFFF || walked + ww > lookahead_cells) {
                walking = false;
            } else {
                ci += kk < 2 ? 1 - 2 * kk : (kk < 4 ? 0 : (kk < 6 ? 1 : -1));
                cj += kk < 2 ? 0 : (kk < 4 ? 5 - 2 * kk : ((kk & 1) ? -1 : 1));
                walked += ww;
                dcur = (unsigned)(key >> 3) - (unsigned)ww;
            }
        }
    }
}

// Steps 5 and 6 behind goal_walk: the target (tx, ty) and the float32 distance; dx, dy = target - robot for the caller's sub-goal
__device__ __forceinline__ float goal_distance(double origin_x, double origin_y, double resolution, bool off, bool reached, int ci, int cj,
                                               unsigned dcur, double rx, double ry, double gx, double gy, double& dx, double& dy) {
    double tx = gx, ty = gy;
    unsigned rem = 0u;
    if (!off && !reached) {
        tx = origin_x + ((double)(5 * ci) + 2.5) * resolution;
        ty = origin_y + ((double)(5 * cj) + 2.5) * resolution;
        rem = dcur;
    }
    dx = tx - rx; dy = ty - ry;
    return (float)(sqrt(dx * dx + dy * dy) + (double)rem * resolution);
}

template <typename Field>
__global__ __launch_bounds__(64 * kGoalWaves) void goal_query_kernel(navsim_config c, navsim_state st, GoalPathArgs a) {
    const int lane = threadIdx.x & 63, k = lane & 7;
    const int e = ((int)blockIdx.x * kGoalWaves + (int)(threadIdx.x >> 6)) * 8 + (lane >> 3);
    if (e - (lane >> 3) >= c.n_envs) return;                             // wave-uniform: no arena on this wavefront
    const bool in = e < c.n_envs;
    const bool skipped = in && a.skip && a.skip[e] != 0;                 // step 1
    const int Hc = a.Hc, Wc = a.Wc;
    double rx = 0.0, ry = 0.0, th = 0.0, gx = 0.0, gy = 0.0;
    const size_t ee = in ? (size_t)e : 0;
    const uint16_t* dist = a.field.dist + ee * Hc * Wc;
    const Field field(st.field, st.field_overflow, (in && !skipped) ? map_slot_of(c, st, e) : 0, c.map_h, c.map_w);
    if (in && !skipped) {                                                // step 2
        rx = st.robot_pose[3 * ee]; ry = st.robot_pose[3 * ee + 1]; th = st.robot_pose[3 * ee + 2];
        gx = st.robot_goal[2 * ee]; gy = st.robot_goal[2 * ee + 1];
    }
    int ci, cj, gi, gj;
    unsigned dcur;
    bool off;
    goal_walk(field, dist, Hc, Wc, a.hard, a.lookahead_cells, (float)c.origin_x, (float)c.origin_y, (float)c.resolution, c.map_h,
              c.map_w, lane, in && !skipped, rx, ry, gx, gy, ci, cj, gi, gj, dcur, off);
    if (!in || k != 0) return;
    float* sub = a.out.subgoal + 2 * ee;
    if (skipped) {
        a.out.distance[e] = 0.0f; sub[0] = 0.0f; sub[1] = 0.0f; a.out.status[e] = 0;
        return;
    }
    // ---- steps 5 and 6
    const bool reached = !off && ci == gi && cj == gj;
    double dx, dy;
    const float distance = goal_distance(c.origin_x, c.origin_y, c.resolution, off, reached, ci, cj, dcur, rx, ry, gx, gy, dx, dy);
    double sn, cs;
    nv::sincos(th, sn, cs);
    a.out.distance[e] = distance;
    sub[0] = (float)(cs * dx + sn * dy);
    sub[1] = (float)(cs * dy - sn * dx);
    a.out.status[e] = (uint8_t)(off ? NAVSIM_GOAL_PATH_OFF_FIELD
                                    : (reached ? (NAVSIM_GOAL_PATH_OK | NAVSIM_GOAL_PATH_REACHED_GOAL_CELL) : NAVSIM_GOAL_PATH_OK));
}
