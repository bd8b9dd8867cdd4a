// kernels_ped_orca.hpp -- NavGym-v0 pedestrians driven by ORCA, computed from the simulator's own state (navsim_ped_orca).
// Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace, after
// kernels_crowd_orca.hpp whose orca:: functions it shares; not a standalone header).
// Specification: include/navsim.h navsim_ped_orca -- waypoint pop, preferred velocity, the agent list (self, the other
// live pedestrians in ascending index, the robot), one step of navsim_crowd_orca_cpu's algorithm without obstacle
// polygons, ActionRot -> ped_cmd.  UNPINNED like navsim_crowd_orca: rvo2 is absent from the reference tree.
//
// One lane per pedestrian, one wavefront per workgroup.  A wavefront serves G = 64 / N whole arenas (N = cfg.max_peds;
// one arena when N > 32), so W = G * N lanes work.  Dynamic LDS, in floats:
//   agents  5 arrays [G][N + 1]: px, py, vx, vy, radius of every live pedestrian (entry i) and the robot (entry N),
//           rounded to float32 once; every query reads its neighbours from here
//   lists   10 arrays [L][W], L = min(max_neighbors, N - 1 + robot_visible) entries per lane: neighbour index, neighbour
//           distance, the half-planes (4 floats), lp3's projected half-planes (4 floats).  Entry k of lane l is word
//           k * W + l of its array: lanes that walk their lists in step touch W consecutive words (no bank conflict), and
//           a lane's dynamic index never leaves LDS -- the kernel has no private arrays and needs no scratch.
//
// WALLS (navsim_ped_orca_walls): the arena's listed rectangles are ORCA obstacles.  A lane keeps the K = max_rects nearest
// rectangles of its arena's rect_index list within the obstacle range, hands them to the obstacle code crowd_orca_kernel runs
// (orca::obstacle_neighbors / obstacle_lines, written once in kernels_crowd_orca.hpp) as 4-vertex polygons, and solves with the
// obstacle half-planes in front of the agent half-planes.  An axis-aligned rectangle shows a point outside it at most two
// edges, so a lane holds at most 2 K obstacle edges and lines.  Per lane, in words of the same interleaved scheme:
//   neighbours    2 L          index, distance
//   lines         4 (L + 2 K)  obstacle half-planes first, then the agents'
//   projection    4 (L + 2 K)  lp3's; until the lines are built its first 8 K words hold
//                   verts [4 K]   xa, ya, xb, yb of the kept rectangles in ascending list index, float32
//                   edges [4 K]   index and distance of the obstacle edges in range (2 K each); the selection list (list index
//                                 and distance of the kept rectangles, K each) lies on the distances: it is dead once the
//                                 vertices are written, before the first edge is
// The rectangle list is read from the arena's row in global memory (lanes of one arena read the same 32 bytes at a time):
// 2 KB per arena would not fit LDS at N = 1, where a wavefront serves 64 arenas.

namespace orca {

// entry k of this lane's list is base[k * stride]
struct LdsLines {
    float* base; int stride, plane;                                  // plane = L * stride: distance between the components
    __device__ __forceinline__ Line get(int i) const {
        const float* q = base + i * stride;
        Line l;
        l.point = v2(q[0], q[plane]);
        l.direction = v2(q[2 * plane], q[3 * plane]);
        return l;
    }
    __device__ __forceinline__ void set(int i, const Line& l) const {
        float* q = base + i * stride;
        q[0] = l.point.x; q[plane] = l.point.y; q[2 * plane] = l.direction.x; q[3 * plane] = l.direction.y;
    }
};
struct LdsNeighbors {
    int* id; float* d; int stride;
    __device__ __forceinline__ float dist(int i) const { return d[i * stride]; }
    __device__ __forceinline__ int index(int i) const { return id[i * stride]; }
    __device__ __forceinline__ void set(int i, int k, float v) const { id[i * stride] = k; d[i * stride] = v; }
};

// The kept rectangles of one lane as the polygon set of orca::obstacle_neighbors / obstacle_lines: polygon o = k >> 2 has the
// counter-clockwise vertices (xa,ya), (xb,ya), (xb,yb), (xa,yb); every vertex of a rectangle is convex.
struct Rects {
    const float* v; int stride, plane;                               // component c of rectangle o: v[c * plane + o * stride]
    __device__ __forceinline__ V2 point(int k) const {
        const float* q = v + (k >> 2) * stride;
        const int i = k & 3;
        return v2(q[(i == 1 || i == 2) ? 2 * plane : 0], q[i >= 2 ? 3 * plane : plane]);
    }
    __device__ __forceinline__ int next(int k) const { return (k & ~3) | ((k + 1) & 3); }
    __device__ __forceinline__ int prev(int k) const { return (k & ~3) | ((k + 3) & 3); }
    __device__ __forceinline__ V2 unit_dir(int k) const { return normalize(point(next(k)) - point(k)); }
    __device__ __forceinline__ bool convex(int) const { return true; }
};

}  // namespace orca

// arenas per wavefront, and the bytes of dynamic LDS of one wavefront (host and device agree through these)
__host__ __device__ __forceinline__ int ped_orca_pack(int N) { return N <= 32 ? 64 / N : 1; }
__host__ __device__ __forceinline__ int ped_orca_list_len(int N, int max_neighbors, int robot_visible) {
    const int others = N - 1 + (robot_visible ? 1 : 0);
    return max_neighbors < others ? max_neighbors : others;
}
// bytes = 4 * (5 G (N + 1) + (10 L + 16 K) G N): the agents, then per lane 2 L neighbour words and twice 4 (L + 2 K) words of
// half-planes (K = 0: navsim_ped_orca).  N = 20, L = 10: 25 260 B at K = 0, 55 980 B at K = 8 (two wavefronts per CU),
// 148 140 B at K = 32.
__host__ __device__ __forceinline__ size_t ped_orca_lds_bytes(int N, int L, int K = 0) {
    const int G = ped_orca_pack(N);
    return ((size_t)5 * G * (N + 1) + ((size_t)10 * L + (size_t)16 * K) * G * N) * sizeof(float);
}

template <bool WALLS>
__global__ __launch_bounds__(64) void ped_orca_kernel(navsim_config c, navsim_state st, navsim_ped_orca_params p, int max_rects,
                                                      double* __restrict__ ped_cmd, int32_t* __restrict__ dropped) {
    using namespace orca;
    extern __shared__ float orca_lds[];
    const int N = c.max_peds, P = c.max_waypoints, A = N + 1;
    const int G = ped_orca_pack(N), W = G * N;
    const int L = ped_orca_list_len(N, p.orca.max_neighbors, p.robot_visible);
    const int K = WALLS ? max_rects : 0, LL = L + 2 * K;             // LL: half-planes per lane at most
    const int lane = threadIdx.x;
    const int s = lane / N, i = lane - s * N;
    const int e = (int)blockIdx.x * G + s;
    const bool slot_ok = s < G && e < c.n_envs;
    int n = slot_ok ? st.n_peds[e] : 0;
    n = n > N ? N : (n < 0 ? 0 : n);
    const bool is_ped = slot_ok && i < n;
    float* ax = orca_lds + (slot_ok ? s : 0) * A;                    // this arena's agents
    float* ay = ax + G * A; float* avx = ay + G * A; float* avy = avx + G * A; float* ar = avy + G * A;
    float* lists = orca_lds + 5 * G * A + (lane < W ? lane : 0);     // this lane's entry 0 of the first list
    const int nplane = L * W, plane = LL * W;                        // distance between the components of a neighbour / a line
    const size_t pq = (size_t)(slot_ok ? e : 0) * N + (is_ped ? i : 0);
    // ---- stage: every agent is read from HBM once
    double pp[3] = {0.0, 0.0, 0.0};
    V2 position = v2(0.0f, 0.0f), velocity = v2(0.0f, 0.0f);
    const float radius = (float)(p.ped_radius + 0.01 + p.safety_space);
    int head = 0;
    const double* wp = st.ped_waypoints + (pq * P) * 2;
    if (is_ped) {
        pp[0] = st.ped_pose[pq * 3]; pp[1] = st.ped_pose[pq * 3 + 1]; pp[2] = st.ped_pose[pq * 3 + 2];
        head = ped_pop_waypoints(wp, st.ped_wp_head[pq], st.ped_n_waypoints[pq], pp);
        st.ped_wp_head[pq] = head;
        position = v2((float)pp[0], (float)pp[1]);
        velocity = v2((float)st.ped_vel[pq * 2], (float)st.ped_vel[pq * 2 + 1]);
        ax[i] = position.x; ay[i] = position.y; avx[i] = velocity.x; avy[i] = velocity.y; ar[i] = radius;
    }
    if (slot_ok && i == 0 && n > 0 && p.robot_visible) {             // the robot as the pedestrian phase of the step sees it
        const double* rp = st.robot_pose + 3 * (size_t)e;
        const double prev_v = st.prev_action[2 * (size_t)e];
        double sn, cs;
        nv::sincos(rp[2], sn, cs);
        ax[N] = (float)rp[0]; ay[N] = (float)rp[1];
        avx[N] = (float)(prev_v * cs); avy[N] = (float)(prev_v * sn);
        ar[N] = (float)(p.robot_radius + 0.01 + p.safety_space);
    }
    __syncthreads();
    if (!is_ped) return;
    // ---- preferred velocity (orca.py:116-120)
    const double gx = wp[2 * head] - pp[0], gy = wp[2 * head + 1] - pp[1];
    const double gl = sqrt(gx * gx + gy * gy);
    const V2 pref = gl > 1.0 ? v2((float)(gx / gl), (float)(gy / gl)) : v2((float)gx, (float)gy);
    const float max_speed = (float)st.ped_v_pref[pq];
    // ---- Agent::computeNeighbors: the nearest of the arena's other agents, in list order
    const LdsNeighbors nb = {(int*)lists, lists + nplane, W};
    int n_agn = 0;
    if (p.orca.max_neighbors > 0) {
        float range_sq = sqr(p.orca.neighbor_dist);
        const int max_n = p.orca.max_neighbors < NAVSIM_ORCA_MAX_AGENTS ? p.orca.max_neighbors : NAVSIM_ORCA_MAX_AGENTS;
        for (int k = 0; k < n; ++k)
            if (k != i) insert_neighbor(nb, n_agn, max_n, k, abs_sq(position - v2(ax[k], ay[k])), range_sq);
        if (p.robot_visible) insert_neighbor(nb, n_agn, max_n, N, abs_sq(position - v2(ax[N], ay[N])), range_sq);
    }
    const LdsLines lines = {lists + 2 * nplane, W, plane};
    const LdsLines proj = {lists + 2 * nplane + 4 * plane, W, plane};
    int nl = 0;
    if constexpr (WALLS) {
        // ---- the K nearest listed rectangles within the obstacle range (include/navsim.h navsim_ped_orca_walls)
        float* scratch = proj.base;                                  // verts [4 K], edge index [2 K], edge distance [2 K]
        const int kw = K * W;
        const LdsNeighbors edges = {(int*)(scratch + 4 * kw), scratch + 6 * kw, W};
        const LdsNeighbors sel = {(int*)(scratch + 6 * kw), scratch + 7 * kw, W};
        const uint4* row = (const uint4*)((const char*)st.rect_index +
                                          (size_t)map_slot_of(c, st, e) * rect_index_row_bytes(c.map_h, c.map_w));
        const float range0 = sqr(p.orca.time_horizon_obst * max_speed + radius);
        float range_sq = range0;
        int n_sel = 0, n_in = 0;
        auto vert = [&](int cell, double origin) { return (float)(origin + (double)cell * c.resolution); };
        auto offer = [&](int k, unsigned lo, unsigned hi) {
            const int x0 = (short)(lo & 0xFFFFu), y0 = (short)(lo >> 16), x1 = (short)(hi & 0xFFFFu), y1 = (short)(hi >> 16);
            // an unused entry (and the lone cell (0,0)); an inverted entry, which no builder writes, is no rectangle either:
            // what is kept has xa <= xb and ya <= yb, which is what bounds a lane's edges by 2 K
            if ((lo | hi) == 0u || x1 < x0 || y1 < y0) return;
            const float xa = vert(x0, c.origin_x), ya = vert(y0, c.origin_y);
            const float xb = vert(x1 + 1, c.origin_x), yb = vert(y1 + 1, c.origin_y);
            const float dx = fmaxf(fmaxf(xa - position.x, position.x - xb), 0.0f);
            const float dy = fmaxf(fmaxf(ya - position.y, position.y - yb), 0.0f);
            const float d2 = dx * dx + dy * dy;
            n_in += d2 < range0 ? 1 : 0;
            insert_neighbor(sel, n_sel, K, k, d2, range_sq);
        };
        for (int k = 0; k < kRectListLen; k += 4) {                  // 32 bytes = four entries at a time; entry 255 is no rectangle
            const uint4 r0 = row[k >> 1], r1 = row[(k >> 1) + 1];
            offer(k, r0.x, r0.y); offer(k + 1, r0.z, r0.w); offer(k + 2, r1.x, r1.y);
            if (k + 3 < kRectListLen - 1) offer(k + 3, r1.z, r1.w);
        }
        if (dropped) dropped[pq] = n_in - n_sel;
        // the kept rectangles in ascending list index (insertion sort of at most K indices), then their vertices
        for (int a = 1; a < n_sel; ++a) {
            const int v = sel.id[a * W];
            int b = a;
            while (b != 0 && sel.id[(b - 1) * W] > v) { sel.id[b * W] = sel.id[(b - 1) * W]; --b; }
            sel.id[b * W] = v;
        }
        for (int a = 0; a < n_sel; ++a) {
            const uint2 r = ((const uint2*)row)[sel.id[a * W]];
            float* q = scratch + a * W;
            q[0] = vert((short)(r.x & 0xFFFFu), c.origin_x); q[kw] = vert((short)(r.x >> 16), c.origin_y);
            q[2 * kw] = vert((short)(r.y & 0xFFFFu) + 1, c.origin_x); q[3 * kw] = vert((short)(r.y >> 16) + 1, c.origin_y);
        }
        // ---- the obstacle part of Agent::computeNeighbors and of Agent::computeNewVelocity
        const Rects ob = {scratch, W, kw};
        const int n_obn = obstacle_neighbors(ob, 4 * n_sel, position, range0, edges);
        nl = obstacle_lines(ob, edges, n_obn, position, velocity, radius, 1.0f / p.orca.time_horizon_obst, lines);
    } else if (dropped) {
        dropped[pq] = 0;
    }
    // ---- Agent::computeNewVelocity: one half-plane per neighbour, behind the obstacles'
    const int n_obst_lines = nl;
    const float inv_th = 1.0f / p.orca.time_horizon;
    for (int k = 0; k < n_agn; ++k) {
        const int o = nb.index(k);
        lines.set(nl++, agent_line(position, velocity, radius, v2(ax[o], ay[o]), v2(avx[o], avy[o]), ar[o], inv_th, p.orca.time_step));
    }
    V2 nv_;
    const int fail = lp2(lines, nl, max_speed, pref, false, nv_);
    if (fail < nl) lp3(lines, nl, n_obst_lines, fail, max_speed, nv_, proj);
    // ---- ActionRot (orca.py:128-130) as the command Human.set_vel integrates
    const double vx = (double)nv_.x, vy = (double)nv_.y;
    ped_cmd[2 * pq] = sqrt(vx * vx + vy * vy);
    ped_cmd[2 * pq + 1] = (nv::atan2_(vy, vx) - pp[2]) / c.time_step;
}
