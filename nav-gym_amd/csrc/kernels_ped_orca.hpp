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

}  // namespace orca

// arenas per wavefront, and the bytes of dynamic LDS of one wavefront (host and device agree through these)
__host__ __device__ __forceinline__ int ped_orca_pack(int N) { return N <= 32 ? 64 / N : 1; }
__host__ __device__ __forceinline__ int ped_orca_list_len(int N, int max_neighbors, int robot_visible) {
    const int others = N - 1 + (robot_visible ? 1 : 0);
    return max_neighbors < others ? max_neighbors : others;
}
__host__ __device__ __forceinline__ size_t ped_orca_lds_bytes(int N, int L) {
    const int G = ped_orca_pack(N);
    return ((size_t)5 * G * (N + 1) + (size_t)10 * L * G * N) * sizeof(float);
}

__global__ __launch_bounds__(64) void ped_orca_kernel(navsim_config c, navsim_state st, navsim_ped_orca_params p,
                                                      double* __restrict__ ped_cmd) {
    using namespace orca;
    extern __shared__ float orca_lds[];
    const int N = c.max_peds, P = c.max_waypoints, A = N + 1;
    const int G = ped_orca_pack(N), W = G * N;
    const int L = ped_orca_list_len(N, p.orca.max_neighbors, p.robot_visible);
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
    const int plane = L * W;
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
    const LdsNeighbors nb = {(int*)lists, lists + plane, W};
    int n_agn = 0;
    if (p.orca.max_neighbors > 0) {
        float range_sq = sqr(p.orca.neighbor_dist);
        const int max_n = p.orca.max_neighbors < NAVSIM_ORCA_MAX_AGENTS ? p.orca.max_neighbors : NAVSIM_ORCA_MAX_AGENTS;
        for (int k = 0; k < n; ++k)
            if (k != i) insert_neighbor(nb, n_agn, max_n, k, abs_sq(position - v2(ax[k], ay[k])), range_sq);
        if (p.robot_visible) insert_neighbor(nb, n_agn, max_n, N, abs_sq(position - v2(ax[N], ay[N])), range_sq);
    }
    // ---- Agent::computeNewVelocity: one half-plane per neighbour (no obstacle polygons in this model)
    const LdsLines lines = {lists + 2 * plane, W, plane};
    const float inv_th = 1.0f / p.orca.time_horizon;
    for (int k = 0; k < n_agn; ++k) {
        const int o = nb.index(k);
        lines.set(k, agent_line(position, velocity, radius, v2(ax[o], ay[o]), v2(avx[o], avy[o]), ar[o], inv_th, p.orca.time_step));
    }
    V2 nv_;
    const int fail = lp2(lines, n_agn, max_speed, pref, false, nv_);
    if (fail < n_agn) {
        const LdsLines proj = {lists + 6 * plane, W, plane};
        lp3(lines, n_agn, 0, fail, max_speed, nv_, proj);
    }
    // ---- ActionRot (orca.py:128-130) as the command Human.set_vel integrates
    const double vx = (double)nv_.x, vy = (double)nv_.y;
    ped_cmd[2 * pq] = sqrt(vx * vx + vy * vy);
    ped_cmd[2 * pq + 1] = (nv::atan2_(vy, vx) - pp[2]) / c.time_step;
}
