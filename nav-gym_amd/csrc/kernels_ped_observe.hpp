// kernels_ped_observe.hpp -- observed pedestrians (include/navsim.h navsim_ped_observe): the K nearest pedestrians the robot has
// in line of sight, in the robot's frame, sorted by distance -- one launch that reads the state the step left.
// Not a standalone header: a section of navsim_kernels.hip (kernels_field.hpp's fields and march, kernels_step.hpp's wave_lds_sync).
#pragma once

// ============================================================================================
// One wavefront per arena, four arenas per workgroup (kernels_episode.hpp's shape); the wavefronts never meet, so there is no
// workgroup barrier and a wavefront leaves as soon as its arena is done.
//   A  lane i = pedestrian i (N <= 64): relative pose, d, range and field-of-view tests, all float64 on navmath.hpp.  d, the
//      offset and the row payload go to LDS.  The pedestrians that need a march (in range, in view, further than ped_radius,
//      occlusion on) are COMPACTED into a list by a ballot: lanes of pedestrians that cannot be seen anyway issue no march.
//   B  lanes carry (listed pedestrian, ray) pairs: 21 x 3 rays (or 64 x 1) per pass, so the latencies of the marches overlap
//      across rays and pedestrians.  The rays of a pedestrian sit on adjacent lanes: one ballot folds them into `seen`.
//      The field is read straight from global memory -- at most 192 rays an arena.
//   C  rank of a seen pedestrian = seen pedestrians ahead of it in (d, i) order, counted over the set bits of the visibility
//      ballot with broadcast LDS reads: no sort.  Rank < K writes its row; the lanes from min(count, K) to K write the unused rows.
// No private arrays, no scratch.
//
// The march is nv::trace_ray's (navsim_device.hpp) on either field format: same samples, same bounds test, same result -- up to
// a bound per ray.  The specification marches to H W cells; a ray only has to tell whether r_m >= reach, and it stops at
// t_end = min(H W, floor(reach / resolution) + 4) cells (march_limit's argument, kernels_field.hpp): a hit found at parameter
// t > t_end lies at least t - sqrt(2) cells from the origin cell (the sample position's float32 rounding is below 0.1 cell on
// maps of less than 2^20 cells a side), i.e. more than reach / resolution + 2.5 cells: r_m > reach, `clear`.  The two other
// outcomes past t_end -- leaving the map, the H W limit -- return max_range = H W cells, which is `clear` exactly when
// fl32(max_range * resolution) >= reach: the kernel tests that once per ray and uses the bound only where it holds (elsewhere, a
// map smaller than the line of sight is long, the ray is marched to H W like the specification's).  So past t_end every outcome is
// `clear`, which is what returning max_range there gives.  A marched pedestrian is in range, d <= sensor_range + ped_radius, so
// reach <= sqrt(d^2 + ped_radius^2) <= sensor_range + 2 ped_radius: no ray is marched beyond floor((sensor_range + 2 ped_radius)
// / resolution) + 4 cells, and a ray to a near pedestrian stops right behind it instead of creeping up to the wall beyond --
// the creep is where a sphere-traced ray spends its probes (c3 shape, sensor_range 25 m: 41.7 us per launch with the one bound
// of sensor_range for all rays, 29.1 us with the ray's own; profiles/r15_ped_observe/).
// Resources, all nine forms alike (-Rpass-analysis=kernel-resource-usage): 62 VGPRs, 106 SGPRs, no scratch, no spill, 12 KB of
// LDS per workgroup, 7 waves per SIMD.  The launch is latency-bound, not occupancy-bound: 4096 arenas are one wavefront per SIMD
// four times over, all resident at once, and a wavefront's time is its chain of dependent field reads.
// ============================================================================================
constexpr int kObserveWaves = 4;

struct PedObserveArgs {
    navsim_ped_observe_params p;
    navsim_ped_observation out;
    const uint8_t* skip;
    float max_range;                // cells: (float)(H W), what an unobstructed ray returns
};

struct PedObserveLds {              // of one wavefront: 3 KB
    double ax[64], ay[64], d[64];   // pedestrian - robot, world frame; its length
    float4 row[64];                 // x, y, vx, vy in the robot's frame
    int list[64];                   // the pedestrians to march, ascending
    int seen[64];
};

template <typename Field, int RULE>
__global__ __launch_bounds__(64 * kObserveWaves) void ped_observe_kernel(navsim_config c, navsim_state st, PedObserveArgs a) {
    __shared__ PedObserveLds s_all[kObserveWaves];
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kObserveWaves + (threadIdx.x >> 6)));
    if (e >= c.n_envs) return;
    PedObserveLds& s = s_all[threadIdx.x >> 6];
    const int N = c.max_peds, K = a.p.max_obs;
    float* state = a.out.state + (size_t)e * K * 5;
    int32_t* index = a.out.index + (size_t)e * K;
    uint8_t* visible = a.out.visible ? a.out.visible + (size_t)e * N : nullptr;
    if (a.skip && a.skip[e] != 0) {                              // step 1: an empty arena
        for (int k = lane; k < K * 5; k += 64) state[k] = 0.0f;
        if (lane < K) index[lane] = -1;
        if (visible && lane < N) visible[lane] = 0;
        if (lane == 0) a.out.count[e] = 0;
        return;
    }
    // ---- step 2: the robot and the scan's origin cell (wave-uniform)
    int n = st.n_peds[e];
    n = n > N ? N : n;
    const double rx = st.robot_pose[3 * (size_t)e], ry = st.robot_pose[3 * (size_t)e + 1], th = st.robot_pose[3 * (size_t)e + 2];
    double sn, cs;
    nv::sincos(th, sn, cs);
    int i0, j0;
    nv::xy_to_ij_f32((float)rx, (float)ry, c, i0, j0);
    const double pr = a.p.ped_radius;
    // ---- A, step 3: pedestrian i on lane i
    double d = 0.0;
    bool cand = false, need = false;
    if (lane < n) {
        const size_t q = (size_t)e * N + lane;
        const double ax = st.ped_pose[3 * q] - rx, ay = st.ped_pose[3 * q + 1] - ry;
        const double vx = st.ped_vel[2 * q], vy = st.ped_vel[2 * q + 1];
        d = sqrt(ax * ax + ay * ay);
        const double x = cs * ax + sn * ay, y = cs * ay - sn * ax;
        const double vxr = cs * vx + sn * vy, vyr = cs * vy - sn * vx;
        const bool in_range = d - pr <= a.p.sensor_range;
        bool in_fov = true;
        if (a.p.fov) {
            const double b = nv::atan2_(y, x);
            in_fov = c.angle_min <= b && b <= c.angle_last;
        }
        cand = in_range && in_fov;
        need = cand && a.p.occlusion != 0 && !(d <= pr);       // step 4: within ped_radius is seen without a cast
        s.ax[lane] = ax; s.ay[lane] = ay;
        s.row[lane] = make_float4((float)x, (float)y, (float)vxr, (float)vyr);
    }
    s.d[lane] = d;
    s.seen[lane] = cand && !need;
    const unsigned long long need_mask = __ballot(need);
    if (need) s.list[__popcll(need_mask & ((1ull << lane) - 1ull))] = lane;
    const int m = __popcll(need_mask);
    wave_lds_sync();
    // ---- B, step 4: a (listed pedestrian, ray) pair per lane
    if (m > 0) {                                                 // wave-uniform
        const Field field(st.field, st.field_overflow, map_slot_of(c, st, e), c.map_h, c.map_w);
        const int H = c.map_h, W = c.map_w;
        const int rays = a.p.rays, per = rays == 3 ? 21 : 64;
        const int pl = rays == 3 ? lane / 3 : lane, k = lane - pl * rays;
        const float x0 = (float)i0, y0 = (float)j0, res = (float)c.resolution;
        for (int base = 0; base < m; base += per) {
            const int slot = base + pl;
            const bool live = pl < per && slot < m;
            bool clear = false;
            int ped = 0;
            if (live) {
                ped = s.list[slot];
                const double ax = s.ax[ped], ay = s.ay[ped], dd = s.d[ped];
                const double ux = ax / dd, uy = ay / dd;
                const double o = k == 0 ? 0.0 : (k == 1 ? pr : -pr);      // the centre, then the two silhouette points
                const double tx = ax - o * uy, ty = ay + o * ux;
                const float heading = (float)nv::atan2_(ty, tx);
                float dx, dy;
                nv::beam_dir(heading, dx, dy);
                const double reach = sqrt(tx * tx + ty * ty) - (k == 0 ? pr : 0.0);
                float t_end = a.max_range;                                // the ray's bound (above)
                if ((double)(a.max_range * res) >= reach) {
                    const float lim = (float)(floor(reach / c.resolution) + 4.0);
                    t_end = lim < t_end ? lim : t_end;
                }
                float t = 0.0f, r = a.max_range;
                while (t < t_end) {                                       // nv::trace_ray, either field format
                    const float fx = march_pos<RULE>(x0, dx, t), fy = march_pos<RULE>(y0, dy, t);
                    const int px = (int)fx, py = (int)fy;
                    if (px >= W || px < 0 || py < 0 || py >= H) break;    // left the map: max_range
                    const typename Field::raw_t raw = field.load(px, py);
                    if (field.occupied(raw)) {
                        const float xd = (float)px - x0, yd = (float)py - y0;
                        r = sqrtf(xd * xd + yd * yd);
                        break;
                    }
                    t += march_step<RULE>(field.decode_nz(raw, px, py));
                }
                const double r_m = (double)(r * res);                     // the float32 product of env.py:426
                clear = r_m >= reach;
            }
            const unsigned long long cm = __ballot(clear);
            if (live && k == 0) s.seen[ped] = ((cm >> (pl * rays)) & (rays == 3 ? 7ull : 1ull)) != 0ull;
        }
        wave_lds_sync();
    }
    // ---- C, steps 5 and 6
    const bool vis = lane < n && s.seen[lane] != 0;
    const unsigned long long vm = __ballot(vis);
    const int count = __popcll(vm);
    int rank = 0;
    for (unsigned long long rest = vm; rest != 0ull; rest &= rest - 1ull) {      // wave-uniform: broadcast reads
        const int j = __builtin_ctzll(rest);
        const double dj = s.d[j];
        rank += (dj < d || (dj == d && j < lane)) ? 1 : 0;
    }
    if (vis && rank < K) {
        const float4 v = s.row[lane];
        float* o = state + rank * 5;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; o[4] = (float)d;
        index[rank] = lane;
    }
    const int kept = count < K ? count : K;
    if (lane >= kept && lane < K) {
        float* o = state + lane * 5;
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f; o[4] = 0.0f;
        index[lane] = -1;
    }
    if (visible && lane < N) visible[lane] = vis ? 1 : 0;
    if (lane == 0) a.out.count[e] = count;
}
