// kernels_ped_forecast.hpp -- pedestrian forecast (include/navsim.h navsim_ped_forecast): where the pedestrians of an arena will be
// after each of the next H navsim_step calls, under the step's own pedestrian model or at constant velocity, from the current
// state, which is only read.  Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace;
// not a standalone header): the same -ffp-contract=off unit and the same device functions in the same order as the step, which
// is what makes the rows bit-equal to the step's.
//
// One wavefront per arena (a workgroup of kForecastBlock = 64 threads), pedestrian i on lane i (N <= 64), the horizon loop inside,
// no scan.  Nothing of the robot depends on a pedestrian, so its whole trajectory comes first:
//   (0) thread RT (thread 0; lane 0 of wavefront 1 in a build of several wavefronts): the step's phase 0 for h = 0 .. H-1 on the
//       assumed actions (replay_twist of kernels_replay.hpp; HOLD and STOP are this kernel's own), from the carried pose and the carried
//       prev_action -- robot_pose[e,h] goes to global memory, and rob[h] = (x, y, prev_v cos th, prev_v sin th) of time t + h to
//       static LDS: the staged robot of step h (ped_stage_wave's four values; cos / sin are the ones phase 0 needs anyway) and, as
//       rob[h + 1], the pose min_dist measures from.  Barrier.
//   A step h under NAVSIM_FORECAST_TRUE with the social force, two barriers (of one wavefront here):
//   (1) waypoint pop from the carried head, the agents of time t staged (ped_stage_wave's body on the carried values; thread 0
//       copies rob[h]).  Barrier.
//   (2) the n (n - 1) / 2 + n pair terms over all threads of the workgroup (ped_pair_term: each term lands in its own slot,
//       whoever computes it) -- 210 terms at 20 pedestrians are four rounds of the wavefront.  Barrier.
//   (3) ped_sfm_step, the re-plan predicate, the rows of step h (lane i writes slot i: N adjacent rows per array, the slots
//       behind n as zeros), the running minimum of the distance to rob[h + 1].
//   Step (3) of h overlaps nobody's writes in a build of several wavefronts either: ps.ax[i] .. avy[i] are read by lane i alone,
//   the pair table is written behind barrier (1) of h + 1, and rob is read-only after (0).
//   External commands and NAVSIM_FORECAST_CONST_VEL need neither LDS nor a barrier inside the loop: nv::set_vel on the held
//   command, resp. x + vx ((h + 1) dt).
// Carried per pedestrian, in registers (CarriedPed of kernels_replay.hpp, loaded without the lidar's members): pose, velocity,
// waypoint head.  Leg odometry, ped_prev_yaw and the scan are not computed.
//
// Dynamic LDS (ped_forecast_lds_bytes; only with the social force under NAVSIM_FORECAST_TRUE): the four staging arrays
// [N + 1] float64, rounded up to 16 bytes, and the pair table 16 (N (N - 1) / 2 + N) bytes -- 0.7 + 3.4 KB at 20 pedestrians,
// 2.1 + 33.3 KB at 64.  The base is declared 16-byte aligned and every part is a multiple of 16.  Static LDS: rob, 33 x 32 bytes,
// and the frame's cos / sin.
//
// Arguments: the kernel reads cfg, state and PedForecastArgs in place in the kernarg segment (NAVSIM_KERNARGS, kernels_step.hpp).
//
// The two shapes, measured (profiles/r25_ped_forecast/summary.txt; c3-shaped world, 4096 arenas x 20 pedestrians, kernel times
// from a rocprofv3 --kernel-trace run of each build, the step kernel at 145.4 - 145.6 us in the same traces):
//   one workgroup of 256 threads per arena, the pair terms shared over its four wavefronts as rollout_kernel stage (2) does
//   (-DNAVSIM_FORECAST_BLOCK=256: RT is thread 64 beside the loading wavefront 0, 210 terms are one round) -- the form this
//   kernel was first built in, expected to win: H = 8 / 16 / 32 take 315.5 / 622.1 / 1192.7 us under TRUE (39.4 - 37.3 us a
//   forecast step: the rollout's pedestrian chain of ~39 us, no better) and 48.4 / 85.6 / 160.3 us under CONST_VEL;
//   one wavefront per arena, wave-level barriers only -- ped_update_kernel's shape with a pack of one: 213.1 / 419.4 / 814.1 us
//   (26.6 - 25.4 us a step, x 0.67) and 23.8 / 41.0 / 75.7 us (x 0.49).
// The wavefront form wins and is the default: at 4096 arenas the batch is bound by issue slots and residency, not by an arena's
// latency -- three of the four wavefronts of the wide form idle through staging, ped_sfm_step and the stores while they hold
// a quarter of the compute unit's wave slots each, so four arenas are resident where sixteen wavefront-arenas are.  What the
// wide form buys is an ARENA's latency (one round of pair terms instead of four; nine instead of thirty-three at 64
// pedestrians): a caller with a few arenas and full crowds may build it.  Not measured: 128 threads, a pack of two arenas.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage, FieldF32 / FieldU16T / FieldU16TN): 115 VGPRs, 106 SGPRs, 35 / 41 / 34
// SGPRs spilled to VGPR lanes, no VGPR spill, scratch 0 bytes per lane, occupancy 4 waves per SIMD (sixteen arenas a compute
// unit; LDS would allow thirty-nine at 20 pedestrians), 1072 bytes of static LDS.  The 256-thread build reported the same
// registers (29 / 42 / 35 SGPR spills).  No scratch in either.

struct PedForecastArgs {
    navsim_ped_forecast_out out;
    const double* actions;
    const double* ped_cmd;
    const uint8_t* skip;
    int H, robot, model;
};
struct PedForecastKernargs { navsim_config c; navsim_state st; PedForecastArgs a; };

#ifndef NAVSIM_FORECAST_BLOCK
#define NAVSIM_FORECAST_BLOCK 64
#endif
constexpr int kForecastBlock = NAVSIM_FORECAST_BLOCK;
static_assert(kForecastBlock >= 64 && kForecastBlock % 64 == 0, "a lane per pedestrian: at least one wavefront");

// Dynamic LDS of one arena, in the order ped_forecast_kernel carves it
__host__ __device__ inline size_t ped_forecast_stage_bytes(int N) { return lookahead_align16((size_t)4 * (N + 1) * sizeof(double)); }
inline size_t ped_forecast_lds_bytes(const navsim_config* c, int model) {
    if (model != NAVSIM_FORECAST_TRUE || c->ped_model != NAVSIM_PED_SFM) return 0;
    return ped_forecast_stage_bytes(c->max_peds) + ped_pair_bytes(c->max_peds);
}

template <typename Field>
__global__ __launch_bounds__(kForecastBlock) void ped_forecast_kernel(navsim_config c_, navsim_state st_, PedForecastArgs a_) {
    NAVSIM_KERNARGS(PedForecastKernargs, c_, st_, a_);
    const navsim_config& c = ka.c; const navsim_state& st = ka.st; const PedForecastArgs& a = ka.a;
    constexpr int BLOCK = kForecastBlock, RT = BLOCK > 64 ? 64 : 0;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ double rob[NAVSIM_FORECAST_MAX_H + 1][4];     // (x, y, prev_v cos th, prev_v sin th) of the robot at time t + h
    __shared__ double frame[2];                              // cos / sin of the robot's heading at time t (rel)
    const int e = (int)blockIdx.x, tid = threadIdx.x;
    const int N = c.max_peds, HZ = a.H;
    const size_t row0 = (size_t)e * HZ;                      // first row of [E,H]
    if (a.skip && a.skip[e]) {                               // a skipped arena: every row 0, nothing of the arena is read
        for (int q = tid; q < HZ * N; q += BLOCK) {
            const size_t r = row0 * N + q;
            a.out.pose[3 * r] = 0.0; a.out.pose[3 * r + 1] = 0.0; a.out.pose[3 * r + 2] = 0.0;
            a.out.vel[2 * r] = 0.0; a.out.vel[2 * r + 1] = 0.0;
            a.out.rel[2 * r] = 0.0f; a.out.rel[2 * r + 1] = 0.0f;
        }
        for (int h = tid; h < HZ; h += BLOCK) {
            a.out.robot_pose[3 * (row0 + h)] = 0.0; a.out.robot_pose[3 * (row0 + h) + 1] = 0.0; a.out.robot_pose[3 * (row0 + h) + 2] = 0.0;
        }
        for (int i = tid; i < N; i += BLOCK) { a.out.min_dist[(size_t)e * N + i] = 0.0; a.out.min_step[(size_t)e * N + i] = 0; }
        if (tid == 0) { a.out.exact_steps[e] = 0; a.out.status[e] = 0; }
        return;
    }
    const bool truth = a.model == NAVSIM_FORECAST_TRUE;
    const bool sfm = truth && c.ped_model == NAVSIM_PED_SFM;
    PedShared ps = {};
    double2* pair = nullptr;
    if (sfm) {
        double* d = (double*)dyn;
        ps.ax = d; ps.ay = d + (N + 1); ps.avx = d + 2 * (N + 1); ps.avy = d + 3 * (N + 1);      // (seg / disc / info: the lidar's, unused)
        pair = (double2*)(dyn + ped_forecast_stage_bytes(N));
    }
    int n = st.n_peds[e];
    n = n > N ? N : n; n = n < 0 ? 0 : n;
    const double dt = c.time_step;
    const Field field(st.field, st.field_overflow, map_slot_of(c, st, e), c.map_h, c.map_w);

    // ---- the carried values at h = 0: the state's.  Pedestrian i on lane i of wavefront 0
    const bool is_slot = tid < N, is_ped = tid < n;
    const size_t pq = (size_t)e * N + (is_ped ? tid : 0);
    CarriedPed cp;                                                                   // (nothing of the lidar's: no scan here)
    if (is_ped) carried_ped_load<false>(cp, c, st, pq, sfm, truth, a.ped_cmd);       // a command is held for the whole horizon
    // ---- (0) the robot's H poses: the step's phase 0 on the assumed actions, operation for operation
    if (tid == RT) {
        double rp[3] = {st.robot_pose[3 * (size_t)e], st.robot_pose[3 * (size_t)e + 1], st.robot_pose[3 * (size_t)e + 2]};
        const double hold[2] = {st.prev_action[2 * (size_t)e], st.prev_action[2 * (size_t)e + 1]};
        double prev_v = hold[0];
        for (int h = 0; h < HZ; ++h) {
            double a0 = 0.0, a1 = 0.0;                                               // NAVSIM_FORECAST_STOP: the zero twist
            if (a.robot == NAVSIM_FORECAST_ACTIONS) {
                a0 = a.actions[2 * (row0 + h)]; a1 = a.actions[2 * (row0 + h) + 1];
            } else if (a.robot == NAVSIM_FORECAST_HOLD) {
                a0 = hold[0]; a1 = hold[1];                                          // a twist already: the step stored it
            }
            replay_twist(c, a.robot == NAVSIM_FORECAST_ACTIONS, a0, a1);
            const double th_old = rp[2];
            const double th = th_old + a1 * dt;                                      // set_vel's intermediate heading
            double s0, c0, s1, c1;
            nv::sincos(th_old, s0, c0);
            nv::sincos(th, s1, c1);
            if (h == 0) { frame[0] = c0; frame[1] = s0; }
            rob[h][0] = rp[0]; rob[h][1] = rp[1];                                    // the robot as step h stages it (ped_stage_wave)
            rob[h][2] = prev_v * c0; rob[h][3] = prev_v * s0;
            nv::set_vel_with(rp, a0, a1, dt, c.axle_offset, s0, c0, s1, c1, nullptr);   // env.py:664
            a.out.robot_pose[3 * (row0 + h)] = rp[0]; a.out.robot_pose[3 * (row0 + h) + 1] = rp[1]; a.out.robot_pose[3 * (row0 + h) + 2] = rp[2];
            prev_v = a0;                                                             // prev_action as phase 6 stores it
        }
        rob[HZ][0] = rp[0]; rob[HZ][1] = rp[1]; rob[HZ][2] = 0.0; rob[HZ][3] = 0.0;
        a.out.status[e] = 1;
    }
    __syncthreads();

    const double rx0 = rob[0][0], ry0 = rob[0][1], fc = frame[0], fs = frame[1];
    const double x0 = cp.pp[0], y0 = cp.pp[1];                                       // NAVSIM_FORECAST_CONST_VEL starts every row here
    const int n_terms = n * (n - 1) / 2 + n;
    int exact = truth ? HZ : 0;
    double md = INFINITY;
    int mstep = -1;
    for (int h = 0; h < HZ; ++h) {
        bool due = false;
        if (sfm && n > 0) {
            // ---- (1) waypoint pop and staging (ped_stage_wave on the carried values)
            if (is_ped) {
                cp.head = ped_pop_waypoints(cp.wp, cp.head, cp.nw, cp.pp);
                ps.ax[tid] = cp.pp[0]; ps.ay[tid] = cp.pp[1]; ps.avx[tid] = cp.pvel[0]; ps.avy[tid] = cp.pvel[1];
            }
            if (tid == 0) { ps.ax[n] = rob[h][0]; ps.ay[n] = rob[h][1]; ps.avx[n] = rob[h][2]; ps.avy[n] = rob[h][3]; }
            __syncthreads();
            // ---- (2) the pair terms, shared out over the workgroup
            for (int t = tid; t < n_terms; t += BLOCK) ped_pair_term(c, ps, pair, n, t);
            __syncthreads();
            // ---- (3) the pedestrians at t + h + 1
            if (is_ped) {
                ped_sfm_step(c, field, ps, pair, n, tid, cp.vpref, cp.wp + 2 * cp.head, dt, cp.pp, cp.pvel);
                // the step's predicate for ped_due (ped_finish): the post-move distance to the LAST waypoint under 0.5 m
                const double ddx = cp.pp[0] - cp.wp[2 * (cp.nw - 1)], ddy = cp.pp[1] - cp.wp[2 * (cp.nw - 1) + 1];
                due = sqrt(ddx * ddx + ddy * ddy) < 0.5;
            }
        } else if (is_ped) {
            if (truth) {
                nv::set_vel(cp.pp, cp.cmd[0], cp.cmd[1], dt, 0.0, cp.pvel);          // env.py:662
            } else {
                const double span = (double)(h + 1) * dt;
                cp.pp[0] = x0 + cp.pvel[0] * span;
                cp.pp[1] = y0 + cp.pvel[1] * span;
            }
        }
        if (tid < 64 && mask_of(due) != 0 && exact == HZ) exact = h + 1;             // wave-uniform; thread 0 reports it
        if (is_slot) {                                                               // the rows of step h: slot i on lane i
            const size_t r = (row0 + h) * N + tid;
            double ax = 0.0, ay = 0.0, x = 0.0, y = 0.0;
            if (is_ped) {
                ax = cp.pp[0] - rx0; ay = cp.pp[1] - ry0;
                x = fc * ax + fs * ay; y = fc * ay - fs * ax;                        // navsim_ped_observe's rule 3
                const double dx = cp.pp[0] - rob[h + 1][0], dy = cp.pp[1] - rob[h + 1][1];
                const double dist = sqrt(dx * dx + dy * dy);
                if (dist < md) { md = dist; mstep = h; }
            }
            a.out.pose[3 * r] = cp.pp[0]; a.out.pose[3 * r + 1] = cp.pp[1]; a.out.pose[3 * r + 2] = cp.pp[2];
            a.out.vel[2 * r] = cp.pvel[0]; a.out.vel[2 * r + 1] = cp.pvel[1];
            a.out.rel[2 * r] = (float)x; a.out.rel[2 * r + 1] = (float)y;
        }
    }
    if (is_slot) { a.out.min_dist[(size_t)e * N + tid] = md; a.out.min_step[(size_t)e * N + tid] = mstep; }
    if (tid == 0) a.out.exact_steps[e] = exact;
}
