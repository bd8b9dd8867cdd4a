// kernels_episode.hpp -- episode statistics behind the step (include/navsim.h navsim_episode_stats_update / _clear): one launch
// that reads what the step just wrote -- the rows, reward, done and the info flags -- and keeps per-arena accumulators.
// Not a standalone header: a section of navsim_kernels.hip (preamble.hpp, kernels_field.hpp's wave_min_f64).
#pragma once

// ============================================================================================
// One wavefront per arena, four arenas per workgroup.  The workgroup stages the two threshold tables in LDS once (every
// arena compares against the same two), the wavefront's lanes stride the B beams of the newest scan of the arena's row --
// coalesced float loads -- and one reduction gives the row's minimum clearance and its two any-flags; lane 0 then does the
// arena's scalar bookkeeping.  No private arrays, no scratch.
// ============================================================================================
constexpr int kEpisodeWaves = 4;

struct EpisodeArgs {
    int32_t n_envs, n_beams, n_scan_stack, auto_reset;
    const float* obs;
    const float* final_obs;
    const double* reward;
    const uint8_t* done;
    const float* is_success;
    const float* is_crash;
    const uint8_t* truncated;
    const uint8_t* reset_mask;
    const float* thr;
    const float* dthr;
    navsim_episode_stats s;
};

__global__ __launch_bounds__(64 * kEpisodeWaves) void episode_stats_kernel(EpisodeArgs a) {
    extern __shared__ float s_thr[];                            // [2 B]: scan_threshold, scan_discomfort
    const int B = a.n_beams, S = a.n_scan_stack;
    for (int k = threadIdx.x; k < B; k += 64 * kEpisodeWaves) {
        s_thr[k] = a.thr[k];
        s_thr[B + k] = a.dthr[k];
    }
    __syncthreads();                                            // (every wavefront arrives: nobody has left yet)
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kEpisodeWaves + (threadIdx.x >> 6)));
    if (e >= a.n_envs) return;
    // NEXT_STEP: the call reset this arena -- reward 0, done 0 -- which is no step of any episode
    if (a.auto_reset == NAVSIM_AUTORESET_NEXT_STEP && a.reset_mask[e] != 0) return;
    const bool done = a.done[e] != 0;
    // SAME_STEP: a finished arena's row in obs already is the next episode's first one; the terminal row is in final_obs
    const float* rows = (a.auto_reset == NAVSIM_AUTORESET_SAME_STEP && done) ? a.final_obs : a.obs;
    const float* row = rows + (size_t)e * ((size_t)S * B + NAVSIM_OBS_TAIL);
    const float* scan = row + (size_t)(S - 1) * B;              // the newest scan of the stack; older slots are not read
    // the arena's scalars first (wave-uniform addresses: scalar loads that are in flight while the lanes read the row)
    const navsim_episode_stats& s = a.s;
    const float* tail = row + (size_t)S * B;                    // prev_xy, xy, ... (env.py:455)
    const float x0 = tail[0], y0 = tail[1], x1 = tail[2], y1 = tail[3];
    const double reward = a.reward[e], ret0 = s.ret[e], path0 = s.path_length[e], clear0 = s.min_clearance[e];
    const int32_t length0 = s.length[e], dsteps0 = s.discomfort_steps[e];
    double cmin = __builtin_inf();
    int crash = 0, disc = 0;
    auto beam = [&](float v, int k) {
        const float t = s_thr[k], d = s_thr[B + k];
        const double c = (double)v - (double)t;
        cmin = c < cmin ? c : cmin;
        crash |= v < t;
        disc |= v < d;
    };
    // (four loads in flight per lane; eight, with the table's loads batched as well, measured slower: 7.4 against 6.6 us)
    int k = lane;
    for (; k + 192 < B; k += 256) {
        const float v0 = scan[k], v1 = scan[k + 64], v2 = scan[k + 128], v3 = scan[k + 192];
        beam(v0, k); beam(v1, k + 64); beam(v2, k + 128); beam(v3, k + 192);
    }
    for (; k < B; k += 64) beam(scan[k], k);
    cmin = wave_min_f64(cmin);
    const bool crash_row = __ballot(crash) != 0;
    const bool disc_row = __ballot(disc) != 0 && !crash_row;    // env.py:543-547: discomfort and not crash
    if (lane != 0) return;
    const int32_t length = length0 + 1;
    const double ret = ret0 + reward;
    const double dx = (double)x1 - (double)x0;
    const double dy = (double)y1 - (double)y0;
    const double path = path0 + sqrt(dx * dx + dy * dy);
    const double clear = cmin < clear0 ? cmin : clear0;
    const int32_t dsteps = dsteps0 + (disc_row ? 1 : 0);
    if (!done) {
        s.ret[e] = ret; s.length[e] = length; s.path_length[e] = path; s.min_clearance[e] = clear; s.discomfort_steps[e] = dsteps;
        return;
    }
    const int success = a.is_success[e] != 0.0f, crashed = a.is_crash[e] != 0.0f;
    const int limit = a.truncated != nullptr && a.truncated[e] != 0;
    s.ep_return[e] = ret; s.ep_length[e] = length; s.ep_path_length[e] = path; s.ep_min_clearance[e] = clear;
    s.ep_discomfort_steps[e] = dsteps;
    s.ep_outcome[e] = (uint8_t)(success | (crashed << 1) | (limit << 2));
    if (s.totals) {                                             // integer adds: the sums do not depend on their order
        atomicAdd(&s.totals[0], 1ull);
        if (success) atomicAdd(&s.totals[1], 1ull);
        if (crashed) atomicAdd(&s.totals[2], 1ull);
        if (limit) atomicAdd(&s.totals[3], 1ull);
        atomicAdd(&s.totals[4], (unsigned long long)length);
    }
    s.ret[e] = 0.0; s.length[e] = 0; s.path_length[e] = 0.0; s.min_clearance[e] = __builtin_inf(); s.discomfort_steps[e] = 0;
}

// the accumulators of the masked arenas (mask NULL: all) back to "no step yet": (0, 0, 0, +inf, 0)
__global__ __launch_bounds__(256) void episode_stats_clear_kernel(int n_envs, navsim_episode_stats s, const uint8_t* __restrict__ mask) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_envs || (mask && mask[e] == 0)) return;
    s.ret[e] = 0.0; s.length[e] = 0; s.path_length[e] = 0.0; s.min_clearance[e] = __builtin_inf(); s.discomfort_steps[e] = 0;
}
