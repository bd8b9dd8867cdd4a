// kernels_scan_labels.hpp -- scan ground truth (include/navsim.h navsim_scan_labels): the robot's scan of the current state
// without noise, and per beam what it fell on -- nothing, a wall, a pedestrian's body or a pedestrian's leg, and which
// pedestrian.  Part of the single translation unit navsim_kernels.hip (included inside its anonymous namespace; not a
// standalone header).
//
// One workgroup of kScanLabelsBlock threads per arena, the launch shape of ped_scan_core (kernels_pedscan.hpp) with the robot
// as the lidar: wavefront 0 stages the pedestrians' primitives in dynamic LDS IN THE ORACLE'S ORDER (gather_prims: the sides
// of the pedestrians without legs by ascending pedestrian, then the discs of those with legs -- a ballot gives every
// pedestrian its slot, no atomic counter as in the step, whose slots come in any order); prim_in_range culls them; the beams
// are marched with probe_round / ray_result under march_limit (the step's functions: the same floats); the step's own
// merge_prims_culled_core lowers rng[] -- so `range` is the step's scan by construction.
//
// The attributed merge is a SECOND pass over the same culled beam intervals (form (b) of the two the design weighed; a 64-bit
// (float bits, rank) key reduced by one atomicMin would be a second merge beside the proven one, whose `range` would have to be
// shown equal to the step's): a primitive whose t EQUALS the merged range of a beam does atomicMin(rank[k], p), p its index in
// the oracle's order.  The sequential rule of include/navsim.h -- candidates in order, replace iff t < r, the winner the last
// that lowered r -- names the FIRST candidate in order whose t equals the final minimum, and that is what the minimum over p
// is.  Candidate 0, the static ray, wins every tie: rank[k] holds its value's bits until the merge is done, and a beam whose
// merged range equals it is marked -1 there, below every primitive's index, before the second pass starts.  The comparison is by VALUE, so -0.0f and +0.0f tie (a lidar origin exactly on two primitives' lines): the winner is
// the sequential rule's; the sign of that zero in `range` is whatever the step's atomicMin on the float bits leaves.
// A primitive the cull leaves out cannot come within range_max (prim_in_range), so it lowers no clipped range and labels
// no beam: a beam it would have won clips to range_max and is NAVSIM_BEAM_NONE either way.
// Cost of the second pass: the 10 - 50 beams a primitive spans, evaluated once more.
//
// hits: LDS integer atomics per pedestrian in the last pass over the beams, one store per pedestrian.
//
// No private array survives to the ISA and nothing spills.  Resources (gfx950, -Rpass-analysis=kernel-resource-usage) of the
// eleven forms: 58 - 59 VGPRs, 99 - 106 SGPRs, occupancy 7 - 8 waves per SIMD, scratch 0 bytes per lane, no VGPR or SGPR spill,
// 16 bytes of static LDS (the chunk counter); the dynamic LDS is scan_labels_lds_bytes below.
//
// Measured (profiles/r21_scan_labels/summary.txt, 4096 arenas x 1081 beams): 171.1 us with 20 pedestrians an arena, 138.0 us
// with none -- x 1.14 resp. x 1.67 of the whole step kernel in the same trace, not "about its scan phase".  The march is the
// same probe_round, but in the pedestrian scans' form: a probe reads its tile's 16-byte record from global memory (RECT = 1),
// so a ray is a chain of 8 - 13 dependent global loads, and the kernel is bound by their latency at full occupancy.  The step
// stages the arena's record index in LDS (RECT = 2 on closed maps, no bounds test) and parks its slow rays; neither is here.

struct ScanLabelsArgs { navsim_scan_labels_out out; const uint8_t* skip; };

constexpr int kScanLabelsBlock = 256;

// Dynamic LDS of one arena, in the order of the pointers scan_labels_kernel derives: per beam dir (8 B), rng and rank (4 B
// each: 16 B a beam); per pedestrian slot four sides x 16 B, two discs x 8 B, four intervals x 8 B (a pedestrian is four sides
// or two discs), four owner bytes and one hit counter.  1081 beams and 20 pedestrians: 17.3 + 2.4 KB, eight arenas -- the 2048
// threads a compute unit holds -- resident at once (a fourth array for the static range made it six, and beams strided over the threads five rounds for 4.2: 182 us against 171).
inline size_t scan_labels_lds_bytes(const navsim_config* c) {
    return (size_t)c->n_beams * (sizeof(float2) + 2 * sizeof(float)) + (size_t)c->max_peds * (4 * 16 + 2 * 8 + 4 * 8 + 4 + 4);
}

// the second pass: merge_prims_culled_core's walk (same lanes, same intervals, same aliases), its body replaced
template <int BLOCK>
__device__ __forceinline__ void attribute_prims_culled(int B, float lx, float ly, float stepf, int nseg, int ndisc, const Prims pr,
                                                       const float2* __restrict__ dir, const float* __restrict__ rng,
                                                       int* __restrict__ rank) {
    const int lane = (int)threadIdx.x & 63;
    const float kTwoPiF = 6.2831853f;
    const float Kf = (stepf > 0.0f) ? kTwoPiF / stepf : 0.0f;
    const int nprim = nseg + ndisc;
    constexpr int G = NAVSIM_MERGE_G;
    const int sub = lane & (G - 1);
    const int m_first = (kTwoPiF - 2.0f * stepf > 4.8f) ? 0 : -1;
    for (int p = ((int)threadIdx.x) / G; p < nprim; p += block_threads<BLOCK>() / G) {
        const float klo = pr.info[2 * p], khi = pr.info[2 * p + 1];
        if (klo > khi) continue;
        const bool full = klo < -0.5f * kPrimAllBeams;
        const bool is_seg = p < nseg;
        float a0, a1, a2 = 0.f, a3 = 0.f;
        if (is_seg) { a0 = pr.seg[p][0]; a1 = pr.seg[p][1]; a2 = pr.seg[p][2]; a3 = pr.seg[p][3]; }
        else { a0 = pr.disc[p - nseg][0]; a1 = pr.disc[p - nseg][1]; }
        for (int m = full ? 0 : m_first; m <= (full ? 0 : 1); ++m) {
            int k0 = full ? 0 : (int)floorf(klo + (float)m * Kf);
            int k1 = full ? B - 1 : (int)ceilf(khi + (float)m * Kf);
            k0 = k0 < 0 ? 0 : k0;
            k1 = k1 > B - 1 ? B - 1 : k1;
            for (int k = k0 + sub; k <= k1; k += G) {
                float2 d = dir[k];
                float t = INFINITY;                                 // (accepted: the candidate's own t, whatever r is)
                if (is_seg) nv::seg_merge(t, lx, ly, d.x, d.y, a0, a1, a2, a3);
                else        nv::circle_merge(t, lx, ly, d.x, d.y, a0, a1, nv::kLegRadius);
                if (t == rng[k]) atomicMin(&rank[k], p);
            }
        }
    }
}

template <typename Field, int RULE, bool RECT>
__global__ __launch_bounds__(kScanLabelsBlock) void scan_labels_kernel(navsim_config c, navsim_state st, ScanLabelsArgs a) {
    constexpr int BLOCK = kScanLabelsBlock;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int N = c.max_peds, B = c.n_beams, H = c.map_h, W = c.map_w;
    float* out_range = a.out.range + (size_t)e * B;
    uint8_t* out_label = a.out.label + (size_t)e * B;
    int8_t* out_index = a.out.index + (size_t)e * B;
    int32_t* out_hits = a.out.hits ? a.out.hits + (size_t)e * N : nullptr;
    if (a.skip && a.skip[e]) {                                                       // rule 1
        for (int k = tid; k < B; k += BLOCK) { out_range[k] = 0.0f; out_label[k] = NAVSIM_BEAM_NONE; out_index[k] = -1; }
        if (out_hits)
            for (int i = tid; i < N; i += BLOCK) out_hits[i] = 0;
        return;
    }
    float2* dir = (float2*)dyn;
    float* rng = (float*)(dyn + sizeof(float2) * (size_t)B);
    int* rank = (int*)(rng + B);                                                     // (the static range's bits until the merge is done)
    float (*seg)[4] = (float(*)[4])(dyn + 16 * (size_t)B);
    __shared__ int next_chunk;
    if (tid == 0) next_chunk = 0;
    float (*disc)[2] = (float(*)[2])(seg + 4 * N);
    float* info_s = (float*)(disc + 2 * N);
    uint8_t* owner = (uint8_t*)(info_s + 8 * N);
    int* hits = (int*)(owner + 4 * N);

    int n = 0;                                                                       // rule 2
    if (c.ped_model != NAVSIM_PED_NONE) { n = st.n_peds[e]; n = n > N ? N : n; n = n < 0 ? 0 : n; }
    const double* rp = st.robot_pose + 3 * (size_t)e;
    const float lx = (float)rp[0], ly = (float)rp[1], lth = (float)rp[2];          // env.py:386
    int i0, j0;
    nv::xy_to_ij_f32(lx, ly, c, i0, j0);                                             // env.py:419

    // rule 4: the primitives, each pedestrian's at the place the oracle's loop gives it (N <= 64: one lane per pedestrian)
    int nseg = 0, ndisc = 0;
    if (n > 0) {
        bool legged = false;
        if (tid < 64) {
            const size_t pq = (size_t)e * N + (tid < n ? tid : 0);
            legged = tid < n && st.ped_has_legs[pq] && c.lidar_legs;
        }
        // (every wavefront needs the counts: they come through LDS behind the barrier below)
        if (tid < 64) {
            const lanemask_t lm = mask_of(legged);
            const int legs_all = __popcll(lm), legs_below = __popcll(lm & ((1ull << tid) - 1ull));
            const int nseg_w = 4 * (n - legs_all);
            if (tid == 0) { ((int*)info_s)[0] = nseg_w; ((int*)info_s)[1] = 2 * legs_all; }
            if (tid < n) {
                const size_t pq = (size_t)e * N + tid;
                const double* pp = st.ped_pose + pq * 3;
                if (legged) {
                    const double* dd = st.ped_dist + pq * 3;
                    float cc[4];
                    nv::leg_centres((float)pp[0], (float)pp[1], (float)pp[2], (float)dd[0], (float)dd[1], (float)dd[2], cc);
                    const int q = 2 * legs_below;
                    disc[q][0] = cc[0]; disc[q][1] = cc[1];
                    disc[q + 1][0] = cc[2]; disc[q + 1][1] = cc[3];
                    owner[nseg_w + q] = (uint8_t)tid; owner[nseg_w + q + 1] = (uint8_t)tid;
                } else {
                    const double fpx[4] = {0.22, -0.22, -0.22, 0.22};   // human.py:5-10
                    const double fpy[4] = {0.19, 0.19, -0.19, -0.19};
                    double s, cs;
                    nv::sincos(pp[2], s, cs);
                    float vx[4], vy[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        vx[v] = (float)((cs * fpx[v] - s * fpy[v]) + pp[0]);
                        vy[v] = (float)((s * fpx[v] + cs * fpy[v]) + pp[1]);
                    }
                    const int q = 4 * (tid - legs_below);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int w = (v + 1) & 3;
                        seg[q + v][0] = vx[v]; seg[q + v][1] = vy[v]; seg[q + v][2] = vx[w]; seg[q + v][3] = vy[w];
                        owner[q + v] = (uint8_t)tid;
                    }
                }
            }
        }
        __syncthreads();
        nseg = ((const int*)info_s)[0]; ndisc = ((const int*)info_s)[1];
        __syncthreads();                                                             // (prim_in_range writes info_s)
    }
    for (int i = tid; i < N; i += BLOCK) hits[i] = 0;
    const Prims pr = {seg, disc, info_s};
    const double step = nv::linspace_step(c);
    const float rmax = (float)c.range_max;
    if (nseg + ndisc)
        prim_in_range<BLOCK>(nseg + ndisc, nseg, lx, ly, prim_cull_range(c.range_max), pr, (float)step, (float)(c.angle_min + (double)lth));

    // rule 3: the static ray of every beam, as ped_scan_core marches it
    const int ms = map_slot_of(c, st, e);
    const Field field(st.field, st.field_overflow, ms, H, W);
    const char* rects = RECT ? (const char*)st.rect_table + (size_t)ms * rect_tiles_per_map(H, W) * sizeof(uint4) : nullptr;
    const unsigned tpr = (unsigned)((W + 7) >> kRectShift);
    const float max_range = march_limit(H, W, c.range_max, c.resolution);
    const float res = (float)c.resolution;
    const float x0 = (float)i0, y0 = (float)j0;
    double sT = 0.0, cT = 1.0;
    if (st.beam_table) nv::sincos((double)lth, sT, cT);
    __syncthreads();                                                                 // next_chunk (and, with pedestrians, info_s)
    // 64 adjacent beams at a time, handed out as wavefronts finish (1081 beams are 17 such chunks for four wavefronts)
    for (;;) {
        int chunk = 0;
        if ((tid & 63) == 0) chunk = atomicAdd(&next_chunk, 1);
        chunk = __builtin_amdgcn_readfirstlane(chunk);
        if (chunk * 64 >= B) break;
        const int k = chunk * 64 + (tid & 63);
        if (k < B) {
            float dx, dy;
            beam_dir_k(c, st.beam_table, k, step, (double)lth, cT, sT, dx, dy);
            dir[k] = make_float2(dx, dy);
            float t = 0.0f;
            lanemask_t active = mask_of(true), hit = 0;
            while (active != 0)
                probe_round<Field, RULE, RECT>(field, rects, tpr, x0, y0, dx, dy, (unsigned)W, (unsigned)H, max_range, t, active, hit);
            const float r = ray_result<RULE>(hit, int_range_ok(H, W), i0, j0, x0, y0, dx, dy, t, max_range) * res;
            rng[k] = r; rank[k] = __float_as_int(r);
        }
    }
    __syncthreads();
    const bool merged = (nseg + ndisc) != 0;
    if (merged) {                                                                    // rule 5
        merge_prims_culled_core<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng);
        __syncthreads();
        for (int k = tid; k < B; k += BLOCK) rank[k] = (rng[k] == __int_as_float(rank[k])) ? -1 : 0x7FFFFFFF;
        __syncthreads();
        attribute_prims_culled<BLOCK>(B, lx, ly, (float)step, nseg, ndisc, pr, dir, rng, rank);
        __syncthreads();
    }
    for (int k = tid; k < B; k += BLOCK) {                                           // rule 6
        float r = rng[k];
        const int w = rank[k];
        const bool wall = !merged || w < 0 || w == 0x7FFFFFFF;
        r = r < 0.0f ? 0.0f : r;                                                     // env.py:435
        r = r > rmax ? rmax : r;
        int label = NAVSIM_BEAM_WALL, idx = -1;
        if (r == rmax) label = NAVSIM_BEAM_NONE;
        else if (!wall) {
            label = w < nseg ? NAVSIM_BEAM_PED_BODY : NAVSIM_BEAM_PED_LEG;
            idx = owner[w];
            atomicAdd(&hits[idx], 1);
        }
        out_range[k] = r; out_label[k] = (uint8_t)label; out_index[k] = (int8_t)idx;
    }
    if (out_hits) {                                                                  // rule 7
        __syncthreads();
        for (int i = tid; i < N; i += BLOCK) out_hits[i] = hits[i];
    }
}
