// navsim_kernels.hip -- hand-written gfx950 kernels + the C ABI of include/navsim.h.
//
// Hot path: NavGymEnv.step (nav_gym/src/nav_gym_env/env.py:591-728 of leekwoon/nav-gym), batched
// over E independent arenas.  One workgroup owns one arena for the whole step: pedestrian update,
// robot integration, lidar ray-march over the arena's distance field, reward / done / info,
// crash revert (or respawn) with re-scan and observation packing all happen in ONE launch, so the
// only HBM traffic is the distance-field sectors the rays touch, the arena's small state and the
// observation row written once.  No MFMA on that path (there is no dense contraction in it); the one dense
// layer of the widened rows, HumanPolicy's 4096 -> 256, runs on v_mfma_f32_32x32x2_f32 (kernels_policy.hpp).
//
// Nine translation units (csrc/Makefile builds them in parallel): this file -- every kernel but the fused step, the launch
// geometry / dispatch and the C ABI -- and navsim_step_inst.hip compiled once per (threads per arena, pedestrians or not)
// family of the step kernel.  The sections (included inside each unit's anonymous namespace; not standalone headers):
//   kernels_field.hpp    distance transform, field formats, march step, mirror primitives
//   kernels_rect.hpp     two-rectangle records of the field's 8x8 tiles: builder and decode
//   kernels_step.hpp     probe round / scan / merge / pedestrian phase / the fused step kernel
//   kernels_plan.hpp     shortest paths on the costmap, waypoints, the re-plan of one pedestrian
//   kernels_reset.hpp    navsim_regen, costmap, navsim_plan, navsim_replan
//   kernels_policy.hpp   pedestrian control block with the HumanPolicy actor
//   kernels_pedscan.hpp  pedestrian scans (+ ped_scan_lds_bytes, host side), CrowdSim collision block, beam table, test hooks
//   kernels_crowd_maps.hpp  CrowdSim local maps;  kernels_crowd_orca.hpp  CrowdSim pedestrians (ORCA, Agent.step)
//   kernels_ped_orca.hpp  NavGym pedestrians driven by ORCA from the simulator's state (navsim_ped_orca)
//   kernels_episode.hpp  episode statistics behind the step;  kernels_ped_observe.hpp  the K nearest pedestrians in line of sight
//   kernels_goal_path.hpp  distance-to-goal field per arena, the robot's path distance and steering sub-goal (navsim_goal_path)
//   kernels_dwa.hpp  local planner: a dynamic-window action per arena (navsim_dwa)
//   kernels_local_map.hpp  egocentric local map: wall and pedestrian grids per arena in the robot's frame (navsim_local_map)
//   kernels_scan_labels.hpp  scan ground truth: the robot's clean scan and per-beam hit labels (navsim_scan_labels)
//   kernels_replay.hpp   the pieces of the step that the read-only kernels below re-enact (twist, scan pose, primitives, march,
//                        verdict, reward, carried pedestrian, LDS layout), each stated once
//   kernels_lookahead.hpp    action lookahead: the step's outcomes for K candidate actions per arena (navsim_lookahead)
//   kernels_lookahead_obs.hpp  lookahead observations: the step's whole return for K candidate actions per arena (navsim_lookahead_obs)
//   kernels_rollout.hpp      action-sequence rollout: the next H steps' outcomes for K action sequences per arena (navsim_rollout)
//   kernels_rollout_obs.hpp  rollout observations: the next H steps' whole returns for K action sequences per arena (navsim_rollout_obs)
//   kernels_mppi.hpp         MPPI local planner: sampled plans, the rollout's launch, the weighted update (navsim_mppi)
//   kernels_ped_forecast.hpp pedestrian forecast: the pedestrians' next H poses per arena, one launch (navsim_ped_forecast)
//   step_plan.hpp        launch geometry of the fused step, the descriptors of a launch and the march-rule dispatch (shared by this
//                        file and navsim_step_inst.hip; included behind the namespace, its two descriptors are global types)
// Host code of this file, ahead of the C ABI: dispatch_step and the argument checks; the workspaces (Carver and one layout
// function per workspace -- rect_ws, regen_ws, replan_ws, policy_ws -- which the size queries run without a base); the
// shared launchers launch_dt, launch_build_rects, launch_ped_scan, launch_ped_scan_features.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off per unit (nav-gym_amd/csrc/Makefile, driven by build.sh).
#include "preamble.hpp"

namespace {

#include "kernels_field.hpp"
#include "kernels_rect.hpp"
#include "kernels_plan.hpp"
#include "kernels_regen_dev.hpp"
#include "kernels_step.hpp"
#include "kernels_reset.hpp"
#include "kernels_policy.hpp"
#include "kernels_pedscan.hpp"
#include "kernels_crowd_maps.hpp"
#include "kernels_crowd_orca.hpp"
#include "kernels_ped_orca.hpp"
#include "kernels_episode.hpp"
#include "kernels_ped_observe.hpp"
#include "kernels_goal_path.hpp"
#include "kernels_dwa.hpp"
#include "kernels_local_map.hpp"
#include "kernels_scan_labels.hpp"
#include "kernels_replay.hpp"
#include "kernels_lookahead.hpp"
#include "kernels_lookahead_obs.hpp"
#include "kernels_rollout.hpp"
#include "kernels_rollout_obs.hpp"
#include "kernels_mppi.hpp"
#include "kernels_ped_forecast.hpp"

}  // namespace
#include "step_plan.hpp"

// the step kernel's instantiations live in eight units of their own (navsim_step_inst.hip): one launcher per
// (threads per arena, pedestrians or not)
#define NAVSIM_STEP_FAMILY(B, P) \
    extern "C" int navsim_step_launch_##B##_##P(const navsim_config*, const navsim_state*, const navsim_step_io*, \
                                                const StepLaunch*, const StepPlan*); \
    extern "C" int navsim_step_set_stamps_##B##_##P(unsigned long long*);
NAVSIM_STEP_FAMILY(64, 0) NAVSIM_STEP_FAMILY(64, 1) NAVSIM_STEP_FAMILY(256, 0) NAVSIM_STEP_FAMILY(256, 1)
NAVSIM_STEP_FAMILY(512, 0) NAVSIM_STEP_FAMILY(512, 1) NAVSIM_STEP_FAMILY(1024, 0) NAVSIM_STEP_FAMILY(1024, 1)
#undef NAVSIM_STEP_FAMILY

#ifndef NAVSIM_PLAN_MANY_SEARCHES
#define NAVSIM_PLAN_MANY_SEARCHES 4096          // searches per planner launch of navsim_regen ABOVE which 512 threads per search are used (staging passes; the per-step calls stay below)
#endif

namespace {

// navsim_debug_kernarg_layout: the views against the copies (the four leading parameters of the install kernels + one scalar)
__global__ void kernarg_layout_probe_kernel(navsim_config c_, navsim_state st_, navsim_step_io io_, StepInstall in_, int tail, int* out) {
    const StepInstallKernargs& ka = *(const StepInstallKernargs*)__builtin_amdgcn_kernarg_segment_ptr();
    if (threadIdx.x != 0) return;
    auto same = [](const void* a, const void* b, size_t n) {
        const unsigned char* x = (const unsigned char*)a;
        const unsigned char* y = (const unsigned char*)b;
        for (size_t i = 0; i < n; ++i) if (x[i] != y[i]) return false;
        return true;
    };
    const int tail_view = *(const int*)((const char*)&ka + sizeof(StepInstallKernargs));     // the scalar behind the structs
    *out = (same(&c_, &ka.c, sizeof(c_)) && same(&st_, &ka.st, sizeof(st_)) && same(&io_, &ka.io, sizeof(io_)) &&
            same(&in_, &ka.in, sizeof(in_)) && tail_view == tail && tail == 0x1234567) ? 1 : 0;
}

// One launch of the fused step: plans it and hands it to the family's launcher (navsim_step_inst.hip).
int dispatch_step(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, StepLaunch l) {
    // (a NAVSIM_STEP_DUE launch and the front of the re-plan are the ordinary step on other workgroups: their grid does not change the plan)
    const StepPlan p = plan_step(c, st, l.part == NAVSIM_STEP_DUE || l.part == kStepPartReplan ? 0 : l.grid);
    const bool peds = c->ped_model != NAVSIM_PED_NONE;
    // the culled merge of pedestrian primitives walks the 2 pi aliases m <= 1 of a bearing (kernels_step.hpp
    // merge_prims_culled_core): a field of view above 2 pi has beams that need m = 2, and is refused where anything is merged
    if (peds && c->angle_last - c->angle_min > nv::kTwoPi) return NAVSIM_E_UNSUPPORTED;
    const bool split = peds && !l.reset_only && ped_split_on(c);               // pedestrians ahead of the step (ped_split_on)
    // a state with slot tables (navsim_state.map_slot): only the INSTALL instantiations look a map up through the table -- every
    // launch goes to them, with nothing to install unless navsim_step_install says so
    const StepInstall no_install = {};
    if (st->map_slot && !l.install) {
        if (l.part != NAVSIM_STEP_ALL || c->field_format != NAVSIM_FIELD_U16T || split)
            return NAVSIM_E_UNSUPPORTED;                                    // navsim_step_part / navsim_step_replan, float32 fields
        l.install = &no_install;
    }
    if (split && !l.prepare_only) {
        const size_t pl = ped_update_lds_bytes(c);
        const int G = ped_pack(c->max_peds), pgrid = (c->n_envs + G - 1) / G;
        if (c->field_format == NAVSIM_FIELD_U16T) ped_update_kernel<FieldU16T><<<pgrid, kPedUpdateBlock, pl, l.stream>>>(*c, *st);
        else                                      ped_update_kernel<FieldF32><<<pgrid, kPedUpdateBlock, pl, l.stream>>>(*c, *st);
        l.peds_done = true;
    }
    int rc;
#define NAVSIM_STEP_CASE(B) \
    case B: rc = peds ? navsim_step_launch_##B##_1(c, st, io, &l, &p) : navsim_step_launch_##B##_0(c, st, io, &l, &p); break;
    switch (p.block) {
        NAVSIM_STEP_CASE(64) NAVSIM_STEP_CASE(256) NAVSIM_STEP_CASE(512) NAVSIM_STEP_CASE(1024)
        default:   return NAVSIM_E_UNSUPPORTED;
    }
#undef NAVSIM_STEP_CASE
    return rc != NAVSIM_OK ? rc : launch_status();
}

// workgroups of navsim_step_part's compact launch and of navsim_step_replan's front: the arenas with a waiting pedestrian are
// few (~2 % per step on the c3 world) -- E / 16, as many as wait in an ordinary step several times over
int compact_grid(const navsim_config* c) {
    const int g = c->n_envs / 16 < 32 ? 32 : (c->n_envs / 16 > 1024 ? 1024 : c->n_envs / 16);
    return g > c->n_envs ? c->n_envs : g;
}

// May navsim_replan of the previous step's flags run inside this step's launch (navsim_step_replan, navsim_step_install_replan)?
// NAVSIM_OK, or the code the entry points refuse the call with.  navsim_prepare asks about the configuration alone
// (strict = false: no pair of flag buffers, any costmap plan_fits accepts) and skips the form where the answer is no.
int replan_in_step(const navsim_config* c, const navsim_state* st, bool strict) {
    if (c->ped_model == NAVSIM_PED_NONE || !st->costmap) return NAVSIM_E_ARG;
    if (strict && (!st->ped_due_prev || !st->ped_due || st->ped_due == st->ped_due_prev)) return NAVSIM_E_ARG;
    if (ped_split_on(c)) return NAVSIM_E_UNSUPPORTED;                  // ped_update_kernel advances the pedestrians ahead of the launch
    const int Hc = c->map_h / 5, Wc = c->map_w / 5;
    if (!plan_fits(Hc, Wc) || (strict && (Hc < 1 || Wc < 1 || plan_lds(Hc, Wc) > 64 * 1024))) return NAVSIM_E_UNSUPPORTED;
    // the search inside the step's launch owns one costmap word per thread (its registers are the step kernel's): costmaps of
    // more words than the arena's workgroup has threads go through navsim_replan + navsim_step_part
    return (int)plan_words(Hc, Wc) > plan_step(c, st).block ? NAVSIM_E_UNSUPPORTED : NAVSIM_OK;
}

int check_step_args(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, int reset_only) {
    if (!c || !st || !io) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->n_beams < 1 || c->n_scan_stack < 1 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (c->max_peds > NAVSIM_MAX_PEDS) return NAVSIM_E_UNSUPPORTED;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (c->march_rule < NAVSIM_MARCH_F64 || c->march_rule > NAVSIM_MARCH_F32_FMA) return NAVSIM_E_ARG;
    if (c->action_kind != NAVSIM_ACTION_TWIST && c->action_kind != NAVSIM_ACTION_WHEELS) return NAVSIM_E_ARG;
    if (c->action_kind == NAVSIM_ACTION_WHEELS && !(c->wheel_track > 0.0)) return NAVSIM_E_ARG;
    if (c->defer_reset_scan != 0 && c->defer_reset_scan != 1) return NAVSIM_E_ARG;
    if (c->auto_reset < NAVSIM_AUTORESET_NONE || c->auto_reset > NAVSIM_AUTORESET_NEXT_STEP) return NAVSIM_E_ARG;
    if (io->final_goals && !io->final_obs) return NAVSIM_E_ARG;
    if (io->reset_mask && !reset_only) {
        if (io->reset_mask == io->done) return NAVSIM_E_ARG;                       // the launch reads one and writes the other
        if (c->ped_model != NAVSIM_PED_NONE && ped_split_on(c)) return NAVSIM_E_UNSUPPORTED;   // ped_update_kernel advances every arena
    }
    if (c->regen_min_steps < 0 || c->max_episode_steps < 0) return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;              // one map for all arenas has no slots to choose from
    if (c->ped_model != NAVSIM_PED_NONE && (c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS)) return NAVSIM_E_ARG;
    if (st->rect_table && (c->field_format != NAVSIM_FIELD_U16T || c->map_h > 1024 || c->map_w > 1024)) return NAVSIM_E_UNSUPPORTED;
    if (st->rect_index && !st->rect_table) return NAVSIM_E_ARG;
    if (c->step_block != 0 && c->step_block != 64 && c->step_block != 256 && c->step_block != 512 &&
        c->step_block != 1024) return NAVSIM_E_ARG;
    if (c->ped_split < 0 || c->ped_split > 2 || c->rect_lds < 0 || c->rect_lds > 2) return NAVSIM_E_ARG;
    if (c->ped_model != NAVSIM_PED_NONE && c->max_peds < 1) return NAVSIM_E_ARG;
    if (plan_step(c, st).lds > kLdsPerCu) return NAVSIM_E_UNSUPPORTED;   // beams x pedestrians beyond one CU's LDS
    // navsim_regen's first observations are a launch of their own geometry (plan_step's `lone` rule): validate it here too
    if (c->regen_cap > 0 && plan_step(c, st, c->regen_cap).lds > kLdsPerCu) return NAVSIM_E_UNSUPPORTED;
    if (!st->field || !st->scan_threshold || !st->scan_discomfort || !st->robot_pose || !st->robot_goal ||
        !st->prev_action || !st->prev_pose || !st->n_hist || !st->episode || !st->steps || !io->obs)
        return NAVSIM_E_ARG;
    if (!reset_only && (!io->action || !io->reward || !io->done || !io->is_success || !io->is_crash ||
                        !io->distance))
        return NAVSIM_E_ARG;
    if (!reset_only && c->n_scan_stack > 1 && !io->obs_prev) return NAVSIM_E_ARG;
    if (c->ped_model != NAVSIM_PED_NONE) {
        if (!st->n_peds || !st->ped_pose || !st->ped_vel || !st->ped_prev_yaw || !st->ped_dist ||
            !st->ped_has_legs || !st->ped_waypoints || !st->ped_n_waypoints || !st->ped_wp_head)
            return NAVSIM_E_ARG;
        if (c->ped_model == NAVSIM_PED_EXTERNAL && !st->ped_cmd && !reset_only) return NAVSIM_E_ARG;
        if (c->ped_model == NAVSIM_PED_SFM && !st->ped_v_pref) return NAVSIM_E_ARG;
    }
    if (c->auto_reset && c->n_spawn > 0 && (!st->spawn_pose || !st->spawn_goal)) return NAVSIM_E_ARG;
    return NAVSIM_OK;
}

// navsim_regen_swap / navsim_step_install: the live and the staged state as a pair
int check_stage_pair(const navsim_config* c, const navsim_state* live, const navsim_state* stage) {
    if (c->regen_cap < 1 || c->n_spawn < 1 || !c->auto_reset) return NAVSIM_E_ARG;
    if (c->defer_reset_scan) return NAVSIM_E_UNSUPPORTED;     // a staged world brings its own first observation; arenas beyond the cap would get none
    if (!live->field || !stage->field || !live->episode || !stage->episode || !live->spawn_pose || !stage->spawn_pose ||
        !live->spawn_goal || !stage->spawn_goal || !stage->robot_pose || !stage->robot_goal)
        return NAVSIM_E_ARG;
    // the two states must hold the same optional buffers
    if ((live->field_overflow != nullptr) != (stage->field_overflow != nullptr) ||
        (live->rect_table != nullptr) != (stage->rect_table != nullptr) || (live->rect_index != nullptr) != (stage->rect_index != nullptr) ||
        (live->costmap != nullptr) != (stage->costmap != nullptr) || (live->ped_goal != nullptr) != (stage->ped_goal != nullptr))
        return NAVSIM_E_ARG;
    return NAVSIM_OK;
}
// navsim_state.map_slot: both states or neither, and then over the SAME five arrays
int check_map_slots(const navsim_state* live, const navsim_state* stage) {
    if ((live->map_slot != nullptr) != (stage->map_slot != nullptr)) return NAVSIM_E_ARG;
    if (live->map_slot && (live->map_slot == stage->map_slot || live->field != stage->field || live->field_overflow != stage->field_overflow ||
                           live->rect_table != stage->rect_table || live->rect_index != stage->rect_index || live->costmap != stage->costmap))
        return NAVSIM_E_ARG;
    return NAVSIM_OK;
}
template <typename Big>
void stage_big_buffers(const navsim_config* c, const navsim_state* live, const navsim_state* stage, Big big[5]) {
    const int H = c->map_h, W = c->map_w;
    big[0] = {(char*)live->field, (const char*)stage->field, navsim_field_bytes(1, H, W, c->field_format)};
    if (live->field_overflow) big[1] = {(char*)live->field_overflow, (const char*)stage->field_overflow, (size_t)H * W * sizeof(float)};
    if (live->rect_table) big[2] = {(char*)live->rect_table, (const char*)stage->rect_table, navsim_rect_table_bytes(1, H, W)};
    if (live->costmap) big[3] = {(char*)live->costmap, (const char*)stage->costmap, (size_t)(H / 5) * (W / 5)};
    if (live->rect_index) big[4] = {(char*)live->rect_index, (const char*)stage->rect_index, rect_index_row_bytes(H, W)};
}

int step_install_impl(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const navsim_state* stage,
                      const float* stage_obs, uint8_t* mark, const long long* ready, uint8_t* late, uint8_t* late_next,
                      const uint8_t* late_prev, int32_t max_queries, void* stream) {
    (void)hipGetLastError();
    int rc = check_step_args(c, st, io, 0);
    if (rc != NAVSIM_OK) return rc;
    if (!stage || !stage_obs || !mark || !ready || ((uintptr_t)mark & 3) != 0 || !st->done_steps) return NAVSIM_E_ARG;
    // what makes the outcome independent of the staging passes' timing: the rule (cfg.regen_min_steps, with the caller's order of
    // passes and waits) or the fallback (late: arenas whose world was not ready are generated by the caller's navsim_regen)
    // NEXT_STEP, neither: an arena that finds nothing staged regenerates its own world inside the launch (regen_lone) -- worlds of
    // outdoor maps without planning / costmap, at least 256 threads per arena
    const bool lone = c->auto_reset == NAVSIM_AUTORESET_NEXT_STEP && !late && !late_next && c->regen_min_steps < 1;
    if (lone && (c->regen_indoor_ratio > 0.0 || c->regen_plan || st->costmap || plan_step(c, st).block < 256 || c->map_h != c->map_w ||
                 march_rule_variant(c) != NAVSIM_MARCH_F32 ||
                 c->obstacle_number > 64 || c->obstacle_number_hi > 64))
        return NAVSIM_E_UNSUPPORTED;
    if (c->regen_min_steps < 1 && !late && !late_next && !lone) return NAVSIM_E_ARG;
    rc = check_stage_pair(c, st, stage);
    if (rc != NAVSIM_OK) return rc;
    // every finished arena decides for itself: there is no cap to apply in index order (navsim_regen_swap has one)
    if (c->regen_cap < c->n_envs) return NAVSIM_E_UNSUPPORTED;
    if (c->field_format != NAVSIM_FIELD_U16T || (c->ped_model != NAVSIM_PED_NONE && ped_split_on(c))) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    rc = check_map_slots(st, stage);
    if (rc != NAVSIM_OK) return rc;
    StepInstall in = {};
    in.stage = *stage; in.stage_obs = stage_obs; in.mark = mark; in.ready = ready; in.late = late;
    in.late_next = late_next; in.late_prev = late_prev; in.lone = lone ? 1 : 0;
    if (!st->map_slot) stage_big_buffers(c, st, stage, in.big);             // (with slot tables the maps stay where they are)
    StepLaunch l;
    l.install = &in;
    l.stream = (hipStream_t)stream;
    if (max_queries >= 0) {     // ... with navsim_replan of the previous step's flags inside the launch (navsim_step_replan's conditions)
        rc = replan_in_step(c, st, true);
        if (rc != NAVSIM_OK) return rc;
        l.part = kStepPartReplan;
        l.grid = compact_grid(c);
        l.max_queries = max_queries;
    }
    return dispatch_step(c, st, io, l);
}

// navsim_regen's fork: the distance transform of the new corridor maps beside the planner's first stage (which needs the
// occupancy grid and the costmap only).  One helper stream and two events per host thread and device, created on first use;
// inside a hipGraph capture the helper joins the capture through the first wait and leaves it through the second.
struct RegenFork { int device = -1; hipStream_t side = nullptr; hipEvent_t forked = nullptr, joined = nullptr; };
thread_local hipStream_t g_regen_helper = nullptr;          // navsim_regen_helper: the caller's choice of helper stream
RegenFork* regen_fork() {
    thread_local RegenFork f;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (f.device == dev && g_regen_helper && f.side != g_regen_helper) f.side = g_regen_helper;     // (the events stay)
    if (f.device != dev) {
        RegenFork n;
        if (g_regen_helper) n.side = g_regen_helper;
        else if (hipStreamCreateWithFlags(&n.side, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&n.forked, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&n.joined, hipEventDisableTiming) != hipSuccess) return nullptr;
        n.device = dev;
        f = n;                                               // (what an earlier device of this thread held stays allocated)
    }
    return &f;
}

// ---- workspaces: each layout is written once; its size query is the same walk without a base ----
// Carves a caller's buffer: every sub-buffer starts on a 256-byte boundary.  base may be null: the pointers are then
// null and only the offset, the bytes needed so far, means anything.
struct Carver {
    char* base;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};
template <typename T> T* at(T* p, size_t i) { return p ? p + i : nullptr; }       // an element of one take (null stays null)

// the rect builder's scratch for m maps: transposed occupancy, then the four int16 run arrays hl, hr, vt, vb
struct RectWs { uint8_t* occT; int16_t* run[4]; size_t bytes; };
RectWs rect_ws(void* base, size_t m, size_t cells) {
    Carver w{(char*)base};
    RectWs r;
    r.occT = w.take<uint8_t>(m * cells);
    int16_t* runs = w.take<int16_t>(4 * m * cells);
    for (int k = 0; k < 4; ++k) r.run[k] = at(runs, k * m * cells);
    r.bytes = w.off;
    return r;
}

// navsim_regen.  ovf: the exact float plane of large packed maps; rects: rect records to rebuild; plan: cfg.regen_plan
struct RegenWs {
    int *count, *list, *slots;      // the selection: count (4 words), the listed arenas, the map slots of the list (navsim_state.map_slot)
    uint8_t *occ, *grids;           // occupancy scratch, corridor grids
    uint16_t* cols;                 // column pass of the distance transform
    char* field;                    // the new maps' fields, fbytes each
    int* kind; float* ovf; RectWs rect;
    RegenPlanWs plan;               // (its pointers; navsim_regen fills in the rest)
    size_t fbytes, bytes;
};
RegenWs regen_ws(const navsim_config* c, void* base, bool ovf, bool rects, bool plan) {
    const size_t M = (size_t)c->regen_cap, cells = (size_t)c->map_h * c->map_w;
    Carver w{(char*)base};
    RegenWs r = {};
    r.count = w.take<int>(4 + 2 * M);
    r.list = at(r.count, 4);
    r.slots = at(r.list, M);
    w.take<uint8_t>((size_t)c->n_envs);                     // (a mask per arena: no kernel uses it any more)
    r.occ = w.take<uint8_t>(M * cells);
    r.cols = w.take<uint16_t>(M * cells);
    r.fbytes = navsim_field_bytes(1, c->map_h, c->map_w, c->field_format);
    r.field = w.take<char>(M * r.fbytes);
    r.grids = w.take<uint8_t>(M * 10000);
    r.kind = w.take<int>(M);
    if (ovf) r.ovf = w.take<float>(M * cells);
    if (rects) r.rect = rect_ws(w.take<char>(rect_ws(nullptr, M, cells).bytes), M, cells);
    if (plan) {
        const size_t cc = (size_t)(c->map_h / 5) * (c->map_w / 5), P = (size_t)(c->max_waypoints > 0 ? c->max_waypoints : 1);
        const size_t n = M * kRegenRounds * (size_t)(c->n_spawn > c->max_peds ? c->n_spawn : c->max_peds);     // [M, R, Q]
        r.plan.cost = w.take<uint8_t>(M * cc);
        r.plan.qstart = w.take<double>(n * 2);
        r.plan.qgoal = w.take<double>(n * 2);
        r.plan.qtheta = w.take<double>(n);
        r.plan.qwp = w.take<double>(n * P * 2);
        r.plan.qlen = w.take<double>(n);
        r.plan.qcut = w.take<unsigned long long>(n);
        r.plan.qnwp = w.take<int32_t>(n);
        r.plan.active = w.take<uint8_t>(n);
        r.plan.res_robot = w.take<uint8_t>(M * (size_t)c->n_spawn);
    }
    r.bytes = w.off;
    return r;
}
// The layout of a call on `st`: the optional parts that state asks for.  Every sub-buffer sits at a sum of 256-rounded sizes
// of the parts taken before it, so a call that leaves parts out puts nothing further back and never needs more than
// navsim_regen_workspace_bytes, which takes every part that cfg alone cannot exclude.
RegenWs regen_ws_of(const navsim_config* c, const navsim_state* st, void* base) {
    return regen_ws(c, base, c->field_format == NAVSIM_FIELD_U16T && st->field_overflow,
                    st->rect_table && c->regen_indoor_ratio > 0.0, c->regen_plan != 0);
}

// navsim_replan.  due: the flags of the pass over the state (a state without ped_due).  The 256 bytes and the max_queries
// words ahead of them are not used: they held an earlier form's counter and query list, and keep the query what it was.
struct ReplanWs { uint64_t* due; size_t bytes; };
ReplanWs replan_ws(const navsim_config* c, int32_t max_queries, void* base, bool due) {
    Carver w{(char*)base};
    ReplanWs r = {};
    w.take<char>(256);
    w.take<int32_t>((size_t)max_queries);
    if (due) r.due = w.take<uint64_t>((size_t)c->n_envs);
    r.bytes = w.off;
    return r;
}

// navsim_ped_policy / navsim_ped_scan_policy, `chunk` pedestrians per pass
constexpr int kPolicyChunk = 32768;          // pedestrians per pass: bounds the feature scratch (512 MiB)
size_t policy_chunk(const navsim_config* c) {
    const size_t P = (size_t)c->n_envs * (size_t)c->max_peds;
    return P < (size_t)kPolicyChunk ? P : (size_t)kPolicyChunk;
}
struct PolicyWs {
    float *w2t, *cv2t;              // fc2 and conv2 weights, transposed (policy_transpose_kernel)
    double* tab;                    // cos / sin of the 512 beam angles
    float *feat, *h1;               // [chunk, kPolFeat], [chunk, kPolH1]
    size_t bytes;
};
PolicyWs policy_ws(void* base, size_t chunk) {
    Carver w{(char*)base};
    PolicyWs r;
    r.w2t = w.take<float>(kPolH2 * kPolIn2);
    r.cv2t = w.take<float>(32 * 32 * 3);
    r.tab = w.take<double>(2 * 512);
    r.feat = w.take<float>(chunk * kPolFeat);
    r.h1 = w.take<float>(chunk * kPolH1);
    r.bytes = w.off;
    return r;
}

// the two passes of the distance transform for `m` maps: columns into cols, rows into field (format; a packed field also
// fills overflow / n_saturated where given); count + kind: navsim_regen's slot list and map kinds
void launch_dt(const uint8_t* occ, int m, int H, int W, uint16_t* cols, int format, void* field, float* overflow,
               int32_t* n_saturated, const int* count, const int* kind, hipStream_t s) {
    dt_columns_kernel<<<dim3((W + 63) / 64, m), 64 * kColSeg, 0, s>>>(occ, cols, H, W, count, kind);
    if (format == NAVSIM_FIELD_F32)
        dt_rows_kernel<0><<<dim3(H, m), 256, (size_t)W * 4, s>>>(cols, field, nullptr, nullptr, H, W, count, kind);
    else
        dt_rows_kernel<1><<<dim3(H, m), 256, (size_t)W * 4, s>>>(cols, field, overflow, n_saturated, H, W, count, kind);
}

// the three builder passes for `m` maps whose occupancy / field start at occ / field (per-map strides cells /
// field_stride), on the scratch r = rect_ws(m maps); n_live + list: navsim_regen's slot indirection (see rect_tiles_kernel)
void launch_build_rects(const uint8_t* occ, int m, int H, int W, const void* field, size_t field_stride, int format,
                        const float* overflow, uint4* table, const RectWs& r, const int* n_live, const int* list, hipStream_t s) {
    int16_t *hl = r.run[0], *hr = r.run[1], *vt = r.run[2], *vb = r.run[3];
    rect_transpose_kernel<<<dim3((W + 31) / 32, (H + 31) / 32, m), 256, 0, s>>>(occ, r.occT, H, W, n_live);
    rect_runs_kernel<<<dim3(H > W ? H : W, m, 2), 256, (size_t)(H > W ? H : W) * 2 * sizeof(int16_t), s>>>(
        occ, hl, hr, r.occT, vt, vb, H, W, n_live);
    const int n_tiles = (int)rect_tiles_per_map(H, W);
    rect_tiles_kernel<<<dim3((n_tiles + 3) / 4, m), 256, 0, s>>>(occ, hl, hr, vt, vb, H, W, field, overflow, format,
                                                                field_stride, table, n_live, list);
}

// the pedestrian scans' kernels for one field type: the march rule becomes their template argument (with_march_rule)
#ifndef NAVSIM_ONLY_RULE
// (Never launched: a float32 field takes no kMarchF64Exact32.  The library has always carried the two; pruning is another change.)
template __global__ void ped_scan_kernel<FieldF32, 128, kMarchF64Exact32, false>(navsim_config, navsim_state, float* __restrict__, int);
template __global__ void ped_scan_features_kernel<FieldF32, kMarchF64Exact32, false>(
    navsim_config, navsim_state, int, int, const double* __restrict__, float* __restrict__, const float* __restrict__,
    const float* __restrict__, const float* __restrict__, const float* __restrict__, float* __restrict__);
#endif
template <typename F, bool RECT>
int launch_ped_scan(const navsim_config* c, const navsim_state* st, float* out, int e0, int n_e, hipStream_t s) {
    // 128 threads per pedestrian (measured 64 / 128 / 256 / 512: 1.11 / 0.78 / 0.93 / 1.50 ms on c3)
    return with_march_rule<F>(march_rule_variant(c), [&](auto rule) {
        ped_scan_kernel<F, 128, decltype(rule)::value, RECT><<<dim3(c->max_peds, n_e), 128, ped_scan_lds_bytes(c), s>>>(*c, *st, out, e0);
        return NAVSIM_OK;
    });
}
template <typename F, bool RECT>
int launch_ped_scan_features(const navsim_config* c, const navsim_state* st, int p0, int n, const PolicyWs& ws, float* scans_out,
                             const navsim_policy_weights* w, hipStream_t s) {
    // dynamic LDS: the scan region (navsim_ped_scans) and conv1's output [kConvCh][258] share it
    const size_t lds = ped_scan_lds_bytes(c) < kConvLdsBytes ? kConvLdsBytes : ped_scan_lds_bytes(c);
    return with_march_rule<F>(march_rule_variant(c), [&](auto rule) {
        ped_scan_features_kernel<F, decltype(rule)::value, RECT><<<n, 256, lds, s>>>(*c, *st, p0, n, ws.tab, scans_out, w->cv1_w, w->cv1_b,
                                                                                  ws.cv2t, w->cv2_b, ws.feat);
        return NAVSIM_OK;
    });
}

// navsim_ped_observe: one kernel per (field type, cfg.march_rule) -- nine forms.  NAVSIM_MARCH_F64 keeps its float64 form here
// (kernels_field.hpp's float32-only evaluation would be a tenth and an eleventh form for a kernel that marches a few rays).
template <typename F>
int launch_ped_observe(const navsim_config* c, const navsim_state* st, const PedObserveArgs& a, hipStream_t s) {
    const int grid = (c->n_envs + kObserveWaves - 1) / kObserveWaves, block = 64 * kObserveWaves;
    switch (c->march_rule) {
        case NAVSIM_MARCH_F64:     ped_observe_kernel<F, NAVSIM_MARCH_F64><<<grid, block, 0, s>>>(*c, *st, a); break;
        case NAVSIM_MARCH_F32:     ped_observe_kernel<F, NAVSIM_MARCH_F32><<<grid, block, 0, s>>>(*c, *st, a); break;
        case NAVSIM_MARCH_F32_FMA: ped_observe_kernel<F, NAVSIM_MARCH_F32_FMA><<<grid, block, 0, s>>>(*c, *st, a); break;
        default: return NAVSIM_E_ARG;
    }
    return launch_status();
}

// navsim_goal_path: the grid of one rebuilding workgroup in LDS -- 2 bytes of dist (the array rounded up to 16) + 1 byte of class
// per cell of the padded grid (kernels_goal_path.hpp)
size_t goal_lds_bytes(int Hc, int Wc) {
    const size_t cells = (size_t)(Hc + 2) * (Wc + 2);
    return ((cells * 2 + 15) & ~(size_t)15) + ((cells + 15) & ~(size_t)15);
}
constexpr size_t kGoalLdsMax = kLdsPerCu - 8 * 1024;       // the kernel's static LDS (the list: 4 KB) and headroom

thread_local int32_t* g_goal_sweeps = nullptr;      // navsim_debug_goal_path_sweeps

template <typename F>
int launch_goal_path(const navsim_config* c, const navsim_state* st, const GoalFieldArgs& f, const GoalPathArgs& a, hipStream_t s) {
    const size_t lds = goal_lds_bytes(a.Hc, a.Wc);
    if (allow_lds((const void*)goal_field_kernel<F>, lds) != NAVSIM_OK) return NAVSIM_E_UNSUPPORTED;
    // workgroups of launch 1: as many as are resident at once (LDS and the 2048 threads of a compute unit), at most one per arena
    // -- and no fewer than E / 1024: a workgroup tests its arenas' keys one per thread
    const size_t fit = kLdsPerCu / (lds + 4 * 1024 + 64);
    long g = (long)device_cu_count() * (fit >= 2 ? 2 : 1);
    const long least = ((long)c->n_envs + kGoalBlock - 1) / kGoalBlock;
    g = g < least ? least : g;
    const int grid = (int)(g < (long)c->n_envs ? g : (long)c->n_envs);
    goal_field_kernel<F><<<grid, kGoalBlock, lds, s>>>(f);
    const int per = kGoalWaves * 8;                        // arenas per workgroup of launch 2
    goal_query_kernel<F><<<(c->n_envs + per - 1) / per, 64 * kGoalWaves, 0, s>>>(*c, *st, a);
    return launch_status();
}

// navsim_dwa: a workgroup per arena, a lane per candidate; the pedestrians of every step in dynamic LDS (kernels_dwa.hpp)
template <typename F>
int launch_dwa(const navsim_config* c, const navsim_state* st, const DwaArgs& a, hipStream_t s) {
    const int C = a.p.n_v * a.p.n_w, block = 64 * ((C + 63) / 64);
    const size_t lds = a.use_peds ? (size_t)a.p.horizon * c->max_peds * sizeof(double2) : 0;
    dwa_kernel<F><<<c->n_envs, block, lds, s>>>(*c, *st, a);
    return launch_status();
}

// navsim_local_map: arena x strip of cells, four cells and one 16-byte store per thread and channel where the grid and the
// output's alignment allow (kernels_local_map.hpp)
template <typename F>
int launch_local_map(const navsim_config* c, const navsim_state* st, const LocalMapArgs& a, hipStream_t s) {
    const int cells = a.p.size * a.p.size;
    const bool vec = a.p.size % 4 == 0 && ((uintptr_t)a.out & 15u) == 0;
    const int items = vec ? cells / 4 : cells;
    const int block = items <= 64 ? 64 : (items <= 128 ? 128 : kLocalMapBlock);
    const dim3 grid((unsigned)c->n_envs, (unsigned)((items + block - 1) / block));
    if (vec) local_map_kernel<F, 4><<<grid, block, 0, s>>>(*c, *st, a);
    else     local_map_kernel<F, 1><<<grid, block, 0, s>>>(*c, *st, a);
    return launch_status();
}

// The marched launches -- navsim_scan_labels, navsim_lookahead, navsim_lookahead_obs, navsim_rollout, navsim_rollout_obs -- have one
// kernel per (field type, march rule, rect records or not) as the pedestrian scans have them (launch_ped_scan): eleven forms
// each.  A family names its kernel template; launch_marched picks the form and launches it.
#define NAVSIM_MARCHED_FAMILY(NAME, KERNEL) \
    struct NAME { template <typename F, int RULE, bool RECT> static constexpr auto kernel() { return KERNEL<F, RULE, RECT>; } }
NAVSIM_MARCHED_FAMILY(ScanLabelsFamily, scan_labels_kernel);
NAVSIM_MARCHED_FAMILY(LookaheadFamily, lookahead_kernel);
NAVSIM_MARCHED_FAMILY(LookObsFamily, lookahead_obs_kernel);
NAVSIM_MARCHED_FAMILY(RolloutFamily, rollout_kernel);
NAVSIM_MARCHED_FAMILY(RolloutObsFamily, rollout_obs_kernel);
#undef NAVSIM_MARCHED_FAMILY

// f(field_tag<Field>, std::bool_constant<RECT>) for the state's field format and rect records (the argument checks have refused
// every other format, and rect records beside a float32 field)
template <typename F>
int with_field_rects(const navsim_config* c, const navsim_state* st, F&& f) {
    if (c->field_format != NAVSIM_FIELD_U16T) return f(field_tag<FieldF32>{}, std::false_type{});
    return st->rect_table ? f(field_tag<FieldU16T>{}, std::true_type{}) : f(field_tag<FieldU16T>{}, std::false_type{});
}

template <typename Family, typename Args>
int launch_marched(const navsim_config* c, const navsim_state* st, const Args& a, size_t grid, int block, size_t lds, hipStream_t s) {
    return with_field_rects(c, st, [&](auto field, auto rect) {
        using F = typename decltype(field)::type;
        return with_march_rule<F>(march_rule_variant(c), [&](auto rule) {
            auto kernel = Family::template kernel<F, decltype(rule)::value, decltype(rect)::value>();
            if (allow_lds((const void*)kernel, lds) != NAVSIM_OK) return (int)NAVSIM_E_UNSUPPORTED;
            kernel<<<(unsigned)grid, block, lds, s>>>(*c, *st, a);
            return launch_status();
        });
    });
}

// navsim_ped_forecast: a workgroup per arena; one kernel per field type -- three forms (nothing is marched)
template <typename F>
int launch_ped_forecast(const navsim_config* c, const navsim_state* st, const PedForecastArgs& a, hipStream_t s) {
    const size_t lds = ped_forecast_lds_bytes(c, a.model);
    auto kernel = ped_forecast_kernel<F>;
    if (allow_lds((const void*)kernel, lds) != NAVSIM_OK) return NAVSIM_E_UNSUPPORTED;
    kernel<<<c->n_envs, kForecastBlock, lds, s>>>(*c, *st, a);
    return launch_status();
}

}  // namespace


// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

int navsim_abi_version(void) { return NAVSIM_ABI_VERSION; }

const char* navsim_error_string(int code) {
    switch (code) {
        case NAVSIM_OK: return "ok";
        case NAVSIM_E_ARG: return "invalid argument";
        case NAVSIM_E_LAUNCH: return "kernel launch failed";
        case NAVSIM_E_UNSUPPORTED: return "configuration outside compiled limits";
        case NAVSIM_E_NODEVICE: return "no HIP device";
        default: return "unknown error";
    }
}

int navsim_default_config(navsim_config* c) {
    if (!c) return NAVSIM_E_ARG;
    memset(c, 0, sizeof(*c));
    c->n_envs = 1;
    c->n_beams = 512;                          // keti_robot.py:48
    c->map_h = 400; c->map_w = 400;            // map_generator.py:133
    c->max_peds = 16;
    c->n_scan_stack = 1;                       // __init__.py:11
    c->ped_model = NAVSIM_PED_NONE;
    c->lidar_legs = 1;                         // env.py:697
    c->resolution = 0.05;                      // map_generator.py:139
    c->time_step = 0.2;                        // __init__.py:8
    c->angle_min = -3.141592;                  // keti_robot.py:45
    c->angle_last = 3.141592 - 0.0122718463;   // keti_robot.py:44,46 / env.py:389
    c->range_max = 25.0;                       // keti_robot.py:47
    c->axle_offset = 0.14474;                  // keti_robot.py:73
    c->min_turning_radius = 0.0;               // __init__.py:9
    c->distance_threshold = 0.5;               // __init__.py:10
    c->reward_scale = 15.0;                    // __init__.py:19-25
    c->reward_success_factor = 1.0;
    c->reward_crash_factor = 1.0;
    c->reward_progress_factor = 0.001;
    c->reward_forward_factor = 0.0;
    c->reward_rotation_factor = 0.005;
    c->reward_discomfort_factor = 0.01;
    c->sfm_tau = 0.5;
    c->sfm_k_desired = 1.0;
    c->sfm_k_social = 2.1;
    c->sfm_k_obstacle = 10.0;
    c->sfm_lambda = 2.0;
    c->sfm_gamma = 0.35;
    c->sfm_n = 2.0;
    c->sfm_n_prime = 3.0;
    c->sfm_sigma_obstacle = 0.8;
    c->sfm_agent_radius = 0.35;
    c->ped_angle_min = -1.57079632679;      // human.py:13 
    c->ped_angle_last = 1.57079632679 - 0.00613592315;   // human.py:12,14; env.py:389 
    c->ped_range_max = 6.0;                 // human.py:15 
    c->ped_n_beams = 512;                   // human.py:16 
    {   // keti_robot.py:18-23 threshold_footprint 
        const double fp[8] = {0.6, 0.6, -0.7, 0.6, -0.7, -0.6, 0.6, -0.6};
        for (int i = 0; i < 8; ++i) c->robot_seen_footprint[i] = fp[i];
    }
    c->regen_cap = 64;
    c->obstacle_number = 10;                // __init__.py:34
    c->obstacle_width_lo = 0.3;             // __init__.py:35
    c->obstacle_width_hi = 1.0;
    c->spawn_clearance = 1.2;
    c->ped_clearance = 0.5;
    c->min_goal_dist = 10.0;                // __init__.py:17-18
    c->max_goal_dist = 20.0;
    c->ped_min_robot_dist = 4.0;            // env.py:372
    c->ped_min_goal_dist = 10.0;            // env.py:788-791
    c->v_pref_lo = 0.0;                     // __init__.py:14
    c->v_pref_hi = 0.6;
    c->has_legs_ratio = 0.5;                // __init__.py:15
    c->regen_indoor_ratio = 0.0;
    c->obstacle_number_hi = 0;              // = obstacle_number: __init__.py:34 is [10, 10]
    c->corridor_width_lo = 3; c->corridor_width_hi = 4;      // __init__.py:32
    c->iterations_lo = 80; c->iterations_hi = 150;           // __init__.py:33
    c->num_humans_lo = 0; c->num_humans_hi = 0;              // 0: navsim_regen keeps n_peds
    c->scan_noise_std_lo = 0.0; c->scan_noise_std_hi = -1.0; // < 0: navsim_regen keeps scan_noise_std
    c->march_rule = NAVSIM_MARCH_F32;          // RangeLib.h: `float step_coeff = 0.999;` (include/navsim.h NAVSIM_MARCH_*)
    c->max_waypoints = 64;                     // 128 m of route at the 2 m interval (include/navsim.h)
    c->action_kind = NAVSIM_ACTION_TWIST;      // env.py:591
    c->clamp_action = 0;                       // env.py:611-613: never clipped
    c->wheel_radius = 0.1651;                  // third_party/husky_description/urdf/husky.urdf.xacro:67
    c->wheel_track = 0.5708;                   // husky.urdf.xacro:62
    c->linvel_lo = 0.0; c->linvel_hi = 0.5;    // __init__.py:12
    c->rotvel_lo = -0.64; c->rotvel_hi = 0.64; // __init__.py:13
    c->closed_maps = 0;
    c->defer_reset_scan = 0;
    c->regen_check_discomfort = 1;          // env.py:776-781
    c->rect_lds = 0;
    c->step_block = 0;
    c->ped_split = 0;
    c->seed = 1234;
    return NAVSIM_OK;
}

size_t navsim_rect_index_bytes(int32_t n_maps, int32_t H, int32_t W) {
    if (n_maps <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)n_maps * rect_index_row_bytes(H, W);
}

int navsim_build_rect_index(const void* table, int32_t n_maps, int32_t H, int32_t W, void* index, int32_t* n_rects, void* stream) {
    (void)hipGetLastError();
    if (!table || !index || n_maps < 0 || H <= 0 || W <= 0) return NAVSIM_E_ARG;
    if (H > 1024 || W > 1024) return NAVSIM_E_UNSUPPORTED;
    if (n_maps == 0) return NAVSIM_OK;
    rect_index_kernel<<<n_maps, 256, 0, (hipStream_t)stream>>>((const uint4*)table, H, W, (char*)index, n_rects, nullptr, nullptr);
    return launch_status();
}

int navsim_maps_closed(const uint8_t* occ, int32_t n_maps, int32_t H, int32_t W, int32_t* closed, void* stream) {
    (void)hipGetLastError();
    if (!occ || !closed || n_maps < 0 || H <= 0 || W <= 0) return NAVSIM_E_ARG;
    if (n_maps == 0) return NAVSIM_OK;
    maps_closed_kernel<<<n_maps, 256, 0, (hipStream_t)stream>>>(occ, H, W, closed);
    return launch_status();
}

int navsim_world_closed(const navsim_config* c, const navsim_state* st, int32_t* n_open, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !st->field || !n_open || c->n_envs < 0 || c->map_h <= 0 || c->map_w <= 0) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    const int n = c->shared_field ? (c->n_envs > 0 ? 1 : 0) : c->n_envs;
    if (n == 0) return NAVSIM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (c->field_format == NAVSIM_FIELD_F32) world_closed_kernel<FieldF32><<<n, 256, 0, s>>>(st->field, nullptr, c->map_h, c->map_w, n_open, st->map_slot);
    else if (st->field_overflow)             world_closed_kernel<FieldU16T><<<n, 256, 0, s>>>(st->field, st->field_overflow, c->map_h, c->map_w, n_open, st->map_slot);
    else                                     world_closed_kernel<FieldU16TN><<<n, 256, 0, s>>>(st->field, nullptr, c->map_h, c->map_w, n_open, st->map_slot);
    return launch_status();
}

size_t navsim_sizeof_config(void) { return sizeof(navsim_config); }
size_t navsim_sizeof_state(void) { return sizeof(navsim_state); }
size_t navsim_sizeof_step_io(void) { return sizeof(navsim_step_io); }

size_t navsim_build_dt_workspace_bytes(int32_t n_maps, int32_t H, int32_t W) {
    if (n_maps <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)n_maps * H * W * sizeof(uint16_t);
}

size_t navsim_field_bytes(int32_t n_maps, int32_t H, int32_t W, int32_t format) {
    if (n_maps <= 0 || H <= 0 || W <= 0) return 0;
    if (format == NAVSIM_FIELD_F32) return (size_t)n_maps * H * W * sizeof(float);
    if (format == NAVSIM_FIELD_U16T) return (size_t)n_maps * ((H + 7) / 8) * ((W + 7) / 8) * 64 * sizeof(uint16_t);
    return 0;
}

int navsim_build_field(const uint8_t* occ, int32_t n_maps, int32_t H, int32_t W, int32_t format, void* field,
                       float* overflow, int32_t* n_saturated, void* workspace, size_t workspace_bytes,
                       void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!occ || !field || !workspace || n_maps < 0 || H <= 0 || W <= 0) return NAVSIM_E_ARG;
    if (format != NAVSIM_FIELD_F32 && format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (H >= kDtInf || W >= kDtInf || (size_t)W * 4 > 64 * 1024) return NAVSIM_E_UNSUPPORTED;
    size_t per_map = (size_t)H * W * sizeof(uint16_t);
    size_t chunk = workspace_bytes / per_map;
    if (chunk == 0) return NAVSIM_E_ARG;
    if (chunk > 65535) chunk = 65535;
    hipStream_t s = (hipStream_t)stream;
    const size_t field_per_map = navsim_field_bytes(1, H, W, format);
    if (format != NAVSIM_FIELD_F32)        // padding cells of edge tiles are never read; keep them defined
        (void)hipMemsetAsync(field, 0xFF, field_per_map * (size_t)n_maps, s);
    for (int32_t m0 = 0; m0 < n_maps; m0 += (int32_t)chunk) {
        int32_t m = (n_maps - m0 < (int32_t)chunk) ? n_maps - m0 : (int32_t)chunk;
        launch_dt(occ + (size_t)m0 * H * W, m, H, W, (uint16_t*)workspace, format, (char*)field + field_per_map * (size_t)m0,
                  overflow ? overflow + (size_t)m0 * H * W : nullptr, n_saturated, nullptr, nullptr, s);
    }
    return launch_status();
}

size_t navsim_rect_table_bytes(int32_t n_maps, int32_t H, int32_t W) {
    if (n_maps <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)n_maps * rect_tiles_per_map(H, W) * sizeof(uint4);
}

// Scratch per map: transposed occupancy (1 byte per cell) + four int16 run arrays, rounded up to 256 bytes.  A caller who
// wants n_maps maps built in a single pass adds 256 bytes to the product (rect_ws rounds once per array, not per map);
// with less, navsim_build_rects takes the maps in chunks.
constexpr size_t kRectWsPerCell = 1 + 4 * sizeof(int16_t);
size_t navsim_build_rects_workspace_bytes(int32_t n_maps, int32_t H, int32_t W) {
    if (n_maps <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)n_maps * (((size_t)H * W * kRectWsPerCell + 255) & ~(size_t)255);
}

int navsim_build_rects(const uint8_t* occ, int32_t n_maps, int32_t H, int32_t W, const void* field, int32_t format,
                       const float* overflow, void* table, void* workspace, size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!occ || !field || !table || !workspace || n_maps < 0 || H <= 0 || W <= 0) return NAVSIM_E_ARG;
    if (format != NAVSIM_FIELD_F32 && format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (H > 1024 || W > 1024) return NAVSIM_E_UNSUPPORTED;                 // int16 runs, 4 cells per thread in the scans
    const size_t cells = (size_t)H * W;
    size_t chunk = workspace_bytes / (cells * kRectWsPerCell);             // the largest chunk whose layout fits
    if (chunk > 32768) chunk = 32768;
    while (chunk > 0 && rect_ws(nullptr, chunk, cells).bytes > workspace_bytes) --chunk;
    if (chunk == 0) return NAVSIM_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t fstride = navsim_field_bytes(1, H, W, format);
    const size_t n_tiles = rect_tiles_per_map(H, W);
    for (int32_t m0 = 0; m0 < n_maps; m0 += (int32_t)chunk) {
        const int32_t m = (n_maps - m0 < (int32_t)chunk) ? n_maps - m0 : (int32_t)chunk;
        launch_build_rects(occ + (size_t)m0 * cells, m, H, W, (const char*)field + fstride * (size_t)m0, fstride, format,
                           overflow ? overflow + (size_t)m0 * cells : nullptr, (uint4*)table + (size_t)m0 * n_tiles,
                           rect_ws(workspace, (size_t)m, cells), nullptr, nullptr, s);
    }
    return launch_status();
}

int navsim_build_dt(const uint8_t* occ, int32_t n_maps, int32_t H, int32_t W, float* field,
                    void* workspace, size_t workspace_bytes, void* stream) {
    return navsim_build_field(occ, n_maps, H, W, NAVSIM_FIELD_F32, field, nullptr, nullptr, workspace,
                              workspace_bytes, stream);
}

int navsim_cast_static(const float* field, int32_t E, int32_t H, int32_t W, const float* q,
                       int32_t n_per_env, float max_range, int32_t march_rule, float* out, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!field || E < 0 || n_per_env < 0 || H <= 0 || W <= 0) return NAVSIM_E_ARG;
    if (march_rule < NAVSIM_MARCH_F64 || march_rule > NAVSIM_MARCH_F32_FMA) return NAVSIM_E_ARG;
    long long total = (long long)E * n_per_env;
    if (total == 0) return NAVSIM_OK;
    if (!q || !out) return NAVSIM_E_ARG;
    cast_static_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        field, H, W, q, n_per_env, total, max_range, march_rule, out);
    return launch_status();
}

int navsim_render_polys(float* ranges, const double* angles, int32_t E, int32_t B, const float* verts,
                        const int32_t* n_verts, int32_t V, const float* origin, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!ranges || !angles || !verts || !n_verts || !origin || E < 0 || B < 0 || V < 0) return NAVSIM_E_ARG;
    if (E == 0 || B == 0) return NAVSIM_OK;
    render_polys_kernel<<<dim3((B + 255) / 256, E), 256, 0, (hipStream_t)stream>>>(ranges, angles, B, verts,
                                                                                  n_verts, V, origin);
    return launch_status();
}

int navsim_render_legs(float* ranges, const double* angles, int32_t E, int32_t B, const float* agents,
                       const int32_t* n_agents, int32_t A, const float* origin, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!ranges || !angles || !agents || !n_agents || !origin || E < 0 || B < 0 || A < 0) return NAVSIM_E_ARG;
    if (E == 0 || B == 0) return NAVSIM_OK;
    render_legs_kernel<<<dim3((B + 255) / 256, E), 256, 0, (hipStream_t)stream>>>(ranges, angles, B, agents,
                                                                                 n_agents, A, origin);
    return launch_status();
}

int navsim_integrate(double* pose, const double* cmd, double* vel_out, int32_t n, double dt, double off,
                     void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!pose || !cmd || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    integrate_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(pose, cmd, vel_out, n, dt, off);
    return launch_status();
}

int navsim_reward_done(const navsim_config* c, const void* obs, const void* goals, int32_t is64, int32_t n,
                       const float* thr, const float* dthr, double* reward, uint8_t* done,
                       float* is_success, float* is_crash, double* distance, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!c || !obs || !goals || !thr || !dthr || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    if (is64)
        reward_done_kernel<double><<<n, 256, 0, (hipStream_t)stream>>>(
            *c, (const double*)obs, (const double*)goals, thr, dthr, reward, done, is_success, is_crash, distance);
    else
        reward_done_kernel<float><<<n, 256, 0, (hipStream_t)stream>>>(
            *c, (const float*)obs, (const float*)goals, thr, dthr, reward, done, is_success, is_crash, distance);
    return launch_status();
}

int navsim_scan_threshold(const navsim_config* c, const float* fp, int32_t nvert, float* out, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!c || !fp || !out || nvert < 2 || nvert > 16) return NAVSIM_E_ARG;
    scan_threshold_kernel<<<(c->n_beams + 255) / 256, 256, 0, (hipStream_t)stream>>>(*c, fp, nvert, out);
    return launch_status();
}

int navsim_beam_table(const navsim_config* c, double* table, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!c || !table || c->n_beams < 1) return NAVSIM_E_ARG;
    beam_table_kernel<<<(c->n_beams + 255) / 256, 256, 0, (hipStream_t)stream>>>(*c, table);
    return launch_status();
}

int navsim_ped_scans(const navsim_config* c, const navsim_state* st, float* out, void* stream) {
    if (!c) return NAVSIM_E_ARG;
    return navsim_ped_scans_part(c, st, out, 0, c->n_envs, stream);
}

int navsim_ped_scans_part(const navsim_config* c, const navsim_state* st, float* out, int32_t e0, int32_t n_e, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !out || c->ped_model == NAVSIM_PED_NONE || !st->n_peds || !st->ped_pose || !st->robot_pose ||
        !st->field || c->ped_n_beams < 1 || c->max_peds < 1) return NAVSIM_E_ARG;
    if (e0 < 0 || n_e < 0 || (long)e0 + n_e > c->n_envs) return NAVSIM_E_ARG;
    if (c->max_peds > NAVSIM_MAX_PEDS || c->ped_n_beams > 4096) return NAVSIM_E_UNSUPPORTED;
    if (c->ped_angle_last - c->ped_angle_min > nv::kTwoPi) return NAVSIM_E_UNSUPPORTED;     // the culled merge: dispatch_step
    if (n_e == 0) return NAVSIM_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc = NAVSIM_E_UNSUPPORTED;
    if (c->field_format == NAVSIM_FIELD_U16T)
        rc = st->rect_table ? launch_ped_scan<FieldU16T, true>(c, st, out, e0, n_e, s) : launch_ped_scan<FieldU16T, false>(c, st, out, e0, n_e, s);
    else if (c->field_format == NAVSIM_FIELD_F32)
        rc = launch_ped_scan<FieldF32, false>(c, st, out, e0, n_e, s);
    if (rc != NAVSIM_OK) return rc;
    return launch_status();
}

int navsim_costmap(const uint8_t* occ, int32_t n_maps, int32_t H, int32_t W, uint8_t* cost, void* stream) {
    (void)hipGetLastError();
    if (!occ || !cost || n_maps < 0 || H < 5 || W < 5) return NAVSIM_E_ARG;
    if (n_maps == 0) return NAVSIM_OK;
    if (n_maps > 65535) return NAVSIM_E_UNSUPPORTED;
    int cells = (H / 5) * (W / 5);
    costmap_kernel<<<dim3((cells + 255) / 256, n_maps), 256, 0, (hipStream_t)stream>>>(occ, H, W, cost, nullptr, nullptr);
    return launch_status();
}

int navsim_plan(const uint8_t* cost, const int32_t* map_index, int32_t n, int32_t Hc, int32_t Wc, double res_c,
                double ox, double oy, const double* start, const double* goal, double interval, int32_t max_wp,
                double* wp, int32_t* n_wp, int32_t* path_cells, double* path_len, void* stream) {
    (void)hipGetLastError();
    if (!cost || !start || !goal || !wp || !n_wp || n < 0 || Hc <= 0 || Wc <= 0 || max_wp < 1) return NAVSIM_E_ARG;
    if (!plan_fits(Hc, Wc)) return NAVSIM_E_UNSUPPORTED;                // LDS-resident search
    if (n == 0) return NAVSIM_OK;
    if (allow_lds((const void*)plan_kernel, plan_lds(Hc, Wc)) != NAVSIM_OK) return NAVSIM_E_UNSUPPORTED;
    plan_kernel<<<n, 256, plan_lds(Hc, Wc), (hipStream_t)stream>>>(
        cost, map_index, Hc, Wc, res_c, ox, oy, start, goal, interval, max_wp, wp, n_wp, path_cells, path_len);
    return launch_status();
}

size_t navsim_regen_workspace_bytes(const navsim_config* c) {
    if (!c || c->regen_cap < 1) return 0;
    // no state to ask: a packed field may keep rect records, and comes with the float plane above kRegenMaxPackedSide cells per side
    const bool packed = c->field_format == NAVSIM_FIELD_U16T;
    return regen_ws(c, nullptr, packed && c->map_h > kRegenMaxPackedSide, packed, c->regen_plan != 0).bytes;
}

int navsim_regen_helper(void* stream) {
    g_regen_helper = (hipStream_t)stream;
    return NAVSIM_OK;
}

int navsim_regen(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, void* workspace,
                 size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !io || !io->done || !io->obs || !workspace) return NAVSIM_E_ARG;
    if (c->obstacle_number < 0 || c->corridor_width_lo < 1 ||
        c->corridor_width_hi < c->corridor_width_lo || c->iterations_lo < 1 || c->iterations_hi < c->iterations_lo ||
        c->num_humans_lo < 0 || (c->num_humans_hi > 0 && c->num_humans_hi < c->num_humans_lo))
        return NAVSIM_E_ARG;
    if (c->map_h != c->map_w || c->n_spawn < 1 || c->regen_cap < 1 || c->obstacle_number > 64 || c->obstacle_number_hi > 64 ||
        c->corridor_width_hi > 16 ||
        (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) || c->shared_field)
        return NAVSIM_E_UNSUPPORTED;
    // A packed field needs its float32 overflow plane wherever a cell reaches d2 >= 65535.  Every map this function
    // draws has a 5-cell border wall: the farthest a cell can be from it is map_h / 2 - 5 cells, which stays below
    // 255.99 up to 520 cells per side -- such worlds never have a plane (and must not: the step then uses the
    // decoder without the escape test).  Larger packed maps MUST come with the plane; it is regenerated with the field.
    const bool big = c->map_h > kRegenMaxPackedSide;
    if (c->field_format == NAVSIM_FIELD_U16T && (big != (st->field_overflow != nullptr))) return NAVSIM_E_UNSUPPORTED;
    if (c->field_format == NAVSIM_FIELD_F32 && st->field_overflow) return NAVSIM_E_UNSUPPORTED;
    if (st->rect_table && (c->field_format != NAVSIM_FIELD_U16T || c->map_h > 1024)) return NAVSIM_E_UNSUPPORTED;
    const RegenWs ws = regen_ws_of(c, st, workspace);
    if (ws.bytes > workspace_bytes || !st->spawn_pose || !st->spawn_goal) return NAVSIM_E_ARG;
    if (c->regen_plan && (c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS)) return NAVSIM_E_ARG;
    if (c->regen_min_steps < 0 || (c->regen_min_steps > 0 && !st->done_steps)) return NAVSIM_E_ARG;
    if (c->regen_plan && (c->n_spawn > 256 || c->map_h < 5 || !plan_fits(c->map_h / 5, c->map_w / 5) ||
                          plan_lds(c->map_h / 5, c->map_w / 5) > 64 * 1024))
        return NAVSIM_E_UNSUPPORTED;
    int rc = check_step_args(c, st, io, 1);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int M = c->regen_cap, H = c->map_h, W = c->map_w;
    const size_t cells = (size_t)H * W;
    int *count = ws.count, *list = ws.list, *kind = ws.kind;
    int* mlist = st->map_slot ? ws.slots : list;            // where the maps of the listed arenas live (regen_map_list_kernel)
    uint8_t *occ = ws.occ, *grids = ws.grids;
    char* fscratch = ws.field;
    const size_t fbytes = ws.fbytes;
    float* ovf_scratch = ws.ovf;                            // exact float plane of the new maps (large packed maps), or null
    // opens the call: every workgroup selects its arena from the done flags (list[b], -1 = none; count), draws the
    // per-episode parameters and the map kind, grows the corridor tree of a corridor map
    // (worlds of outdoor maps only: regen_maps_kernel opens the call itself, one launch less)
    // (a world of outdoor maps that keeps rect records: regen_maps_kernel writes the records of a new map from the
    // generator's rectangles, regen_rect_records -- no search, no verification pass, no builder launches)
    const bool direct = !(c->regen_indoor_ratio > 0.0);
    uint4* direct_rects = (direct && st->rect_table) ? (uint4*)st->rect_table : nullptr;
    char* direct_index = (direct_rects && st->rect_index) ? (char*)st->rect_index : nullptr;
    if (!direct) regen_indoor_kernel<<<M, 256, 0, s>>>(*c, *st, io->done, M, count, list, grids, kind);
    // Outdoor maps only and no rect records to rebuild: the field of a new map is written straight into the arena's
    // own buffers (no per-slot scratch, no copy kernel), and the occupancy scratch only if a costmap wants it.
    const bool need_occ = !direct || c->regen_plan || st->costmap;
    if (!direct && c->field_format == NAVSIM_FIELD_U16T) (void)hipMemsetAsync(fscratch, 0xFF, fbytes * (size_t)M, s);
    // maps and, for outdoor maps, their exact field from the geometry; corridor maps go through the distance transform
    regen_maps_kernel<<<regen_grid(M), 256, 0, s>>>(*c, *st, count, list, need_occ ? occ : nullptr, grids, kind,
                                                            fscratch, fbytes, ovf_scratch, direct ? 1 : 0,
                                                            direct ? io->done : nullptr, M, direct_rects, direct_index);
    // (the slots of the listed arenas' maps: read by the distance transform's install, the record builders and the costmap --
    //  a world of outdoor maps without a costmap writes its fields through the arena's own table entry and needs no list:
    //  one launch less in c5's per-step fallback, round 6)
    const bool need_mlist = st->map_slot && (!direct || c->regen_plan || st->costmap);
    if (need_mlist) regen_map_list_kernel<<<(M + 255) / 256, 256, 0, s>>>(list, st->map_slot, mlist, M);
    // Corridor maps with planned starts: the distance transform, the rect records and the field's install go to a helper
    // stream, beside the costmap and the robot stage's searches -- those read the occupancy grid only; the stage's accept
    // kernel (first-scan test on the new field) waits for the helper.  (reference defaults, 1024 arenas: dt 150 us of a
    // 1.1 ms step beside 150-400 us of searches.)  NAVSIM_REGEN_FORK=0 keeps one stream.
    static const bool fork_on = !(getenv("NAVSIM_REGEN_FORK") && atoi(getenv("NAVSIM_REGEN_FORK")) == 0);
    RegenFork* fk = (fork_on && !direct && c->regen_plan) ? regen_fork() : nullptr;
    if (fk && fk->side == s) fk = nullptr;                   // navsim_regen_helper(this call's own stream): no fork for this call
    hipStream_t sf = s;                                      // the stream of the field's kernels
    if (fk) {
        if (hipEventRecord(fk->forked, s) != hipSuccess || hipStreamWaitEvent(fk->side, fk->forked, 0) != hipSuccess) fk = nullptr;
        else sf = fk->side;
    }
    if (!direct) launch_dt(occ, M, H, W, ws.cols, c->field_format, fscratch, ovf_scratch, nullptr, count, kind, sf);
    if (st->rect_table && !direct) {                        // keep the rect records of the regenerated arenas current
        launch_build_rects(occ, M, H, W, fscratch, fbytes, c->field_format, ovf_scratch, (uint4*)st->rect_table, ws.rect,
                           count, mlist, sf);
        if (st->rect_index)
            rect_index_kernel<<<M, 256, 0, sf>>>((const uint4*)st->rect_table, H, W, (char*)st->rect_index, nullptr, count, mlist);
    }
    if (!direct) {
        regen_field_kernel<<<regen_grid(M), 256, 0, sf>>>((char*)st->field, count, mlist, fscratch, fbytes);
        if (ovf_scratch)
            regen_field_kernel<<<regen_grid(M), 256, 0, sf>>>((char*)st->field_overflow, count, mlist,
                                                                     (const char*)ovf_scratch, cells * sizeof(float));
    }
    bool join_pending = fk != nullptr;
    if (fk && hipEventRecord(fk->joined, fk->side) != hipSuccess) return NAVSIM_E_LAUNCH;
    auto join = [&]() {                                      // the caller's stream waits for the field (once)
        if (join_pending) { (void)hipStreamWaitEvent(s, fk->joined, 0); join_pending = false; }
    };
    if (c->regen_plan) {
        const int Hc = H / 5, Wc = W / 5, R = kRegenRounds;
        RegenPlanWs pw = ws.plan;                            // the scratch arrays; the costmap is the resident one where there is one
        pw.Q = c->n_spawn > c->max_peds ? c->n_spawn : c->max_peds;
        pw.kind = kind;
        pw.cost_by_arena = st->costmap != nullptr;
        if (st->costmap) pw.cost = st->costmap;
        const size_t lds = plan_lds(Hc, Wc);
        costmap_kernel<<<dim3((Hc * Wc + 255) / 256, M), 256, 0, s>>>(occ, H, W, pw.cost, count,
                                                                      st->costmap ? mlist : nullptr);
        // the rounds of the reference's rejection loops (kernels_reset.hpp): all candidates drawn at once, round 0 planned, then
        // rounds 1-3 of the slots it left open in one launch, the first round that passes taken -- four launches per stage
        auto plan_pass = [&](int ped_stage, int pass) {
            const int Qs = ped_stage ? c->max_peds : c->n_spawn;
            const int grid = M * R * Qs;
            // Threads per search.  1024 (a costmap word per thread) is the shortest search -- and two searches per CU; 512 (two words
            // per thread) is longer and four per CU.  A call that serves a handful of arenas (the per-step reset: under one search per
            // CU) waits for its longest search; a staging pass of dozens of arenas is thousands of searches -- generations of
            // workgroups -- and gets through them faster twice as many at a time (round 6).
            const bool many = (long long)grid > (long long)NAVSIM_PLAN_MANY_SEARCHES && plan_words(Hc, Wc) <= 2 * 512;
            if (plan_block(Hc, Wc) == 1024 && many) regen_plan_kernel<512><<<grid, 512, lds, s>>>(*c, *st, count, list, pw, ped_stage, pass, Qs);
            else if (plan_block(Hc, Wc) == 1024)    regen_plan_kernel<1024><<<grid, 1024, lds, s>>>(*c, *st, count, list, pw, ped_stage, pass, Qs);
            else                                    regen_plan_kernel<256><<<grid, 256, lds, s>>>(*c, *st, count, list, pw, ped_stage, pass, Qs);
        };
        regen_robot_sample_kernel<<<M, 256, 0, s>>>(*c, *st, count, list, pw);
        plan_pass(0, 0);
        plan_pass(0, 1);
        join();
        if (c->field_format == NAVSIM_FIELD_F32) regen_robot_accept_kernel<FieldF32><<<M, 256, 0, s>>>(*c, *st, count, list, pw);
        else                                     regen_robot_accept_kernel<FieldU16T><<<M, 256, 0, s>>>(*c, *st, count, list, pw);
        if (c->ped_model != NAVSIM_PED_NONE && c->max_peds > 0) {
            regen_ped_sample_kernel<<<M, 256, 0, s>>>(*c, *st, count, list, pw);
            plan_pass(1, 0);
            plan_pass(1, 1);
            regen_ped_accept_kernel<<<M, 256, 0, s>>>(*c, *st, count, list, pw);
        }
    } else if (st->costmap) {
        costmap_kernel<<<dim3(((H / 5) * (W / 5) + 255) / 256, M), 256, 0, s>>>(occ, H, W, st->costmap, count, mlist);
    }
    join();
    if (!c->regen_plan) {
        if (c->field_format == NAVSIM_FIELD_F32)
            regen_commit_kernel<FieldF32><<<M, kCommitBlock, 0, s>>>(*c, *st, count, list, fscratch, fbytes, kind);
        else
            regen_commit_kernel<FieldU16T><<<M, kCommitBlock, 0, s>>>(*c, *st, count, list, fscratch, fbytes, kind);
    }
    if (launch_status() != NAVSIM_OK) return NAVSIM_E_LAUNCH;
    // first observation of the new episodes: ONE workgroup per list slot (list[b] = its arena, -1 = empty slot); the
    // other arenas keep the row the step just wrote -- nothing is launched for them
    navsim_step_io io2 = *io;
    io2.obs_prev = io->obs;
    io2.reset_mask = nullptr;                                // (a reset-only launch: its mask is the kernel's own argument)
    io2.final_obs = nullptr; io2.final_goals = nullptr; io2.truncated = nullptr;
    navsim_state st2 = *st;
    st2.arena_cost = nullptr;
    StepLaunch l;
    l.reset_only = true;
    l.stream = s;
    if (c->defer_reset_scan) {
        // the step left every restart's first observation to this call: one launch over all arenas, masked by the done
        // flags -- the regenerated arenas and those beyond the cap that restarted in place (a workgroup whose flag is
        // clear returns at once)
        st2.launch_order = nullptr;
        l.mask = io->done;
    } else {
        st2.launch_order = list;
        l.grid = M;
    }
    return dispatch_step(c, &st2, &io2, l);
}

int navsim_step_install(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const navsim_state* stage,
                        const float* stage_obs, uint8_t* mark, const long long* ready, uint8_t* late, void* stream) {
    return navsim_step_install_replan(c, st, io, stage, stage_obs, mark, ready, late, -1, stream);
}

int navsim_step_install_replan(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const navsim_state* stage,
                               const float* stage_obs, uint8_t* mark, const long long* ready, uint8_t* late, int32_t max_queries,
                               void* stream) {
    return step_install_impl(c, st, io, stage, stage_obs, mark, ready, late, nullptr, nullptr, max_queries, stream);
}

int navsim_step_install_next(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const navsim_state* stage,
                             const float* stage_obs, uint8_t* mark, const long long* ready, uint8_t* late_next, const uint8_t* late_prev,
                             int32_t max_queries, void* stream) {
    if (!c || c->auto_reset != NAVSIM_AUTORESET_NEXT_STEP || !late_next || !late_prev || late_next == late_prev || !io || !io->reset_mask)
        return NAVSIM_E_ARG;
    return step_install_impl(c, st, io, stage, stage_obs, mark, ready, nullptr, late_next, late_prev, max_queries, stream);
}

int navsim_regen_swap(const navsim_config* c, const navsim_state* live, const navsim_state* stage, const navsim_step_io* io,
                      const float* stage_obs, const uint8_t* want, uint8_t* mark, const long long* ready, void* stream) {
    (void)hipGetLastError();
    if (!c || !live || !stage || !io || !io->done || !io->obs || !stage_obs || !want || !mark) return NAVSIM_E_ARG;
    if (((uintptr_t)mark & 3) != 0) return NAVSIM_E_ARG;                 // mark[] is accessed through 32-bit atomics
    if (ready && (c->regen_min_steps < 1 || !live->done_steps)) return NAVSIM_E_ARG;    // the pipelined form rests on the rule
    const int rcp = check_stage_pair(c, live, stage);
    if (rcp != NAVSIM_OK) return rcp;
    if (c->auto_reset != NAVSIM_AUTORESET_SAME_STEP) return NAVSIM_E_UNSUPPORTED;     // (NEXT_STEP installs inside navsim_step_install)
    if (c->n_envs == 0) return NAVSIM_OK;
    const int rcs = check_map_slots(live, stage);
    if (rcs != NAVSIM_OK) return rcs;
    SwapBig big[5] = {};
    if (!live->map_slot) stage_big_buffers(c, live, stage, big);
    // (pipelined form that copies maps: one slice per arena, so that the arena's request for its next world leaves behind ALL of
    //  its copies -- kernels_reset.hpp regen_swap_kernel)
    const int slices = (ready && !live->map_slot) ? 1 : kRegenSlices;
    regen_swap_kernel<<<dim3(c->regen_cap, slices), 256, 0, (hipStream_t)stream>>>(*c, *live, *stage, *io, stage_obs, want, mark, ready,
                                                                                        c->regen_cap, big[0], big[1], big[2], big[3], big[4]);
    return launch_status();
}

int navsim_regen_stage(const navsim_config* c, const navsim_state* stage, const navsim_step_io* io, uint8_t* want, uint8_t* mark,
                       long long* ready, void* workspace, size_t workspace_bytes, void* stream) {
    return navsim_regen_stage_part(c, stage, io, want, mark, ready, workspace, workspace_bytes, 0, 1, stream);
}

int navsim_regen_stage_part(const navsim_config* c, const navsim_state* stage, const navsim_step_io* io, uint8_t* want, uint8_t* mark,
                            long long* ready, void* workspace, size_t workspace_bytes, int32_t part, int32_t n_parts, void* stream) {
    (void)hipGetLastError();
    if (!c || !stage || !io || !want || !mark || !workspace || io->done != want || !stage->episode) return NAVSIM_E_ARG;
    if (((uintptr_t)mark & 3) != 0 || n_parts < 1 || part < 0 || part >= n_parts) return NAVSIM_E_ARG;
    if (c->n_envs == 0) return NAVSIM_OK;
    regen_merge_want_kernel<<<((c->n_envs + 3) / 4 + 255) / 256, 256, 0, (hipStream_t)stream>>>(want, mark, c->n_envs, ready, stage->episode,
                                                                                                part, n_parts);
    // the staged state takes EVERY arena in want[], whatever its last episode's length (cfg.regen_min_steps is the live state's rule)
    navsim_config cs = *c;
    cs.regen_min_steps = 0;
    const int rc = navsim_regen(&cs, stage, io, workspace, workspace_bytes, stream);
    if (rc != NAVSIM_OK) return rc;
    const RegenWs ws = regen_ws_of(&cs, stage, workspace);   // navsim_regen's selection: count, list
    regen_clear_want_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws.count, ws.list, want, ready, c->n_envs);
    return launch_status();
}

size_t navsim_replan_workspace_bytes(const navsim_config* c, int32_t max_queries) {
    if (!c || max_queries < 0) return 0;
    return replan_ws(c, max_queries, nullptr, true).bytes;
}

int navsim_replan(const navsim_config* c, const navsim_state* st, int32_t max_queries, void* workspace,
                  size_t workspace_bytes, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !workspace || max_queries < 0 || !st->costmap || !st->ped_pose || !st->ped_waypoints ||
        !st->ped_n_waypoints || !st->ped_wp_head || !st->n_peds || !st->steps || !st->episode)
        return NAVSIM_E_ARG;
    // (without the flags' array the layout is only shorter: it comes last)
    const ReplanWs ws = replan_ws(c, max_queries, workspace, st->ped_due == nullptr);
    if (ws.bytes > workspace_bytes) return NAVSIM_E_ARG;
    if (c->ped_model == NAVSIM_PED_NONE || c->n_envs == 0) return NAVSIM_OK;
    if (c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS) return NAVSIM_E_ARG;
    const int Hc = c->map_h / 5, Wc = c->map_w / 5;
    if (Hc < 1 || Wc < 1 || !plan_fits(Hc, Wc) || plan_lds(Hc, Wc) > 64 * 1024) return NAVSIM_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // who is due: the flags the last step left in st->ped_due (ABI 5), else a pass over the state
    const uint64_t* flags = (const uint64_t*)st->ped_due;
    if (!flags) { replan_flag_kernel<<<c->n_envs, 64, 0, s>>>(*c, *st, ws.due); flags = ws.due; }
    // one workgroup per query slot; each finds its own pedestrian in the flags (replan_pick), slot 0 counts.  At least one
    // workgroup even at max_queries = 0: the call still counts who waits.
    if (plan_block(Hc, Wc) == 1024) replan_kernel<1024><<<max_queries > 0 ? max_queries : 1, 1024, plan_lds(Hc, Wc), s>>>(*c, *st, flags, max_queries);
    else                            replan_kernel<256><<<max_queries > 0 ? max_queries : 1, 256, plan_lds(Hc, Wc), s>>>(*c, *st, flags, max_queries);
    return launch_status();
}

size_t navsim_ped_policy_workspace_bytes(const navsim_config* c) {
    return c ? policy_ws(nullptr, policy_chunk(c)).bytes : 0;
}

// ped_scans != NULL: the network reads those scans (navsim_ped_policy); NULL: every chunk's scans are taken by the fused
// scan + features kernel from the current state and, when scans_out != NULL, also written there (navsim_ped_scan_policy)
static int ped_policy_run(const navsim_config* c, const navsim_state* st, const navsim_policy_weights* w,
                          const float* ped_scans, float* scans_out, float* prev_actions, double* ped_cmd, void* workspace,
                          size_t workspace_bytes, void* stream, long p_begin = 0, long p_count = -1) {
    (void)hipGetLastError();
    if (!c || !st || !w || !prev_actions || !ped_cmd || !workspace || !st->ped_pose ||
        !st->ped_waypoints || !st->ped_n_waypoints || !st->ped_wp_head || !st->ped_v_pref || !st->n_peds)
        return NAVSIM_E_ARG;
    if (!w->cv1_w || !w->cv1_b || !w->cv2_w || !w->cv2_b || !w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b ||
        !w->a1_w || !w->a1_b || !w->a2_w || !w->a2_b)
        return NAVSIM_E_ARG;
    if (c->ped_n_beams != 512 || c->max_peds < 1) return NAVSIM_E_UNSUPPORTED;
    if (c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS) return NAVSIM_E_ARG;
    const size_t chunk = policy_chunk(c);                             // (the workspace's capacity)
    const PolicyWs ws = policy_ws(workspace, chunk);
    if (ws.bytes > workspace_bytes) return NAVSIM_E_ARG;
    const bool fused = ped_scans == nullptr;
    if (fused) {                                  // what navsim_ped_scans checks
        if (c->ped_model == NAVSIM_PED_NONE || !st->robot_pose || !st->field) return NAVSIM_E_ARG;
        if (c->max_peds > NAVSIM_MAX_PEDS) return NAVSIM_E_UNSUPPORTED;
        if (c->field_format != NAVSIM_FIELD_U16T && c->field_format != NAVSIM_FIELD_F32) return NAVSIM_E_UNSUPPORTED;
        if (c->ped_angle_last - c->ped_angle_min > nv::kTwoPi) return NAVSIM_E_UNSUPPORTED;
    }
    const size_t P_all = (size_t)c->n_envs * (size_t)c->max_peds;
    if (p_count < 0) p_count = (long)P_all - p_begin;
    if (p_begin < 0 || (size_t)(p_begin + p_count) > P_all) return NAVSIM_E_ARG;
    const size_t P = (size_t)(p_begin + p_count);                     // the chunks below walk [p_begin, P)
    if (p_count == 0) return NAVSIM_OK;
    hipStream_t s = (hipStream_t)stream;
    constexpr size_t fc1_lds = (size_t)2 * (128 + 128) * 33 * sizeof(float);       // 67,584 B
    if (allow_lds((const void*)policy_fc1_kernel, fc1_lds) != NAVSIM_OK) return NAVSIM_E_UNSUPPORTED;
    policy_transpose_kernel<<<(kPolH2 * kPolIn2 + 255) / 256, 256, 0, s>>>(w->fc2_w, ws.w2t, w->cv2_w, ws.cv2t, *c, fused ? ws.tab : nullptr);
    for (size_t p0 = (size_t)p_begin; p0 < P; p0 += chunk) {
        const int n = (int)(P - p0 < chunk ? P - p0 : chunk);
        int rc = NAVSIM_OK;
        if (!fused) {
            policy_features_kernel<<<n, 256, 0, s>>>(ped_scans, (int)p0, n, w->cv1_w, w->cv1_b, ws.cv2t, w->cv2_b, ws.feat);
        } else if (c->field_format == NAVSIM_FIELD_U16T) {
            rc = st->rect_table ? launch_ped_scan_features<FieldU16T, true>(c, st, (int)p0, n, ws, scans_out, w, s)
                                : launch_ped_scan_features<FieldU16T, false>(c, st, (int)p0, n, ws, scans_out, w, s);
        } else {
            rc = launch_ped_scan_features<FieldF32, false>(c, st, (int)p0, n, ws, scans_out, w, s);
        }
        if (rc != NAVSIM_OK) return rc;
        policy_fc1_kernel<<<dim3((n + 127) / 128, 2), 256, fc1_lds, s>>>(ws.feat, n, w->fc1_w, w->fc1_b, ws.h1);
        policy_head_kernel<<<(n + kHeadPeds - 1) / kHeadPeds, 128, 0, s>>>(*c, *st, (int)p0, n, ws.h1, ws.w2t, *w, prev_actions, ped_cmd);
    }
    return launch_status();
}

int navsim_ped_policy(const navsim_config* c, const navsim_state* st, const navsim_policy_weights* w,
                      const float* ped_scans, float* prev_actions, double* ped_cmd, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!ped_scans) return NAVSIM_E_ARG;
    return ped_policy_run(c, st, w, ped_scans, nullptr, prev_actions, ped_cmd, workspace, workspace_bytes, stream);
}

int navsim_ped_policy_part(const navsim_config* c, const navsim_state* st, const navsim_policy_weights* w,
                           const float* ped_scans, float* prev_actions, double* ped_cmd, void* workspace,
                           size_t workspace_bytes, int32_t e0, int32_t n_e, void* stream) {
    if (!ped_scans || !c || e0 < 0 || n_e < 0 || (long)e0 + n_e > c->n_envs) return NAVSIM_E_ARG;
    return ped_policy_run(c, st, w, ped_scans, nullptr, prev_actions, ped_cmd, workspace, workspace_bytes, stream,
                          (long)e0 * c->max_peds, (long)n_e * c->max_peds);
}

int navsim_ped_scan_policy(const navsim_config* c, const navsim_state* st, const navsim_policy_weights* w,
                           float* scans_out, float* prev_actions, double* ped_cmd, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return ped_policy_run(c, st, w, nullptr, scans_out, prev_actions, ped_cmd, workspace, workspace_bytes, stream);
}

int navsim_crowd_check(const navsim_crowd_params* p, int32_t n_envs, int32_t max_agents, int32_t grid,
                       const uint8_t* free_map, const double* robot, const double* agents, const int32_t* n_agents,
                       const double* global_time, double* reward, uint8_t* done, int32_t* info, double* min_dist,
                       void* stream) {
    (void)hipGetLastError();
    if (!p || !free_map || !robot || !global_time || !reward || !done || !info || n_envs < 0 || max_agents < 0 ||
        grid < 1 || (max_agents > 0 && !agents))
        return NAVSIM_E_ARG;
    if (n_envs == 0) return NAVSIM_OK;
    crowd_check_kernel<<<n_envs, 64, 0, (hipStream_t)stream>>>(*p, max_agents, grid, free_map, robot, agents, n_agents,
                                                               global_time, reward, done, info, min_dist);
    return launch_status();
}

int navsim_crowd_angular_map(const navsim_crowd_map_params* p, int32_t n_envs, int32_t max_obst, int32_t n_vert,
                             const double* robot, const double* verts, const int32_t* n_obst, double* out, void* stream) {
    (void)hipGetLastError();
    if (!p || !robot || !out || n_envs < 0 || max_obst < 0 || n_vert < 1 || n_vert > NAVSIM_CROWD_MAX_VERTS ||
        p->angular_dim < 1 || (max_obst > 0 && !verts))
        return NAVSIM_E_ARG;
    if (p->angular_dim > 4096) return NAVSIM_E_UNSUPPORTED;
    if (n_envs == 0) return NAVSIM_OK;
    crowd_angular_map_kernel<<<n_envs, 64, (size_t)p->angular_dim * sizeof(unsigned long long), (hipStream_t)stream>>>(
        *p, max_obst, n_vert, robot, verts, n_obst, out);
    return launch_status();
}

int navsim_crowd_local_map(const navsim_crowd_map_params* p, int32_t n_envs, int32_t grid, const uint8_t* free_map,
                           const double* robot, int32_t rotate, uint8_t* out, void* stream) {
    (void)hipGetLastError();
    if (!p || !free_map || !robot || !out || n_envs < 0 || grid < 1) return NAVSIM_E_ARG;
    const int S = (int)nearbyint(p->submap_size_m / p->map_resolution);
    if (S < 1 || (size_t)S * S > 64 * 1024) return NAVSIM_E_UNSUPPORTED;           // the window lives in LDS
    if (n_envs == 0) return NAVSIM_OK;
    crowd_local_map_kernel<<<n_envs, 256, (size_t)S * S, (hipStream_t)stream>>>(*p, grid, S, free_map, robot, rotate, out);
    return launch_status();
}

int navsim_crowd_orca(const navsim_orca_params* p, int32_t n_queries, int32_t max_agents, const double* agents,
                      const int32_t* n_agents, const double* pref_vel, int32_t max_obst, int32_t n_vert,
                      const double* verts, const int32_t* n_obst, const int32_t* obst_set, const double* theta,
                      double* out_vel, double* out_action, void* stream) {
    (void)hipGetLastError();
    if (!p || !agents || !pref_vel || !out_vel || n_queries < 0 || max_agents < 1 || max_agents > NAVSIM_ORCA_MAX_AGENTS ||
        max_obst < 0 || n_vert < 2 || (size_t)max_obst * n_vert > NAVSIM_ORCA_MAX_EDGES || (max_obst > 0 && !verts))
        return NAVSIM_E_ARG;
    if (n_queries == 0) return NAVSIM_OK;
    crowd_orca_kernel<<<(n_queries + 63) / 64, 64, 0, (hipStream_t)stream>>>(*p, n_queries, max_agents, agents, n_agents,
                                                                          pref_vel, max_obst, n_vert, verts, n_obst,
                                                                          obst_set, theta, out_vel, out_action);
    return launch_status();
}

// navsim_ped_orca and navsim_ped_orca_walls: the refusals, the layout's LDS, one launch
static int ped_orca_run(const navsim_config* c, const navsim_state* st, const navsim_ped_orca_params* p, int32_t max_rects,
                        double* ped_cmd, int32_t* dropped, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !ped_cmd) return NAVSIM_E_ARG;
    if (c->ped_model != NAVSIM_PED_EXTERNAL || c->n_envs < 0 || c->max_peds < 1) return NAVSIM_E_ARG;
    if (p->robot_visible != 0 && p->robot_visible != 1) return NAVSIM_E_ARG;
    if ((long)c->max_peds + p->robot_visible > NAVSIM_ORCA_MAX_AGENTS) return NAVSIM_E_ARG;
    if (!(p->ped_radius > 0.0) || !(p->robot_radius > 0.0) || !(p->orca.time_step > 0.0f) || !(p->orca.time_horizon > 0.0f) ||
        !(c->time_step > 0.0) || p->orca.max_neighbors < 0)
        return NAVSIM_E_ARG;
    if (c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS) return NAVSIM_E_ARG;
    if (!st->n_peds || !st->ped_pose || !st->ped_vel || !st->ped_v_pref || !st->ped_waypoints || !st->ped_n_waypoints ||
        !st->ped_wp_head || (p->robot_visible && (!st->robot_pose || !st->prev_action)))
        return NAVSIM_E_ARG;
    if (max_rects < 0 || max_rects > NAVSIM_PED_ORCA_MAX_RECTS) return NAVSIM_E_ARG;
    if (max_rects > 0 && (!st->rect_index || !(p->orca.time_horizon_obst > 0.0f) || !(c->resolution > 0.0) || c->map_h < 1 ||
                          c->map_w < 1 || (st->map_slot && c->shared_field)))
        return NAVSIM_E_ARG;
    const int N = c->max_peds, G = ped_orca_pack(N);
    const size_t lds = ped_orca_lds_bytes(N, ped_orca_list_len(N, p->orca.max_neighbors, p->robot_visible), max_rects);
    if (lds > kLdsPerCu) return NAVSIM_E_UNSUPPORTED;               // (before any device call, whatever n_envs is)
    if (c->n_envs == 0) return NAVSIM_OK;
    const void* kernel = max_rects > 0 ? (const void*)ped_orca_kernel<true> : (const void*)ped_orca_kernel<false>;
    const int rc = allow_lds(kernel, lds);
    if (rc != NAVSIM_OK) return rc;
    const int grid = (c->n_envs + G - 1) / G;
    if (max_rects > 0) ped_orca_kernel<true><<<grid, 64, lds, (hipStream_t)stream>>>(*c, *st, *p, max_rects, ped_cmd, dropped);
    else               ped_orca_kernel<false><<<grid, 64, lds, (hipStream_t)stream>>>(*c, *st, *p, 0, ped_cmd, dropped);
    return launch_status();
}

int navsim_ped_orca(const navsim_config* c, const navsim_state* st, const navsim_ped_orca_params* p, double* ped_cmd, void* stream) {
    return ped_orca_run(c, st, p, 0, ped_cmd, nullptr, stream);
}

int navsim_ped_orca_walls(const navsim_config* c, const navsim_state* st, const navsim_ped_orca_params* p, int32_t max_rects,
                          double* ped_cmd, int32_t* dropped, void* stream) {
    return ped_orca_run(c, st, p, max_rects, ped_cmd, dropped, stream);
}

int navsim_crowd_agent_step(double* pose, const double* action, double* vel, int32_t n, double time_step, void* stream) {
    (void)hipGetLastError();
    if (!pose || !action || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    crowd_agent_step_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(pose, action, vel, n, time_step);
    return launch_status();
}

int navsim_launch_order(const uint32_t* cost, int32_t* order, int32_t n, void* stream) {
    (void)hipGetLastError();
    if (!cost || !order || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    launch_order_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(cost, order, n);
    return launch_status();
}

int navsim_step(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    int rc = check_step_args(c, st, io, 0);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    StepLaunch l;
    l.stream = (hipStream_t)stream;
    return dispatch_step(c, st, io, l);
}

int navsim_step_sorted(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const uint32_t* sort_cost,
                       int32_t* sort_order, void* stream) {
    (void)hipGetLastError();
    int rc = check_step_args(c, st, io, 0);
    if (rc != NAVSIM_OK) return rc;
    // the launch writes st->arena_cost and reads st->launch_order: the sorter's buffers are others
    if (!sort_cost || !sort_order || (const void*)sort_cost == (const void*)st->arena_cost ||
        (const void*)sort_order == (const void*)st->launch_order)
        return NAVSIM_E_ARG;
    // the front workgroup exists in navsim_step_kernel alone (a state with slot tables goes to the install kernels), behind
    // no other launch (ped_update_kernel), and sorts in the step's own dynamic LDS
    if (st->map_slot || c->ped_split == 2 || plan_step(c, st).lds < kOrderLdsBytes) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    StepLaunch l;
    l.sort_cost = sort_cost;
    l.sort_order = sort_order;
    l.stream = (hipStream_t)stream;
    return dispatch_step(c, st, io, l);
}

int navsim_step_part(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, int32_t part, void* stream) {
    (void)hipGetLastError();
    if (part == NAVSIM_STEP_ALL) return navsim_step(c, st, io, stream);
    if (part != NAVSIM_STEP_NOT_DUE && part != NAVSIM_STEP_DUE) return NAVSIM_E_ARG;
    int rc = check_step_args(c, st, io, 0);
    if (rc != NAVSIM_OK) return rc;
    if (!st->ped_due_prev || !st->ped_due || st->ped_due == st->ped_due_prev) return NAVSIM_E_ARG;
    if (c->ped_model == NAVSIM_PED_NONE) return NAVSIM_E_ARG;                               // nobody ever waits: there are no parts
    if (ped_split_on(c)) return NAVSIM_E_UNSUPPORTED;                                       // ped_update_kernel advances every arena
    if (c->n_envs == 0) return NAVSIM_OK;
    StepLaunch l;
    l.part = part;
    l.stream = (hipStream_t)stream;
    navsim_config c2 = *c;
    if (part == NAVSIM_STEP_DUE) {
        // a compact launch, each workgroup of which takes the b-th, (b + grid)-th, ... arena with a waiting pedestrian
        // (kernels_step.hpp due_arena_pick)
        l.grid = compact_grid(c);
        // twice the other part's threads per arena: the compact launch ends the step, and its arenas share their SIMDs with the
        // other part's wavefronts (c3 world through the gym API, 256 / 512 / 1024 threads: 19.3 / 19.8 / 18.8 M env-steps/s --
        // a 1024-thread workgroup has to wait for 16 free wave slots on one CU; profiles/r05_replan/README.md)
        if (!c->step_block) { const int b = pick_step_block(c); c2.step_block = b >= 512 ? 1024 : (b >= 256 ? 512 : b); }
    }
    return dispatch_step(&c2, st, io, l);
}

int navsim_step_replan(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, int32_t max_queries, void* stream) {
    (void)hipGetLastError();
    int rc = check_step_args(c, st, io, 0);
    if (rc != NAVSIM_OK) return rc;
    if (max_queries < 0) return NAVSIM_E_ARG;
    rc = replan_in_step(c, st, true);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    StepLaunch l;
    l.part = kStepPartReplan;
    l.grid = compact_grid(c);      // front workgroups, one per arena with a waiting pedestrian; more than that and the arena's own
    l.max_queries = max_queries;   // workgroup plans (kernels_step.hpp)
    l.stream = (hipStream_t)stream;
    return dispatch_step(c, st, io, l);
}

int navsim_prepare(const navsim_config* c, const navsim_state* st, const navsim_step_io* io) {
    (void)hipGetLastError();
    int rc = check_step_args(c, st, io, 1);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    // every form of the launch this configuration can ask for, walked down to its kernel
    const bool fused_peds = c->ped_model != NAVSIM_PED_NONE && !ped_split_on(c);
    const StepInstall none = {};
    StepLaunch l;
    l.prepare_only = true;
    rc = dispatch_step(c, st, io, l);                                                                // the step
    l.reset_only = true;
    if (rc == NAVSIM_OK) rc = dispatch_step(c, st, io, l);                                           // first observations of a reset
    l.grid = c->regen_cap;
    if (rc == NAVSIM_OK && c->regen_cap > 0) rc = dispatch_step(c, st, io, l);                       // navsim_regen's lone launch
    l.reset_only = false; l.grid = 32; l.part = NAVSIM_STEP_DUE;
    if (rc == NAVSIM_OK && fused_peds) rc = dispatch_step(c, st, io, l);                             // navsim_step_part's pair
    l.part = kStepPartReplan;
    if (rc == NAVSIM_OK && replan_in_step(c, st, false) == NAVSIM_OK) rc = dispatch_step(c, st, io, l);   // navsim_step_replan
    l.grid = 0; l.part = NAVSIM_STEP_ALL; l.install = &none;
    if (rc == NAVSIM_OK && c->field_format == NAVSIM_FIELD_U16T && (c->ped_model == NAVSIM_PED_NONE || fused_peds))
        rc = dispatch_step(c, st, io, l);                                                            // navsim_step_install
    if (rc != NAVSIM_OK) return rc;
    if (c->regen_plan && c->regen_indoor_ratio > 0.0) (void)regen_fork();     // navsim_regen's helper stream: not created inside a capture
    const int Hc = c->map_h / 5, Wc = c->map_w / 5;
    if (Hc >= 1 && Wc >= 1 && plan_fits(Hc, Wc)) {                           // the planners' LDS-resident search
        (void)allow_lds((const void*)plan_kernel, plan_lds(Hc, Wc));
    }
    return NAVSIM_OK;
}

int navsim_reset_obs(const navsim_config* c, const navsim_state* st, const navsim_step_io* io,
                     const uint8_t* mask, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    int rc = check_step_args(c, st, io, 1);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    StepLaunch l;
    l.reset_only = true;
    l.mask = mask;
    l.stream = (hipStream_t)stream;
    return dispatch_step(c, st, io, l);
}

int navsim_restart(const navsim_config* c, const navsim_state* st, const uint8_t* mask, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !mask || c->n_envs < 0 || c->n_spawn < 1 || !st->spawn_pose || !st->spawn_goal || !st->robot_pose ||
        !st->robot_goal || !st->episode || !st->steps)
        return NAVSIM_E_ARG;
    if (c->n_envs == 0) return NAVSIM_OK;
    restart_kernel<<<(c->n_envs + 255) / 256, 256, 0, (hipStream_t)stream>>>(*c, *st, mask);
    return launch_status();
}

int navsim_reset_install(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const navsim_state* stage,
                         const float* stage_obs, uint8_t* mark, const long long* ready, const uint8_t* mask, uint8_t* late,
                         void* stream) {
    (void)hipGetLastError();
    int rc = check_step_args(c, st, io, 1);
    if (rc != NAVSIM_OK) return rc;
    if (!stage || !stage_obs || !mark || !ready || !mask || !late || ((uintptr_t)mark & 3) != 0 || !st->done_steps) return NAVSIM_E_ARG;
    rc = check_stage_pair(c, st, stage);                     // (auto-reset, no deferred first scan, the same optional buffers)
    if (rc != NAVSIM_OK) return rc;
    if (c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    rc = check_map_slots(st, stage);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    StepInstall in = {};
    in.stage = *stage; in.stage_obs = stage_obs; in.mark = mark; in.ready = ready; in.late = late;
    if (!st->map_slot) stage_big_buffers(c, st, stage, in.big);             // (with slot tables the maps stay where they are)
    reset_install_kernel<<<c->n_envs, 256, 0, (hipStream_t)stream>>>(*c, *st, *io, in, mask);
    return launch_status();
}

// navsim_episode_stats_update / _clear: the pointers both need
static bool episode_stats_complete(const navsim_episode_stats* s) {
    return s && s->ret && s->length && s->path_length && s->min_clearance && s->discomfort_steps && s->ep_return &&
           s->ep_length && s->ep_path_length && s->ep_min_clearance && s->ep_discomfort_steps && s->ep_outcome;
}

int navsim_episode_stats_update(const navsim_config* c, const navsim_state* st, const navsim_step_io* io,
                                const navsim_episode_stats* s, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !io || !episode_stats_complete(s)) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->n_beams < 1 || c->n_scan_stack < 1) return NAVSIM_E_ARG;
    if (!io->obs || !io->reward || !io->done || !io->is_success || !io->is_crash || !st->scan_threshold || !st->scan_discomfort)
        return NAVSIM_E_ARG;
    if (c->auto_reset == NAVSIM_AUTORESET_SAME_STEP && !io->final_obs) return NAVSIM_E_ARG;
    if (c->auto_reset == NAVSIM_AUTORESET_NEXT_STEP && !io->reset_mask) return NAVSIM_E_ARG;
    const size_t lds = (size_t)c->n_beams * 2 * sizeof(float);         // the two threshold tables
    if (lds > 64 * 1024) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    EpisodeArgs a = {};
    a.n_envs = c->n_envs; a.n_beams = c->n_beams; a.n_scan_stack = c->n_scan_stack; a.auto_reset = c->auto_reset;
    a.obs = io->obs; a.final_obs = io->final_obs; a.reward = io->reward; a.done = io->done; a.is_success = io->is_success;
    a.is_crash = io->is_crash; a.truncated = io->truncated; a.reset_mask = io->reset_mask;
    a.thr = st->scan_threshold; a.dthr = st->scan_discomfort; a.s = *s;
    episode_stats_kernel<<<(c->n_envs + kEpisodeWaves - 1) / kEpisodeWaves, 64 * kEpisodeWaves, lds, (hipStream_t)stream>>>(a);
    return launch_status();
}

int navsim_episode_stats_clear(const navsim_config* c, const navsim_episode_stats* s, const uint8_t* mask, void* stream) {
    (void)hipGetLastError();
    if (!c || !episode_stats_complete(s) || c->n_envs < 0) return NAVSIM_E_ARG;
    if (c->n_envs == 0) return NAVSIM_OK;
    episode_stats_clear_kernel<<<(c->n_envs + 255) / 256, 256, 0, (hipStream_t)stream>>>(c->n_envs, *s, mask);
    return launch_status();
}

int navsim_ped_observe(const navsim_config* c, const navsim_state* st, const navsim_ped_observe_params* p, const uint8_t* skip,
                       const navsim_ped_observation* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !out || !out->state || !out->index || !out->count) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->n_peds || !st->ped_pose || !st->ped_vel || !st->field) return NAVSIM_E_ARG;
    if (c->ped_model == NAVSIM_PED_NONE) return NAVSIM_E_ARG;
    if (p->max_obs < 1 || p->max_obs > NAVSIM_MAX_PEDS || (p->rays != 1 && p->rays != 3)) return NAVSIM_E_ARG;
    if (!(p->ped_radius >= 0.0) || !(p->sensor_range >= 0.0) || std::isinf(p->ped_radius) || std::isinf(p->sensor_range)) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->max_peds < 1 || c->max_peds > NAVSIM_MAX_PEDS || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (c->march_rule < NAVSIM_MARCH_F64 || c->march_rule > NAVSIM_MARCH_F32_FMA) return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    PedObserveArgs a = {};
    a.p = *p; a.out = *out; a.skip = skip;
    a.max_range = (float)((long long)c->map_h * c->map_w);
    hipStream_t s = (hipStream_t)stream;
    return with_field(c, st, [&](auto field) { return launch_ped_observe<typename decltype(field)::type>(c, st, a, s); });
}

size_t navsim_goal_field_bytes(const navsim_config* c) {
    if (!c || c->n_envs < 0 || c->map_h / 5 < 1 || c->map_w / 5 < 1) return 0;
    return (size_t)c->n_envs * (size_t)(c->map_h / 5) * (size_t)(c->map_w / 5) * sizeof(uint16_t);
}

int navsim_goal_path(const navsim_config* c, const navsim_state* st, const navsim_goal_path_params* p, const uint8_t* rebuild,
                     const uint8_t* skip, const navsim_goal_field* field, const navsim_goal_path_out* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !field || !out) return NAVSIM_E_ARG;
    if (!field->dist || !field->key || !out->distance || !out->subgoal || !out->status) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->robot_goal || !st->episode || !st->field) return NAVSIM_E_ARG;
    if (!std::isfinite(p->hard_clearance) || !std::isfinite(p->clearance) || !std::isfinite(p->lookahead)) return NAVSIM_E_ARG;
    if (!(c->resolution > 0.0) || !std::isfinite(c->resolution)) return NAVSIM_E_ARG;
    if (p->hard_clearance < 3.0 * c->resolution || p->clearance < p->hard_clearance) return NAVSIM_E_ARG;
    if (p->band_cost < 1 || p->band_cost > 16 || p->lookahead < 0.0) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->map_h / 5 < 1 || c->map_w / 5 < 1) return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    GoalPathArgs a = {};
    a.Hc = c->map_h / 5; a.Wc = c->map_w / 5;
    if ((long long)a.Hc * a.Wc > (1ll << 26) || goal_lds_bytes(a.Hc, a.Wc) > kGoalLdsMax) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    a.field = *field; a.out = *out; a.skip = skip;
    a.hard = (float)(p->hard_clearance / c->resolution);
    const double look = floor(p->lookahead / c->resolution);
    a.lookahead_cells = (int)(look < 1048576.0 ? look : 1048576.0);
    GoalFieldArgs f = {};
    f.field = st->field; f.overflow = st->field_overflow; f.map_slot = st->map_slot;
    f.robot_goal = st->robot_goal; f.episode = st->episode;
    f.out = *field; f.rebuild = rebuild; f.skip = skip; f.sweeps = g_goal_sweeps;
    f.ox = (float)c->origin_x; f.oy = (float)c->origin_y; f.res = (float)c->resolution;
    f.hard = a.hard;
    f.clear = (float)(p->clearance / c->resolution);
    f.band_cost = p->band_cost;
    f.n_envs = c->n_envs; f.map_h = c->map_h; f.map_w = c->map_w; f.shared_field = c->shared_field; f.Hc = a.Hc; f.Wc = a.Wc;
    hipStream_t s = (hipStream_t)stream;
    return with_field(c, st, [&](auto field) { return launch_goal_path<typename decltype(field)::type>(c, st, f, a, s); });
}

int navsim_debug_goal_path_sweeps(int32_t* sweeps) {
    g_goal_sweeps = sweeps;
    return NAVSIM_OK;
}

int navsim_dwa(const navsim_config* c, const navsim_state* st, const navsim_dwa_params* p, const float* subgoal, const uint8_t* skip,
               const navsim_dwa_out* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !out) return NAVSIM_E_ARG;
    if (!out->twist || !out->action || !out->clearance || !out->best || !out->status) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->robot_goal || !st->prev_action || !st->field) return NAVSIM_E_ARG;
    const bool use_peds = p->use_peds != 0 && c->ped_model != NAVSIM_PED_NONE;
    if (use_peds && (!st->n_peds || !st->ped_pose || !st->ped_vel || c->max_peds < 1 || c->max_peds > NAVSIM_MAX_PEDS)) return NAVSIM_E_ARG;
    const double nonneg[] = {p->acc_lin, p->acc_rot, p->body_radius, p->ped_radius, p->margin, p->clearance_cap};
    for (double x : nonneg)
        if (!std::isfinite(x) || x < 0.0) return NAVSIM_E_ARG;
    const double finite[] = {p->w_progress, p->w_heading, p->w_clearance, p->w_speed, p->body_offset[0], p->body_offset[1],
                             p->body_offset[2], p->body_offset[3], c->linvel_lo, c->linvel_hi, c->rotvel_lo, c->rotvel_hi,
                             c->axle_offset, c->origin_x, c->origin_y};
    for (double x : finite)
        if (!std::isfinite(x)) return NAVSIM_E_ARG;
    if (p->n_discs < 1 || p->n_discs > NAVSIM_DWA_MAX_DISCS || p->n_v < 1 || p->n_v > 16 || p->n_w < 1 || p->n_w > 32) return NAVSIM_E_ARG;
    if (p->horizon < 1 || p->horizon > 32) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (!(c->resolution > 0.0) || !std::isfinite(c->resolution) || !(c->time_step > 0.0) || !std::isfinite(c->time_step)) return NAVSIM_E_ARG;
    if (c->action_kind != NAVSIM_ACTION_TWIST && c->action_kind != NAVSIM_ACTION_WHEELS) return NAVSIM_E_ARG;
    if (c->action_kind == NAVSIM_ACTION_WHEELS && (!(c->wheel_radius > 0.0) || !std::isfinite(c->wheel_radius) || !std::isfinite(c->wheel_track)))
        return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    DwaArgs a = {};
    a.p = *p; a.out = *out; a.subgoal = subgoal; a.skip = skip; a.use_peds = use_peds ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    return with_field(c, st, [&](auto field) { return launch_dwa<typename decltype(field)::type>(c, st, a, s); });
}

int navsim_local_map(const navsim_config* c, const navsim_state* st, const navsim_local_map_params* p, const uint8_t* visible,
                     const uint8_t* skip, float* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !out) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->field) return NAVSIM_E_ARG;
    if (p->channels != 1 && p->channels != 2 && p->channels != 4) return NAVSIM_E_ARG;
    if (p->size < 1 || p->size > NAVSIM_LOCAL_MAP_MAX) return NAVSIM_E_ARG;
    if (!std::isfinite(p->cell) || !(p->cell > 0.0) || !std::isfinite(p->cap) || !(p->cap > 0.0)) return NAVSIM_E_ARG;
    if (!std::isfinite(p->ahead) || !std::isfinite(p->ped_radius) || p->ped_radius < 0.0) return NAVSIM_E_ARG;
    if (p->channels > 1 && (c->ped_model == NAVSIM_PED_NONE || !st->n_peds || !st->ped_pose || !st->ped_vel || c->max_peds < 1 ||
                            c->max_peds > NAVSIM_MAX_PEDS))
        return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (!(c->resolution > 0.0) || !std::isfinite(c->resolution) || !std::isfinite(c->origin_x) || !std::isfinite(c->origin_y))
        return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    LocalMapArgs a = {};
    a.p = *p; a.visible = p->channels > 1 ? visible : nullptr; a.skip = skip; a.out = out;
    hipStream_t s = (hipStream_t)stream;
    return with_field(c, st, [&](auto field) { return launch_local_map<typename decltype(field)::type>(c, st, a, s); });
}

int navsim_scan_labels(const navsim_config* c, const navsim_state* st, const uint8_t* skip, const navsim_scan_labels_out* out,
                       void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !out || !out->range || !out->label || !out->index) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->field) return NAVSIM_E_ARG;
    const bool peds = c->ped_model != NAVSIM_PED_NONE;
    if (peds && (!st->n_peds || !st->ped_pose || !st->ped_dist || !st->ped_has_legs)) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->n_beams < 1 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (c->max_peds < (peds ? 1 : 0) || c->max_peds > NAVSIM_MAX_PEDS) return NAVSIM_E_ARG;
    if (c->march_rule < NAVSIM_MARCH_F64 || c->march_rule > NAVSIM_MARCH_F32_FMA) return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (st->rect_table && (c->field_format != NAVSIM_FIELD_U16T || c->map_h > 1024 || c->map_w > 1024)) return NAVSIM_E_UNSUPPORTED;
    if (peds && c->angle_last - c->angle_min > nv::kTwoPi) return NAVSIM_E_UNSUPPORTED;     // the culled merge: dispatch_step
    if (scan_labels_lds_bytes(c) > kLdsPerCu) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    ScanLabelsArgs a = {};
    a.out = *out; a.skip = skip;
    return launch_marched<ScanLabelsFamily>(c, st, a, c->n_envs, kScanLabelsBlock, scan_labels_lds_bytes(c), (hipStream_t)stream);
}

// what navsim_lookahead, navsim_lookahead_obs, navsim_rollout, navsim_rollout_obs and navsim_mppi refuse alike of a state and its
// configuration, before anything touches the device.  wp_cap: the rollouts also refuse max_waypoints > NAVSIM_MAX_WAYPOINTS;
// lds: the entry's dynamic LDS
static int replay_check(const navsim_config* c, const navsim_state* st, const double* ped_cmd, bool wp_cap, size_t lds) {
    if (!st->robot_pose || !st->robot_goal || !st->prev_action || !st->prev_pose || !st->steps || !st->field ||
        !st->scan_threshold || !st->scan_discomfort)
        return NAVSIM_E_ARG;
    if (c->ped_model != NAVSIM_PED_NONE && c->ped_model != NAVSIM_PED_EXTERNAL && c->ped_model != NAVSIM_PED_SFM) return NAVSIM_E_ARG;
    const bool peds = c->ped_model != NAVSIM_PED_NONE;
    if (peds && (!st->n_peds || !st->ped_pose || !st->ped_vel || !st->ped_prev_yaw || !st->ped_dist || !st->ped_has_legs)) return NAVSIM_E_ARG;
    if (c->ped_model == NAVSIM_PED_SFM && (!st->ped_v_pref || !st->ped_waypoints || !st->ped_n_waypoints || !st->ped_wp_head ||
                                           c->max_waypoints < 1 || (wp_cap && c->max_waypoints > NAVSIM_MAX_WAYPOINTS)))
        return NAVSIM_E_ARG;
    if (c->ped_model == NAVSIM_PED_EXTERNAL && !ped_cmd && !st->ped_cmd) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->n_beams < 1 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (c->max_peds < (peds ? 1 : 0) || c->max_peds > NAVSIM_MAX_PEDS) return NAVSIM_E_ARG;
    if (c->march_rule < NAVSIM_MARCH_F64 || c->march_rule > NAVSIM_MARCH_F32_FMA) return NAVSIM_E_ARG;
    if (!(c->resolution > 0.0) || !std::isfinite(c->resolution) || !(c->time_step > 0.0) || !std::isfinite(c->time_step)) return NAVSIM_E_ARG;
    if (c->action_kind != NAVSIM_ACTION_TWIST && c->action_kind != NAVSIM_ACTION_WHEELS) return NAVSIM_E_ARG;
    if (c->action_kind == NAVSIM_ACTION_WHEELS && (!(c->wheel_radius > 0.0) || !std::isfinite(c->wheel_radius) || !std::isfinite(c->wheel_track)))
        return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (st->rect_table && (c->field_format != NAVSIM_FIELD_U16T || c->map_h > 1024 || c->map_w > 1024)) return NAVSIM_E_UNSUPPORTED;
    if (peds && c->angle_last - c->angle_min > nv::kTwoPi) return NAVSIM_E_UNSUPPORTED;     // the culled merge: dispatch_step
    if (lds > kLdsPerCu) return NAVSIM_E_UNSUPPORTED;
    return NAVSIM_OK;
}

// navsim_lookahead and navsim_lookahead_obs (K: the number of candidates)
static int lookahead_check(const navsim_config* c, const navsim_state* st, int K, const double* ped_cmd) {
    if (K < 1 || K > NAVSIM_LOOKAHEAD_MAX) return NAVSIM_E_ARG;
    return replay_check(c, st, ped_cmd, false, lookahead_lds_bytes(c, K));
}

int navsim_lookahead(const navsim_config* c, const navsim_state* st, const navsim_lookahead_params* p, const double* actions,
                     const double* ped_cmd, const uint8_t* skip, const navsim_lookahead_out* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !actions || !out) return NAVSIM_E_ARG;
    if (!out->reward || !out->done || !out->is_success || !out->is_crash || !out->discomfort || !out->distance || !out->margin ||
        !out->pose || !out->status)
        return NAVSIM_E_ARG;
    if (!std::isfinite(p->range) || !(p->range > 0.0) || !(p->range <= c->range_max)) return NAVSIM_E_ARG;
    const int rc = lookahead_check(c, st, p->n_actions, ped_cmd);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    LookaheadArgs a = {};
    a.out = *out; a.actions = actions; a.ped_cmd = c->ped_model == NAVSIM_PED_EXTERNAL ? ped_cmd : nullptr; a.skip = skip;
    a.K = p->n_actions; a.range = p->range;
    return launch_marched<LookaheadFamily>(c, st, a, c->n_envs, kLookaheadBlock, lookahead_lds_bytes(c, a.K), (hipStream_t)stream);
}

int navsim_lookahead_obs(const navsim_config* c, const navsim_state* st, const navsim_lookahead_obs_params* p, const double* actions,
                         const double* ped_cmd, const float* obs_prev, const uint8_t* skip, const navsim_lookahead_obs_out* out,
                         void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !actions || !out) return NAVSIM_E_ARG;
    if (!out->reward || !out->done || !out->is_success || !out->is_crash || !out->discomfort || !out->distance || !out->margin ||
        !out->pose || !out->status || !out->scan || !out->tail || !out->goals || !out->truncated)
        return NAVSIM_E_ARG;
    if (p->noise != NAVSIM_LOOKOBS_NOISE_OFF && p->noise != NAVSIM_LOOKOBS_NOISE_STEP) return NAVSIM_E_ARG;
    if (c->n_scan_stack < 1) return NAVSIM_E_ARG;
    if (out->obs && c->n_scan_stack > 1 && (!obs_prev || !st->n_hist)) return NAVSIM_E_ARG;
    const bool noise = p->noise == NAVSIM_LOOKOBS_NOISE_STEP && c->add_scan_noise;
    if (noise && (!st->scan_noise_std || !st->episode)) return NAVSIM_E_ARG;
    const int rc = lookahead_check(c, st, p->n_actions, ped_cmd);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    LookObsArgs a = {};
    a.out = *out; a.actions = actions; a.ped_cmd = c->ped_model == NAVSIM_PED_EXTERNAL ? ped_cmd : nullptr; a.obs_prev = obs_prev;
    a.skip = skip; a.K = p->n_actions; a.noise = noise ? 1 : 0;
    return launch_marched<LookObsFamily>(c, st, a, c->n_envs, kLookaheadBlock, lookahead_lds_bytes(c, a.K), (hipStream_t)stream);
}

// what navsim_rollout refuses, before anything touches the device (navsim_mppi refuses the same with the same codes)
static int rollout_check(const navsim_config* c, const navsim_state* st, const navsim_rollout_params* p, const double* actions,
                         const double* ped_cmd, const navsim_rollout_out* out) {
    if (!c || !st || !p || !actions || !out) return NAVSIM_E_ARG;
    if (!out->reward || !out->pose || !out->ret || !out->length || !out->outcome || !out->discomfort_steps || !out->min_margin ||
        !out->distance || !out->exact_steps || !out->status)
        return NAVSIM_E_ARG;
    if (p->n_seq < 1 || p->n_seq > NAVSIM_ROLLOUT_MAX_K || p->horizon < 1 || p->horizon > NAVSIM_ROLLOUT_MAX_H) return NAVSIM_E_ARG;
    if (!std::isfinite(p->range) || !(p->range > 0.0) || !(p->range <= c->range_max)) return NAVSIM_E_ARG;
    if (!(p->gamma >= 0.0) || !(p->gamma <= 1.0)) return NAVSIM_E_ARG;
    const int rc = replay_check(c, st, ped_cmd, true, rollout_lds_bytes(c));
    if (rc != NAVSIM_OK) return rc;
    if ((long long)c->n_envs * p->n_seq > 0x7FFFFFFFLL) return NAVSIM_E_UNSUPPORTED;         // one workgroup per (arena, sequence)
    return NAVSIM_OK;
}

// navsim_rollout's launch behind rollout_check
static int rollout_launch(const navsim_config* c, const navsim_state* st, const navsim_rollout_params* p, const double* actions,
                          const double* ped_cmd, const uint8_t* skip, const navsim_rollout_out* out, hipStream_t s) {
    RolloutArgs a = {};
    a.out = *out; a.actions = actions; a.ped_cmd = c->ped_model == NAVSIM_PED_EXTERNAL ? ped_cmd : nullptr; a.skip = skip;
    a.K = p->n_seq; a.H = p->horizon; a.range = p->range; a.gamma = p->gamma;
    return launch_marched<RolloutFamily>(c, st, a, (size_t)c->n_envs * a.K, kRolloutBlock, rollout_lds_bytes(c), s);
}

int navsim_rollout(const navsim_config* c, const navsim_state* st, const navsim_rollout_params* p, const double* actions,
                   const double* ped_cmd, const uint8_t* skip, const navsim_rollout_out* out, void* stream) {
    (void)hipGetLastError();
    const int rc = rollout_check(c, st, p, actions, ped_cmd, out);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    return rollout_launch(c, st, p, actions, ped_cmd, skip, out, (hipStream_t)stream);
}

int navsim_rollout_obs(const navsim_config* c, const navsim_state* st, const navsim_rollout_obs_params* p, const double* actions,
                       const double* ped_cmd, const float* obs_prev, const uint8_t* skip, const navsim_rollout_obs_out* out,
                       void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !actions || !out) return NAVSIM_E_ARG;
    if (p->noise != NAVSIM_LOOKOBS_NOISE_OFF && p->noise != NAVSIM_LOOKOBS_NOISE_STEP) return NAVSIM_E_ARG;
    if (!out->obs_last || !out->goals_last || (out->obs_all == nullptr) != (out->goals_all == nullptr)) return NAVSIM_E_ARG;
    if (c->n_scan_stack < 1) return NAVSIM_E_ARG;
    if (c->n_scan_stack > 1 && (!obs_prev || !st->n_hist)) return NAVSIM_E_ARG;
    const bool noise = p->noise == NAVSIM_LOOKOBS_NOISE_STEP && c->add_scan_noise;
    if (noise && (!st->scan_noise_std || !st->episode)) return NAVSIM_E_ARG;
    // everything navsim_rollout refuses, at R = range_max (a range_max that is no valid R is refused as its R would be); the
    // dynamic LDS is the rollout's
    const navsim_rollout_params rp = {p->n_seq, p->horizon, c->range_max, p->gamma};
    const navsim_rollout_out ro = {out->reward, out->pose, out->ret, out->length, out->outcome, out->discomfort_steps,
                                   out->min_margin, out->distance, out->exact_steps, out->status};
    const int rc = rollout_check(c, st, &rp, actions, ped_cmd, &ro);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    RolloutObsArgs a = {};
    a.out = *out; a.actions = actions; a.ped_cmd = c->ped_model == NAVSIM_PED_EXTERNAL ? ped_cmd : nullptr; a.obs_prev = obs_prev;
    a.skip = skip; a.K = p->n_seq; a.H = p->horizon; a.noise = noise ? 1 : 0; a.gamma = p->gamma;
    return launch_marched<RolloutObsFamily>(c, st, a, (size_t)c->n_envs * a.K, kRolloutBlock, rollout_lds_bytes(c), (hipStream_t)stream);
}

int navsim_ped_forecast(const navsim_config* c, const navsim_state* st, const navsim_ped_forecast_params* p, const double* actions,
                        const double* ped_cmd, const uint8_t* skip, const navsim_ped_forecast_out* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !out) return NAVSIM_E_ARG;
    if (!out->pose || !out->vel || !out->rel || !out->robot_pose || !out->min_dist || !out->min_step || !out->exact_steps || !out->status)
        return NAVSIM_E_ARG;
    if (p->horizon < 1 || p->horizon > NAVSIM_FORECAST_MAX_H) return NAVSIM_E_ARG;
    if (p->robot != NAVSIM_FORECAST_HOLD && p->robot != NAVSIM_FORECAST_STOP && p->robot != NAVSIM_FORECAST_ACTIONS) return NAVSIM_E_ARG;
    if (p->model != NAVSIM_FORECAST_TRUE && p->model != NAVSIM_FORECAST_CONST_VEL) return NAVSIM_E_ARG;
    if (p->robot == NAVSIM_FORECAST_ACTIONS && !actions) return NAVSIM_E_ARG;
    if (c->ped_model != NAVSIM_PED_EXTERNAL && c->ped_model != NAVSIM_PED_SFM) return NAVSIM_E_ARG;      // NAVSIM_PED_NONE: nobody to forecast
    if (c->max_peds < 1 || c->max_peds > NAVSIM_MAX_PEDS) return NAVSIM_E_ARG;
    if (!st->robot_pose || !st->prev_action || !st->n_peds || !st->ped_pose || !st->ped_vel) return NAVSIM_E_ARG;
    const bool truth = p->model == NAVSIM_FORECAST_TRUE;
    if (truth && c->ped_model == NAVSIM_PED_SFM && (!st->field || !st->ped_v_pref || !st->ped_waypoints || !st->ped_n_waypoints ||
                                                    !st->ped_wp_head || c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS))
        return NAVSIM_E_ARG;
    if (truth && c->ped_model == NAVSIM_PED_EXTERNAL && !ped_cmd && !st->ped_cmd) return NAVSIM_E_ARG;
    if (c->n_envs < 0 || c->map_h < 1 || c->map_w < 1) return NAVSIM_E_ARG;
    if (!(c->resolution > 0.0) || !std::isfinite(c->resolution) || !(c->time_step > 0.0) || !std::isfinite(c->time_step)) return NAVSIM_E_ARG;
    if (c->action_kind != NAVSIM_ACTION_TWIST && c->action_kind != NAVSIM_ACTION_WHEELS) return NAVSIM_E_ARG;
    if (c->action_kind == NAVSIM_ACTION_WHEELS && (!(c->wheel_radius > 0.0) || !std::isfinite(c->wheel_radius) || !std::isfinite(c->wheel_track)))
        return NAVSIM_E_ARG;
    if (st->map_slot && c->shared_field) return NAVSIM_E_ARG;
    if (c->field_format != NAVSIM_FIELD_F32 && c->field_format != NAVSIM_FIELD_U16T) return NAVSIM_E_UNSUPPORTED;
    if (st->rect_table && (c->field_format != NAVSIM_FIELD_U16T || c->map_h > 1024 || c->map_w > 1024)) return NAVSIM_E_UNSUPPORTED;
    if (c->n_envs == 0) return NAVSIM_OK;
    PedForecastArgs a = {};
    a.out = *out; a.actions = p->robot == NAVSIM_FORECAST_ACTIONS ? actions : nullptr;
    a.ped_cmd = truth && c->ped_model == NAVSIM_PED_EXTERNAL ? ped_cmd : nullptr; a.skip = skip;
    a.H = p->horizon; a.robot = p->robot; a.model = p->model;
    hipStream_t s = (hipStream_t)stream;
    return with_field(c, st, [&](auto field) { return launch_ped_forecast<typename decltype(field)::type>(c, st, a, s); });
}

int navsim_mppi(const navsim_config* c, const navsim_state* st, const navsim_mppi_params* p, const navsim_goal_field* field,
                const navsim_goal_path_params* gp, const double* ped_cmd, const uint8_t* skip, const navsim_mppi_ws* ws,
                const navsim_mppi_out* out, void* stream) {
    (void)hipGetLastError();
    if (!c || !st || !p || !ws || !out) return NAVSIM_E_ARG;
    if (!ws->plan || !ws->plan_key || !ws->actions || !ws->cost) return NAVSIM_E_ARG;
    if (!out->action || !out->best || !out->cost_best || !out->ess || !out->status) return NAVSIM_E_ARG;
    if (p->n_samples < 1 || p->n_samples > NAVSIM_ROLLOUT_MAX_K || p->horizon < 1 || p->horizon > NAVSIM_ROLLOUT_MAX_H) return NAVSIM_E_ARG;
    if (p->iterations < 1 || p->iterations > 8) return NAVSIM_E_ARG;
    if ((p->stop_sample != 0 && p->stop_sample != 1) || (p->select != 0 && p->select != 1)) return NAVSIM_E_ARG;
    for (int i = 0; i < 2; ++i) {
        if (!std::isfinite(p->sigma[i]) || p->sigma[i] < 0.0) return NAVSIM_E_ARG;
        if (!std::isfinite(p->lo[i]) || !std::isfinite(p->hi[i]) || !std::isfinite(p->init_action[i])) return NAVSIM_E_ARG;
        if (!(p->lo[i] <= p->hi[i]) || !(p->lo[i] <= p->init_action[i]) || !(p->init_action[i] <= p->hi[i])) return NAVSIM_E_ARG;
        if (p->stop_sample && !(p->lo[i] <= 0.0 && 0.0 <= p->hi[i])) return NAVSIM_E_ARG;
    }
    if (!(p->beta >= 0.0) || !(p->beta < 1.0)) return NAVSIM_E_ARG;
    if (!(fabs(p->alpha - sqrt(1.0 - p->beta * p->beta)) <= 1e-12)) return NAVSIM_E_ARG;
    if (!std::isfinite(p->lambda) || !(p->lambda > 0.0)) return NAVSIM_E_ARG;
    const double nonneg[] = {p->w_goal, p->w_crash, p->off_field_cost};
    for (double x : nonneg)
        if (!std::isfinite(x) || x < 0.0) return NAVSIM_E_ARG;
    if (!st->episode) return NAVSIM_E_ARG;
    if (field) {
        if (!gp || !field->dist) return NAVSIM_E_ARG;
        if (!std::isfinite(gp->hard_clearance) || !std::isfinite(gp->lookahead) || gp->lookahead < 0.0) return NAVSIM_E_ARG;
        if (!(c->resolution > 0.0) || !std::isfinite(c->resolution) || gp->hard_clearance < 3.0 * c->resolution) return NAVSIM_E_ARG;
        if (c->map_h / 5 < 1 || c->map_w / 5 < 1) return NAVSIM_E_ARG;
    }
    const navsim_rollout_params rp = {p->n_samples, p->horizon, p->range, p->gamma};
    const int rc = rollout_check(c, st, &rp, ws->actions, ped_cmd, &ws->roll);
    if (rc != NAVSIM_OK) return rc;
    if (c->n_envs == 0) return NAVSIM_OK;
    MppiArgs a = {};
    a.p = *p; a.ws = *ws; a.out = *out; a.skip = skip;
    a.episode = st->episode; a.steps = st->steps; a.robot_goal = st->robot_goal;
    a.field = st->field; a.overflow = st->field_overflow; a.map_slot = st->map_slot;
    a.seed = c->seed; a.origin_x = c->origin_x; a.origin_y = c->origin_y; a.resolution = c->resolution;
    a.env_index_base = c->env_index_base; a.map_h = c->map_h; a.map_w = c->map_w; a.shared_field = c->shared_field;
    if (field) {
        a.goal_dist = field->dist;
        a.Hc = c->map_h / 5; a.Wc = c->map_w / 5;
        a.hard = (float)(gp->hard_clearance / c->resolution);
        const double look = floor(gp->lookahead / c->resolution);
        a.lookahead_cells = (int)(look < 1048576.0 ? look : 1048576.0);
    }
    hipStream_t s = (hipStream_t)stream;
    const int block = 64 * ((2 * p->n_samples + 63) / 64);
    for (int it = 0; it < p->iterations; ++it) {
        a.it = it; a.last = it == p->iterations - 1;
        mppi_sample_kernel<<<c->n_envs, block, 0, s>>>(a);
        int rc2 = launch_status();
        if (rc2 != NAVSIM_OK) return rc2;
        rc2 = rollout_launch(c, st, &rp, ws->actions, ped_cmd, skip, &ws->roll, s);
        if (rc2 != NAVSIM_OK) return rc2;
        rc2 = with_field(c, st, [&](auto f) {
            mppi_update_kernel<typename decltype(f)::type><<<c->n_envs, kMppiUpdateBlock, 0, s>>>(a);
            return launch_status();
        });
        if (rc2 != NAVSIM_OK) return rc2;
    }
    return NAVSIM_OK;
}

const char* navsim_step_kernel_name(void) { return "navsim_step_kernel"; }

// test hook (declared in include/navsim.h under "test hooks")
int navsim_debug_math(int32_t fn, const double* x, const double* x2, double* out, int32_t n, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!x || !out || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    math_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(fn, x, x2, out, n);
    return launch_status();
}

// test hook: batch_xy_to_ij (env.py:1228-1253) as the scan uses it.  as_f32 = 1: the inputs are first rounded to
// float32 and divided in float32 (the lidar origin, env.py:386, 419); 0: float64 inputs (env.py:348-349).
int navsim_debug_xy_to_ij(const navsim_config* c, const double* xy, int32_t as_f32, int32_t* ij, int32_t n, void* stream) {
    (void)hipGetLastError();
    if (!c || !xy || !ij || n < 0) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    xy_to_ij_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(*c, xy, as_f32, ij, n);
    return launch_status();
}

// text of the HIP error behind the last NAVSIM_E_LAUNCH on this thread
const char* navsim_last_hip_error(void) { return hipGetErrorString(g_last_hip_error); }

// tests only: the spawn loops' acceptance rules on supplied candidates (include/navsim.h)
int navsim_debug_spawn_decisions(const navsim_config* c, const uint8_t* cost, int32_t Hc, int32_t Wc, int32_t n,
                                 const int32_t* kind, const double* start, const double* goal, const double* robot,
                                 double* wp_scratch, int32_t* code, void* stream) {
    (void)hipGetLastError();
    if (!c || !cost || !kind || !start || !goal || !wp_scratch || !code || n < 0 || Hc < 1 || Wc < 1 ||
        c->max_waypoints < 1 || c->max_waypoints > NAVSIM_MAX_WAYPOINTS) return NAVSIM_E_ARG;
    if (n == 0) return NAVSIM_OK;
    if (!plan_fits(Hc, Wc) || allow_lds((const void*)spawn_decisions_kernel, plan_lds(Hc, Wc)) != NAVSIM_OK)
        return NAVSIM_E_UNSUPPORTED;
    spawn_decisions_kernel<<<n, 256, plan_lds(Hc, Wc), (hipStream_t)stream>>>(*c, cost, Hc, Wc, kind, start, goal, robot,
                                                                            wp_scratch, code);
    return launch_status();
}

// microbenchmark hook, see gather_probe_kernel
int navsim_debug_gather(const float* x, uint64_t n_words, int32_t mode, int32_t iters, int32_t n_threads,
                        float* out, void* stream) {
    (void)hipGetLastError();   // drop stale errors of unrelated earlier runtime calls
    if (!x || !out || n_threads <= 0) return NAVSIM_E_ARG;
    gather_probe_kernel<<<(n_threads + 255) / 256, 256, 0, (hipStream_t)stream>>>(x, n_words, mode, iters, 12345, out);
    return launch_status();
}

// self-test of NAVSIM_KERNARGS (kernels_step.hpp): the views into the kernarg segment against the by-value copies, byte for byte
int navsim_debug_kernarg_layout(void* stream) {
    hipStream_t s = (hipStream_t)stream;
    navsim_config c; navsim_state st; navsim_step_io io; StepInstall in;
    memset(&c, 0x5A, sizeof(c)); memset(&st, 0xA7, sizeof(st)); memset(&io, 0x3C, sizeof(io)); memset(&in, 0xE1, sizeof(in));
    for (size_t i = 0; i < sizeof(c); ++i) ((unsigned char*)&c)[i] ^= (unsigned char)(i * 7u);
    for (size_t i = 0; i < sizeof(st); ++i) ((unsigned char*)&st)[i] ^= (unsigned char)(i * 13u);
    for (size_t i = 0; i < sizeof(io); ++i) ((unsigned char*)&io)[i] ^= (unsigned char)(i * 29u);
    for (size_t i = 0; i < sizeof(in); ++i) ((unsigned char*)&in)[i] ^= (unsigned char)(i * 31u);
    int* out = nullptr;
    if (hipMalloc((void**)&out, sizeof(int)) != hipSuccess) return NAVSIM_E_LAUNCH;
    int res = -1;
    (void)hipMemcpyAsync(out, &res, sizeof(int), hipMemcpyHostToDevice, s);
    kernarg_layout_probe_kernel<<<1, 64, 0, s>>>(c, st, io, in, 0x1234567, out);
    const bool ok = hipMemcpyAsync(&res, out, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    (void)hipFree(out);
    if (!ok) return NAVSIM_E_LAUNCH;
    return res == 1 ? NAVSIM_OK : NAVSIM_E_UNSUPPORTED;
}

// diagnostic build only: where the per-arena stamps go (NULL disables)
int navsim_debug_set_stamps(unsigned long long* buf) {
#ifdef NAVSIM_STAMPS
    int rc = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)) == hipSuccess ? NAVSIM_OK : NAVSIM_E_LAUNCH;
#define NAVSIM_SET(B, P) if (rc == NAVSIM_OK) rc = navsim_step_set_stamps_##B##_##P(buf);
    NAVSIM_SET(64, 0) NAVSIM_SET(64, 1) NAVSIM_SET(256, 0) NAVSIM_SET(256, 1) NAVSIM_SET(512, 0) NAVSIM_SET(512, 1)
    NAVSIM_SET(1024, 0) NAVSIM_SET(1024, 1)
#undef NAVSIM_SET
    return rc;
#else
    (void)buf;
    return NAVSIM_E_UNSUPPORTED;
#endif
}

}  // extern "C"
