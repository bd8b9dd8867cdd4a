// navsim_step_inst.hip -- ONE (threads per arena, pedestrians or not) family of the fused step kernel.
//
// The step kernel is a template over <BLOCK, PEDS, Field, RULE, RECT, PINL>; compiled from one translation unit its 200-odd
// instantiations made the library a four-minute build (round-4 verdict: "build time is unreported").  This file is compiled
// once per (NAVSIM_INST_BLOCK, NAVSIM_INST_PEDS) pair -- eight objects, in parallel (csrc/Makefile) -- and exports one
// launcher per pair, navsim_step_launch_<BLOCK>_<PEDS>, which navsim_kernels.hip's dispatch_step calls with what to launch
// (StepLaunch) and how (StepPlan; both step_plan.hpp).  Same kernels, same code objects as the single unit produced; the
// launchers are internal to the library (hidden visibility).
#include "preamble.hpp"

#if !defined(NAVSIM_INST_BLOCK) || !defined(NAVSIM_INST_PEDS)
#error "compile with -DNAVSIM_INST_BLOCK=64|256|512|1024 -DNAVSIM_INST_PEDS=0|1 (csrc/Makefile)"
#endif

namespace {
#include "kernels_field.hpp"
#include "kernels_rect.hpp"
#include "kernels_plan.hpp"
#include "kernels_regen_dev.hpp"
#include "kernels_step.hpp"
}  // namespace
#include "step_plan.hpp"

namespace {

// one launch: the kernel's LDS grant, nothing more for navsim_prepare, else the launch itself
template <typename Kernel, typename... Args>
int launch(Kernel kernel, const StepLaunch& l, int blocks, int block, size_t lds, const Args&... args) {
    if (allow_lds((const void*)kernel, lds) != NAVSIM_OK) return NAVSIM_E_UNSUPPORTED;
    if (l.prepare_only) return NAVSIM_OK;
    kernel<<<blocks, block, lds, l.stream>>>(args...);
    return NAVSIM_OK;
}

// which kernel, and its arguments
template <int BLOCK, bool PEDS, typename Field, int RECT, int RULE, bool PINL>
int launch_step_pinl(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const StepLaunch& l, const StepPlan& p) {
    constexpr bool kPacked = !std::is_same<Field, FieldF32>::value;
    const unsigned scan = (unsigned)step_lds_scan_bytes(c, p.park);
    const int blocks = l.grid > 0 ? l.grid : c->n_envs;
    // navsim_step_sorted's front workgroup exists in navsim_step_kernel only
    if (l.sort_cost && (l.part != NAVSIM_STEP_ALL || l.install)) return NAVSIM_E_UNSUPPORTED;
    if constexpr (PEDS && PINL) {
        if (l.part == kStepPartReplan) {                           // navsim_step_replan: the re-plan inside the step's launch
            const size_t pl = plan_lds(c->map_h / 5, c->map_w / 5), lds = p.lds > pl ? p.lds : pl;
            if (l.install) {                                       // ... with the install of the staged worlds (packed fields)
                if constexpr (kPacked)
                    return launch(navsim_step_replan_install_kernel<BLOCK, Field, RULE, RECT>, l, l.grid + c->n_envs, BLOCK, lds,
                                  *c, *st, *io, *l.install, scan, p.park, p.rect_off, l.grid, l.max_queries);
                return NAVSIM_E_UNSUPPORTED;
            }
            return launch(navsim_step_replan_kernel<BLOCK, Field, RULE, RECT>, l, l.grid + c->n_envs, BLOCK, lds,
                          *c, *st, *io, scan, p.park, p.rect_off, l.grid, l.max_queries);
        }
        if (l.part == NAVSIM_STEP_DUE)                             // navsim_step_part's compact launch (kernels_step.hpp)
            return launch(navsim_step_due_kernel<BLOCK, Field, RULE, RECT>, l, blocks, BLOCK, p.lds, *c, *st, *io, scan, p.park, p.rect_off);
    }
    if constexpr (PINL == PEDS && kPacked) {
        if (l.install)                                             // navsim_step_install: packed fields, pedestrians inside the step
            return launch(navsim_step_install_kernel<BLOCK, PEDS, Field, RULE, RECT>, l, blocks, BLOCK, p.lds,
                          *c, *st, *io, *l.install, step_kernel_word(l), l.mask, scan, p.park, p.rect_off);
    }
    if (l.install) return NAVSIM_E_UNSUPPORTED;
    if constexpr (!PEDS) {
        // the plain form (kernels_step.hpp step_arena FEAT = false: no terminal observation, no next-step reset compiled in) for
        // the calls that use neither -- round 5's code, and what the c2 / c4 bench lines run.  A step under a time limit
        // (cfg.max_episode_steps) takes the featured form too; reset-only launches count no steps and need none of it.
        const bool feat = io->final_obs || io->reset_mask || c->auto_reset == NAVSIM_AUTORESET_NEXT_STEP ||
                          (c->max_episode_steps > 0 && !l.reset_only);
        if (!feat)
            return launch(navsim_step_kernel<BLOCK, PEDS, Field, RULE, RECT, PINL, false>, l, step_kernel_blocks(c, l), BLOCK, p.lds,
                          *c, *st, *io, step_kernel_word(l), l.mask, scan, p.park, p.rect_off, l.sort_cost, l.sort_order);
    }
    return launch(navsim_step_kernel<BLOCK, PEDS, Field, RULE, RECT, PINL, true>, l, step_kernel_blocks(c, l), BLOCK, p.lds,
                  *c, *st, *io, step_kernel_word(l), l.mask, scan, p.park, p.rect_off, l.sort_cost, l.sort_order);
}
// pedestrian variants: the form without the pedestrian phase when ped_update_kernel has run or nothing is integrated at all
// (a reset-only launch), else -- and for every install -- the form that carries it
template <int BLOCK, bool PEDS, typename Field, int RECT, int RULE>
int launch_step_kernel(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const StepLaunch& l, const StepPlan& p) {
    if constexpr (PEDS) {
        if ((!l.reset_only && !l.peds_done) || l.install) return launch_step_pinl<BLOCK, PEDS, Field, RECT, RULE, true>(c, st, io, l, p);
    }
    return launch_step_pinl<BLOCK, PEDS, Field, RECT, RULE, false>(c, st, io, l, p);
}

template <int BLOCK, bool PEDS, typename Field, int RECT>
int launch_step_rule(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const StepLaunch& l,
                     const StepPlan& p) {
    return with_march_rule<Field>(march_rule_variant(c), [&](auto rule) {
        return launch_step_kernel<BLOCK, PEDS, Field, RECT, decltype(rule)::value>(c, st, io, l, p);
    });
}

template <int BLOCK, bool PEDS, typename Field>
int launch_step_field(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const StepLaunch& l,
                      const StepPlan& p) {
    if (p.rect == 2) return launch_step_rule<BLOCK, PEDS, Field, 2>(c, st, io, l, p);
    return p.rect ? launch_step_rule<BLOCK, PEDS, Field, 1>(c, st, io, l, p)
                  : launch_step_rule<BLOCK, PEDS, Field, 0>(c, st, io, l, p);
}

template <int BLOCK, bool PEDS>
int launch_step_family(const navsim_config* c, const navsim_state* st, const navsim_step_io* io, const StepLaunch& l,
                       const StepPlan& p) {
    return with_field(c, st, [&](auto field) {
        typedef typename decltype(field)::type Field;
        if constexpr (std::is_same<Field, FieldF32>::value) return launch_step_rule<BLOCK, PEDS, Field, 0>(c, st, io, l, p);   // (no record table)
        else return launch_step_field<BLOCK, PEDS, Field>(c, st, io, l, p);
    });
}

}  // namespace

#define NAVSIM_CAT_(a, b, c) a##b##_##c
#define NAVSIM_CAT(a, b, c) NAVSIM_CAT_(a, b, c)

// what dispatch_step (navsim_kernels.hip) calls with the launch it was given and the plan it made of it
extern "C" __attribute__((visibility("hidden")))
int NAVSIM_CAT(navsim_step_launch_, NAVSIM_INST_BLOCK, NAVSIM_INST_PEDS)(const navsim_config* c, const navsim_state* st,
                                                                        const navsim_step_io* io, const StepLaunch* l, const StepPlan* p) {
    return launch_step_family<NAVSIM_INST_BLOCK, (NAVSIM_INST_PEDS != 0)>(c, st, io, *l, *p);
}

// diagnostic builds (-DNAVSIM_STAMPS): every unit has its own copy of the stamp pointer
extern "C" __attribute__((visibility("hidden")))
int NAVSIM_CAT(navsim_step_set_stamps_, NAVSIM_INST_BLOCK, NAVSIM_INST_PEDS)(unsigned long long* buf) {
#ifdef NAVSIM_STAMPS
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)) == hipSuccess ? NAVSIM_OK : NAVSIM_E_LAUNCH;
#else
    (void)buf;
    return NAVSIM_E_UNSUPPORTED;
#endif
}
