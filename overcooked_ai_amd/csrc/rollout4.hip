// rollout4.hip — the instances of k_rollout4 (step_lut4.hpp) and k_rollout5 (step_duo5.hpp), in three translation units: this
// file is compiled with -DOC_R4_PART=0 (joint move table + event logging), 1 (per-env terrain: k_rollout5's mover / interact
// workgroups and MODE 2, the pose one step ahead in one wavefront) and 2 (MODE 0: arithmetic movement), so that a clean build runs four hipcc processes side by side (overcooked_ai_amd/build.py) instead
// of one 80-second compile.  oc_amd.hip (choose_rollout) picks the instance; the unit that compiles it launches it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "shared.hpp"

#ifndef OC_R4_PART
#error "compile with -DOC_R4_PART=0, 1 or 2"
#endif

namespace {

#include "common.hpp"
#include "host_util.hpp"
#include "reset.hpp"
#include "step_predicate.hpp"
#include "step_table.hpp"
#include "step_lut4.hpp"
#if OC_R4_PART == 1
#include "step_duo5.hpp"
#endif

// dynamic LDS of a k_rollout4 instance: its tables + the cell words of a workgroup's 256 envs
// (EV: + the per-episode event counters, [N_EVENT_TYPES][BLOCK] u32 behind the cell words; REC: + the packed object planes,
//  [n_obj][BLOCK] x 16 bytes, last: behind the counters when both are on)
template <class P>
constexpr size_t lds4_bytes(size_t cell_rows) {
    return (size_t)Lds4<P>::CELLS + cell_rows * BLOCK * P::CW + (P::EV ? (size_t)N_EVENT_TYPES * BLOCK * 4 : 0) +
           (P::REC ? (cell_rows - 2) * BLOCK : 0);
}

using oc_detail::g_describe;
using oc_detail::Rollout4Call;

const char* tf(bool v) { return v ? "true" : "false"; }

// launches k_rollout4<P> (oc_rollout_plan: names it instead)
template <class P>
void go4(const Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = lds4_bytes<P>((size_t)c.n_obj * 16 + 2);  // (+ two spare words per lane: nopot_off)
    if (g_describe) {
        snprintf(g_describe, 256, "k_rollout4<UNIFORM=%s, MAXP=%d, LAY_LDS=%s, MODE=%d, OUT=%s, OLD=%s, NF=%d, EV=%s, PIPE=%s, RU=%s, CW=%d, "
                 "NOCONF=%s, FT8=%s, REC=%s> one wavefront per 64 envs, %zu B LDS", tf(P::UNIFORM), P::MAXP, tf(P::LAY_LDS), P::MODE,
                 tf(P::OUT), tf(P::OLD), P::NF, tf(P::EV), tf(P::PIPE), tf(P::RU), P::CW, tf(P::NOCONF), tf(P::FT8), tf(P::REC), smem);
        return;
    }
    if (!want_lds(k_rollout4<P>, smem)) return;
    hipLaunchKernelGGL(k_rollout4<P>, dim3(grid_for(b->n_envs)), dim3(BLOCK), smem, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id,
                       (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon,
                       c.options, (uint32_t)c.seed, (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, c.sa, c.ea, c.ra);
}

// launches instance c.r4 of the list if this unit compiles it
template <class... P>
void go4_listed(const Rollout4Call& c, oc_detail::R4List<P...>) {
    int id = 0;
    auto one = [&](auto p) {
        using Q = decltype(p);
        if constexpr (Q::PART == OC_R4_PART)
            if (id == c.r4) go4<Q>(c);
        ++id;
    };
    (one(P()), ...);
}

#if OC_R4_PART == 1
// launches k_rollout5 (step_duo5.hpp): the per-env-terrain mover / interact kernel of round 6; two spare cell rows per lane
template <bool LAY_LDS, bool FT8, bool OLD, bool BIG, bool EV, bool NOOUT>
void go5(const Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = oc_detail::rollout5_lds_bytes(LAY_LDS, BIG, EV, c.n_obj);
    if (g_describe) {
        const int64_t per_round = (simd_count() / 4) * BLOCK;
        snprintf(g_describe, 256, "k_rollout5<LAY_LDS=%s, FT8=%s, OLD=%s, BIG=%s, EV=%s%s> mover + interact wavefronts, %d round(s), %zu B LDS",
                 tf(LAY_LDS), tf(FT8), tf(OLD), tf(BIG), tf(EV), NOOUT ? ", NOOUT=true" : "", (int)((b->n_envs + per_round - 1) / per_round), smem);
        return;
    }
    if (!want_lds(k_rollout5<LAY_LDS, FT8, OLD, BIG, EV, NOOUT>, smem)) return;
    hipLaunchKernelGGL((k_rollout5<LAY_LDS, FT8, OLD, BIG, EV, NOOUT>), dim3(grid_for(b->n_envs)), dim3(2 * BLOCK), smem, c.stream,
                       b->d_layouts, b->n_layouts, b->d_layout_id, (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags,
                       (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon, c.options, (uint32_t)c.seed,
                       (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, c.sa, c.ea);
}

// k_rollout5's 24 instances: four table kinds x {tiled flags, flat flags, no output arrays} x {new, old dynamics}
template <bool LAY_LDS, bool BIG, bool EV>
void go5_table(const Rollout4Call& c) {
    const bool old = c.r5.old;
    if (c.r5.noout) old ? go5<LAY_LDS, false, true, BIG, EV, true>(c) : go5<LAY_LDS, false, false, BIG, EV, true>(c);
    else if (c.r5.ft8) old ? go5<LAY_LDS, true, true, BIG, EV, false>(c) : go5<LAY_LDS, true, false, BIG, EV, false>(c);
    else old ? go5<LAY_LDS, false, true, BIG, EV, false>(c) : go5<LAY_LDS, false, false, BIG, EV, false>(c);
}
#endif

}  // namespace

namespace oc_detail {

#if OC_R4_PART == 1
// dynamic LDS of a k_rollout5 workgroup: tables, ring, the cell words of 256 envs (+ two spare rows) and, with the event log,
// N_EVENT_TYPES rows of counters (9 x 5 grids: 163 120 of the CU's 163 840 bytes)
size_t rollout5_lds_bytes(bool lay_lds, bool big, bool ev, int n_obj) {
    return (size_t)(lay_lds ? Lds5<true>::CELLS : Lds5<false>::CELLS) + ((size_t)n_obj * 16 + 2) * BLOCK * (big ? 2 : 4) +
           (ev ? (size_t)N_EVENT_TYPES * BLOCK * 4 : 0);
}
#endif

template <int UNIT>
void launch_rollout(const Rollout4Call& c) {
#if OC_R4_PART == 1
    if (c.r4 < 0) {
        if (c.r5.ev) go5_table<true, false, true>(c);  // (event counters: tables in LDS, at most 64 cells)
        else if (c.r5.big) go5_table<true, true, false>(c);  // (65..128 cells: tables in LDS only)
        else if (c.r5.lay_lds) go5_table<true, false, false>(c);
        else go5_table<false, false, false>(c);
        return;
    }
#endif
    go4_listed(c, R4Instances());
}
template void launch_rollout<OC_R4_PART>(const Rollout4Call& c);

}  // namespace oc_detail
