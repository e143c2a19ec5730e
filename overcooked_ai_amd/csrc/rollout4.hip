// rollout4.hip — the instances of k_rollout4 (step_lut4.hpp) and k_rollout5 (step_duo5.hpp), in three translation units: this
// file is compiled with -DOC_R4_PART=0 (joint move table + event logging), 1 (per-env terrain: k_rollout5's mover / interact
// workgroups and MODE 2, the pose one step ahead in one wavefront) and 2 (MODE 0: arithmetic movement), so that a clean build runs four hipcc processes side by side (overcooked_ai_amd/build.py) instead
// of one 80-second compile.  oc_amd.hip (choose_rollout) picks the instance; the unit that compiles it launches it
// (launch_rollout) or, for oc_rollout_plan, names it and its LDS bytes (describe_rollout).
// The OC_R4_PART == 2 unit, the shortest of the four, also compiles mlp_tile.hpp (the MFMA tile of the dense network: device functions
// for the kernels of partner.hpp, partner_pool.hpp, policy.hpp and bc_fused.hpp), partner.hpp (k_partner_logits and its two entry points) and
// gae.hpp (k_gae, k_gae_moments and theirs), ppo_loss.hpp (k_ppo_loss, k_ppo_loss_stats and theirs) and policy.hpp (k_policy_forward,
// k_policy_backward, k_policy_grad_sum and theirs), adam.hpp (k_adam_step and its two), bc_loss.hpp (k_bc_loss, k_bc_loss_stats and theirs),
// update_chain.hpp (host code only: oc_ppo_update and oc_bc_update), bc_fused.hpp (k_bc_epoch_fused and its two) and sample_index.hpp (k_sample_count, k_sample_scan, k_sample_write,
// k_sample_permute and their three), and outcomes.hpp (k_outcomes, k_outcome_sum and their two).
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

using oc_detail::Rollout4Call;

const char* tf(bool v) { return v ? "true" : "false"; }

// ---- k_rollout4<P>: its dynamic LDS for c's grid (+ two spare words per lane: nopot_off), its launch, its description
template <class P>
size_t smem4(const Rollout4Call& c) { return lds4_bytes<P>((size_t)c.n_obj * 16 + 2); }

template <class P>
void go4(const Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = smem4<P>(c);
    if (!want_lds(k_rollout4<P>, smem)) return;
    hipLaunchKernelGGL(k_rollout4<P>, dim3(grid_for(b->n_envs)), dim3(BLOCK), smem, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id,
                       (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon,
                       c.options, (uint32_t)c.seed, (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, c.sa, c.ea, c.ra);
}

template <class P>
void describe4(const Rollout4Call& c, char* out, size_t out_size) {
    snprintf(out, out_size, "k_rollout4<UNIFORM=%s, MAXP=%d, LAY_LDS=%s, MODE=%d, OUT=%s, OLD=%s, NF=%d, EV=%s, PIPE=%s, RU=%s, CW=%d, "
             "NOCONF=%s, FT8=%s, REC=%s> one wavefront per 64 envs, %zu B LDS", tf(P::UNIFORM), P::MAXP, tf(P::LAY_LDS), P::MODE,
             tf(P::OUT), tf(P::OLD), P::NF, tf(P::EV), tf(P::PIPE), tf(P::RU), P::CW, tf(P::NOCONF), tf(P::FT8), tf(P::REC), smem4<P>(c));
}

// f(Q()) for instance r4 of the list if this unit compiles it
template <class F, class... P>
void with_r4(int r4, oc_detail::R4List<P...>, F f) {
    int id = 0;
    auto one = [&](auto p) {
        using Q = decltype(p);
        if constexpr (Q::PART == OC_R4_PART)
            if (id == r4) f(p);
        ++id;
    };
    (one(P()), ...);
}

#if OC_R4_PART == 1
// ---- k_rollout5 (step_duo5.hpp): the per-env-terrain mover / interact kernel of round 6; two spare cell rows per lane
template <bool LAY_LDS_, bool FT8_, bool OLD_, bool BIG_, bool EV_, bool NOOUT_>
struct R5 {
    static constexpr bool LAY_LDS = LAY_LDS_, FT8 = FT8_, OLD = OLD_, BIG = BIG_, EV = EV_, NOOUT = NOOUT_;
};
template <class K>
size_t smem5(const Rollout4Call& c) { return oc_detail::rollout5_lds_bytes(K::LAY_LDS, K::BIG, K::EV, c.n_obj); }

// The pot slots of an instance are resolved here, where it is launched and described: the six instances of new dynamics, 32-bit cell
// words and no event log ({table in LDS, through L2} x {tiled flags, flat flags, no output arrays}) exist with one slot as well, for
// tables whose layouts all have one pot (R5Sel.one_pot); every other instance has two
template <class K>
constexpr bool r5_has_one_pot() { return !K::OLD && !K::BIG && !K::EV; }
template <class K>
bool one_pot5(const Rollout4Call& c) { return r5_has_one_pot<K>() && c.r5.one_pot; }

template <class K, int MAXP>
void go5_slots(const Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = smem5<K>(c);
    if (!want_lds(k_rollout5<K::LAY_LDS, K::FT8, K::OLD, K::BIG, K::EV, K::NOOUT, MAXP>, smem)) return;
    hipLaunchKernelGGL((k_rollout5<K::LAY_LDS, K::FT8, K::OLD, K::BIG, K::EV, K::NOOUT, MAXP>), dim3(grid_for(b->n_envs)), dim3(2 * BLOCK), smem,
                       c.stream, b->d_layouts, b->n_layouts, b->d_layout_id, (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags,
                       (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon, c.options, (uint32_t)c.seed,
                       (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, c.sa, c.ea);
}
template <class K>
void go5(const Rollout4Call& c) {
    if constexpr (r5_has_one_pot<K>())
        if (c.r5.one_pot) return go5_slots<K, 1>(c);
    go5_slots<K, 2>(c);
}

template <class K>
void describe5(const Rollout4Call& c, char* out, size_t out_size) {
    const int64_t per_round = (simd_count() / 4) * BLOCK;
    snprintf(out, out_size, "k_rollout5<LAY_LDS=%s, FT8=%s, OLD=%s, BIG=%s, EV=%s%s>%s mover + interact wavefronts, %d round(s), %zu B LDS",
             tf(K::LAY_LDS), tf(K::FT8), tf(K::OLD), tf(K::BIG), tf(K::EV), K::NOOUT ? ", NOOUT=true" : "",
             one_pot5<K>(c) ? " one pot slot," : "", (int)((c.b->n_envs + per_round - 1) / per_round), smem5<K>(c));
}

// f(R5<...>()) for the instance s selects, of k_rollout5's 24: four table kinds x {tiled flags, flat flags, no output arrays} x
// {new, old dynamics} (go5 / describe5 then take the one-slot form of the six that have one)
template <bool LAY_LDS, bool BIG, bool EV, class F>
void with_r5_table(const oc_detail::R5Sel& s, F f) {
    if (s.noout) s.old ? f(R5<LAY_LDS, false, true, BIG, EV, true>()) : f(R5<LAY_LDS, false, false, BIG, EV, true>());
    else if (s.ft8) s.old ? f(R5<LAY_LDS, true, true, BIG, EV, false>()) : f(R5<LAY_LDS, true, false, BIG, EV, false>());
    else s.old ? f(R5<LAY_LDS, false, true, BIG, EV, false>()) : f(R5<LAY_LDS, false, false, BIG, EV, false>());
}
template <class F>
void with_r5(const oc_detail::R5Sel& s, F f) {
    if (s.ev) with_r5_table<true, false, true>(s, f);  // (event counters: tables in LDS, at most 64 cells)
    else if (s.big) with_r5_table<true, true, false>(s, f);  // (65..128 cells: tables in LDS only)
    else if (s.lay_lds) with_r5_table<true, false, false>(s, f);
    else with_r5_table<false, false, false>(s, f);
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
    if (c.r4 < 0) return with_r5(c.r5, [&](auto k) { go5<decltype(k)>(c); });
#endif
    with_r4(c.r4, R4Instances(), [&](auto p) { go4<decltype(p)>(c); });
}
template void launch_rollout<OC_R4_PART>(const Rollout4Call& c);

template <int UNIT>
void describe_rollout(const Rollout4Call& c, char* out, size_t out_size) {
#if OC_R4_PART == 1
    if (c.r4 < 0) return with_r5(c.r5, [&](auto k) { describe5<decltype(k)>(c, out, out_size); });
#endif
    with_r4(c.r4, R4Instances(), [&](auto p) { describe4<decltype(p)>(c, out, out_size); });
}
template void describe_rollout<OC_R4_PART>(const Rollout4Call& c, char* out, size_t out_size);

}  // namespace oc_detail

#if OC_R4_PART == 2
#include "mlp_tile.hpp" // the MFMA tile of the dense network under the five kernels of partner.hpp, partner_pool.hpp, policy.hpp and bc_fused.hpp
#include "partner.hpp"  // k_partner_logits, oc_partner_logits, oc_partner_logits_plan
#include "gae.hpp"      // k_gae, k_gae_moments, oc_gae, oc_gae_plan
#include "outcomes.hpp" // k_outcomes, k_outcome_sum, oc_outcome_table, oc_outcome_plan
#include "ppo_loss.hpp" // k_ppo_loss, k_ppo_loss_stats, oc_ppo_loss, oc_ppo_loss_plan
#include "policy.hpp"   // k_policy_forward, k_policy_backward, k_policy_grad_sum, oc_policy_forward, oc_policy_backward, oc_policy_plan
#include "adam.hpp"     // k_adam_step, oc_adam_step, oc_adam_plan
#include "bc_loss.hpp"  // k_bc_loss, k_bc_loss_stats, oc_bc_loss, oc_bc_loss_plan
#include "update_chain.hpp"  // oc_ppo_update, oc_bc_update and their plans (host code: the launches of the files above, minibatch after minibatch)
#include "bc_fused.hpp"      // k_bc_epoch_fused, oc_bc_epoch_fused, oc_bc_epoch_fused_plan (oc_bc_update's chain for minibatches of one workgroup, in one kernel)
#include "sample_index.hpp"  // k_sample_count, k_sample_scan, k_sample_write, k_sample_permute, oc_sample_select, oc_sample_permute, oc_sample_index_plan
#include "partner_pool.hpp"  // k_pool_seat, k_pool_write, k_pool_logits, oc_partner_pool_logits, oc_partner_pool_plan (after partner.hpp and sample_index.hpp)
#endif
