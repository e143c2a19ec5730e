// rollout_dispatch.hpp — host only: the random-rollout family.  oc_rollout_random is planned first (plan_rollout: every check, then
// the family and, for k_rollout4 / k_rollout5, the one to three launches choose_rollout picks; no launch, no device memory), then
// launched — or, by oc_rollout_plan, described; oc_rollout_record and oc_rollout_record_ex share their checks and their launch
// (rollout_record).  The k_rollout4 / k_rollout5 instances are compiled in rollout4.hip's three units (shared.hpp: R4Instances,
// Rollout4Call) and launched through oc_detail::launch_rollout; k_rollout_pair and k_rollout are launched here.
// Part of liboc_amd.so: included by oc_amd.hip at file scope.  The kernels are step_lut4.hpp and step_duo5.hpp (rollout4.hip),
// rollout_pair.hpp and step_predicate.hpp.
#pragma once

namespace {
// Which kernel serves a call of oc_rollout_random (without OC_OPT_LANE_PAIR / OC_OPT_PREDICATE_INTERACT) or of oc_rollout_record /
// oc_rollout_record_ex (record): the one place that reads the batch and the call for it.  rollout4.hip's units launch what it returns.
struct RolloutChoice {
    int r4 = -1;                    // a k_rollout4 instance: its index in R4Instances (shared.hpp); -1: k_rollout5, r5
    oc_detail::R5Sel r5 = {};
    int head = 0, bulk = 0;         // bulk > 0: not one launch but three, of head, bulk (whole 8-step blocks) and the other steps
    const char* refusal = nullptr;  // the call is refused (OC_EINVAL) with this message
};
// What a choice needs to know of a call's arrays: which ones are there (oc_rollout_plan has no more than that to give)
struct RolloutArrays {
    bool state, rewards, flags, flags_aligned8;
    bool ev_masks, ev_counts;  // the event sink's per-step masks / per-episode counters
    bool rewards_aligned16 = true, ep_returns_aligned16 = true;
};
inline bool ev_on(const RolloutArrays& have) { return have.ev_masks || have.ev_counts; }

template <class P>
RolloutChoice pick() {
    static_assert(oc_detail::R4Instances::id<P>() >= 0, "not in R4Instances");
    return RolloutChoice{oc_detail::R4Instances::id<P>()};
}

RolloutChoice choose_launch(const OcBatch* b, int n_obj, uint32_t options, int64_t t0, int n_steps, const RolloutArrays& have,
                            bool record) {
    using namespace oc_detail;
    const bool uniform = b->n_layouts == 1, lds = b->n_layouts <= LDS_LAYOUT_MAX, small = b->max_pots >= 1 && b->max_pots <= 2;
    if (record && ev_on(have)) return uniform && small ? pick<R4RecEvUniform>() : small ? pick<R4RecEvSmall>() : pick<R4RecEvGeneral>();
    if (record) return uniform && small ? pick<R4RecUniform>() : small ? pick<R4RecSmall>() : pick<R4RecGeneral>();
    // Which family runs:
    //   joint   one two-player, one-pot, new-dynamics layout with at most 6 free cells (cramped_room): the JOINT move table.
    //           Launches of a few steps cannot amortise the ~10 us the workgroups spend building it: they move arithmetically
    //   mode2   two players everywhere, at most two pots and 64 cells, one set of shaping rewards: per-env terrain with
    //           the pose one step ahead on a floor mask (BASELINE configs[3] / [4], single layouts with more free cells)
    //   else    arithmetic movement (MODE 0): any table, either dynamics, event logging
    const bool two = (b->batch_flags & OC_BATCH_TWO_PLAYERS) != 0, events = ev_on(have), tiled8 = (options & OC_OPT_FLAGS_TILED8) != 0;
    const bool old_dyn = (b->batch_flags & OC_BATCH_NEW_DYNAMICS) == 0;  // some layout may use old dynamics
    const bool out = have.rewards && have.flags, noout = !have.rewards && !have.flags;  // (noout: a rollout run for its final states / returns / event counters)
    static const int forced_pipe = tuning_int("OC_ROLLOUT_PIPE", -1), forced_rounds = tuning_int("OC_DUO_ROUNDS", 0);
    static const bool no_mode2 = tuning_set("OC_ROLLOUT_NO_MODE2");
    // big batches (more than ~1.5 wavefronts per SIMD) hide latency with the other wavefronts: no one-step-ahead reads
    const bool pipe = forced_pipe >= 0 ? forced_pipe != 0 : b->n_envs <= simd_count() * 64 * 3 / 2;
    const bool joint = uniform && two && b->max_pots == 1 && b->max_free_cells >= 2 && b->max_free_cells <= 6u && out && !old_dyn &&
                       n_steps >= 8 && !events;
    const bool shaping_uniform = uniform || (b->batch_flags & OC_BATCH_UNIFORM_SHAPING) != 0;
    // what the per-env-terrain kernels serve: two players everywhere, at most two pots, 64 cells (k_rollout5: 128 with the table
    // in LDS), one set of shaping rewards, both output arrays (a one-pot joint-table layout is such a batch too)
    // (one dynamics flag for the whole table — OC_BATCH_UNIFORM_SHAPING —: old dynamics is served by k_rollout5, not by MODE 2)
    const int n_cells = b->width * b->height;
    // (an event log: per-episode counters only — no per-step masks —, table in LDS, <= 64 cells, and the counters must fit the
    //  CU's LDS beside the cell words: grids of up to 48 cells)
    const bool ev_ok = !events || (!have.ev_masks && lds && n_cells <= 64 && rollout5_lds_bytes(true, false, true, n_obj) <= (size_t)160 * 1024);
    const bool terrain_shape = two && small && shaping_uniform && (n_cells <= 64 || (n_cells <= 128 && lds)) && ev_ok && !no_mode2;
    const bool terrain_ok = terrain_shape && out;
    const bool mode2 = !joint && terrain_ok && !old_dyn && n_cells <= 64 && !events;
    // k_rollout5 (step_duo5.hpp): the step split between mover and interact wavefronts — whole workgroups of envs (every
    // wavefront meets every barrier) and whole 8-step blocks; a workgroup's 127-154 KB of LDS leave room for one per CU.
    // Bigger batches run these workgroups in ROUNDS, one per CU at a time — the next round's workgroups start as the first ones
    // finish their launch's steps — which keeps the one-workgroup-per-CU rate where the one-wavefront instances fall behind
    // (round 6, same box: the 5-layout mix at 65 536 / 131 072 / 262 144 envs 343 / 344 / 343 G env-steps/s; generated
    // terrains, table read through L2, 131 072 envs: 332 G in two rounds against 315 G with one wavefront per env group).
    // Beyond 8 rounds the one-wavefront instances win (round 5: 1 M cramped_room envs 356 G in 16 rounds against 384 G).
    const int64_t per_round = (simd_count() / 4) * BLOCK;
    const int64_t max_rounds = forced_rounds > 0 ? forced_rounds : 8;
    const bool duo_batch = (terrain_ok || (terrain_shape && noout)) && !(options & OC_OPT_ONE_WAVEFRONT) && b->n_envs % BLOCK == 0 &&
                           b->n_envs <= per_round * max_rounds;
    // A long launch that is not made of whole 8-step blocks (t0 or n_steps not a multiple of 8 — e.g. every call after one
    // rollout of 150 steps): the steps up to the next block boundary and the last < 8 steps go through the one-wavefront
    // instances, the whole blocks between them through the mover / interact kernel — three launches on the stream, the same
    // results (the state lives in d_state between them, every random draw is keyed by the global step)
    if (duo_batch && !tiled8 && (((t0 & 7) != 0) || ((n_steps & 7) != 0))) {
        const int head = (int)((8 - (t0 & 7)) & 7), bulk = head < n_steps ? ((n_steps - head) & ~7) : 0;
        if (bulk >= 256) return RolloutChoice{-1, {}, head, bulk};
    }
    RolloutChoice ch;
    if (duo_batch && n_steps >= 8 && (t0 & 7) == 0 && (n_steps & 7) == 0) {
        // (event counters: tables in LDS, at most 64 cells; 65..128 cells: tables in LDS only)
        const bool big = !events && n_cells > 64;
        // (one pot everywhere: the one-slot instances, where they exist — cooking starts without the rare branch)
        const bool one_pot = b->max_pots == 1 && !old_dyn && !big && !events;
        ch.r5 = R5Sel{events || big || lds, tiled8, old_dyn, big, events, noout, one_pot};
    } else if (events) {  // the general instances (arithmetic movement, either dynamics; mixed tables: the records are read through L2)
        ch = uniform && small ? pick<R4EvUniform>() : small ? pick<R4EvSmall>() : pick<R4EvGeneral>();
    } else if (joint) {  // (32-bit cell words and the faced cells read a step ahead where no two players can face the same cell)
        const bool noconf = (b->batch_flags & OC_BATCH_NO_SHARED_FACES) != 0;
        ch = !(pipe && n_cells <= 64 && noconf) ? pick<R4JointLean>() : tiled8 ? pick<R4JointTiled>() : pick<R4JointPipe>();
    } else if (mode2) {
        if (uniform) ch = b->max_pots == 1 && pipe ? pick<R4TerrainUniform1>() : pipe ? pick<R4TerrainUniform>() : pick<R4TerrainUniformLean>();
        else if (lds) ch = !pipe ? pick<R4TerrainLdsLean>() : tiled8 ? pick<R4TerrainLdsTiled>() : pick<R4TerrainLds>();
        else if (b->max_pots == 1)
            ch = pipe ? (tiled8 ? pick<R4TerrainL2OnePotTiled>() : pick<R4TerrainL2OnePot>())
                      : (tiled8 ? pick<R4TerrainL2OnePotLeanTiled>() : pick<R4TerrainL2OnePotLean>());
        else ch = pipe ? pick<R4TerrainL2>() : pick<R4TerrainL2Lean>();
    } else if (small && !old_dyn && out) {  // new dynamics, both output arrays: no per-step NULL / old-dynamics tests
        ch = uniform ? pick<R4ArithUniformOut>() : lds ? pick<R4ArithLdsOut>() : pick<R4ArithL2Out>();
    } else {  // (old dynamics / no output arrays: the records through L2 unless one layout; more than two pots: one general instance)
        ch = uniform && small ? pick<R4ArithUniform>() : small ? pick<R4ArithSmall>() : pick<R4ArithGeneral>();
    }
    const bool ft8 = ch.r4 < 0 ? ch.r5.ft8 : R4Instances::FT8[ch.r4];  // (OC_OPT_FLAGS_TILED8: served where the choice writes tiled flags)
    if (tiled8 && (!ft8 || b->n_envs >= ((int64_t)1 << 24)))
        ch.refusal = "oc_rollout_random: OC_OPT_FLAGS_TILED8 is served by the pipelined joint-table kernel (one two-player, "
                     "one-pot layout with <= 6 free cells and no shared faced cells, <= ~98 000 envs) and by the per-env-"
                     "terrain kernels of mixed tables (<= 32 layouts: <= ~98 000 envs; one-pot tables beyond that), or by the mover / interact kernel "
                     "(whole 256-env workgroups, <= 524 288 envs)";
    return ch;
}

// One launch of a rollout call: n_steps' steps [off, off + len), the options word its kernel receives, its kernel
struct RolloutPart {
    int off, len;
    uint32_t options;
    RolloutChoice ch;
};
// ... and the launches of the whole call, in stream order: one, or the head / bulk / tail split (see choose_launch; a part may be
// empty).  Head and tail run with OC_OPT_ONE_WAVEFRONT.
struct RolloutParts {
    int n = 0;
    RolloutPart part[3];
    const char* refusal = nullptr;
};
RolloutParts choose_rollout(const OcBatch* b, int n_obj, uint32_t options, int64_t t0, int n_steps, const RolloutArrays& have,
                            bool record) {
    RolloutParts r;
    const RolloutChoice whole = choose_launch(b, n_obj, options, t0, n_steps, have, record);
    if (whole.bulk == 0) {
        r.part[r.n++] = RolloutPart{0, n_steps, options, whole};
        r.refusal = whole.refusal;
        return r;
    }
    const int lens[3] = {whole.head, whole.bulk, n_steps - whole.head - whole.bulk};
    int off = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t opt = options | (k == 1 ? 0u : (uint32_t)OC_OPT_ONE_WAVEFRONT);
        r.part[r.n++] = RolloutPart{off, lens[k], opt, lens[k] > 0 ? choose_launch(b, n_obj, opt, t0 + off, lens[k], have, record) : RolloutChoice{}};
        if (!r.refusal) r.refusal = r.part[k].ch.refusal;
        off += lens[k];
    }
    return r;
}

// the rollout4.hip unit that compiles c's instance
int rollout_unit(const oc_detail::Rollout4Call& c) { return c.r4 < 0 ? 1 : oc_detail::R4Instances::PART[c.r4]; }

// launches the parts of c, the whole call, each through its unit.  Part k gets step t0 + off, the output rows from off on, and
// draws a restart at its step j from epoch + off + j, as the whole call would.
int launch_rollout(const RolloutParts& parts, const oc_detail::Rollout4Call& c, const char* who) {
    static void (*const unit[3])(const oc_detail::Rollout4Call&) = {oc_detail::launch_rollout<0>, oc_detail::launch_rollout<1>,
                                                                     oc_detail::launch_rollout<2>};
    for (int k = 0; k < parts.n; ++k) {
        const RolloutPart& pt = parts.part[k];
        if (pt.len == 0) continue;
        oc_detail::Rollout4Call ck = c;
        const int64_t rows = (int64_t)pt.off * c.b->n_envs;
        if (c.d_rewards) ck.d_rewards = c.d_rewards + rows * 4;
        if (c.d_flags) ck.d_flags = c.d_flags + rows;
        ck.t0 = c.t0 + pt.off;
        ck.n_steps = pt.len;
        ck.options = pt.options;
        if (c.sa.enabled) ck.sa.epoch = c.sa.epoch + (uint32_t)pt.off;
        ck.r4 = pt.ch.r4;
        ck.r5 = pt.ch.r5;
        unit[rollout_unit(ck)](ck);
        if (int rc = check_launch(who)) return rc;
    }
    return OC_OK;
}

// oc_rollout_record and oc_rollout_record_ex: the checks both make (every one before the first device call) and the launch.
// ex: re-draws and an event sink are accepted, the messages name oc_rollout_record_ex.
int rollout_record(bool ex, const OcBatch* b, void* d_state, const oc_detail::RecArgs& ra, float* d_rewards, uint8_t* d_flags,
                   float* d_ep_returns, int horizon, uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0, int n_steps,
                   const OcStartSpec* start, const OcEventSink* events, void* stream) {
    const char* const who = ex ? "oc_rollout_record_ex" : "oc_rollout_record";
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (!ra.actions && !ra.states && !ra.layout_ids)
        return refuse(who, ex ? "the record sink is NULL or all its arrays are" : "d_actions_out and d_states_out are both NULL");
    if (!aligned16(ra.states)) return refuse(who, ex ? "d_states must be 16-byte aligned" : "d_states_out must be 16-byte aligned");
    if (((uintptr_t)ra.actions & 1u) != 0) return refuse(who, ex ? "d_actions must be 2-byte aligned" : "d_actions_out must be 2-byte aligned");
    if (((uintptr_t)ra.layout_ids & 1u) != 0) return refuse(who, "d_layout_ids must be 2-byte aligned");
    if (options & ~(uint32_t)(OC_OPT_AUTO_RESET | OC_OPT_ONE_WAVEFRONT)) return refuse(who, "options other than OC_OPT_AUTO_RESET / OC_OPT_ONE_WAVEFRONT");
    if (!ex && start && start->regen_count) return refuse(who, "per-episode layout re-draws (start.regen_count > 0) are not recorded");
    if ((b->batch_flags & OC_BATCH_TWO_PLAYERS) == 0) return refuse(who, "needs a two-player table (OC_BATCH_TWO_PLAYERS)");
    StartArgs sa;
    if (!start_args(start, &sa, b)) return refuse(who, ex ? START_SPEC_RULE : "start.rnd_obj_prob_thresh must be in [0, 1]");
    if (start && start->env_offset != env_offset) return refuse(who, "start.env_offset differs from env_offset");
    if (!d_state) return refuse(who, "NULL state pointer");
    if (int rc = check_horizon(who, horizon)) return rc;
    if (n_steps < 0 || n_steps > (1 << 30)) return refuse(who, "n_steps must be in 0..2^30");
    if (int rc = check_quads(who, aligned16(d_rewards), aligned16(d_ep_returns))) return rc;
    if (b->n_envs == 0 || n_steps == 0) return OC_OK;
    const EvArgs ea = ev_args(events, nullptr);
    const RolloutArrays have = {true, d_rewards != nullptr, d_flags != nullptr, false, ea.events != nullptr, ea.counts != nullptr};
    const oc_detail::Rollout4Call c = {b, n_obj, d_state, d_rewards, d_flags, d_ep_returns, horizon, options & OC_OPT_AUTO_RESET, seed,
                                       env_offset, t0, n_steps, sa, ea, (hipStream_t)stream, -1, {}, ra};
    return launch_rollout(choose_rollout(b, n_obj, c.options, t0, n_steps, have, true), c, who);
}

// ---- oc_rollout_random: the call is planned first (every check, every choice; no launch, no device memory), then launched —
//      or, by oc_rollout_plan, described
struct RolloutPlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    enum Family { NOTHING, PAIR, PREDICATE, LUT } family = NOTHING;  // no envs or steps / k_rollout_pair / k_rollout / k_rollout4, k_rollout5
    int n_obj = 0;
    StartArgs sa = {};
    RolloutParts parts;  // LUT: its launches
};

RolloutPlan plan_rollout(const OcBatch* b, const RolloutArrays& have, int horizon, uint32_t options, int64_t env_offset, int64_t t0,
                         int n_steps, const OcStartSpec* start) {
    const char* const who = "oc_rollout_random";
    RolloutPlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
    if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
    if ((start || ev_on(have)) && (options & (OC_OPT_LANE_PAIR | OC_OPT_PREDICATE_INTERACT)))
        return refused(refuse(who, "drawn start states / event logging need the default kernel (k_rollout4)"));
    if (start && start->env_offset != env_offset) return refused(refuse(who, "start.env_offset differs from env_offset"));
    if (!have.state) return refused(refuse(who, "NULL state pointer"));
    if (int rc = check_horizon(who, horizon)) return refused(rc);
    if (n_steps < 0 || n_steps > (1 << 30)) return refused(refuse(who, "n_steps must be in 0..2^30"));
    if (int rc = check_quads(who, have.rewards_aligned16, have.ep_returns_aligned16)) return refused(rc);
    if (options & OC_OPT_FLAGS_TILED8) {  // the launch-shape half of the option's conditions (the batch half: choose_launch)
        if (!have.rewards || !have.flags || !have.flags_aligned8)
            return refused(refuse(who, "OC_OPT_FLAGS_TILED8 needs d_rewards and an 8-byte aligned d_flags"));
        if ((t0 & 7) != 0 || (n_steps & 7) != 0) return refused(refuse(who, "OC_OPT_FLAGS_TILED8 needs t0 and n_steps to be multiples of 8"));
        if (have.ev_masks || (options & (OC_OPT_LANE_PAIR | OC_OPT_PREDICATE_INTERACT)))
            return refused(refuse(who, "OC_OPT_FLAGS_TILED8 goes with the default kernel and no per-step event masks "
                                       "(per-episode counters: the mover / interact kernel writes it)"));
    }
    if (b->n_envs == 0 || n_steps == 0) return p;
    // Lane pairs (two lanes per env) halve the per-wavefront instruction stream at ~1.5x the total VALU work.  They
    // used to win for batches that leave SIMDs without a wavefront (<= 32 768 envs); with the table-driven step built
    // for ILP the lane-per-env kernel is faster at every batch size (us per batched step, lane vs pair, cramped_room:
    // 0.55 vs 0.73 at 4 096 envs, 0.57 vs 0.76 at 32 768), so pairs run only when OC_OPT_LANE_PAIR asks for them.
    const bool pair_ok = b->max_pots >= 1 && b->max_pots <= 2 && (b->batch_flags & OC_BATCH_TWO_PLAYERS) != 0;
    if (pair_ok && (options & OC_OPT_LANE_PAIR)) {
        p.family = RolloutPlan::PAIR;
    } else if (options & OC_OPT_PREDICATE_INTERACT) {
        p.family = RolloutPlan::PREDICATE;
    } else {  // k_rollout4 / k_rollout5 (their instances are compiled in rollout4.hip)
        p.family = RolloutPlan::LUT;
        p.parts = choose_rollout(b, p.n_obj, options, t0, n_steps, have, false);
        if (p.parts.refusal) return refused(fail(OC_EINVAL, p.parts.refusal));
    }
    return p;
}

// two lanes per env (k_rollout_pair)
void launch_rollout_pair(const oc_detail::Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = (size_t)c.n_obj * 8 * PAIR_ENVS * sizeof(uint32_t);
    const dim3 grid((unsigned)((b->n_envs + PAIR_ENVS - 1) / PAIR_ENVS)), block(BLOCK);
    const auto go = [&](auto uniform, auto lay_lds) {
        hipLaunchKernelGGL((k_rollout_pair<decltype(uniform)::value, decltype(lay_lds)::value>), grid, block, smem, c.stream, b->d_layouts,
                           b->n_layouts, b->d_layout_id, (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns,
                           b->n_envs, b->width, c.n_obj, c.horizon, c.options, (uint32_t)c.seed, (uint32_t)(c.seed >> 32),
                           c.env_offset, c.t0, c.n_steps);
    };
    if (b->n_layouts == 1) go(std::true_type(), std::true_type());
    else if (b->n_layouts <= LDS_LAYOUT_MAX) go(std::false_type(), std::true_type());
    else go(std::false_type(), std::false_type());
}

// the predicate-network interact (k_rollout)
void launch_rollout_predicate(const oc_detail::Rollout4Call& c) {
    const OcBatch* b = c.b;
    const size_t smem = (size_t)c.n_obj * 8 * BLOCK * sizeof(uint32_t);
    const dim3 grid(grid_for(b->n_envs)), block(BLOCK);
    const auto go = [&](auto kernel) {
        if (!want_lds(kernel, smem)) return;
        hipLaunchKernelGGL(kernel, grid, block, smem, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id, (uint4*)c.d_state, (float4*)c.d_rewards,
                           c.d_flags, (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon, c.options, (uint32_t)c.seed,
                           (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps);
    };
    if (b->n_layouts == 1) { if (b->max_pots >= 1 && b->max_pots <= 2) go(k_rollout<true, 2, true>); else go(k_rollout<true, 8, true>); }
    else go(k_rollout<false, 8, false>);
}
}  // namespace

extern "C" {

int oc_rollout_random(const OcBatch* b, void* d_state, float* d_rewards, uint8_t* d_flags, float* d_ep_returns,
                      int horizon, uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0, int n_steps,
                      const OcStartSpec* start, const OcEventSink* events, void* stream) {
    const EvArgs ea = ev_args(events, nullptr);
    const RolloutArrays have = {d_state != nullptr, d_rewards != nullptr, d_flags != nullptr, ((uintptr_t)d_flags & 7u) == 0,
                                ea.events != nullptr, ea.counts != nullptr, aligned16(d_rewards), aligned16(d_ep_returns)};
    const RolloutPlan p = plan_rollout(b, have, horizon, options, env_offset, t0, n_steps, start);
    if (p.rc != OC_OK || p.family == RolloutPlan::NOTHING) return p.rc;
    const oc_detail::Rollout4Call c = {b, p.n_obj, d_state, d_rewards, d_flags, d_ep_returns, horizon, options, seed,
                                       env_offset, t0, n_steps, p.sa, ea, (hipStream_t)stream, -1, {}};
    if (p.family == RolloutPlan::LUT) return launch_rollout(p.parts, c, "oc_rollout_random");
    if (p.family == RolloutPlan::PAIR) launch_rollout_pair(c);
    else launch_rollout_predicate(c);
    return check_launch("oc_rollout_random");
}

int oc_rollout_record(const OcBatch* b, void* d_state, uint8_t* d_actions_out, void* d_states_out, float* d_rewards,
                      uint8_t* d_flags, float* d_ep_returns, int horizon, uint32_t options, uint64_t seed, int64_t env_offset,
                      int64_t t0, int n_steps, const OcStartSpec* start, void* stream) {
    return rollout_record(false, b, d_state, oc_detail::RecArgs{d_actions_out, d_states_out, nullptr}, d_rewards, d_flags,
                          d_ep_returns, horizon, options, seed, env_offset, t0, n_steps, start, nullptr, stream);
}

int oc_rollout_record_ex(const OcBatch* b, void* d_state, const OcRecordSink* rec, float* d_rewards, uint8_t* d_flags,
                         float* d_ep_returns, int horizon, uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0,
                         int n_steps, const OcStartSpec* start, const OcEventSink* events, void* stream) {
    if (!rec) return fail(OC_EINVAL, "oc_rollout_record_ex: the record sink is NULL or all its arrays are");
    return rollout_record(true, b, d_state, oc_detail::RecArgs{rec->d_actions, rec->d_states, rec->d_layout_ids}, d_rewards,
                          d_flags, d_ep_returns, horizon, options, seed, env_offset, t0, n_steps, start, events, stream);
}

int oc_rollout_plan(const OcBatch* b, int horizon, uint32_t options, int64_t t0, int n_steps, int with_outputs, int event_sink,
                    const OcStartSpec* start, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_rollout_plan: no output buffer");
    out[0] = 0;
    // the call oc_rollout_random would get: a state, both output arrays (8-byte aligned) or none, the named kind of event sink
    const RolloutArrays have = {true, with_outputs != 0, with_outputs != 0, true, event_sink == 2, event_sink >= 1};
    const RolloutPlan p = plan_rollout(b, have, horizon, options, start ? start->env_offset : 0, t0, n_steps, start);
    if (p.rc != OC_OK) return p.rc;
    char buf[256] = "nothing to launch (no envs or no steps)";
    if (p.family == RolloutPlan::PAIR) snprintf(buf, sizeof(buf), "k_rollout_pair (OC_OPT_LANE_PAIR: two lanes per env)");
    if (p.family == RolloutPlan::PREDICATE) snprintf(buf, sizeof(buf), "k_rollout (OC_OPT_PREDICATE_INTERACT: the predicate-network interact)");
    if (p.family == RolloutPlan::LUT) {  // its unit names the instance; of a split call, that of the whole blocks
        static void (*const unit[3])(const oc_detail::Rollout4Call&, char*, size_t) = {
            oc_detail::describe_rollout<0>, oc_detail::describe_rollout<1>, oc_detail::describe_rollout<2>};
        const bool split = p.parts.n == 3;
        const RolloutChoice& ch = p.parts.part[split ? 1 : 0].ch;
        oc_detail::Rollout4Call c = {};
        c.b = b; c.n_obj = p.n_obj; c.r4 = ch.r4; c.r5 = ch.r5;
        unit[rollout_unit(c)](c, buf, sizeof(buf));
        const size_t used = strlen(buf);
        if (split)
            snprintf(buf + used, sizeof(buf) - used, "; %d + %d steps around the whole blocks: one-wavefront launches", p.parts.part[0].len,
                     p.parts.part[2].len);
    }
    snprintf(out, out_size, "%s", buf);
    return OC_OK;
}

}  // extern "C"
