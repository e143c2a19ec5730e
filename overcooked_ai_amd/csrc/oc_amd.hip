// oc_amd.hip — MI355X (gfx950 / CDNA4) kernels and C-ABI for the batched Overcooked hot path.
//
// Layout of this translation unit (reference = HumanCompatibleAI/overcooked_ai, "mdp.py" =
// src/overcooked_ai_py/mdp/overcooked_mdp.py); the kernels live in the headers included below:
//   common.hpp          constants, OcLayout accessor, Philox4x32-10, layout staging
//   step_predicate.hpp  get_state_transition, mdp.py:1375 (interacts 1432 -> movement 1644 -> env effects 1691) with
//                       the predicate-network interact that also emits event_infos: k_step, k_rollout
//   step_table.hpp      the same transition with the table-driven interact: k_step3 (oc_step_many, grids above 64 cells)
//   step_one.hpp        one transition per launch on the wire format itself: k_step1 (oc_step)
//   step_lut4.hpp       the rollout path: key-byte cell words, 16-byte interact LUT, joint move table: k_rollout4 — compiled in
//                       rollout4.hip (three units, see shared.hpp), chosen here (choose_rollout), launched through oc_detail::launch_rollout
//   rollout_pair.hpp    two lanes per env: k_rollout_pair
//   reset.hpp           get_standard_start_state mdp.py:1297, get_random_start_state_fn 1307: k_reset, k_reset_random
//   encode.hpp          lossless_state_encoding mdp.py:2385-2561: k_encode, k_encode_uniform
//   rollout_encode.hpp  K transitions with the observation of every step in one launch: k_rollout_encode
//   featurize.hpp       featurize_state mdp.py:2579-2898: k_featurize
//   rollout_featurize.hpp  K transitions with the featurize_state observation of every step in one launch: k_rollout_featurize
//   potential.hpp       potential_function mdp.py:2920-3238: k_potential, k_potential2
//   shaping.hpp         OvercookedMultiAgent.step reward, rllib.py:306-329: k_shape_rewards
//   train_obs.hpp       the training step with its observation in one kernel: k_train_step_obs
//   train_feat.hpp      the training step with the featurize_state observation in one kernel: k_train_step_feat
//   sample.hpp          both players' actions drawn from policy logits: sample_env, k_sample_actions
//   train_dispatch.hpp  host only: the training-step family — one call record, one plan, one launch path; oc_multi_agent_step,
//                       oc_multi_agent_step_featurize, oc_multi_agent_step_sample, their *_plan entry points and oc_sample_actions
//   stores_only.hpp     the output stores of a rollout and nothing else: k_output_stores_only (oc_output_stores_only)
//   observation_plan.hpp  host only: the observation geometry and the plans of oc_encode_lossless / oc_rollout_encode / oc_rollout_featurize
//   this file           launch dispatch and the extern "C" entry points declared in include/oc_amd.h: oc_rollout_random,
//                       oc_multi_agent_step, oc_multi_agent_step_featurize, oc_encode_lossless, oc_rollout_encode, oc_step, oc_step_many and oc_step_server_open plan
//                       a call (checks, then choices; no launch, no device address), then launch from the plan; oc_rollout_plan,
//                       oc_multi_agent_plan, oc_multi_agent_step_featurize_plan, oc_observation_plan, oc_step_plan, oc_potential_plan and oc_featurize_plan put the plans into words
//
// Execution model: one lane per env, 64-lane wavefronts, 256-lane workgroups.  This is integer /
// indexing work (no MFMA).  Per-env state arrives as coalesced 16-byte planes (1 KiB per wavefront
// per plane), the object bytes of the grid are staged in LDS in [dword][lane] order — bank =
// lane % 32 whatever cell a lane touches, so divergent per-lane cell indices never conflict — and
// the compiled layout table (terrain tile, pot cells, recipe LUTs) is staged in LDS once per
// workgroup.  See DESIGN.md for the data layout and the roofline of each kernel.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "shared.hpp"

namespace oc_detail {
__thread char g_err[256] = "";
__thread bool g_lds_refused = false;
}  // namespace oc_detail

namespace {

#include "common.hpp"
#include "host_util.hpp"
#include "reset.hpp"
#include "step_predicate.hpp"
#include "step_table.hpp"
#include "step_one.hpp"
#include "mailbox.hpp"
#include "step_server.hpp"
#include "rollout_pair.hpp"
#include "encode.hpp"
#include "rollout_encode.hpp"
#include "featurize.hpp"
#include "rollout_featurize.hpp"
#include "potential.hpp"
#include "sample.hpp"
#include "shaping.hpp"
#include "train_obs.hpp"
#include "train_feat.hpp"
#include "stores_only.hpp"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int check_batch(const OcBatch* b, int* n_obj) {
    if (!b) return fail(OC_EINVAL, "batch is NULL");
    if (!b->d_layouts) return fail(OC_EINVAL, "batch.d_layouts is NULL");
    if (b->n_envs < 0) return fail(OC_EINVAL, "batch.n_envs < 0");
    if (b->n_layouts < 1 || b->n_layouts > 65536) return fail(OC_EINVAL, "batch.n_layouts out of range (1..65536)");
    if (b->n_layouts > 1 && !b->d_layout_id) return fail(OC_EINVAL, "d_layout_id required when n_layouts > 1");
    if (b->width < 3 || b->height < 3 || b->width * b->height > OC_MAX_CELLS)
        return fail(OC_EINVAL, "grid shape out of range (3x3 .. 128 cells)");
    *n_obj = (b->width * b->height + 15) / 16;
    return OC_OK;
}

// The library reads no environment variable unless it is built with -DOC_AMD_TUNING (the knobs of the measurement scripts under
// tools/: OC_ENC_LDS, OC_STEP_NO_LEAN, OC_ROLLOUT_PIPE, OC_ROLLOUT_NO_MODE2, OC_ROLLOUT_ENCODE_WAVES, ...): a knob's value, or
// whether it is set at all.  Every other build: the default, a constant.
#ifdef OC_AMD_TUNING
inline int tuning_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline bool tuning_set(const char* name) { return getenv(name) != nullptr; }
#else
constexpr int tuning_int(const char*, int dflt) { return dflt; }
constexpr bool tuning_set(const char*) { return false; }
#endif

// LDS bytes one encode workgroup may fill with output (40 KiB = 3 workgroups per CU)
inline int enc_lds_budget() {
    static const int v = tuning_int("OC_ENC_LDS", 40 * 1024);
    return v;
}
// ... for the persistent single-layout kernel: ~19 envs per group is the measured sweet spot (65 536 cramped_room envs,
// u8: 18.1 us with a 20 KB image, 20.6 us with 40 KB, 25.2 us with 12 KB; 9x5 grids: 40 KB = 17 envs is best)
inline size_t enc_uniform_budget(size_t env_bytes) {
    static const bool forced = tuning_set("OC_ENC_LDS");
    const size_t cap = (size_t)enc_lds_budget();
    if (forced) return cap;
    const size_t want = 19 * env_bytes;
    return want < cap ? want : cap;
}

// the keys every draw of a start spec is made with (seed, epoch, env offset), as a kernel argument
void start_keys(const OcStartSpec* sp, StartArgs* sa) {
    memset(sa, 0, sizeof(*sa));
    sa->enabled = 1;
    sa->seed_lo = (uint32_t)sp->seed;
    sa->seed_hi = (uint32_t)(sp->seed >> 32);
    sa->epoch = sp->epoch;
    sa->env_offset = sp->env_offset;
}

// OcStartSpec -> kernel argument; false when the spec is malformed
bool start_args(const OcStartSpec* sp, StartArgs* sa, const OcBatch* b = nullptr) {
    memset(sa, 0, sizeof(*sa));
    if (!sp) return true;
    if (!(sp->rnd_obj_prob_thresh >= 0.0 && sp->rnd_obj_prob_thresh <= 1.0)) return false;
    start_keys(sp, sa);
    if (sp->regen_count) {  // per-episode layout re-draw: the ids must exist, be writable and in range
        if (!b || (uint64_t)sp->regen_first + sp->regen_count > (uint64_t)(b ? b->n_layouts : 0)) return false;
        if (b->n_layouts > 1) {
            if (!b->d_layout_id) return false;
            sa->regen_first = sp->regen_first;
            sa->regen_count = sp->regen_count;
            sa->layout_ids = const_cast<uint16_t*>(b->d_layout_id);
        }  // (one layout: nothing to draw)
    }
    sa->thresh = (uint64_t)(sp->rnd_obj_prob_thresh * 4294967296.0);  // floor(thresh * 2^32); 1.0 -> 2^32: always
    sa->random_start_pos = sp->random_start_pos != 0;
    return true;
}

// ---- checks that many entry points make, each said once; who: the entry point's name, in front of the message
int refuse(const char* who, const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail(OC_EINVAL, msg);
}
int check_horizon(const char* who, int horizon) {
    return horizon < 1 || horizon > 65535 ? refuse(who, "horizon must be in 1..65535") : OC_OK;
}
const char* const START_SPEC_RULE = "start.rnd_obj_prob_thresh must be in [0, 1] and its regen range within the table";
int check_start(const char* who, const OcStartSpec* sp, StartArgs* sa, const OcBatch* b) {
    return start_args(sp, sa, b) ? OC_OK : refuse(who, START_SPEC_RULE);
}
inline bool obs_dtype_ok(int obs_dtype) { return obs_dtype == OC_OBS_U8 || obs_dtype == OC_OBS_F32; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// d_rewards and d_ep_returns (either may be NULL where the entry point allows it): every kernel writes them as float4 rows
int check_quads(const char* who, bool rewards_aligned16, bool ep_returns_aligned16) {
    if (!rewards_aligned16) return refuse(who, "d_rewards must be 16-byte aligned");
    return ep_returns_aligned16 ? OC_OK : refuse(who, "d_ep_returns must be 16-byte aligned");
}
int check_obs(const char* who, int obs_dtype, bool obs_aligned16) {
    if (!obs_dtype_ok(obs_dtype)) return refuse(who, "bad obs_dtype");
    return obs_aligned16 ? OC_OK : refuse(who, "d_obs must be 16-byte aligned");
}

// tuning builds: OC_STEP_NO_LEAN sends every single step to the general kernels (k_step3, k_train_step)
inline bool step_no_lean() {
    static const bool v = tuning_set("OC_STEP_NO_LEAN");
    return v;
}

#include "observation_plan.hpp"

EvArgs ev_args(const OcEventSink* sink, uint64_t* d_events, uint32_t clear_on_done = 0) {
    EvArgs ea = {d_events, nullptr, nullptr, clear_on_done};
    if (sink) {
        if (sink->d_events) ea.events = sink->d_events;
        ea.counts = sink->d_counts;
        ea.counts_done = sink->d_counts_done;
    }
    return ea;
}
inline bool ev_on(const EvArgs& ea) { return ea.events || ea.counts; }

#define DISPATCH_NOBJ(NOBJ_VALUE, ...)                                  \
    switch (NOBJ_VALUE) {                                               \
        case 1: { constexpr int NOBJ = 1; __VA_ARGS__; } break;         \
        case 2: { constexpr int NOBJ = 2; __VA_ARGS__; } break;         \
        case 3: { constexpr int NOBJ = 3; __VA_ARGS__; } break;         \
        case 4: { constexpr int NOBJ = 4; __VA_ARGS__; } break;         \
        case 5: { constexpr int NOBJ = 5; __VA_ARGS__; } break;         \
        case 6: { constexpr int NOBJ = 6; __VA_ARGS__; } break;         \
        case 7: { constexpr int NOBJ = 7; __VA_ARGS__; } break;         \
        default: { constexpr int NOBJ = 8; __VA_ARGS__; } break;        \
    }

// ---- the caller-actions family (oc_step, oc_step_many, oc_step_server_*): the call is planned first (every check, every choice; no
//      launch, no device address), then launched from the plan — or, by oc_step_plan, described
// kernel variant selection: UNIFORM (one layout for the whole batch -> layout constants in SGPRs),
// MAXP (pot slots kept in registers: 1 for single-pot batches of one layout such as cramped_room, 2 covers every
// canonical layout, 8 is the format's maximum),
// LAY_LDS (layout table staged in LDS vs read from HBM/L2 for tables of more than 32 layouts),
// FAST (k_step3: two players everywhere and at most 64 cells, the 64-bit floor mask), EVENTS (an event sink is there)
struct StepChoice {
    enum Family { NOTHING, STEP1, STEP3, PREDICATE, SERVER } family = NOTHING;  // no envs or steps / k_step1 / k_step3 / k_step / k_step_server
    bool uniform = false;
    int maxp = 0;
    bool lay_lds = false, fast = false, events = false;
    unsigned grid = 0;
    size_t lds = 0;  // dynamic LDS bytes of the launch
};
enum StepEntry { ENTRY_STEP = 0, ENTRY_STEP_MANY = 1, ENTRY_SERVER = 2 };

// Which kernel instance serves a call of the family: the one place that reads the batch and the call for it.  launch_step_from and
// sv_launch launch what it returns.
StepChoice choose_step(const OcBatch* b, int n_obj, uint32_t options, int n_steps, bool events, bool server) {
    const bool uniform = b->n_layouts == 1;
    const bool lds = b->n_layouts <= LDS_LAYOUT_MAX;
    const bool small = b->max_pots >= 1 && b->max_pots <= 2;
    const bool fast = (b->batch_flags & OC_BATCH_TWO_PLAYERS) != 0 && b->width * b->height <= 64;
    StepChoice c;
    c.grid = grid_for(b->n_envs);
    c.lds = (size_t)n_obj * 8 * BLOCK * sizeof(uint32_t);  // the cell words of a workgroup's envs (k_step1: see below)
    c.events = events && !server;
    const auto as = [&c](StepChoice::Family f, bool u, int mp, bool ll, bool fa = false) {
        c.family = f; c.uniform = u; c.maxp = mp; c.lay_lds = ll; c.fast = fa;
        return c;
    };
    if (server) {  // the resident step: no event logging
        if (uniform && small) return as(StepChoice::SERVER, true, 2, true);
        if (lds && small) return as(StepChoice::SERVER, false, 2, true);
        return as(StepChoice::SERVER, false, 8, false);
    }
    if (options & OC_OPT_PREDICATE_INTERACT) {  // the predicate network is the independent second implementation: three instances cover every table
        if (uniform) return small ? as(StepChoice::PREDICATE, true, 2, true) : as(StepChoice::PREDICATE, true, 8, true);
        return as(StepChoice::PREDICATE, false, 8, false);
    }
    // one step on a grid of at most 64 cells: the transition on the wire format itself (step_one.hpp) — in place or out of place,
    // with or without event logging
    if (n_steps == 1 && n_obj <= STEP1_MAX_PLANES && !step_no_lean()) {
        c.lds = (size_t)n_obj * BLOCK * sizeof(uint4);  // the object planes as they are, one 16-byte row per lane and plane
        if (uniform) return b->max_pots == 1 ? as(StepChoice::STEP1, true, 1, true) : small ? as(StepChoice::STEP1, true, 2, true) : as(StepChoice::STEP1, true, 8, true);
        if (lds && small) return as(StepChoice::STEP1, false, 2, true);
        if (small) return as(StepChoice::STEP1, false, 2, false);
        return as(StepChoice::STEP1, false, 8, false);  // (more than two pots on a mixed table: the general instance reads the table through L2)
    }
    // what is left for k_step3: oc_step_many's K transitions per launch and grids above 64 cells
    if (uniform && fast && b->max_pots == 1) return as(StepChoice::STEP3, true, 1, true, true);
    if (uniform && fast && small) return as(StepChoice::STEP3, true, 2, true, true);
    if (lds && small) return as(StepChoice::STEP3, false, 2, true, false);
    return as(StepChoice::STEP3, false, 8, false, false);
}

// an instance's template arguments as one switch label
#define STEP_KEY(U, MP, LL, F) (((U) ? 1 : 0) | ((LL) ? 2 : 0) | ((F) ? 4 : 0) | ((MP) << 3))
inline int step_key(const StepChoice& c) { return STEP_KEY(c.uniform, c.maxp, c.lay_lds, c.fast); }
const char* const NO_STEP_INSTANCE = "no kernel instance for the planned step (internal error)";

// launch what choose_step chose (EVENTS: the event-logging instances)
template <bool EVENTS>
int launch_step_as(const StepChoice& ch, const OcBatch* b, int n_obj, const void* d_state_in, void* d_state_out, const uint8_t* d_actions,
                   float* d_rewards, uint8_t* d_flags, float* d_ep_returns, int horizon, uint32_t options, hipStream_t s,
                   const StartArgs& sa, const EvArgs& ea, int n_steps) {
    const size_t smem = ch.lds;
    const dim3 grid(ch.grid), block(BLOCK);
    if (ch.family == StepChoice::STEP1) {
#define GO1(U, MP, LL)                                                                                                \
    case STEP_KEY(U, MP, LL, false):                                                                                  \
        hipLaunchKernelGGL((k_step1<U, MP, LL, EVENTS>), grid, block, smem, s, b->d_layouts, b->n_layouts, b->d_layout_id, \
                           (uint4*)d_state_in, (uint4*)d_state_out, d_actions, (float4*)d_rewards, d_flags,           \
                           (float4*)d_ep_returns, b->n_envs, b->width, n_obj, horizon, options, sa, ea);              \
        return OC_OK
        switch (step_key(ch)) {
            GO1(true, 1, true);
            GO1(true, 2, true);
            GO1(true, 8, true);
            GO1(false, 2, true);
            GO1(false, 2, false);
            GO1(false, 8, false);
        }
#undef GO1
    } else if (ch.family == StepChoice::STEP3) {
#define GO3(U, MP, LL, F)                                                                                            \
    case STEP_KEY(U, MP, LL, F):                                                                                     \
        if (!want_lds(k_step3<U, MP, LL, F, EVENTS>, smem)) return OC_OK;                                            \
        hipLaunchKernelGGL((k_step3<U, MP, LL, F, EVENTS>), grid, block, smem, s, b->d_layouts, b->n_layouts, b->d_layout_id,   \
                           (const uint4*)d_state_in, (uint4*)d_state_out, d_actions, (float4*)d_rewards, d_flags,    \
                           (float4*)d_ep_returns, b->n_envs, b->width, n_obj, horizon, options, n_steps, sa, ea);    \
        return OC_OK
        switch (step_key(ch)) {
            GO3(true, 1, true, true);
            GO3(true, 2, true, true);
            GO3(false, 2, true, false);
            GO3(false, 8, false, false);
        }
#undef GO3
    } else if (ch.family == StepChoice::PREDICATE) {
#define GO(U, MP, LL)                                                                                       \
    case STEP_KEY(U, MP, LL, false):                                                                        \
        if (!want_lds(k_step<U, MP, LL, EVENTS>, smem)) return OC_OK;                                       \
        hipLaunchKernelGGL((k_step<U, MP, LL, EVENTS>), grid, block, smem, s, b->d_layouts, b->n_layouts,   \
                           b->d_layout_id, (const uint4*)d_state_in, (uint4*)d_state_out, d_actions,        \
                           (float4*)d_rewards, d_flags, (float4*)d_ep_returns, ea.events, b->n_envs,        \
                           b->width, n_obj, horizon, options);                                              \
        return OC_OK
        switch (step_key(ch)) {
            GO(true, 2, true);
            GO(true, 8, true);
            GO(false, 8, false);
        }
#undef GO
    }
    return fail(OC_ELAUNCH, NO_STEP_INSTANCE);  // (a missing kernel is an error, never another kernel)
}
// (a refused LDS request returns OC_OK above: check_launch reports it, as it reports a failed launch)
int launch_step_from(const StepChoice& ch, const OcBatch* b, int n_obj, const void* d_state_in, void* d_state_out, const uint8_t* d_actions,
                     float* d_rewards, uint8_t* d_flags, float* d_ep_returns, int horizon, uint32_t options, hipStream_t s,
                     const StartArgs& sa, const EvArgs& ea, int n_steps) {
    const auto go = ch.events ? launch_step_as<true> : launch_step_as<false>;
    return go(ch, b, n_obj, d_state_in, d_state_out, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options, s, sa, ea, n_steps);
}
// one step of a batch that another entry point has checked (the training step's sequence)
void launch_step(const OcBatch* b, int n_obj, const void* d_state_in, void* d_state_out, const uint8_t* d_actions,
                 float* d_rewards, uint8_t* d_flags, float* d_ep_returns, int horizon, uint32_t options, hipStream_t s,
                 const StartArgs& sa, const EvArgs& ea) {
    (void)launch_step_from(choose_step(b, n_obj, options, 1, ev_on(ea), false), b, n_obj, d_state_in, d_state_out, d_actions, d_rewards,
                           d_flags, d_ep_returns, horizon, options, s, sa, ea, 1);
}

// What a plan needs to know of a call's arrays: which ones are there, never where (oc_step_plan has no more than that to give)
struct StepArrays {
    bool required;             // the state(s), actions, rewards and flags of the entry point (the server: the state)
    bool ev_masks, ev_counts;  // per-step event masks (oc_step's d_events or the sink's) / per-episode counters
    bool rewards_aligned16 = true, ep_returns_aligned16 = true;  // (the server: d_ep_returns; its rewards come with oc_step_server_play)
};
struct StepPlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    int n_obj = 0;
    StartArgs sa = {};
    StepChoice ch;                  // NOTHING: no envs or no steps (`nothing` says which)
    bool step_by_step = false;      // oc_step_many with OC_OPT_PREDICATE_INTERACT: n_steps calls of oc_step, each ch
    const char* nothing = nullptr;
};
const char* const STEP_ENTRY_NAME[3] = {"oc_step", "oc_step_many", "oc_step_server_open"};

// every check of the entry point, in its order and under its name, then the choice
StepPlan plan_step(const OcBatch* b, int entry, const StepArrays& have, int horizon, uint32_t options, int n_steps, const OcStartSpec* start) {
    const char* const who = STEP_ENTRY_NAME[entry];
    StepPlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    const bool predicate = (options & OC_OPT_PREDICATE_INTERACT) != 0, ev = have.ev_masks || have.ev_counts;
    if (entry == ENTRY_STEP_MANY) {
        if (n_steps < 0) return refused(refuse(who, "n_steps < 0"));
        if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
        if ((start || ev) && predicate) return refused(refuse(who, "drawn start states / event logging need the table-driven kernel"));
        if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
    } else {
        if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
        if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
    }
    if (entry == ENTRY_STEP && predicate) {
        if (start) return refused(refuse(who, "drawn start states need the table-driven kernel (no PREDICATE_INTERACT)"));
        if (have.ev_counts) return refused(refuse(who, "event counters need the table-driven kernel (no PREDICATE_INTERACT)"));
    }
    if (!have.required) return refused(refuse(who, entry == ENTRY_SERVER ? "NULL state pointer" : "NULL state/actions/rewards/flags pointer"));
    if (int rc = check_horizon(who, horizon)) return refused(rc);
    if (int rc = check_quads(who, have.rewards_aligned16, have.ep_returns_aligned16)) return refused(rc);
    if (entry == ENTRY_SERVER) {
        if (options & ~(uint32_t)OC_OPT_AUTO_RESET) return refused(refuse(who, "the only option is OC_OPT_AUTO_RESET"));
        if (b->n_envs < 1) return refused(refuse(who, "no envs"));
        p.ch = choose_step(b, p.n_obj, options, 1, false, true);
        return p;
    }
    if (b->n_envs == 0) { p.nothing = "no envs"; return p; }
    if (entry == ENTRY_STEP_MANY && n_steps == 0) { p.nothing = "no steps"; return p; }
    p.step_by_step = entry == ENTRY_STEP_MANY && predicate;
    p.ch = choose_step(b, p.n_obj, options, entry == ENTRY_STEP || p.step_by_step ? 1 : n_steps, ev, false);
    return p;
}

// A choice in words (oc_step_plan): up to and including '>' the kernel instance, as tests match it
void describe_step(const StepChoice& c, char* out, size_t out_size) {
    const char* const tf[2] = {"false", "true"};
    char name[160];
    if (c.family == StepChoice::STEP3)
        snprintf(name, sizeof(name), "k_step3<UNIFORM=%s, MAXP=%d, LAY_LDS=%s, FAST=%s, EVENTS=%s>", tf[c.uniform], c.maxp, tf[c.lay_lds],
                 tf[c.fast], tf[c.events]);
    else if (c.family == StepChoice::SERVER)
        snprintf(name, sizeof(name), "k_step_server<UNIFORM=%s, MAXP=%d, LAY_LDS=%s>", tf[c.uniform], c.maxp, tf[c.lay_lds]);
    else
        snprintf(name, sizeof(name), "%s<UNIFORM=%s, MAXP=%d, LAY_LDS=%s, EVENTS=%s>", c.family == StepChoice::STEP1 ? "k_step1" : "k_step",
                 tf[c.uniform], c.maxp, tf[c.lay_lds], tf[c.events]);
    snprintf(out, out_size, "%s grid=%u, %zu B LDS", name, c.grid, c.lds);
}

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
#define GO(U, MP, LL)                                                                                       \
    do {                                                                                                    \
        if (!want_lds(k_rollout<U, MP, LL>, smem)) break;                                                   \
        hipLaunchKernelGGL((k_rollout<U, MP, LL>), grid, block, smem, c.stream, b->d_layouts, b->n_layouts, \
                           b->d_layout_id, (uint4*)c.d_state, (float4*)c.d_rewards, c.d_flags,              \
                           (float4*)c.d_ep_returns, b->n_envs, b->width, c.n_obj, c.horizon, c.options,     \
                           (uint32_t)c.seed, (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps);      \
    } while (0)
    if (b->n_layouts == 1) { if (b->max_pots >= 1 && b->max_pots <= 2) GO(true, 2, true); else GO(true, 8, true); }
    else GO(false, 8, false);
#undef GO
}

// ---- oc_featurize / oc_potential: plan a call (the argument checks, the kernel instance, the grid, the dynamic LDS bytes; no
//      launch, no device address), then launch from the plan — or, by oc_featurize_plan / oc_potential_plan, describe it
struct FeaturizePlan {
    int rc = OC_OK;
    bool nothing = false;  // no envs
    bool lay_lds = false;  // the layout table fits LDS: k_featurize<true>
    int n_planes = 0;
    unsigned grid = 0;
    size_t smem = 0;
};

// have: every required pointer is there; aligned: d_features is 16-byte aligned
FeaturizePlan plan_featurize(const OcBatch* b, bool have, bool aligned, int num_pots) {
    FeaturizePlan p;
    int n_obj = 0;
    if ((p.rc = check_batch(b, &n_obj)) != OC_OK) return p;
    if (!have) { p.rc = fail(OC_EINVAL, "oc_featurize: NULL pointer"); return p; }
    if (num_pots < 0 || num_pots > 4) { p.rc = fail(OC_EINVAL, "oc_featurize: num_pots must be in 0..4"); return p; }
    if (!(b->batch_flags & OC_BATCH_TWO_PLAYERS)) { p.rc = fail(OC_EINVAL, "oc_featurize: needs 2-player layouts"); return p; }
    if (!aligned) { p.rc = fail(OC_EINVAL, "oc_featurize: d_features must be 16-byte aligned"); return p; }
    if (b->n_envs == 0) { p.nothing = true; return p; }
    p.n_planes = 1 + n_obj;
    const int total = 2 * (num_pots * 10 + 26) + 4;
    p.smem = (size_t)FEAT_ENVS * p.n_planes * 16 + (size_t)FEAT_ENVS * 2 * (total + 2) * sizeof(int16_t);
    p.grid = (unsigned)((b->n_envs + FEAT_ENVS - 1) / FEAT_ENVS);
    p.lay_lds = b->n_layouts <= LDS_LAYOUT_MAX;
    return p;
}

template <bool LAY_LDS>
void launch_featurize(const FeaturizePlan& p, const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off,
                      const void* d_state, float* d_features, int num_pots, hipStream_t s) {
    if (!want_lds(k_featurize<LAY_LDS>, p.smem)) return;
    hipLaunchKernelGGL((k_featurize<LAY_LDS>), dim3(p.grid), dim3(BLOCK), p.smem, s, b->d_layouts, b->n_layouts, b->d_layout_id,
                       d_plan_blob, d_plan_off, (const uint4*)d_state, d_features, b->n_envs, b->width, b->height, p.n_planes, num_pots);
}

struct PotentialPlan {
    int rc = OC_OK;
    bool nothing = false;   // no envs
    bool two_pots = false;  // the table's hint promises one or two pots everywhere: k_potential2
    unsigned grid = 0;
};

// have: every required pointer is there; aligned: d_phi_tables and d_phi are 8-byte aligned
PotentialPlan plan_potential(const OcBatch* b, bool have, bool aligned) {
    PotentialPlan p;
    int n_obj = 0;
    if ((p.rc = check_batch(b, &n_obj)) != OC_OK) return p;
    if (!have) { p.rc = fail(OC_EINVAL, "oc_potential: NULL pointer"); return p; }
    if (!aligned) { p.rc = fail(OC_EINVAL, "oc_potential: d_phi_tables / d_phi must be 8-byte aligned"); return p; }
    if (b->n_envs == 0) { p.nothing = true; return p; }
    p.two_pots = b->max_pots >= 1 && b->max_pots <= 2;  // (0 = unknown: the general kernel)
    p.grid = (unsigned)grid_for(b->n_envs);
    return p;
}

}  // namespace

extern "C" {

int oc_abi_version(void) { return OC_ABI_VERSION; }
size_t oc_layout_size(void) { return sizeof(OcLayout); }
const char* oc_last_error(void) { return g_err; }
int oc_state_planes(int width, int height) { return 1 + (width * height + 15) / 16; }

int oc_batch_hints(const OcLayout* h_layouts, int n_layouts, OcBatch* batch) {
    if (!h_layouts || !batch || n_layouts < 1) return fail(OC_EINVAL, "oc_batch_hints: NULL table / batch or no layouts");
    int max_pots = 0;
    uint32_t max_free = 0;
    bool two = true, any_old = false, same_shaping = true, shared_faces = false;
    for (int i = 0; i < n_layouts; ++i) {
        const OcLayout& l = h_layouts[i];
        any_old = any_old || l.old_dynamics != 0;
        same_shaping = same_shaping && l.old_dynamics == h_layouts[0].old_dynamics &&
                       l.rew_placement_in_pot == h_layouts[0].rew_placement_in_pot &&
                       l.rew_dish_pickup == h_layouts[0].rew_dish_pickup && l.rew_soup_pickup == h_layouts[0].rew_soup_pickup;
        if (l.n_pots > OC_MAX_POTS || l.n_cells > OC_MAX_CELLS) return fail(OC_EINVAL, "oc_batch_hints: corrupt layout record");
        max_pots = l.n_pots > max_pots ? l.n_pots : max_pots;
        two = two && l.n_players == 2;
        uint32_t free_cells = 0;
        for (int c = 0; c < l.n_cells; ++c) free_cells += (l.terrain[c] & 7) == OC_T_FLOOR ? 1u : 0u;
        for (int c = 0; c < l.n_cells && l.width; ++c) {  // does some non-floor cell touch two floor cells (two players could face it)?
            if ((l.terrain[c] & 7) == OC_T_FLOOR) continue;
            const int x = c % l.width, y = c / l.width;
            int touching = 0;
            const int nb[4][2] = {{x, y - 1}, {x, y + 1}, {x + 1, y}, {x - 1, y}};
            for (int k = 0; k < 4; ++k) {
                const int nx = nb[k][0], ny = nb[k][1];
                if (nx < 0 || ny < 0 || nx >= l.width || ny >= l.height) continue;
                touching += (l.terrain[ny * l.width + nx] & 7) == OC_T_FLOOR ? 1 : 0;
            }
            shared_faces = shared_faces || touching >= 2;
        }
        max_free = free_cells > max_free ? free_cells : max_free;
    }
    batch->max_pots = max_pots;
    batch->batch_flags = (two ? OC_BATCH_TWO_PLAYERS : 0u) | (any_old ? 0u : OC_BATCH_NEW_DYNAMICS) |
                         (same_shaping ? OC_BATCH_UNIFORM_SHAPING : 0u) | (shared_faces ? 0u : OC_BATCH_NO_SHARED_FACES);
    batch->max_free_cells = max_free;
    return OC_OK;
}

int oc_step(const OcBatch* b, const void* d_state_in, void* d_state_out, const uint8_t* d_actions, float* d_rewards,
            uint8_t* d_flags, float* d_ep_returns, uint64_t* d_events, int horizon, uint32_t options,
            const OcStartSpec* start, const OcEventSink* events, void* stream) {
    const EvArgs ea = ev_args(events, d_events);
    const StepArrays have = {d_state_in && d_state_out && d_actions && d_rewards && d_flags, ea.events != nullptr, ea.counts != nullptr,
                             aligned16(d_rewards), aligned16(d_ep_returns)};
    const StepPlan p = plan_step(b, ENTRY_STEP, have, horizon, options, 1, start);
    if (p.rc != OC_OK || p.ch.family == StepChoice::NOTHING) return p.rc;
    if (int rc = launch_step_from(p.ch, b, p.n_obj, d_state_in, d_state_out, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options,
                                  (hipStream_t)stream, p.sa, ea, 1))
        return rc;
    return check_launch("oc_step");
}

int oc_step_many(const OcBatch* b, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                 float* d_ep_returns, int n_steps, int horizon, uint32_t options, const OcStartSpec* start,
                 const OcEventSink* events, void* stream) {
    const EvArgs ea = ev_args(events, nullptr);
    const StepArrays have = {d_state && d_actions && d_rewards && d_flags, ea.events != nullptr, ea.counts != nullptr,
                             aligned16(d_rewards), aligned16(d_ep_returns)};
    const StepPlan p = plan_step(b, ENTRY_STEP_MANY, have, horizon, options, n_steps, start);
    if (p.rc != OC_OK || p.ch.family == StepChoice::NOTHING) return p.rc;
    if (!p.step_by_step) {  // all K transitions in one launch, the envs stay on chip in between
        if (int rc = launch_step_from(p.ch, b, p.n_obj, d_state, d_state, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options,
                                      (hipStream_t)stream, p.sa, ea, n_steps))
            return rc;
        return check_launch("oc_step_many");
    }
    for (int k = 0; k < n_steps; ++k) {
        const int64_t off = (int64_t)k * b->n_envs;
        if (int rc = oc_step(b, d_state, d_state, d_actions + 2 * off, d_rewards + 4 * off, d_flags + off, d_ep_returns,
                             nullptr, horizon, options, nullptr, nullptr, stream))
            return rc;
    }
    return OC_OK;
}

int oc_step_plan(const OcBatch* b, int entry, int horizon, uint32_t options, int n_steps, int with_masks, int with_counts,
                 const OcStartSpec* start, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_step_plan: no output buffer");
    out[0] = 0;
    if (entry < ENTRY_STEP || entry > ENTRY_SERVER) return fail(OC_EINVAL, "oc_step_plan: entry must be 0 (oc_step), 1 (oc_step_many) or 2 (oc_step_server_open)");
    // the call the entry point would get: every required array, the named event arrays (the server takes no event sink)
    const StepArrays have = {true, entry != ENTRY_SERVER && with_masks != 0, entry != ENTRY_SERVER && with_counts != 0};
    const StepPlan p = plan_step(b, entry, have, horizon, options, n_steps, start);
    if (p.rc != OC_OK) return p.rc;
    char buf[256];
    if (p.ch.family == StepChoice::NOTHING) {
        snprintf(buf, sizeof(buf), "nothing to launch (%s)", p.nothing);
    } else {
        const int used = p.step_by_step ? snprintf(buf, sizeof(buf), "step by step: oc_step + ") : 0;
        describe_step(p.ch, buf + used, sizeof(buf) - (size_t)used);
    }
    snprintf(out, out_size, "%s", buf);
    return OC_OK;
}

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

int oc_featurize(const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const void* d_state,
                 float* d_features, int num_pots, void* stream) {
    const FeaturizePlan p = plan_featurize(b, d_plan_blob && d_plan_off && d_state && d_features, ((uintptr_t)d_features & 15u) == 0, num_pots);
    if (p.rc != OC_OK || p.nothing) return p.rc;
    if (p.lay_lds) launch_featurize<true>(p, b, d_plan_blob, d_plan_off, d_state, d_features, num_pots, (hipStream_t)stream);
    else launch_featurize<false>(p, b, d_plan_blob, d_plan_off, d_state, d_features, num_pots, (hipStream_t)stream);
    return check_launch("oc_featurize");
}

int oc_featurize_plan(const OcBatch* b, int num_pots, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_featurize_plan: no output buffer");
    out[0] = 0;
    const FeaturizePlan p = plan_featurize(b, true, true, num_pots);
    if (p.rc != OC_OK) return p.rc;
    if (p.nothing) snprintf(out, out_size, "nothing to launch (no envs)");
    else snprintf(out, out_size, "k_featurize<LAY_LDS=%s> grid=%u, %zu B LDS", p.lay_lds ? "true" : "false", p.grid, p.smem);
    return OC_OK;
}

int oc_phi_table_size(void) { return PHI_BYTES; }

int oc_shape_rewards(const OcBatch* b, const float* d_rewards, const uint8_t* d_flags, const double* d_phi_next,
                     double* d_phi_cur, const double* d_phi_start, double reward_shaping_factor, double* d_out,
                     uint8_t* d_done, void* stream) {
    if (!b) return fail(OC_EINVAL, "batch is NULL");
    if (!d_rewards || !d_flags || !d_out) return fail(OC_EINVAL, "oc_shape_rewards: NULL rewards/flags/out pointer");
    if (d_phi_next && (!d_phi_cur || !d_phi_start)) return fail(OC_EINVAL, "oc_shape_rewards: phi_next needs phi_cur and phi_start");
    if (((uintptr_t)d_out & 15u) != 0) return fail(OC_EINVAL, "oc_shape_rewards: d_out must be 16-byte aligned");
    if (b->n_envs == 0) return OC_OK;
    hipLaunchKernelGGL(k_shape_rewards, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const float4*)d_rewards, d_flags, b->n_layouts > 1 ? b->d_layout_id : nullptr, d_phi_next, d_phi_cur,
                       d_phi_start, reward_shaping_factor, d_out, d_done, b->n_envs);
    return check_launch("oc_shape_rewards");
}

int oc_potential(const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const uint8_t* d_phi_tables,
                 const void* d_state, double* d_phi, void* stream) {
    const PotentialPlan p = plan_potential(b, d_plan_blob && d_plan_off && d_phi_tables && d_state && d_phi,
                                           ((uintptr_t)d_phi_tables & 7u) == 0 && ((uintptr_t)d_phi & 7u) == 0);
    if (p.rc != OC_OK || p.nothing) return p.rc;
    if (p.two_pots)
        hipLaunchKernelGGL(k_potential2, dim3(p.grid), dim3(BLOCK), 0, (hipStream_t)stream, b->d_layouts, b->d_layout_id, d_plan_blob,
                           d_plan_off, d_phi_tables, (const uint4*)d_state, d_phi, b->n_envs, b->width, b->height);
    else
        hipLaunchKernelGGL(k_potential, dim3(p.grid), dim3(BLOCK), 0, (hipStream_t)stream, b->d_layouts, b->d_layout_id, d_plan_blob,
                           d_plan_off, d_phi_tables, (const uint4*)d_state, d_phi, b->n_envs, b->width, b->height);
    return check_launch("oc_potential");
}

int oc_potential_plan(const OcBatch* b, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_potential_plan: no output buffer");
    out[0] = 0;
    const PotentialPlan p = plan_potential(b, true, true);
    if (p.rc != OC_OK) return p.rc;
    if (p.nothing) snprintf(out, out_size, "nothing to launch (no envs)");
    else snprintf(out, out_size, "%s grid=%u", p.two_pots ? "k_potential2" : "k_potential", p.grid);
    return OC_OK;
}

int oc_reset(const OcBatch* b, void* d_state, const uint8_t* d_mask, float* d_ep_returns, void* stream) {
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (!d_state) return fail(OC_EINVAL, "oc_reset: NULL state pointer");
    if (b->n_envs == 0) return OC_OK;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_NOBJ(n_obj, {
        hipLaunchKernelGGL((k_reset<NOBJ>), dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, s, b->d_layouts, b->d_layout_id,
                           (uint4*)d_state, d_mask, (float4*)d_ep_returns, b->n_envs);
    });
    return check_launch("oc_reset");
}

}  // extern "C"

#include "train_dispatch.hpp"  // oc_multi_agent_step, oc_multi_agent_step_featurize, oc_multi_agent_step_sample (+ their plans), oc_sample_actions

extern "C" {

int oc_regen_layouts(const OcBatch* b, uint16_t* d_layout_id, const uint8_t* d_mask, uint8_t mask_bits, const OcStartSpec* start,
                     void* stream) {
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (!d_layout_id || !start || !start->regen_count) return fail(OC_EINVAL, "oc_regen_layouts: needs d_layout_id and a start spec with regen_count > 0");
    if ((uint64_t)start->regen_first + start->regen_count > (uint64_t)b->n_layouts)
        return fail(OC_EINVAL, "oc_regen_layouts: regen_first + regen_count exceeds the layout table");
    if (b->n_envs == 0) return OC_OK;
    StartArgs sa;  // (the ids of the call, not the batch's; one layout is a range too: nothing else of the spec is read or checked)
    start_keys(start, &sa);
    sa.regen_first = start->regen_first;
    sa.regen_count = start->regen_count;
    sa.layout_ids = d_layout_id;
    hipLaunchKernelGGL(k_regen_layouts, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, (hipStream_t)stream, d_layout_id, d_mask,
                       mask_bits, b->n_envs, sa);
    return check_launch("oc_regen_layouts");
}

int oc_reset_random(const OcBatch* b, void* d_state, const uint8_t* d_mask, float* d_ep_returns, uint64_t seed,
                    int64_t env_offset, uint32_t epoch, int random_start_pos, double rnd_obj_prob_thresh, void* stream) {
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (!d_state) return fail(OC_EINVAL, "oc_reset_random: NULL state pointer");
    if (!(rnd_obj_prob_thresh >= 0.0 && rnd_obj_prob_thresh <= 1.0))
        return fail(OC_EINVAL, "oc_reset_random: rnd_obj_prob_thresh must be in [0, 1]");
    if (b->n_envs == 0) return OC_OK;
    const uint64_t thresh = (uint64_t)(rnd_obj_prob_thresh * 4294967296.0);  // floor(thresh * 2^32); 1.0 -> 2^32: always
    hipLaunchKernelGGL(k_reset_random, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, (hipStream_t)stream, b->d_layouts,
                       b->d_layout_id, (uint4*)d_state, d_mask, (float4*)d_ep_returns, b->n_envs, n_obj, (uint32_t)seed,
                       (uint32_t)(seed >> 32), env_offset, epoch, random_start_pos, thresh);
    return check_launch("oc_reset_random");
}

}  // extern "C"

namespace {
// ---- the observation paths: oc_encode_lossless and oc_rollout_encode plan a call first (observation_plan.hpp: every check, every
//      choice; no launch, no device memory), then launch from that plan — or, by oc_observation_plan, describe it
int launch_encode(const EncodePlan& p, const OcBatch* b, const void* d_state, void* d_obs, int horizon, hipStream_t s) {
    const auto generic = [&](auto t, auto lay_lds) {
        using T = decltype(t);
        constexpr bool LAY_LDS = decltype(lay_lds)::value;
        if (!want_lds(k_encode<T, LAY_LDS>, p.smem)) return;
        hipLaunchKernelGGL((k_encode<T, LAY_LDS>), dim3(p.grid), dim3(BLOCK), p.smem, s, b->d_layouts, b->n_layouts, b->d_layout_id,
                           (const uint4*)d_state, (T*)d_obs, b->n_envs, b->width, b->height, p.n_planes, p.epb, horizon);
    };
    if (p.kernel == EncodePlan::UNIFORM) {
        if (want_lds(k_encode_uniform<uint8_t>, p.smem))
            hipLaunchKernelGGL((k_encode_uniform<uint8_t>), dim3(p.grid), dim3(BLOCK), p.smem, s, b->d_layouts, (const uint4*)d_state,
                               (uint8_t*)d_obs, b->n_envs, b->width, b->height, p.n_planes, p.unit, p.upg, horizon);
    } else if (!p.f32) {
        if (p.lay_lds) generic(uint8_t(), std::true_type()); else generic(uint8_t(), std::false_type());
    } else {
        if (p.lay_lds) generic(float(), std::true_type()); else generic(float(), std::false_type());
    }
    return check_launch("oc_encode_lossless");
}

// What a workgroup of the k_rollout_encode instances that would serve the batch may ask for on top of their static LDS (160 KiB
// per CU; the instances of one FAST and T keep the same, the eight-wavefront ones 32 bytes more)
LdsBudget rollout_encode_lds(const OcBatch* b, int obs_dtype) {
    const bool fast = b && rollout_encode_fast(b);
    const void* const kernel = obs_dtype == OC_OBS_U8
        ? (fast ? (const void*)k_rollout_encode<2, 3, uint8_t, 4> : (const void*)k_rollout_encode<2, 0, uint8_t, 4>)
        : (fast ? (const void*)k_rollout_encode<2, 3, float, 4> : (const void*)k_rollout_encode<2, 0, float, 4>);
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) { (void)hipGetLastError(); return lds_budget_fallback(); }
    return {(size_t)160 * 1024 - (size_t)fa.sharedSizeBytes - 64, true};
}

// The arrays and scalars of one oc_rollout_encode call
struct RolloutEncodeCall {
    const OcBatch* b;
    void* d_state;
    const uint8_t* d_actions;
    float* d_rewards;
    uint8_t* d_flags;
    float* d_ep_returns;
    void* d_obs;
    int obs_dtype;
    int64_t obs_step_stride;
    int horizon;
    uint32_t step_options;  // OC_OPT_AUTO_RESET or nothing
    uint64_t seed;
    int64_t env_offset, t0;
    int n_steps;
    const OcStartSpec* start;
    hipStream_t stream;
};

// the whole trajectory in one launch (k_rollout_encode)
int launch_rollout_encode(const RolloutEncodePlan& p, const RolloutEncodeCall& c) {
    const OcBatch* b = c.b;
    const auto go = [&](auto fast, auto t, auto nw) {
        using T = decltype(t);
        constexpr int FAST = decltype(fast)::value, NW = decltype(nw)::value;
        if (!want_lds(k_rollout_encode<2, FAST, T, NW>, p.smem)) return;
        hipLaunchKernelGGL((k_rollout_encode<2, FAST, T, NW>), dim3(grid_for(b->n_envs)), dim3(NW * 64), p.smem, c.stream, b->d_layouts,
                           (uint4*)c.d_state, c.d_actions, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, (uint8_t*)c.d_obs,
                           c.obs_step_stride, b->n_envs, b->width, b->height, p.n_obj, c.horizon, c.step_options, (uint32_t)c.seed,
                           (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, p.unit, p.g, p.sa);
    };
    const auto go_t = [&](auto fast, auto nw) { if (!p.f32) go(fast, uint8_t(), nw); else go(fast, float(), nw); };
    using std::integral_constant;
    if (p.nw == 8) {
        if (p.fast) go_t(integral_constant<int, 3>(), integral_constant<int, 8>()); else go_t(integral_constant<int, 0>(), integral_constant<int, 8>());
    } else {
        if (p.fast) go_t(integral_constant<int, 3>(), integral_constant<int, 4>()); else go_t(integral_constant<int, 0>(), integral_constant<int, 4>());
    }
    return check_launch("oc_rollout_encode");
}

// every other table: the same result from the one-step kernels, step by step
int rollout_encode_step_by_step(const RolloutEncodeCall& c) {
    const OcBatch* b = c.b;
    for (int k = 0; k < c.n_steps; ++k) {
        const int64_t off = (int64_t)k * b->n_envs;
        OcStartSpec sk;
        if (c.start) { sk = *c.start; sk.epoch = c.start->epoch + (uint32_t)k; }  // a restart at step k draws from epoch + k
        const OcStartSpec* spk = c.start ? &sk : nullptr;
        int rc;
        if (c.d_actions)
            rc = oc_step(b, c.d_state, c.d_state, c.d_actions + 2 * off, c.d_rewards + 4 * off, c.d_flags + off, c.d_ep_returns, nullptr,
                         c.horizon, c.step_options, spk, nullptr, c.stream);
        else
            rc = oc_rollout_random(b, c.d_state, c.d_rewards ? c.d_rewards + 4 * off : nullptr, c.d_flags ? c.d_flags + off : nullptr,
                                   c.d_ep_returns, c.horizon, c.step_options, c.seed, c.env_offset, c.t0 + k, 1, spk, nullptr, c.stream);
        if (rc) return rc;
        if ((rc = oc_encode_lossless(b, c.d_state, (uint8_t*)c.d_obs + (int64_t)k * c.obs_step_stride, c.obs_dtype, c.horizon, c.stream))) return rc;
    }
    return OC_OK;
}

// ---- oc_rollout_featurize: planned first (observation_plan.hpp: plan_rollout_featurize), then launched from that plan — or, by
//      oc_rollout_featurize_plan, described
// The arrays and scalars of one oc_rollout_featurize call
struct RolloutFeaturizeCall {
    const OcBatch* b;
    const uint8_t* d_plan_blob;
    const uint32_t* d_plan_off;
    void* d_state;
    const uint8_t* d_actions;
    float* d_rewards;
    uint8_t* d_flags;
    float* d_ep_returns;
    float* d_features;
    int64_t feat_step_stride;
    int num_pots, horizon;
    uint32_t step_options;  // OC_OPT_AUTO_RESET or nothing
    uint64_t seed;
    int64_t env_offset, t0;
    int n_steps;
    const OcStartSpec* start;
    hipStream_t stream;
};

// the whole trajectory in one launch (k_rollout_featurize)
int launch_rollout_featurize(const RolloutFeaturizePlan& p, const RolloutFeaturizeCall& c) {
    const OcBatch* b = c.b;
    if (want_lds(k_rollout_featurize<2, 3>, p.smem))
        hipLaunchKernelGGL((k_rollout_featurize<2, 3>), dim3(p.grid), dim3(BLOCK), p.smem, c.stream, b->d_layouts, (uint4*)c.d_state,
                           c.d_actions, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, c.d_plan_blob, c.d_plan_off,
                           (uint8_t*)c.d_features, c.feat_step_stride, b->n_envs, b->width, b->height, p.n_obj, c.num_pots, c.horizon,
                           c.step_options, (uint32_t)c.seed, (uint32_t)(c.seed >> 32), c.env_offset, c.t0, c.n_steps, p.sa);
    return check_launch("oc_rollout_featurize");
}

// every other table: the same result from the one-step entry points and oc_featurize, step by step
int rollout_featurize_step_by_step(const RolloutFeaturizeCall& c) {
    const OcBatch* b = c.b;
    for (int k = 0; k < c.n_steps; ++k) {
        const int64_t off = (int64_t)k * b->n_envs;
        OcStartSpec sk;
        if (c.start) { sk = *c.start; sk.epoch = c.start->epoch + (uint32_t)k; }  // a restart at step k draws from epoch + k
        const OcStartSpec* spk = c.start ? &sk : nullptr;
        int rc;
        if (c.d_actions)
            rc = oc_step(b, c.d_state, c.d_state, c.d_actions + 2 * off, c.d_rewards + 4 * off, c.d_flags + off, c.d_ep_returns, nullptr,
                         c.horizon, c.step_options, spk, nullptr, c.stream);
        else
            rc = oc_rollout_random(b, c.d_state, c.d_rewards ? c.d_rewards + 4 * off : nullptr, c.d_flags ? c.d_flags + off : nullptr,
                                   c.d_ep_returns, c.horizon, c.step_options, c.seed, c.env_offset, c.t0 + k, 1, spk, nullptr, c.stream);
        if (rc) return rc;
        float* feat_k = (float*)((uint8_t*)c.d_features + (int64_t)k * c.feat_step_stride);
        if ((rc = oc_featurize(b, c.d_plan_blob, c.d_plan_off, c.d_state, feat_k, c.num_pots, c.stream))) return rc;
    }
    return OC_OK;
}
}  // namespace

extern "C" {

int oc_encode_lossless(const OcBatch* b, const void* d_state, void* d_obs, int obs_dtype, int horizon, void* stream) {
    const EncodePlan p = plan_encode(b, obs_dtype, d_state != nullptr, d_obs != nullptr, aligned16(d_obs));
    if (p.rc != OC_OK || p.kernel == EncodePlan::NOTHING) return p.rc;
    return launch_encode(p, b, d_state, d_obs, horizon, (hipStream_t)stream);
}

int oc_step_encode(const OcBatch* b, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                   float* d_ep_returns, void* d_obs, int obs_dtype, int horizon, uint32_t options,
                   const OcStartSpec* start, void* stream) {
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (!d_state || !d_actions || !d_rewards || !d_flags || !d_obs) return fail(OC_EINVAL, "oc_step_encode: NULL pointer");
    if (int rc = check_obs("oc_step_encode", obs_dtype, aligned16(d_obs))) return rc;
    if (int rc = check_quads("oc_step_encode", aligned16(d_rewards), aligned16(d_ep_returns))) return rc;
    if (int rc = check_horizon("oc_step_encode", horizon)) return rc;
    StartArgs sa;
    if (int rc = check_start("oc_step_encode", start, &sa, b)) return rc;
    if (b->n_envs == 0) return OC_OK;
    if (!start && !(options & ~(uint32_t)(OC_OPT_AUTO_RESET | OC_OPT_ONE_KERNEL)))  // one kernel where that applies
        return oc_rollout_encode(b, d_state, d_actions, d_rewards, d_flags, d_ep_returns, d_obs, obs_dtype, 0, horizon, options,
                                 0, 0, 0, 1, nullptr, stream);
    if (int rc = oc_step(b, d_state, d_state, d_actions, d_rewards, d_flags, d_ep_returns, nullptr, horizon,
                         options & ~(uint32_t)OC_OPT_ONE_KERNEL, start, nullptr, stream))
        return rc;
    return oc_encode_lossless(b, d_state, d_obs, obs_dtype, horizon, stream);
}

int oc_rollout_encode(const OcBatch* b, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                      float* d_ep_returns, void* d_obs, int obs_dtype, int64_t obs_step_stride, int horizon,
                      uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0, int n_steps,
                      const OcStartSpec* start, void* stream) {
    const RolloutEncodeArrays have = {d_state != nullptr, d_actions != nullptr, d_rewards != nullptr, d_flags != nullptr, d_obs != nullptr,
                                      aligned16(d_obs) && obs_step_stride >= 0 && (obs_step_stride & 15) == 0, aligned16(d_rewards),
                                      aligned16(d_ep_returns)};
    const RolloutEncodePlan p = plan_rollout_encode(b, have, obs_dtype, horizon, options, env_offset, n_steps, start, rollout_encode_lds(b, obs_dtype));
    if (p.rc != OC_OK || p.path == RolloutEncodePlan::NOTHING) return p.rc;
    const RolloutEncodeCall c = {b, d_state, d_actions, d_rewards, d_flags, d_ep_returns, d_obs, obs_dtype, obs_step_stride, horizon,
                                 options & (uint32_t)OC_OPT_AUTO_RESET, seed, env_offset, t0, n_steps, start, (hipStream_t)stream};
    if (p.path == RolloutEncodePlan::ONE_KERNEL) return launch_rollout_encode(p, c);
    return rollout_encode_step_by_step(c);
}

int oc_observation_plan(const OcBatch* b, int obs_dtype, int horizon, uint32_t options, int n_steps, int with_actions, int with_outputs,
                        const OcStartSpec* start, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_observation_plan: no output buffer");
    out[0] = 0;
    if (n_steps == 0) {  // oc_encode_lossless of the batch: a state and an aligned observation array
        const EncodePlan p = plan_encode(b, obs_dtype, true, true, true);
        if (p.rc == OC_OK) describe_encode_plan(p, out, out_size);
        return p.rc;
    }
    // the call oc_rollout_encode would get: a state, an aligned trajectory buffer, the named arrays, the env offset of the start spec
    const RolloutEncodeArrays have = {true, with_actions != 0, with_outputs != 0, with_outputs != 0, true, true};
    const RolloutEncodePlan p = plan_rollout_encode(b, have, obs_dtype, horizon, options, start ? start->env_offset : 0, n_steps, start,
                                                    rollout_encode_lds(b, obs_dtype));
    if (p.rc != OC_OK) return p.rc;
    EncodePlan one_step;
    if (p.path == RolloutEncodePlan::STEP_BY_STEP) {
        one_step = plan_encode(b, obs_dtype, true, true, true);
        if (one_step.rc != OC_OK) return one_step.rc;
    }
    describe_rollout_encode_plan(p, have.actions, one_step, out, out_size);
    return OC_OK;
}

int oc_rollout_featurize(const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, void* d_state,
                         const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags, float* d_ep_returns, float* d_features,
                         int64_t feat_step_stride, int num_pots, int horizon, uint32_t options, uint64_t seed, int64_t env_offset,
                         int64_t t0, int n_steps, const OcStartSpec* start, void* stream) {
    const RolloutFeaturizeArrays have = {d_plan_blob && d_plan_off, d_state != nullptr, d_actions != nullptr, d_rewards != nullptr,
                                         d_flags != nullptr, d_features != nullptr,
                                         aligned16(d_features) && feat_step_stride >= 0 && (feat_step_stride & 15) == 0, aligned16(d_rewards),
                                         aligned16(d_ep_returns)};
    const RolloutFeaturizePlan p = plan_rollout_featurize(b, have, num_pots, horizon, options, env_offset, n_steps, start);
    if (p.rc != OC_OK || p.path == RolloutFeaturizePlan::NOTHING) return p.rc;
    const RolloutFeaturizeCall c = {b, d_plan_blob, d_plan_off, d_state, d_actions, d_rewards, d_flags, d_ep_returns, d_features,
                                    feat_step_stride, num_pots, horizon, options & (uint32_t)OC_OPT_AUTO_RESET, seed, env_offset, t0,
                                    n_steps, start, (hipStream_t)stream};
    if (p.path == RolloutFeaturizePlan::ONE_KERNEL) return launch_rollout_featurize(p, c);
    return rollout_featurize_step_by_step(c);
}

int oc_rollout_featurize_plan(const OcBatch* b, int num_pots, int horizon, uint32_t options, int n_steps, int with_actions,
                              int with_outputs, const OcStartSpec* start, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_rollout_featurize_plan: no output buffer");
    out[0] = 0;
    // the call oc_rollout_featurize would get: the plan blob, a state, an aligned feature buffer, the named arrays, the env offset of
    // the start spec
    const RolloutFeaturizeArrays have = {true, true, with_actions != 0, with_outputs != 0, with_outputs != 0, true, true};
    const RolloutFeaturizePlan p = plan_rollout_featurize(b, have, num_pots, horizon, options, start ? start->env_offset : 0, n_steps, start);
    if (p.rc != OC_OK) return p.rc;
    if (p.path == RolloutFeaturizePlan::NOTHING) {
        snprintf(out, out_size, "nothing to launch (%s)", b->n_envs == 0 ? "no envs" : "no steps");
    } else if (p.path == RolloutFeaturizePlan::ONE_KERNEL) {
        snprintf(out, out_size, "k_rollout_featurize<MAXP=2, FAST=3> G=%d, grid=%u, %zu B LDS", RF_GROUP, p.grid, p.smem);
    } else {  // per step the one-step entry point named here, then oc_featurize, whose own plan follows
        const FeaturizePlan f = plan_featurize(b, true, true, num_pots);
        if (f.rc != OC_OK) return f.rc;
        snprintf(out, out_size, "step by step: %s + k_featurize<LAY_LDS=%s> grid=%u, %zu B LDS", with_actions ? "oc_step" : "oc_rollout_random",
                 f.lay_lds ? "true" : "false", f.grid, f.smem);
    }
    return OC_OK;
}

// ---- the single-env mailbox (mailbox.hpp)
}  // extern "C"

// ---- the resident batched step (step_server.hpp)
struct OcStepServer {
    OcBatch b;
    int n_obj, horizon, device;
    uint32_t options;
    StartArgs sa;
    void* d_state;
    float* d_ep_returns;
    hipStream_t stream;      // the resident kernel's own stream
    hipStream_t ctl_stream;  // posts that must overtake it (SV_STOP)
    hipEvent_t ev0, ev1;
    uint64_t* d_req;         // [n_envs] request granules
    uint4* d_rsp;            // [n_envs][2] response granules
    uint32_t* h_ctl;         // [4 grid + SV_ERR_WORDS] pinned, GPU-mapped: 1 per serving wavefront, then the error / keep-alive words
    unsigned n_flags, n_serving;  // 4 grid; wavefronts with at least one env: ceil(n_envs / 64)
    uint32_t* d_ctl;         // its device address
    uint32_t* d_claims;      // [32] block claims per XCD: [0..8] the server's, [16..24] the client's (sv_claim_block)
    unsigned grid;
    uint32_t seq;            // the tag of the last request served (= steps served since the server was opened)
    uint64_t idle_ticks, life_ticks, client_ticks;
    double idle_s;
    struct timespec last_use;
    bool launched;
};

namespace {
static_assert(OC_SV_STOP == SV_STOP, "command bit of include/oc_amd.h");
// how the two ends wait: bits 0..7 naps (64 clk each) before the first look, 8..15 naps between looks, bit 16 light polls (the
// wavefront's first env alone until it shows the tag), bit 17 never look through the L2, bits 24..26 (client) which XCD's blocks
// a workgroup claims: its own + this.  Measured on MI355X, 65 536 envs, 1 000 dependent steps (gpurun_out -> profiles/
// r06_step_server.txt): naps and light polls change nothing (3.3 us either way, light polls +0.3: one more load round trip);
// both ends of every env on ONE XCD 4.17 us (5.37 without the looks through the L2: 32 pairs share one L2's channels), on
// neighbouring XCDs 3.2, four XCDs apart 3.02 — so the client claims the blocks of the XCD opposite its own; a single pair
// alone: 2.27 same XCD, 2.63 across.  (tuning builds: the named environment variable overrides the value)
uint32_t sv_knobs(const char* name, uint32_t dflt) {
#ifdef OC_AMD_TUNING
    if (const char* e = getenv(name)) return (uint32_t)strtoul(e, nullptr, 0);
#endif
    (void)name;
    return dflt;
}
double sv_since(const struct timespec& t) {
    struct timespec now;
    clock_gettime(CLOCK_MONOTONIC, &now);
    return (double)(now.tv_sec - t.tv_sec) + 1e-9 * (double)(now.tv_nsec - t.tv_nsec);
}
unsigned sv_resident(const OcStepServer* m) {  // wavefronts that say they serve
    unsigned alive = 0;
    for (unsigned i = 0; i < m->n_flags; ++i) alive += __atomic_load_n(m->h_ctl + i, __ATOMIC_ACQUIRE) != 0u;
    return alive;
}
void sv_mark(OcStepServer* m, uint32_t v) {
    for (unsigned i = 0; i < m->n_flags; ++i) __atomic_store_n(m->h_ctl + i, v, __ATOMIC_RELEASE);
}
template <typename K>
bool sv_fits(K kernel, const OcStepServer* m, size_t smem) {  // every workgroup must be resident at once: they all poll
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK, smem) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return (int64_t)m->grid <= (int64_t)per_cu * cus;
}
// the resident kernel leaves (writes the states back) and its stream drains; the host's step count follows the device's
int sv_stop(OcStepServer* m) {
    if (!m->launched) return OC_OK;
    if (sv_resident(m) != 0u)  // (on the control stream: behind the resident kernel on its own stream the post would never run)
        hipLaunchKernelGGL(k_step_server_post, dim3(m->grid), dim3(BLOCK), 0, m->ctl_stream, m->d_req, m->b.n_envs, SV_STOP, m->d_rsp, 1u);
    if (hipStreamSynchronize(m->ctl_stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_step_server: the resident kernel did not leave");
    }
    m->launched = false;
    sv_mark(m, 0u);
    uint32_t tag = 0;  // env 0's last served tag (device-side callers may have advanced it without the host)
    if (hipMemcpy(&tag, reinterpret_cast<const uint8_t*>(m->d_rsp) + 28, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_step_server: reading the step count back failed");
    }
    m->seq = tag;
    return OC_OK;
}
// (re)launch the resident kernel; the requests first lose any stale STOP (a no-op request: the tag already served)
int sv_launch(OcStepServer* m) {
    const OcBatch* b = &m->b;
    const StepChoice ch = choose_step(b, m->n_obj, m->options, 1, false, true);
    const size_t smem = ch.lds;
    sv_mark(m, 0u);  // (every serving wavefront reports in by itself)
    hipLaunchKernelGGL(k_step_server_post, dim3(m->grid), dim3(BLOCK), 0, m->stream, m->d_req, b->n_envs, 0u, m->d_rsp, 0u);
    (void)hipMemsetAsync(m->d_claims, 0, 16 * sizeof(uint32_t), m->stream);
#define GOSV(U, MP, LL)                                                                                              \
    case STEP_KEY(U, MP, LL, false):                                                                                 \
        if (!want_lds(k_step_server<U, MP, LL>, smem)) break;                                                        \
        if (!sv_fits(k_step_server<U, MP, LL>, m, smem)) {                                                           \
            sv_mark(m, 0u);                                                                                          \
            return fail(OC_EINVAL, "oc_step_server: the batch needs more workgroups than the GPU keeps resident at once"); \
        }                                                                                                            \
        hipLaunchKernelGGL((k_step_server<U, MP, LL>), dim3(m->grid), dim3(BLOCK), smem, m->stream, b->d_layouts, b->n_layouts, \
                           b->d_layout_id, (uint4*)m->d_state, (float4*)m->d_ep_returns, m->d_req, m->d_rsp, m->d_ctl, m->d_claims, b->n_envs, \
                           b->width, m->n_obj, m->horizon, m->options, m->sa, m->idle_ticks, m->life_ticks, sv_knobs("OC_SV_SERVER", 0x0100u)); \
        break
    switch (step_key(ch)) {
        GOSV(true, 2, true);
        GOSV(false, 2, true);
        GOSV(false, 8, false);
        default: sv_mark(m, 0u); return fail(OC_ELAUNCH, NO_STEP_INSTANCE);
    }
#undef GOSV
    const int rc = check_launch("oc_step_server");
    if (rc) { sv_mark(m, 0u); return rc; }
    m->launched = true;
    clock_gettime(CLOCK_MONOTONIC, &m->last_use);
    // the server is up when every wavefront that has envs has said so (its states loaded, its first look at the requests next)
    while (sv_resident(m) != m->n_serving) {
        if (sv_since(m->last_use) > 2.0) {
            (void)sv_stop(m);
            return fail(OC_ELAUNCH, "oc_step_server: the resident kernel did not come up within 2 s");
        }
        __builtin_ia32_pause();
    }
    clock_gettime(CLOCK_MONOTONIC, &m->last_use);
    return OC_OK;
}
// resident and fresh (no workgroup about to leave for idleness), or relaunched
// (caller_stream: the stream the caller's work on d_state runs on — a relaunch reads d_state on the server's own stream, so whatever the
//  caller enqueued there since the last sync must be complete first)
int sv_ensure(OcStepServer* m, const hipStream_t* caller_stream = nullptr) {
    if (m->launched) {
        // announce the caller FIRST (a workgroup about to leave for idleness or age looks at this word and stays), give a workgroup
        // that had already looked 20 us to say that it left, THEN count: whoever is counted is still there when the client arrives
        __atomic_fetch_add(m->h_ctl + m->n_flags + SV_KEEPALIVE, 1u, __ATOMIC_RELEASE);
        struct timespec t0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        while (sv_since(t0) < 20e-6) __builtin_ia32_pause();
    }
    if (m->launched && sv_resident(m) == m->n_serving) return OC_OK;
    if (int rc = sv_stop(m)) return rc;
    if (caller_stream && hipStreamSynchronize(*caller_stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_step_server: the caller's stream failed");
    }
    return sv_launch(m);
}
struct SvDevice {  // the server's device current for the scope
    int prev = 0, want;
    explicit SvDevice(int d) : want(d) { (void)hipGetDevice(&prev); if (prev != want) (void)hipSetDevice(want); }
    ~SvDevice() { if (prev != want) (void)hipSetDevice(prev); }
};
}  // namespace

extern "C" {

int oc_step_server_open(const OcBatch* b, void* d_state, float* d_ep_returns, int horizon, uint32_t options,
                        const OcStartSpec* start, double idle_ms, double life_s, OcStepServer** out) {
    if (!out) return fail(OC_EINVAL, "oc_step_server_open: NULL result pointer");
    *out = nullptr;
    const StepPlan p = plan_step(b, ENTRY_SERVER, StepArrays{d_state != nullptr, false, false, true, aligned16(d_ep_returns)}, horizon, options, 1, start);
    if (p.rc != OC_OK) return p.rc;
    const int n_obj = p.n_obj;
    const StartArgs& sa = p.sa;
    if (!(idle_ms >= 0.0 && idle_ms <= 10000.0) || !(life_s >= 0.0 && life_s <= 86400.0))
        return fail(OC_EINVAL, "oc_step_server_open: idle_ms in 0..10 000 (0: 20 ms), life_s in 0..86 400 (0: 600 s)");
    OcStepServer* m = new OcStepServer();
    memset(m, 0, sizeof(*m));
    m->b = *b; m->n_obj = n_obj; m->horizon = horizon; m->options = options; m->sa = sa; m->d_state = d_state; m->d_ep_returns = d_ep_returns;
    m->grid = grid_for(b->n_envs);
    m->n_flags = m->grid * (BLOCK / 64);
    m->n_serving = (unsigned)((b->n_envs + 63) / 64);
    if (idle_ms == 0.0) idle_ms = 20.0;
    if (idle_ms < 0.2) idle_ms = 0.2;  // (a window the host's 20 us announcement always fits in)
    if (life_s == 0.0) life_s = 600.0;
    int khz = 0;
    bool ok = hipGetDevice(&m->device) == hipSuccess;
    if (ok && (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device) != hipSuccess || khz <= 0)) khz = 100000;  // 100 MHz
    m->idle_s = idle_ms * 1e-3;
    m->idle_ticks = (uint64_t)((double)khz * idle_ms);
    m->life_ticks = (uint64_t)((double)khz * 1000.0 * life_s);
    m->client_ticks = (uint64_t)khz * 1000;  // a client wavefront gives up after 1 s without its responses
    const size_t ctl_bytes = ((size_t)m->n_flags + SV_ERR_WORDS) * sizeof(uint32_t);
    ok = ok && hipMalloc((void**)&m->d_req, (size_t)b->n_envs * 8) == hipSuccess;
    ok = ok && hipMalloc((void**)&m->d_rsp, (size_t)b->n_envs * 32) == hipSuccess;
    ok = ok && hipMalloc((void**)&m->d_claims, 32 * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&m->h_ctl, ctl_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    ok = ok && hipHostGetDevicePointer((void**)&m->d_ctl, m->h_ctl, 0) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&m->ctl_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&m->ev0) == hipSuccess && hipEventCreate(&m->ev1) == hipSuccess;
    if (ok) {
        memset(m->h_ctl, 0, ctl_bytes);
        ok = hipMemsetAsync(m->d_req, 0, (size_t)b->n_envs * 8, m->stream) == hipSuccess &&
             hipMemsetAsync(m->d_rsp, 0, (size_t)b->n_envs * 32, m->stream) == hipSuccess &&
             hipMemsetAsync(m->d_claims, 0, 32 * sizeof(uint32_t), m->stream) == hipSuccess &&
             hipStreamSynchronize(m->stream) == hipSuccess;  // (before the resident kernel occupies the stream: clients run on other streams)
    }
    if (!ok) {
        (void)hipGetLastError();
        (void)oc_step_server_close(m);
        return fail(OC_ELAUNCH, "oc_step_server_open: device / pinned memory, streams or events refused");
    }
    if (int rc = sv_launch(m)) { (void)oc_step_server_close(m); return rc; }
    *out = m;
    return OC_OK;
}

void* oc_step_server_requests(OcStepServer* m) { return m ? m->d_req : nullptr; }
void* oc_step_server_responses(OcStepServer* m) { return m ? m->d_rsp : nullptr; }

int oc_step_server_resume(OcStepServer* m) {
    if (!m) return fail(OC_EINVAL, "oc_step_server_resume: NULL server");
    SvDevice dev(m->device);
    return sv_ensure(m);
}

int oc_step_server_play(OcStepServer* m, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags, int n_steps, void* stream,
                        float* elapsed_ms) {
    if (!m) return fail(OC_EINVAL, "oc_step_server_play: NULL server");
    if (!d_actions || !d_rewards || !d_flags) return fail(OC_EINVAL, "oc_step_server_play: NULL actions/rewards/flags pointer");
    if (n_steps < 0 || n_steps > (1 << 24)) return fail(OC_EINVAL, "oc_step_server_play: n_steps must be in 0..2^24");
    if (!aligned16(d_rewards)) return refuse("oc_step_server_play", "d_rewards must be 16-byte aligned");
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (n_steps == 0) return OC_OK;
    SvDevice dev(m->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = sv_ensure(m, &s)) return rc;
    __atomic_store_n(m->h_ctl + m->n_flags + SV_ERR_CLIENT, 0u, __ATOMIC_RELEASE);
    uint32_t* dbg = nullptr;
#ifdef OC_AMD_TUNING
    if (getenv("OC_SV_DEBUG")) (void)hipMalloc((void**)&dbg, (size_t)m->grid * 16);
#endif
    (void)hipEventRecord(m->ev0, s);
    hipLaunchKernelGGL(k_step_client, dim3(m->grid), dim3(BLOCK), 0, s, m->d_req, m->d_rsp, d_actions, (float4*)d_rewards, d_flags,
                       m->d_ctl + m->n_flags, m->d_claims + 16, m->b.n_envs, m->seq + 1u, n_steps, m->client_ticks, sv_knobs("OC_SV_CLIENT", 0x04000100u), dbg);
    (void)hipEventRecord(m->ev1, s);
    if (int rc = check_launch("oc_step_server_play")) return rc;
    if (hipEventSynchronize(m->ev1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_step_server_play: the client kernel failed");
    }
    clock_gettime(CLOCK_MONOTONIC, &m->last_use);
    if (__atomic_load_n(m->h_ctl + m->n_flags + SV_ERR_CLIENT, __ATOMIC_ACQUIRE) != 0u) {
        (void)sv_stop(m);  // (the host's step count follows whatever the device got to)
        (void)hipMemset(m->d_claims + 16, 0, 16 * sizeof(uint32_t));  // (a client that gave up did not hand its block claims back)
        return fail(OC_ELAUNCH, "oc_step_server_play: no answer from the resident kernel within 1 s");
    }
    m->seq += (uint32_t)n_steps;
    if (elapsed_ms) (void)hipEventElapsedTime(elapsed_ms, m->ev0, m->ev1);
#ifdef OC_AMD_TUNING
    if (dbg) {  // where a round trip goes, in 10 ns ticks: the client's post -> response seen, of which the server's seen -> sent
        uint32_t* h = (uint32_t*)malloc((size_t)m->grid * 16);
        (void)hipMemcpy(h, dbg, (size_t)m->grid * 16, hipMemcpyDeviceToHost);
        double rt = 0, sv = 0, worst = 0;
        int cross = 0;
        for (unsigned b = 0; b < m->grid; ++b) {
            rt += h[4 * b]; sv += h[4 * b + 1];
            if (h[4 * b] > worst) worst = h[4 * b];
            cross += (h[4 * b + 2] & 0xFu) != (h[4 * b + 3] & 0xFu);
        }
        fprintf(stderr, "[oc_step_server] %d steps x %u workgroups: round trip mean %.0f ns (in the server %.0f ns), slowest workgroup %.0f ns; %d pairs across XCDs\n",
                n_steps, m->grid, 10.0 * rt / n_steps / m->grid, 10.0 * sv / n_steps / m->grid, 10.0 * worst / n_steps, cross);
        if (getenv("OC_SV_DEBUG_ALL"))
            for (unsigned b = 0; b < m->grid; ++b)
                fprintf(stderr, "  wg %3u: rt %5.0f ns server %4.0f ns  server xcc %u  client xcc %u\n", b, 10.0 * h[4 * b] / n_steps, 10.0 * h[4 * b + 1] / n_steps,
                        h[4 * b + 2] & 0xFu, h[4 * b + 3] & 0xFu);
        free(h);
        (void)hipFree(dbg);
    }
#endif
    return OC_OK;
}

int oc_step_server_sync(OcStepServer* m) {
    if (!m) return fail(OC_EINVAL, "oc_step_server_sync: NULL server");
    SvDevice dev(m->device);
    return sv_stop(m);
}

int64_t oc_step_server_steps(OcStepServer* m) { return m ? (int64_t)m->seq : -1; }

int oc_step_server_close(OcStepServer* m) {
    if (!m) return OC_OK;
    SvDevice dev(m->device);
    int rc = OC_OK;
    if (m->stream && m->ctl_stream) rc = sv_stop(m);
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->ctl_stream) (void)hipStreamDestroy(m->ctl_stream);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    if (m->h_ctl) (void)hipHostFree(m->h_ctl);
    if (m->d_claims) (void)hipFree(m->d_claims);
    if (m->d_rsp) (void)hipFree(m->d_rsp);
    if (m->d_req) (void)hipFree(m->d_req);
    (void)hipGetLastError();
    delete m;
    return rc;
}

}  // extern "C"


struct OcMailbox {
    uint8_t* h;             // the mailbox (pinned host memory, mapped into the GPU's address space)
    uint8_t* d;             // its device address
    hipStream_t stream;     // the resident kernel's own stream
    const OcLayout* d_layout;
    int W, n_obj, horizon, device, max_pots;
    uint32_t seq;
    uint64_t idle_ticks, life_ticks;
};

namespace {
static_assert(OC_MB_STATE_IN == MB_IN && OC_MB_ACTIONS == MB_ACT && OC_MB_STATE_OUT == MB_OUT && OC_MB_REWARDS == MB_REW &&
              OC_MB_FLAGS == MB_FLAGS && OC_MB_EVENTS == MB_EV, "mailbox offsets of include/oc_amd.h");

// the request granules of `tag`: payload = n_state bytes of MB_IN + the two bytes of MB_ACT
void mailbox_post(OcMailbox* m, uint32_t tag, int n_state) {
    alignas(16) uint8_t pay[12 * MB_REQ_MAX + 4] = {0};
    memcpy(pay, m->h + MB_IN, (size_t)n_state);
    memcpy(pay + n_state, m->h + MB_ACT, 2);
    const int n_req = (n_state + 2 + 11) / 12;
    for (int g = 0; g < n_req; ++g) {
        alignas(16) uint32_t q[4];
        memcpy(q, pay + 12 * g, 12);
        q[3] = tag;
        typedef long long mb_i64x2 __attribute__((vector_size(16), aligned(16)));
        *reinterpret_cast<volatile mb_i64x2*>(m->h + MB_REQG + 16 * g) = *reinterpret_cast<const mb_i64x2*>(q);  // one movaps
    }
}

int mailbox_launch(OcMailbox* m) {
    *reinterpret_cast<volatile uint32_t*>(m->h + MB_ALIVE) = 1u;
    DISPATCH_NOBJ(m->n_obj, {
        constexpr int NO = NOBJ <= STEP1_MAX_PLANES ? NOBJ : 1;
        if (NOBJ <= STEP1_MAX_PLANES) {
            if (m->max_pots <= 2)
                hipLaunchKernelGGL((k_mailbox<NO, 2>), dim3(1), dim3(64), 0, m->stream, m->d_layout, m->d, m->W, m->horizon,
                                   m->idle_ticks, m->life_ticks);
            else
                hipLaunchKernelGGL((k_mailbox<NO, OC_MAX_POTS>), dim3(1), dim3(64), 0, m->stream, m->d_layout, m->d, m->W,
                                   m->horizon, m->idle_ticks, m->life_ticks);
        }
    });
    return check_launch("oc_mailbox: launch");
}
}  // namespace

extern "C" {

int oc_mailbox_open(const OcBatch* b, int horizon, OcMailbox** out) {
    int n_obj = 0;
    if (!out) return fail(OC_EINVAL, "oc_mailbox_open: NULL result pointer");
    *out = nullptr;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (b->n_layouts != 1 || n_obj > STEP1_MAX_PLANES) return fail(OC_EINVAL, "oc_mailbox_open: one layout, grids of at most 64 cells");
    if (int rc = check_horizon("oc_mailbox_open", horizon)) return rc;
    OcMailbox* m = new OcMailbox();
    if (hipGetDevice(&m->device) != hipSuccess || hipHostMalloc((void**)&m->h, MB_BYTES, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        delete m;
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_mailbox_open: pinned host memory refused");
    }
    memset(m->h, 0, MB_BYTES);
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device) != hipSuccess || khz <= 0) khz = 100000;  // 100 MHz
    if (hipHostGetDevicePointer((void**)&m->d, m->h, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipHostFree(m->h);
        delete m;
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_mailbox_open: device mapping / stream refused");
    }
    m->d_layout = b->d_layouts; m->W = b->width; m->n_obj = n_obj; m->horizon = horizon; m->seq = 0;
    m->max_pots = b->max_pots > 0 ? b->max_pots : OC_MAX_POTS;  // (hint of oc_batch_hints; unknown: the general instance)
    m->idle_ticks = (uint64_t)khz * 2;     // 2 ms without a request
    m->life_ticks = (uint64_t)khz * 2000;  // 2 s in any case
    if (int rc = mailbox_launch(m)) { (void)oc_mailbox_close(m); return rc; }
    *out = m;
    return OC_OK;
}

void* oc_mailbox_buffer(OcMailbox* m) { return m ? m->h : nullptr; }

int oc_mailbox_step(OcMailbox* m) {
    if (!m) return fail(OC_EINVAL, "oc_mailbox_step: NULL mailbox");
    uint32_t seq = m->seq + 1u;
    if (seq == MB_STOP || seq == 0u) seq = 1u;
    m->seq = seq;
    const int n_state = 16 * (1 + m->n_obj);
    const int n_words = (n_state + 28) / 4;  // payload dwords of the response
    // ---- the request: the caller's plain views (MB_IN, MB_ACT) as granules of {12 payload bytes, tag}, one aligned 16-byte
    //      store each (the kernel's lanes read one granule each with a single 16-byte load: payload and tag arrive together)
    mailbox_post(m, seq, n_state);
    // ---- the response: two 64-byte lines of {15 payload dwords, tag}
    volatile uint32_t* alive = reinterpret_cast<volatile uint32_t*>(m->h + MB_ALIVE);
    uint32_t spins = 0;
    struct timespec t0 = {0, 0};
    for (;;) {
        // the last dword of each response line carries the tag once the line has arrived (line 1 only when the payload needs it)
        int ok = __atomic_load_n(reinterpret_cast<uint32_t*>(m->h + MB_RSPG + 60), __ATOMIC_ACQUIRE) == seq;
        if (ok && n_words > 15) ok = __atomic_load_n(reinterpret_cast<uint32_t*>(m->h + MB_RSPG + 124), __ATOMIC_ACQUIRE) == seq;
        if (ok) break;
        __builtin_ia32_pause();
        if ((++spins & 0x3FFu) != 0u) continue;
        if (*alive == 0u) {  // the kernel has left (idle / lifetime): the next incarnation finds the request
            int dev = 0;
            (void)hipGetDevice(&dev);
            if (dev != m->device) (void)hipSetDevice(m->device);
            const int rc = mailbox_launch(m);
            if (dev != m->device) (void)hipSetDevice(dev);
            if (rc) return rc;
        }
        struct timespec now;
        clock_gettime(CLOCK_MONOTONIC, &now);
        if (t0.tv_sec == 0 && t0.tv_nsec == 0) t0 = now;
        else if ((now.tv_sec - t0.tv_sec) > 5) return fail(OC_ELAUNCH, "oc_mailbox_step: no answer from the resident kernel within 5 s");
    }
    uint8_t rsp[120];
    memcpy(rsp, m->h + MB_RSPG, 60);
    memcpy(rsp + 60, m->h + MB_RSPG + 64, 60);
    memcpy(m->h + MB_OUT, rsp, (size_t)n_state);
    memcpy(m->h + MB_REW, rsp + n_state, 16);
    memcpy(m->h + MB_FLAGS, rsp + n_state + 16, 4);
    memcpy(m->h + MB_EV, rsp + n_state + 20, 8);
    return OC_OK;
}

int oc_mailbox_close(OcMailbox* m) {
    if (!m) return OC_OK;
    mailbox_post(m, MB_STOP, 16 * (1 + m->n_obj));
    (void)hipStreamSynchronize(m->stream);
    (void)hipStreamDestroy(m->stream);
    (void)hipHostFree(m->h);
    (void)hipGetLastError();
    delete m;
    return OC_OK;
}

#ifdef OC_AMD_TUNING
// tuning builds: the phase stamps of the last k_train_step_obs launch (train_obs.hpp: g_obs_dbg), n_words u32
int oc_debug_train_obs(uint32_t* out, int n_words) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_obs_dbg), (size_t)n_words * 4, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
#ifdef OC_AMD_TUNING
// tuning builds: n back-to-back oc_mailbox_step calls from C (no Python / ctypes between them) -> microseconds per call
double oc_mailbox_bench(OcMailbox* m, int n) {
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < n; ++i)
        if (oc_mailbox_step(m)) return -1.0;
    clock_gettime(CLOCK_MONOTONIC, &b);
    return ((b.tv_sec - a.tv_sec) * 1e9 + (b.tv_nsec - a.tv_nsec)) / n * 1e-3;
}
#endif

int oc_output_stores_only(int64_t n_envs, int n_steps, float* d_rewards, uint8_t* d_flags, uint32_t options, void* stream) {
    if (n_envs < 0 || n_steps < 0 || !d_rewards) return fail(OC_EINVAL, "oc_output_stores_only: negative sizes or no rewards array");
    if (((uintptr_t)d_rewards & 15u) != 0) return fail(OC_EINVAL, "oc_output_stores_only: d_rewards must be 16-byte aligned");
    if (options & ~(uint32_t)OC_OPT_FLAGS_TILED8) return fail(OC_EINVAL, "oc_output_stores_only: the only option is OC_OPT_FLAGS_TILED8");
    if (options & OC_OPT_FLAGS_TILED8) {
        if (!d_flags || ((uintptr_t)d_flags & 7u) != 0 || (n_steps & 7) != 0)
            return fail(OC_EINVAL, "oc_output_stores_only: OC_OPT_FLAGS_TILED8 needs an 8-byte aligned d_flags and n_steps a multiple of 8");
        if (n_envs == 0 || n_steps == 0) return OC_OK;
        hipLaunchKernelGGL(k_output_stores_only_tiled8, dim3(grid_for(n_envs)), dim3(BLOCK), 0, (hipStream_t)stream, (float4*)d_rewards,
                           (uint2*)d_flags, n_envs, n_steps / 8);
        return check_launch("oc_output_stores_only");
    }
    if (n_envs == 0 || n_steps == 0) return OC_OK;
    hipLaunchKernelGGL(k_output_stores_only, dim3(grid_for(n_envs)), dim3(BLOCK), 0, (hipStream_t)stream, (float4*)d_rewards, d_flags,
                       n_envs, n_steps);
    return check_launch("oc_output_stores_only");
}

}  // extern "C"
