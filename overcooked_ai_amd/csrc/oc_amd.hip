// oc_amd.hip — MI355X (gfx950 / CDNA4) kernels and C-ABI for the batched Overcooked hot path.
//
// Layout of this translation unit (reference = HumanCompatibleAI/overcooked_ai, "mdp.py" =
// src/overcooked_ai_py/mdp/overcooked_mdp.py).  The kernels live in the kernel headers, the host code of each family in its
// dispatch header (host only: it plans a call — every check, then every choice; no launch, no device address —, launches from the
// plan or puts the plan into words, and defines the family's extern "C" entry points of include/oc_amd.h):
//   common.hpp          constants, OcLayout accessor, Philox4x32-10, layout staging
//   step_predicate.hpp  get_state_transition, mdp.py:1375 (interacts 1432 -> movement 1644 -> env effects 1691) with
//                       the predicate-network interact that also emits event_infos: k_step, k_rollout
//   step_table.hpp      the same transition with the table-driven interact: k_step3 (oc_step_many, grids above 64 cells)
//   step_one.hpp        one transition per launch on the wire format itself: k_step1 (oc_step)
//   mailbox.hpp         one env, resident, fed through pinned host memory: k_mailbox
//   step_server.hpp     the resident batched step and its client: k_step_server, k_step_client
//   step_lut4.hpp       the rollout path: key-byte cell words, 16-byte interact LUT, joint move table: k_rollout4
//   step_duo5.hpp       the rollout path split between mover and interact wavefronts: k_rollout5 — both compiled in rollout4.hip
//                       (three units, see shared.hpp), chosen here (rollout_dispatch.hpp), launched through oc_detail::launch_rollout
//   rollout_pair.hpp    two lanes per env: k_rollout_pair
//   reset.hpp           get_standard_start_state mdp.py:1297, get_random_start_state_fn 1307: k_reset, k_reset_random
//   encode.hpp          lossless_state_encoding mdp.py:2385-2561: k_encode, k_encode_uniform
//   rollout_encode.hpp  K transitions with the observation of every step in one launch: k_rollout_encode
//   featurize.hpp       featurize_state mdp.py:2579-2898: k_featurize
//   rollout_featurize.hpp  K transitions with the featurize_state observation of every step in one launch: k_rollout_featurize
//   potential.hpp       potential_function mdp.py:2920-3238: k_potential, k_potential2
//   sample.hpp          both players' actions drawn from policy logits: sample_env, k_sample_actions
//   shaping.hpp         OvercookedMultiAgent.step reward, rllib.py:306-329: k_shape_rewards
//   train_obs.hpp       the training step with its observation in one kernel: k_train_step_obs
//   train_feat.hpp      the training step with the featurize_state observation in one kernel: k_train_step_feat
//   stores_only.hpp     the output stores of a rollout and nothing else: k_output_stores_only (oc_output_stores_only)
//   observation_plan.hpp  host only: the observation geometry and the plans of oc_encode_lossless / oc_rollout_encode / oc_rollout_featurize
//   step_dispatch.hpp   host only: the caller-actions family — one call record, one plan, the instance rows of k_step1 / k_step3 / k_step /
//                       k_step_server; oc_step, oc_step_many, oc_step_plan
//   rollout_dispatch.hpp  host only: the random rollouts — the choice among k_rollout4 / k_rollout5 / k_rollout_pair / k_rollout;
//                       oc_rollout_random, oc_rollout_record, oc_rollout_record_ex, oc_rollout_plan
//   derived_dispatch.hpp  host only: oc_featurize, oc_potential, their *_plan entry points, oc_phi_table_size, oc_shape_rewards
//   train_dispatch.hpp  host only: the training-step family — one call record, one plan, one launch path; oc_multi_agent_step,
//                       oc_multi_agent_step_featurize, oc_multi_agent_step_sample, their *_plan entry points and oc_sample_actions
//   observation_dispatch.hpp  host only: the launches of observation_plan.hpp's plans and the step-by-step path; oc_encode_lossless,
//                       oc_step_encode, oc_rollout_encode, oc_observation_plan, oc_rollout_featurize, oc_rollout_featurize_plan
//   step_server_host.hpp  host only: the resident batched step's state machine; oc_step_server_*
//   mailbox_host.hpp    host only: the single-env mailbox; oc_mailbox_*
//   this file           what the families share — the error buffer, check_batch, the tuning knobs, the start-spec and alignment checks, ev_args,
//                       DISPATCH_NOBJ — and the entry points that belong to none: oc_abi_version, oc_layout_size, oc_last_error,
//                       oc_state_planes, oc_batch_hints, oc_reset, oc_reset_random, oc_regen_layouts, oc_output_stores_only
//                       (tuning builds: oc_debug_train_obs)
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

}  // namespace

#include "step_dispatch.hpp"     // oc_step, oc_step_many, oc_step_plan
#include "rollout_dispatch.hpp"  // oc_rollout_random, oc_rollout_record, oc_rollout_record_ex, oc_rollout_plan
#include "derived_dispatch.hpp"  // oc_featurize, oc_potential (+ their plans), oc_phi_table_size, oc_shape_rewards

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

#include "observation_dispatch.hpp"  // oc_encode_lossless, oc_step_encode, oc_rollout_encode, oc_observation_plan, oc_rollout_featurize (+ its plan)
#include "step_server_host.hpp"      // oc_step_server_*
#include "mailbox_host.hpp"          // oc_mailbox_*

extern "C" {

#ifdef OC_AMD_TUNING
// tuning builds: the phase stamps of the last k_train_step_obs launch (train_obs.hpp: g_obs_dbg), n_words u32
int oc_debug_train_obs(uint32_t* out, int n_words) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_obs_dbg), (size_t)n_words * 4, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
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
