/*
 * oc_amd.h — C-ABI of liboc_amd.so, the MI355X (gfx950) batched Overcooked hot path.
 *
 * The reference (HumanCompatibleAI/overcooked_ai) is pure Python and has no FFI; the
 * boundary this library sits under is the Python class API
 *     OvercookedGridworld.get_state_transition   src/overcooked_ai_py/mdp/overcooked_mdp.py:1375
 *     OvercookedGridworld.lossless_state_encoding src/overcooked_ai_py/mdp/overcooked_mdp.py:2385
 *     OvercookedEnv.step / reset / is_done        src/overcooked_ai_py/mdp/overcooked_env.py:244,288,321
 * Each entry point below names the reference function(s) it replaces.  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer whose name starts with d_ is a DEVICE pointer (HBM) owned by the caller;
 *    the library never allocates, frees or synchronises.
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - return value: 0 on success, negative OC_E* on error; oc_last_error() gives a message.
 *  - thread-safe per (device, stream); the library keeps no global mutable state except the
 *    thread-local error string.
 *
 * Wire format of one environment ("env") — see DESIGN.md §3.
 *  State is struct-of-arrays over 16-byte words ("planes"): plane p of env e lives at
 *      ((oc_u128*)d_state)[p * n_envs + e]
 *  so a wavefront reading plane p for 64 consecutive envs issues one 1 KiB coalesced load.
 *  Plane 0 (header), byte offsets:
 *      0  player0 cell index (y*W + x)      3  player1 cell index (0xFF = absent, 1-player layouts)
 *      1  player0 orientation (0..3)        4  player1 orientation
 *      2  player0 held object code          5  player1 held object code
 *      6..7  timestep, u16 little endian
 *      8..15 pot slot k: cooking_tick + 1   (0 = idle, i.e. reference _cooking_tick == -1)
 *  Planes 1..n_obj_planes: one object code per grid cell; cell c is byte (c & 15) of plane 1 + (c >> 4).
 *  Object code: 0 none, 1 onion, 2 tomato, 3 dish,
 *               0x80 | (n_ingredients << 3) | tomato_bits   for a soup, where bit i of tomato_bits
 *               says ingredient i (insertion order, SoupState._ingredients, mdp.py:453) is a tomato.
 *  A soup that is held or lies on a counter is always cooked (it left its pot through the
 *  dish pickup at mdp.py:1525-1539); its tick is implied (= the recipe's cook time).
 */
#ifndef OC_AMD_H
#define OC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OC_ABI_VERSION 6

#define OC_MAX_CELLS 128
#define OC_MAX_POTS 8
#define OC_NUM_LAYERS 26 /* lossless_state_encoding layers, mdp.py:2393-2442 */
#define OC_NUM_ACTIONS 6

/* terrain codes = the reference's own TYPE_TO_CODE table (layout_generator.py:18-27) */
#define OC_T_FLOOR 0
#define OC_T_COUNTER 1
#define OC_T_ONION_DISP 2
#define OC_T_TOMATO_DISP 3
#define OC_T_POT 4
#define OC_T_DISH_DISP 5
#define OC_T_SERVE 6

/* action indices = Action.INDEX_TO_ACTION (actions.py:49-52); orientation = Direction index (actions.py:16) */
#define OC_A_NORTH 0
#define OC_A_SOUTH 1
#define OC_A_EAST 2
#define OC_A_WEST 3
#define OC_A_STAY 4
#define OC_A_INTERACT 5

/* object codes */
#define OC_O_NONE 0
#define OC_O_ONION 1
#define OC_O_TOMATO 2
#define OC_O_DISH 3
#define OC_O_SOUP 0x80

/* per-env flag byte written by oc_step / oc_rollout_random */
#define OC_F_DONE 0x01       /* timestep >= horizon after this step (env.py:321-325) */
#define OC_F_BAD_ACTION 0x02 /* action index >= 6: state left untouched (mdp.py:1394-1398 raises) */
#define OC_F_RESET 0x04      /* env was auto-reset to its start state after this step */

/* option bits for oc_step / oc_rollout_random */
#define OC_OPT_AUTO_RESET 0x1u /* reset a done env to its layout's start state inside the kernel */

/* 0x2u: retired (was OC_OPT_LANE_PER_ENV; one lane per env is the default and only automatic choice); ignored when set */
#define OC_OPT_LANE_PAIR 0x4u    /* oc_rollout_random: the lane-pair-per-env kernel where the table allows it
                                   (2-player layouts, <= 2 pots); never chosen automatically */
#define OC_OPT_PREDICATE_INTERACT 0x8u /* oc_rollout_random: one-lane-per-env kernel with the predicate-network
                                         interact instead of the table-driven one (kept for cross-checking) */

/* 0x10u: reserved (ABI <= 3: OC_OPT_ROLLOUT_V3, the round-1 rollout kernel, retired in ABI 4) */
#define OC_OPT_ONE_KERNEL 0x20u /* oc_rollout_encode / oc_step_encode / oc_rollout_featurize /
                                  oc_multi_agent_step_featurize: take the single-kernel
                                  path (k_rollout_encode, k_rollout_featurize, k_train_step_feat)
                                  whenever the table allows it; by default it runs only for batches that give every CU
                                  a workgroup (it keeps 256 envs per CU on chip; smaller batches are faster through the
                                  one-step kernels, whose observation kernel spreads over all CUs) */
#define OC_OPT_FLAGS_TILED8 0x40u /* oc_rollout_random: d_flags is tiled by 8 steps, [n_steps / 8][n_envs][8] — byte
                                     (k / 8, e, k % 8) holds the OC_F_* bits of env e after step k of the call — so that a
                                     wavefront writes the flags of 8 steps as 512 contiguous bytes instead of 64 bytes in each
                                     of 8 rows (worth ~6 % of the rollout rate and its run-to-run spread on MI355X).  Needs
                                     t0 and n_steps to be multiples of 8, d_rewards and an 8-byte aligned d_flags, no event
                                     sink, and a batch one of these kernels serves: the pipelined joint-table kernel (one
                                     two-player, one-pot layout with at most 6 free cells and no shared faced cells —
                                     cramped_room —, at most ~98 000 envs) or the per-env-terrain kernels of mixed two-player
                                     tables (up to 32 layouts: at most ~98 000 envs; one-pot tables of more layouts: any
                                     batch size) — BASELINE configs[1], [3], [4] —, or the mover / interact kernel described
                                     under OC_OPT_ONE_WAVEFRONT (single two-player layouts included; batches of whole 256-env
                                     workgroups up to 524 288 envs); OC_EINVAL otherwise, so a caller can try it once and
                                     fall back */
#define OC_OPT_ONE_WAVEFRONT 0x80u /* oc_rollout_random: keep every env-step in ONE wavefront.  Without this bit, batches of
                                     two-player layouts with at most two pots and 64 cells (new dynamics, one set of shaping
                                     rewards, both output arrays, no event sink) that consist of whole 256-env workgroups —
                                     one per CU at a time: batches above 65 536 envs (MI355X) run in up to 8 rounds, tables
                                     read through L2 from the third round on — and are launched over whole 8-step blocks (t0
                                     and n_steps multiples of 8) run with the step split between two wavefronts per 64 envs: a
                                     mover (actions, resolve_movement, horizon, flag bytes) running up to 16 steps ahead of
                                     an interact wavefront (resolve_interacts, env effects, rewards) through a ring in LDS.
                                     Same results bit for bit; the bit exists so that callers (and the parity tests) can
                                     cross-check the two formulations, as with OC_OPT_LANE_PAIR / OC_OPT_PREDICATE_INTERACT */

/* OcBatch.batch_flags */
#define OC_BATCH_TWO_PLAYERS 0x1u /* every layout of the table has exactly 2 players */
#define OC_BATCH_NEW_DYNAMICS 0x2u /* no layout of the table uses old_dynamics (mdp.py:1696-1701) */
#define OC_BATCH_NO_SHARED_FACES 0x8u /* in no layout of the table does a non-floor cell touch two floor cells: two players can
                                         never face the same cell (cramped_room), so the interact order needs no replay */
#define OC_BATCH_UNIFORM_SHAPING 0x4u /* every layout of the table has the same rew_shaping_params and old_dynamics flag:
                                         the interact table then carries the reward floats for the whole batch */

/* obs dtypes of oc_encode_lossless */
#define OC_OBS_U8 0
#define OC_OBS_F32 1

/* error codes */
#define OC_OK 0
#define OC_EINVAL (-1)
#define OC_ELAUNCH (-2)

/*
 * One compiled layout: terrain + the recipe/reward configuration of one OvercookedGridworld
 * (mdp.py:1090-1148) flattened to look-up tables.  256 bytes, 16-byte aligned.  The table is
 * built on the host by overcooked_ai_amd.layouts.compile_layout and uploaded once.
 *   cook_time[n_onion + 4*n_tomato]      = Recipe.time  (mdp.py:163-188)
 *   delivery_value[n_onion + 4*n_tomato] = get_recipe_value, non-discounted branch (mdp.py:1595-1602):
 *        0 if the recipe is not in all_orders, order_bonus*value if it is a bonus order, else value.
 *   terrain[c] = terrain code | (pot slot << 3) for cell c = y*W + x  (terrain_mtx[y][x], mdp.py:1783)
 */
typedef struct OcLayout {
    uint8_t width, height, n_cells, n_pots;
    uint8_t n_players, old_dynamics, n_obj_planes, reserved0;
    uint8_t start_pos[2];
    uint8_t start_or[2];
    uint8_t reserved1[4];
    uint8_t pot_cell[OC_MAX_POTS];
    uint8_t potting_class[8];   /* [n_onion + 3*n_tomato of the soup BEFORE the potting], low nibble: an onion is
                                   added, high nibble: a tomato; bit 0 optimal, 1 viable, 2 catastrophic, 3 useless
                                   (is_potting_*, mdp.py:2256-2308) */
    float rew_placement_in_pot; /* PLACEMENT_IN_POT_REW, mdp.py:1019 */
    float rew_dish_pickup;      /* DISH_PICKUP_REWARD */
    float rew_soup_pickup;      /* SOUP_PICKUP_REWARD */
    float reserved3;
    uint8_t cook_time[16];
    float delivery_value[16];
    uint8_t terrain[OC_MAX_CELLS];
} OcLayout;

/*
 * A batch of envs: which layouts they use and how many there are.  Host-side POD; the two d_ members
 * are device pointers.  All layouts of one table share width/height (pad smaller grids with counters,
 * as the reference's LayoutGenerator.embed_grid does, layout_generator.py:309-329).
 */
typedef struct OcBatch {
    const OcLayout* d_layouts;   /* [n_layouts] compiled layouts in HBM */
    const uint16_t* d_layout_id; /* [n_envs] layout index per env, or NULL when n_layouts == 1.  WRITTEN by the step kernels
                                    (and oc_regen_layouts) when an OcStartSpec with regen_count > 0 moves restarted envs
                                    to other layouts: keep it in writable device memory then */
    int64_t n_envs;
    int32_t n_layouts;
    int32_t width, height;       /* grid shape shared by every layout of the table */
    int32_t max_pots;            /* max n_pots over the table (1..8), or 0 if unknown: selects how many pot slots
                                    the step kernels keep in registers */
    uint32_t batch_flags;        /* OC_BATCH_* hints about the table */
    uint32_t max_free_cells;     /* max number of free (floor) cells over the table, or 0 if unknown: single two-player
                                    layouts with at most 7 free cells (cramped_room) step through a joint move table */
} OcBatch;

/*
 * max_pots, batch_flags and max_free_cells are HINTS that select kernel variants, and hard preconditions when set:
 * a max_pots below a layout's n_pots drops that layout's extra pots, OC_BATCH_TWO_PLAYERS on a one-player layout or a
 * max_free_cells below the real count index past the tables.  0 / unset is always safe.  oc_batch_hints derives them
 * from a HOST copy of the layout table (call it before uploading the table; it leaves the other fields alone).
 */
int oc_batch_hints(const OcLayout* h_layouts, int n_layouts, OcBatch* batch);

/*
 * How a finished env is restarted by OC_OPT_AUTO_RESET (and by oc_multi_agent_step): NULL = the standard start state
 * (get_standard_start_state, mdp.py:1297-1305); otherwise the start_state_fn of
 * OvercookedGridworld.get_random_start_state_fn(random_start_pos, rnd_obj_prob_thresh) (mdp.py:1307-1369) as
 * OvercookedEnv.reset uses it (env.py:288-319), drawn inside the step kernel with the stream documented at
 * oc_reset_random for global env g = env_offset + e and
 *      epoch of a restart at step k of the call = epoch + k      (k = 0 for single-step entry points),
 * so a caller that passes epoch = 1 + (steps executed so far) never reuses the draws of its initial
 * oc_reset_random(epoch 0) — for 2^32 - 1 steps per env: epoch is a 32-bit word and epoch + k is taken mod 2^32, inside a
 * call as well (a call that starts at epoch 2^32 - 3 draws its restart at step 5 from epoch 2); a caller that counts
 * further passes its counter mod 2^32, and the draws of epoch 0 come round again with step 2^32.
 * The other counters are used in their full 64-bit width: t0 (block index b = t >> 3 of the action stream), env_offset + e
 * and seed each enter the Philox counter or key as a low and a high 32-bit word, and env_offset + e carries from the low
 * word into the high one inside a batch.  t0 and env_offset are int64_t in the signatures and are reinterpreted as
 * uint64_t: a negative value is not refused, it names the counter 2^64 + value (t0 = -8 is block 2^61 - 1, steps
 * -8..-1, and the call's step 8 is global step 0; env_offset = -1 makes local env 0 global env 2^64 - 1 and local env 1
 * global env 0).  Supported by the table-driven kernels (oc_step and oc_step_many without
 * OC_OPT_PREDICATE_INTERACT — with or without event logging —, oc_rollout_random without OC_OPT_LANE_PAIR /
 * PREDICATE_INTERACT, oc_step_encode, oc_rollout_encode, oc_multi_agent_step); the others return OC_EINVAL.
 */
typedef struct OcStartSpec {
    uint64_t seed;
    int64_t env_offset;          /* global index of local env 0 (oc_rollout_random / oc_rollout_encode: must equal their
                                    env_offset argument) */
    uint32_t epoch;
    int32_t random_start_pos;    /* 0 / 1 */
    double rnd_obj_prob_thresh;  /* 0 .. 1 */
    /* Per-episode layout re-draw = OvercookedEnv.reset(regen_mdp=True) over an mdp_generator_fn that yields a different
     * layout every time (env.py:288-302; LayoutGenerator, layout_generator.py:110-160 — BASELINE configs[4]): with
     * regen_count > 0 an env that restarts first moves to layout
     *      regen_first + mulhi32(word 0 of block 15 of the reset stream of oc_reset_random, regen_count)
     * (same epoch as its start-state draws), the new id is stored in OcBatch.d_layout_id[e], and the start state (standard,
     * or drawn per the two fields above) is that of the NEW layout.  regen_first + regen_count <= n_layouts; 0 = off. */
    uint32_t regen_first;
    uint32_t regen_count;
} OcStartSpec;

/*
 * Where the event_infos of a call go (EVENT_TYPES, mdp.py:1027-1058; log_object_* / is_*_useful / is_potting_*,
 * mdp.py:2121-2308); NULL = no event logging.  Bit 2*k + p of a mask is event_infos[EVENT_TYPES[k]][p].
 *   d_events       [n_steps][n_envs] u64: the mask of every step, or NULL
 *   d_counts       [n_envs][25] u32: how often each event happened in the env's RUNNING episode — player 0 in bits
 *                  0..15, player 1 in bits 16..31 (the lengths of game_stats[event][player], env.py:382-401; what
 *                  RLlib reports per agent, human_aware_rl/rllib/rllib.py:453-483).  Accumulated across calls by the
 *                  step kernels; zeroed when the env is auto-reset.  Or NULL
 *   d_counts_done  [n_envs][25] u32: the counts of the last FINISHED episode (ep_game_stats), written at the step that
 *                  ends it, or NULL
 */
typedef struct OcEventSink {
    uint64_t* d_events;
    uint32_t* d_counts;
    uint32_t* d_counts_done;
} OcEventSink;

int oc_abi_version(void);
size_t oc_layout_size(void); /* == sizeof(OcLayout) == 256 */
const char* oc_last_error(void);
/* number of 16-byte planes per env for a width x height grid: 1 + ceil(width*height/16) */
int oc_state_planes(int width, int height);

/*
 * oc_step — one joint transition for n_envs independent envs.
 * Replaces OvercookedGridworld.get_state_transition (mdp.py:1375-1430) = resolve_interacts (1432)
 * -> resolve_movement (1644) -> step_environment_effects (1691), plus OvercookedEnv.step's
 * done/bookkeeping (env.py:244-274, 321-325, 382-392).
 *   d_state_in/out [oc_state_planes * n_envs] 16-byte words; may alias (in-place step)
 *   d_actions      [n_envs][2] action indices 0..5 (player 0, player 1)
 *   d_rewards      [n_envs][4] float: sparse_reward_by_agent[0..1], shaped_reward_by_agent[0..1]; 16-byte aligned (every
 *                  kernel writes a row as one 16-byte store)
 *   d_flags        [n_envs] OC_F_* bits; any address (written a byte at a time)
 *   d_ep_returns   [n_envs][4] float running sums of d_rewards over the episode
 *                  (game_stats cumulative_*_rewards_by_agent, env.py:387-392); 16-byte aligned, or NULL
 * A d_rewards or d_ep_returns that is not 16-byte aligned is OC_EINVAL, here and in every entry point below that takes one
 * (oc_step_many, oc_rollout_random, oc_rollout_record, oc_rollout_record_ex, oc_step_encode, oc_rollout_encode, oc_rollout_featurize,
 * oc_multi_agent_step with its d_ep_returns_out, oc_multi_agent_step_featurize, oc_step_server_open, oc_step_server_play), before
 * any device call.
 *   d_events       [n_envs] u64 event_infos of this step (EVENT_TYPES, mdp.py:1027-1058): bit 2*k + p is
 *                  event_infos[EVENT_TYPES[k]][p]; or NULL (shorthand for an OcEventSink with only d_events)
 *   events         per-episode event counters / masks (OcEventSink), or NULL
 *   horizon        done when timestep >= horizon (1..65535; the stored timestep is a u16 that saturates at 65535 — the
 *                  Python OvercookedEnv keeps the reference's default horizon of 1e10 but raises at that limit)
 * In place (d_state_out == d_state_in) without event logging, on grids of at most 64 cells, the step runs on the wire format
 * itself (k_step1: header + changed object bytes written back, <= 4.3 us per batched step of 65 536 envs, launch-bound); other
 * forms unpack the env (k_step3, 5.7-7.0 us).  Same results.
 */
int oc_step(const OcBatch* batch, const void* d_state_in, void* d_state_out, const uint8_t* d_actions,
            float* d_rewards, uint8_t* d_flags, float* d_ep_returns, uint64_t* d_events, int horizon,
            uint32_t options, const OcStartSpec* start, const OcEventSink* events, void* stream);

/*
 * oc_step_many — n_steps consecutive oc_step transitions (in place) in ONE launch: step k consumes
 * d_actions[k][n_envs][2] and writes d_rewards[k][n_envs][4], d_flags[k][n_envs]; the envs stay on chip between the
 * steps (replaying a fixed joint plan or a pre-sampled action tensor: OvercookedEnv.execute_plan, env.py:334-345;
 * AgentEvaluator._check_trajectories_dynamics, benchmarking.py:366).  Results are those of n_steps oc_step calls.
 * d_rewards and d_ep_returns (or NULL) 16-byte aligned, d_flags at any address, as for oc_step.
 */
int oc_step_many(const OcBatch* batch, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                 float* d_ep_returns, int n_steps, int horizon, uint32_t options, const OcStartSpec* start,
                 const OcEventSink* events, void* stream);

/*
 * oc_rollout_random — n_steps transitions per launch under the uniform random policy
 * (the reference's RandomAgent(all_actions=True) pair, agents/agent.py:223), actions drawn
 * in-kernel.  One Philox4x32-10 block feeds 8 consecutive steps: with b = t >> 3, s = t & 7,
 *      r[0..3] = philox4x32_10(counter = {b_lo, g_lo, g_hi, b_hi}, key = {seed_lo, seed_hi}),
 *      x = r[s >> 1] * (s & 1 ? 36 : 1)  (mod 2^32),
 *      action of player 0 = mulhi32(x, 6),  action of player 1 = mulhi32(x * 6 mod 2^32, 6)
 * for global env g at global step t (base-6 digits of the 32-bit word; bias < 6^4 / 2^32).
 * Same transition function as oc_step; state stays on chip between the fused steps.  A launch costs ~16 us outside its
 * step loop (table staging, state load / store, dispatch): 12 % of a 400-step launch of 65 536 envs, 1.5 % of a 4 000-step
 * one (207 vs 244 G env-steps/s on MI355X) — prefer few long launches.
 * Launch shape and speed: the mover / interact kernel works in whole 8-step blocks of whole 256-env workgroups; a long call off that
 * step grid (t0 or n_steps not a multiple of 8) is split inside the call — head and tail steps through the one-wavefront kernels —, a
 * ragged batch takes the one-wavefront kernels altogether (oc_rollout_plan says which instance a call takes).
 *   d_rewards  [n_steps][n_envs][4] or NULL;  d_flags [n_steps][n_envs] or NULL ([n_steps / 8][n_envs][8] with OC_OPT_FLAGS_TILED8)
 *              alignment: d_rewards and d_ep_returns 16 bytes (rows written as 16-byte stores: OC_EINVAL otherwise); d_flags any
 *              address ([step][env] flags are written a byte at a time), 8 bytes with OC_OPT_FLAGS_TILED8 (tiles are 8-byte stores)
 *   env_offset global index of local env 0 (multi-GPU shards draw disjoint streams)
 *   t0         global step index of the first fused step
 */
int oc_rollout_random(const OcBatch* batch, void* d_state, float* d_rewards, uint8_t* d_flags,
                      float* d_ep_returns, int horizon, uint32_t options, uint64_t seed,
                      int64_t env_offset, int64_t t0, int n_steps, const OcStartSpec* start,
                      const OcEventSink* events, void* stream);

/*
 * oc_rollout_record — oc_rollout_random (same arguments, same Philox stream, same results in d_state, d_rewards, d_flags,
 * d_ep_returns and the start-state epochs) that also records what each step acted on: the trajectory of
 * OvercookedEnv.get_rollouts / AgentEvaluator.evaluate_random_pair (env.py:485-580), its ep_states and ep_actions.
 *   d_actions_out  [n_steps][n_envs][2] u8: the action indices (Action.INDEX_TO_ACTION) drawn at step k of the call — the
 *                  d_actions layout of oc_step_many / oc_rollout_encode, so a recording replays through them; 2-byte aligned, or NULL
 *   d_states_out   [n_steps][n_planes][n_envs][16] (oc_state_planes): slice k is the packed state step k ACTS ON — the pre-step
 *                  state, after the previous step's restart (slice 0 = d_state on entry; the state after the last step is d_state
 *                  on return); each slice is a packed-state array of its own (oc_encode_lossless, oc_featurize, ...); 16-byte
 *                  aligned, or NULL.  Not both NULL.
 *   d_rewards, d_flags: optional, as in oc_rollout_random (d_rewards and d_ep_returns 16-byte aligned, d_flags at any address).  recorded bytes per env-step: 16 per plane + 2 + 16 + 1 — 67 on grids of
 *                  17..32 cells (cramped_room: 48 state, 2 actions, 16 rewards, 1 flags), 83 on 33..48 (asymmetric_advantages).
 * Runs the one-wavefront arithmetic-movement kernel (k_rollout4, MODE 0) with recording stores.  options: OC_OPT_AUTO_RESET;
 * OC_OPT_ONE_WAVEFRONT is accepted and has no effect; any other bit (OC_OPT_FLAGS_TILED8, OC_OPT_LANE_PAIR,
 * OC_OPT_PREDICATE_INTERACT, ...) is OC_EINVAL, as are a start spec with regen_count > 0 (a re-drawn layout would have to be
 * recorded per step too) and a table without OC_BATCH_TWO_PLAYERS.  All checks run before any device call.
 */
int oc_rollout_record(const OcBatch* batch, void* d_state, uint8_t* d_actions_out, void* d_states_out, float* d_rewards,
                      uint8_t* d_flags, float* d_ep_returns, int horizon, uint32_t options, uint64_t seed,
                      int64_t env_offset, int64_t t0, int n_steps, const OcStartSpec* start, void* stream);

/*
 * Where oc_rollout_record_ex records each step k of the call.
 *   d_actions     [n_steps][n_envs][2] u8, as d_actions_out of oc_rollout_record; 2-byte aligned, or NULL
 *   d_states      [n_steps][n_planes][n_envs][16], as d_states_out of oc_rollout_record; 16-byte aligned, or NULL
 *   d_layout_ids  [n_steps][n_envs] u16: the layout id of the state in d_states slice k — the env's id after step k - 1's restart
 *                 and layout re-draw (slice 0: OcBatch.d_layout_id on entry; 0 for a one-layout table); 2-byte aligned, or NULL
 */
typedef struct OcRecordSink {
    uint8_t* d_actions;
    void* d_states;
    uint16_t* d_layout_ids;
} OcRecordSink;

/*
 * oc_rollout_record_ex — oc_rollout_record with the event log and per-episode layout re-draws: the complete trajectory of
 * OvercookedEnv.get_rollouts (env.py:485-580) with each episode's game_stats (env.py:382-401: the event lists of ep_game_stats
 * come from the per-step masks or the counters of `events`), on layouts re-drawn at every restart (start->regen_count > 0:
 * OvercookedEnv.reset(regen_mdp=True), env.py:288-302), each step labelled with its layout in rec->d_layout_ids.
 * With the same arguments, start spec and event sink it gives the results of oc_rollout_random: d_state, d_rewards, d_flags,
 * d_ep_returns, OcBatch.d_layout_id after re-draws, the event masks and counters, the Philox stream and the start-state epochs.
 * recorded bytes per env-step with every array: 16 per plane + 2 (actions) + 2 (layout ids) + 8 (event mask) + 17 (rewards,
 * flags) — 77 on grids of 17..32 cells (cramped_room), 93 on 33..48 (asymmetric_advantages, 9 x 5 tables).
 * Runs the one-wavefront arithmetic-movement kernel (k_rollout4, MODE 0) with recording stores, and with the event log when
 * `events` names masks or counters.  options: OC_OPT_AUTO_RESET; OC_OPT_ONE_WAVEFRONT is accepted and has no effect.  OC_EINVAL,
 * before any device call: any other option bit, a table without OC_BATCH_TWO_PLAYERS, rec NULL or all three of its arrays NULL,
 * a misaligned array (rec's, d_rewards or d_ep_returns: 16 bytes, as in oc_rollout_random), and the start-spec errors of oc_rollout_record (but for regen_count, which is accepted).
 */
int oc_rollout_record_ex(const OcBatch* batch, void* d_state, const OcRecordSink* rec, float* d_rewards, uint8_t* d_flags,
                         float* d_ep_returns, int horizon, uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0,
                         int n_steps, const OcStartSpec* start, const OcEventSink* events, void* stream);

/*
 * oc_encode_lossless — the 26-layer observation of both players.
 * Replaces OvercookedGridworld.lossless_state_encoding (mdp.py:2385-2561) as called through
 * OvercookedEnv.lossless_state_encoding_mdp (env.py:276-280).
 *   d_obs  [n_envs][2][W][H][26] of u8 or f32 (index [x][y][layer], mdp.py:2415-2418, 2550); 16-byte aligned
 */
int oc_encode_lossless(const OcBatch* batch, const void* d_state, void* d_obs, int obs_dtype, int horizon,
                       void* stream);

/*
 * oc_step_encode — oc_step (in place, caller's actions, auto-reset per `options`, drawn start states per `start`)
 * followed by oc_encode_lossless of the resulting states, i.e. the step of a training / evaluation loop that feeds the
 * lossless observation to a policy: OvercookedEnv.step (env.py:244) + lossless_state_encoding_mdp of the state the next
 * step starts from (env.py:276; human_aware_rl/rllib/rllib.py:257-260).  One C call enqueues the two kernels back to
 * back on `stream`; with OC_OPT_ONE_KERNEL (and no `start`) it is oc_rollout_encode with n_steps = 1 — a wash for a
 * single step (36.4 vs 37.2 us on 65 536 asymmetric_advantages envs, 25.1 vs 24.4 us on cramped_room), the gain of the
 * single kernel comes with several steps per launch.  Arguments as in oc_step / oc_encode_lossless.
 */
int oc_step_encode(const OcBatch* batch, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                   float* d_ep_returns, void* d_obs, int obs_dtype, int horizon, uint32_t options,
                   const OcStartSpec* start, void* stream);

/*
 * oc_rollout_encode — n_steps transitions AND the lossless observation after each of them, in one call: BASELINE
 * configs[2] (the rollout of configs[1] "plus oc_encode_lossless every step"), i.e. a trajectory of
 * (reward, flag, observation) per step as a rollout collector (OvercookedEnv.run_agents / get_rollouts, env.py:425-580,
 * over step 244 + lossless_state_encoding_mdp 276) gathers it.
 *   d_actions  NULL: the uniform random policy, the Philox stream of oc_rollout_random (seed, env_offset, t0);
 *              else [n_steps][n_envs][2] action indices as for oc_step_many (illegal: flagged, env untouched)
 *   d_rewards  [n_steps][n_envs][4] / d_flags [n_steps][n_envs] (may be NULL with the random policy)
 *              d_rewards and d_ep_returns 16-byte aligned, d_flags at any address (as for oc_step; oc_step_encode too)
 *   d_obs      observation of step k at (char*)d_obs + k * obs_step_stride: [n_envs][2][W][H][26] of obs_dtype, the state
 *              the NEXT step starts from (after an auto-reset: the start state), exactly what oc_step_encode emits;
 *              obs_step_stride in bytes, a multiple of 16; 0 = every step overwrites the same observation
 *   options    OC_OPT_AUTO_RESET, OC_OPT_ONE_KERNEL;  start: as for oc_rollout_random (NULL = standard start states; a
 *              restart at step k draws from epoch start->epoch + k)
 * One layout, at most two pots, at least two steps and a batch that fills the GPU run as ONE kernel
 * (k_rollout_encode: the env stays on chip for all steps, every wavefront encodes its own 64 envs through a private
 * LDS image, no workgroup barrier in the step loop): 30 us per step on 65 536 asymmetric_advantages envs, the rate at
 * which the observation bytes alone reach HBM (two one-step kernels: 37 us).  Any other case runs the one-step kernels
 * step by step with identical results.
 */
int oc_rollout_encode(const OcBatch* batch, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                      float* d_ep_returns, void* d_obs, int obs_dtype, int64_t obs_step_stride, int horizon,
                      uint32_t options, uint64_t seed, int64_t env_offset, int64_t t0, int n_steps,
                      const OcStartSpec* start, void* stream);

/*
 * oc_featurize — the hand-crafted feature vector of both players.
 * Replaces OvercookedGridworld.featurize_state (mdp.py:2579-2898) as called through
 * OvercookedEnv.featurize_state_mdp (env.py:282-286); needs 2-player layouts.
 *   d_plan_blob / d_plan_off  per-layout motion-cost tables built on the host by overcooked_ai_amd.planner
 *       (the MotionPlanner distances of planning/planners.py:391-423): at byte d_plan_off[layout] of the blob,
 *       floor_index[128] (cell -> index among the free cells, row-major) followed by
 *       cost[(floor_index[cell] * 4 + orientation) * row_stride + feature_cell] = fewest actions to stand next to the
 *       feature facing it, 255 = unreachable or not a motion goal (counters outside MotionPlanner.counter_goals);
 *       row_stride = n_cells rounded up to a multiple of 16 (rows are fetched as 16-byte words), padding = 255.
 *       ABI 4: d_plan_off holds 2 * n_layouts entries; at byte d_plan_off[n_layouts + layout] starts the layout's WALK
 *       SECTION, {u32 record_stride, 12 pad bytes} + one record per (free cell, orientation) state: what a walk over the
 *       whole grid would find as far as it depends on the terrain alone — u32[4] arg-min keys (cost << 9 | cell,
 *       0xFFFFFFFF = none) of the closest onion / tomato / dish dispenser and serving cell, u32[4] the four closest pots in
 *       ascending key order, u8 n + u8[n] the goal counters in ascending (cost, cell) order (planner.walk_records)
 *   d_features  [n_envs][2][2 * (num_pots * 10 + 26) + 4] float32, 16-byte aligned; row i = features for player i
 *   num_pots    0..4 (the reference's default is 2 -> 96 features)
 * Ties between equally cheap counter objects are broken by cell order (row-major); the reference breaks them by the
 * insertion order of its objects dict, which the packed state does not carry.
 */
int oc_featurize(const OcBatch* batch, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const void* d_state,
                 float* d_features, int num_pots, void* stream);

/*
 * oc_rollout_featurize (ABI 6: an entry point added beside the others) — n_steps transitions AND featurize_state of both
 * players after each of them, in one call: the trajectory of (reward, flag, features) per step that a behaviour-cloning data
 * collection or evaluation rollout gathers (OvercookedEnv.featurize_state_mdp per step, env.py:282-286; the "bc" observation of
 * OvercookedMultiAgent, rllib.py).  The counterpart of oc_rollout_encode for the other observation; argument for argument as there.
 *   d_plan_blob / d_plan_off  the motion-cost tables of oc_featurize
 *   d_actions   NULL: the uniform random policy, the Philox stream of oc_rollout_random (seed, env_offset, t0);
 *               else [n_steps][n_envs][2] action indices as for oc_step_many (illegal: flagged OC_F_BAD_ACTION, the env
 *               untouched, its features recomputed unchanged); caller actions need d_rewards and d_flags
 *   d_rewards   [n_steps][n_envs][4] / d_flags [n_steps][n_envs] (may be NULL with the random policy)
 *               d_rewards and d_ep_returns 16-byte aligned, d_flags at any address (as for oc_step)
 *   d_features  features of step k at (char*)d_features + k * feat_step_stride: [n_envs][2][2 * (num_pots * 10 + 26) + 4]
 *               float32 of the state the NEXT step starts from (after an auto-reset: the start state), exactly what oc_featurize
 *               of d_state after step k gives; feat_step_stride in bytes, a multiple of 16; 0 = every step overwrites one buffer
 *   num_pots    0..4, as for oc_featurize, whose every check applies (two-player layouts, 16-byte alignment)
 *   options     OC_OPT_AUTO_RESET, OC_OPT_ONE_KERNEL (any other bit: OC_EINVAL);  start: as for oc_rollout_encode (a restart at
 *               step k draws from epoch start->epoch + k; start->env_offset must equal env_offset)
 * One layout of at most 64 cells with one or two pots, at least two steps and a batch of at least 64 envs per CU (or
 * OC_OPT_ONE_KERNEL) run as ONE kernel (k_rollout_featurize: the env stays on chip for all steps, every wavefront featurizes its
 * own 64 envs through a private int16 LDS image, no workgroup barrier in the step loop).  Any other case runs the one-step entry
 * points and oc_featurize step by step with identical results.  Every check is made before any device call.
 */
int oc_rollout_featurize(const OcBatch* batch, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, void* d_state,
                         const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags, float* d_ep_returns,
                         float* d_features, int64_t feat_step_stride, int num_pots, int horizon, uint32_t options,
                         uint64_t seed, int64_t env_offset, int64_t t0, int n_steps, const OcStartSpec* start, void* stream);

/*
 * oc_shape_rewards — the per-agent training reward of the RLlib environment.
 * Replaces the reward arithmetic of OvercookedMultiAgent.step (human_aware_rl/rllib/rllib.py:306-329):
 *      out[e][i] = (sparse0 + sparse1) + reward_shaping_factor * dense_i
 * with dense_i = phi_next[e] - phi_cur[e] for both agents when d_phi_next != NULL (use_phi), else the shaped
 * reward of agent i from d_rewards.  float64, like the reference's Python floats.
 *   d_rewards [n_envs][4], d_flags [n_envs]   as written by oc_step
 *   d_phi_next [n_envs] phi(s') (oc_potential after the step, before any reset), or NULL
 *   d_phi_cur  [n_envs] in: phi(s); out: the potential of the state the next step starts from — phi(s'), or
 *              d_phi_start[layout] where the episode is done (the caller resets those envs with d_done as the mask)
 *   d_phi_start [n_layouts] potential of each layout's standard start state
 *   d_out  [n_envs][2] float64, 16-byte aligned;  d_done [n_envs] 1 where OC_F_DONE is set, or NULL
 */
int oc_shape_rewards(const OcBatch* batch, const float* d_rewards, const uint8_t* d_flags, const double* d_phi_next,
                     double* d_phi_cur, const double* d_phi_start, double reward_shaping_factor, double* d_out,
                     uint8_t* d_done, void* stream);

/*
 * oc_multi_agent_step — one step of the RLlib training environment, enqueued by a single call.
 * Replaces OvercookedMultiAgent.step (human_aware_rl/rllib/rllib.py:293-342) for a batch: oc_step (no auto-reset) ->
 * oc_potential on s' (when d_phi_tables != NULL: use_phi) -> oc_shape_rewards -> copy of the episode returns ->
 * oc_reset of the finished envs (mask = d_done) -> oc_encode_lossless of the states the next step starts from
 * (when d_obs != NULL).  Arguments as in those entry points (d_rewards, d_ep_returns and d_ep_returns_out 16-byte aligned: float4
 * rows; d_flags and d_done at any address; OC_EINVAL otherwise); d_done is required.  Two-player tables with at most two
 * pots run everything before the encoding as one kernel (k_train_step) with identical results.  With `start`, finished
 * envs restart from drawn start states and d_phi_cur receives the potential of those.
 * ABI 5, round 5: with d_obs, ONE layout on a grid of at most 64 cells, no event sink and a batch that gives at least half
 * of the CUs a workgroup (>= 32 768 envs on MI355X) the whole call is ONE kernel (k_train_step_obs, csrc/train_obs.hpp: eight
 * wavefronts per 256 envs — four step and restart, four compute phi and the shaped rewards, all eight encode and stream the
 * observations): 65 536 cramped_room envs with u8 observations 26.2 -> 20.3 us per call, asymmetric_advantages 37.6 -> 30.7 us
 * (profiles/r05_train_step_obs.txt); same results bit for bit.
 * The paths, chosen once per call by one planner (oc_multi_agent_plan below says which one a call takes, and which kernel
 * instance of it): k_train_step_obs<MAXP, T, NWV> (the step and its observation; ABI 5 above) — k_train_step1<UNIFORM, MAXP,
 * LAY_LDS> (two players, at most two pots, at most 64 cells, no event sink: the whole step in one kernel on the wire format, then
 * oc_encode_lossless) — k_train_step<UNIFORM, EV> (the same with event counters or on 65..128 cells) — the sequence of entry
 * points listed first (any other table).
 */
int oc_multi_agent_step(const OcBatch* batch, void* d_state, const uint8_t* d_actions, float* d_rewards,
                        uint8_t* d_flags, float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                        const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next,
                        double* d_phi_cur, const double* d_phi_start, double reward_shaping_factor, double* d_shaped,
                        uint8_t* d_done, void* d_obs, int obs_dtype, int horizon, const OcStartSpec* start,
                        const OcEventSink* events, void* stream);

/*
 * oc_reset_random — randomized start states drawn on the GPU.
 * Replaces the start_state_fn of OvercookedGridworld.get_random_start_state_fn(random_start_pos,
 * rnd_obj_prob_thresh) (mdp.py:1307-1369) as used by OvercookedEnv.reset (env.py:288-319) for training-time
 * diversity.  Same distribution as the reference: joint positions uniform over ordered tuples of distinct free cells
 * (orientation NORTH), each pot filled with probability thresh (n = 1..3 onions, then 0..3-n tomatoes; cooking from
 * tick 0 with probability thresh, else idle), each player holding an object with probability thresh (dish 0.2,
 * onion 0.6, finished soup 0.2 with the same ingredient draw).  The draws come from this library's counter-based
 * stream, not from numpy's global generator (the numpy-exact version stays on the host:
 * overcooked_ai_amd.mdp.OvercookedGridworld.get_random_start_state_fn):
 *      block(b) = philox4x32_10(counter = {epoch, g_lo, g_hi, b}, key = {seed_lo, seed_hi ^ 0x52535421})
 *      b = 0: word 0 -> joint position index mulhi(word, n_joint) into the row-major product of free cells
 *      b = 1 + i (player i): {u, kind, n, m}: holds iff u < T; kind < 858993459 dish, < 3435973836 onion, else soup;
 *                            n_onion = 1 + mulhi(n, 3), n_tomato = mulhi(m, 4 - n_onion)
 *      b = 3 + k (pot k):    {u, n, m, q}: filled iff u < T, with n_onion and n_tomato from n and m as above; cooking
 *                            (tick 0) iff q < T, else idle (tick -1)
 *      T = floor(rnd_obj_prob_thresh * 2^32)       (1.0 gives 2^32: every 32-bit word is below it)
 * for global env g = env_offset + e, with mulhi(a, b) = floor(a * b / 2^32).  In full:
 *   - a block's words are the four output words of philox4x32_10 in order ({u, kind, n, m} = words 0..3); the key's high
 *     word is seed_hi ^ 0x52535421 whatever the block, and epoch is the 32-bit word the caller passes (OcStartSpec);
 *   - the free cells are the layout's floor cells (' ' in its grid, the players' start cells among them) in row-major order,
 *     cell y * width + x; with F of them and two players n_joint = F * (F - 1) and index j names the ordered pair of distinct
 *     cells (a, b'): a = j / (F - 1), b = j % (F - 1), b' = b + (b >= a); with one player n_joint = F and the cell is j.
 *     Without random_start_pos the players stand on the layout's start cells and block 0 is not drawn.  Orientation NORTH;
 *   - pot k is the layout's k-th pot cell in row-major order; a soup's ingredients are its onions, then its tomatoes; a
 *     held soup is finished (cooking tick = its recipe's cook time);
 *   - with rnd_obj_prob_thresh = 0 no block but block 0 is drawn: empty hands, empty pots;
 *   - no object lies on a counter, timestep 0, and the episode returns of the env are cleared.
 * d_mask as in oc_reset.
 */
int oc_reset_random(const OcBatch* batch, void* d_state, const uint8_t* d_mask, float* d_ep_returns, uint64_t seed,
                    int64_t env_offset, uint32_t epoch, int random_start_pos, double rnd_obj_prob_thresh,
                    void* stream);

/*
 * oc_regen_layouts — new layout ids for the envs an explicit reset is about to restart (regen_mdp=True semantics for
 * oc_reset / oc_reset_random: call this first, then the reset with the same mask).  Env e is selected when d_mask is NULL
 * or (d_mask[e] & mask_bits) != 0 — mask_bits = OC_F_RESET selects from a flags array the envs a step has just restarted;
 * its new id is the draw documented at OcStartSpec for (start->seed, start->env_offset + e, start->epoch).
 *   d_layout_id  [n_envs], writable; start->regen_count > 0 required
 */
int oc_regen_layouts(const OcBatch* batch, uint16_t* d_layout_id, const uint8_t* d_mask, uint8_t mask_bits,
                     const OcStartSpec* start, void* stream);

/*
 * oc_potential — phi(s), the potential used for potential-based reward shaping.
 * Replaces OvercookedGridworld.potential_function(state, mp, gamma) (mdp.py:2920-3238) as called by
 * get_state_transition(display_phi=True) (mdp.py:1421-1429) for `phi_s` / `phi_s_prime`, which the RLlib
 * environment turns into the dense reward gamma * phi_s_prime - phi_s (human_aware_rl/rllib/rllib.py:314-319).
 *   d_plan_blob / d_plan_off  the motion-cost tables of oc_featurize (any counter_goals: only pots and serving
 *       cells are looked up)
 *   d_phi_tables [n_layouts][oc_phi_table_size()] per-layout records for ONE discount factor, built on the host by
 *       overcooked_ai_amd.potential.pack_phi_tables (layout documented there): steady-state value, the best
 *       completion of every ingredient multiset (_get_optimal_possible_recipe, mdp.py:1976-2016), gamma ** k;
 *       8-byte aligned
 *   d_phi  [n_envs] float64
 * Arithmetic is float64 in the reference's operand order without contraction: results are bit-identical to the
 * reference under CPython 3.8-3.12 (whose set iteration order decides ties between partially full pots,
 * mdp.py:1882-1890).
 */
int oc_potential(const OcBatch* batch, const uint8_t* d_plan_blob, const uint32_t* d_plan_off,
                 const uint8_t* d_phi_tables, const void* d_state, double* d_phi, void* stream);
int oc_phi_table_size(void);

/*
 * oc_reset — write the standard start state (OvercookedGridworld.get_standard_start_state,
 * mdp.py:1297-1305: players at start positions facing NORTH, no objects, timestep 0) into every
 * env whose d_mask byte is non-zero (all envs when d_mask is NULL).  Replaces OvercookedEnv.reset
 * (env.py:288-319) for the default start_state_fn.  d_ep_returns (nullable) is zeroed for reset envs.
 */
int oc_reset(const OcBatch* batch, void* d_state, const uint8_t* d_mask, float* d_ep_returns, void* stream);

/*
 * oc_mailbox_* — ONE env stepped per call without a kernel launch per call: what the reference's
 * OvercookedEnv.step (overcooked_env.py:244) -> OvercookedGridworld.get_state_transition (overcooked_mdp.py:1375) does for
 * an agent loop.  oc_mailbox_open starts a resident one-wavefront kernel that serves transitions of the batch's single
 * layout from a 4 KiB mailbox in pinned, GPU-mapped host memory; the caller writes the packed state (oc_state_planes()
 * planes of 16 bytes, as [plane][16]) at OC_MB_STATE_IN and the two action indices at OC_MB_ACTIONS of oc_mailbox_buffer(),
 * calls oc_mailbox_step (which posts the request and spins until the kernel has answered: ~7 us instead of the ~16 us of a
 * launch + stream wait) and reads the next state at OC_MB_STATE_OUT, float rewards[4] = (sparse0, sparse1, shaped0, shaped1) at
 * OC_MB_REWARDS, the OC_F_* flags (u32; DONE when the new timestep >= horizon, BAD_ACTION leaves the state as it was) at
 * OC_MB_FLAGS and the event_infos mask (u64, bit 2*k + p) at OC_MB_EVENTS.  Same transition, bit for bit, as oc_step.
 * The kernel leaves on its own after ~2 ms without a request (and after ~2 s in any case) and is relaunched by the next
 * oc_mailbox_step, so a device-wide synchronisation elsewhere waits at most that long.  One layout (batch.n_layouts == 1),
 * grids of at most 64 cells; not thread-safe per mailbox.  Returns OC_EINVAL for other batches (use oc_step).
 */
typedef struct OcMailbox OcMailbox;
#define OC_MB_STATE_IN 256
#define OC_MB_ACTIONS 336
#define OC_MB_STATE_OUT 512
#define OC_MB_REWARDS 592
#define OC_MB_FLAGS 608
#define OC_MB_EVENTS 616
int oc_mailbox_open(const OcBatch* batch, int horizon, OcMailbox** mailbox);
void* oc_mailbox_buffer(OcMailbox* mailbox);
int oc_mailbox_step(OcMailbox* mailbox);
int oc_mailbox_close(OcMailbox* mailbox);

/*
 * The resident batched step (ABI 6) — OvercookedEnv.step (overcooked_env.py:244-274) for the whole batch WITHOUT a launch per step.
 * oc_step costs a dependent kernel boundary plus its own load -> transition -> store chain per call (4.5 us for 65 536 envs); a
 * caller that lives on the GPU (a persistent policy kernel, the last kernel of a forward pass) can instead talk to a resident
 * kernel that keeps the envs in registers / LDS between steps, through per-env mailboxes in device memory:
 *   request   uint64 [n_envs]     low word  a0 | a1 << 8 (| OC_SV_STOP) [| caller's XCD << 20 | 1 << 24: lets the server look
 *                                 through its L2 between device-scope looks when both ends share an XCD], high word = tag;
 *                                 ONE aligned 8-byte store per env,
 *                                 written through to device scope (gfx950: `global_store_dwordx2 ... sc1`)
 *   response  uint32 [n_envs][8]  {sparse0, sparse1, shaped0 (float bits), tag} {shaped1, flags (OC_F_*), info, tag}
 *                                 info = timestep (bits 0..15) | XCD the server's workgroup runs on (20..23) | 1 << 24;
 *                                 two aligned 16-byte stores by the server; a granule that shows the tag is complete
 * tag = 1, 2, 3, ... = the number of the step since the server was opened (every env is sent every step; a wavefront steps when
 * its 64 envs all show the next tag).  Readers poll with device-scope loads (`sc1`): plain loads may be served from the reader's
 * own L2.  The transition, the bookkeeping, OC_OPT_AUTO_RESET and the drawn starts of `start` (restart at step k: epoch
 * start->epoch + k - 1, as k consecutive oc_step calls) are oc_step's, bit for bit (tests/test_gpu_step_server.py).
 * While the server is resident the states live on chip: d_state / d_ep_returns are current again after oc_step_server_sync (or
 * close, or once the kernel has left by itself).  The kernel leaves after idle_ms without a request (0: 20 ms) and after life_s in
 * any case (0: 600 s), writing the states back; oc_step_server_resume / _play relaunch it.  Device-wide synchronisation
 * (hipDeviceSynchronize, torch.cuda.synchronize()) waits for it to leave — synchronise streams or events instead.
 * Not served: OcEventSink, OC_OPT_PREDICATE_INTERACT; the batch's workgroups (n_envs / 256) must fit the GPU at once.
 *   oc_step_server_play  the caller's side as a kernel on `stream` (k_step_client: lane = env; per step post the request, poll the
 *                        response, leave rewards [n_steps][n_envs][4] / flags [n_steps][n_envs]) for actions uint8
 *                        [n_steps][n_envs][2] — n_steps = 1: a drop-in oc_step; n_steps > 1: the parity tests' replay of
 *                        oc_step_many's inputs and bench.py's round-trip measurement.  Host-synchronous; elapsed_ms (or NULL)
 *                        receives the client kernel's duration (HIP events on `stream`).
 *   oc_step_server_steps steps served so far (the host's count; exact after _play / _sync)
 * One caller at a time: the entry points of a server are not thread-safe, and two clients must not play on it concurrently.
 * d_ep_returns (oc_step_server_open; or NULL) and d_rewards (oc_step_server_play) are 16-byte aligned, d_flags sits at any address.
 * The resident kernel reads d_state / d_ep_returns on a stream of its own whenever it is (re)launched — at _open, and at a _play /
 * _resume that finds it gone: work of the caller's on those arrays must be complete by then (_play waits for `stream` before a
 * relaunch; before _open and _resume the caller synchronises its stream itself).
 */
#define OC_SV_STOP 0x10000u
typedef struct OcStepServer OcStepServer;
int oc_step_server_open(const OcBatch* batch, void* d_state, float* d_ep_returns, int horizon, uint32_t options,
                        const OcStartSpec* start, double idle_ms, double life_s, OcStepServer** server);
void* oc_step_server_requests(OcStepServer* server);  /* device pointer, uint64 [n_envs] */
void* oc_step_server_responses(OcStepServer* server); /* device pointer, uint32 [n_envs][8] */
int oc_step_server_resume(OcStepServer* server);
int oc_step_server_play(OcStepServer* server, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags, int n_steps,
                        void* stream, float* elapsed_ms);
int oc_step_server_sync(OcStepServer* server);
int64_t oc_step_server_steps(OcStepServer* server);
int oc_step_server_close(OcStepServer* server);

/*
 * Measurement aid (round 4): nothing but oc_rollout_random's OUTPUT STORES — one lane per env, per step one reward quad
 * (16 bytes, zeros) at d_rewards[k][e] and one flag byte (0) at d_flags[k][e], same workgroup shape and row addressing as the
 * rollout kernels, no state, no game.  Timing it says what the [step][env] output format of oc_rollout_random admits on the
 * device at this batch size (MI355X, 65 536 envs: 370-375 G env-steps/s = 0.79-0.80 of the HBM peak on one box, and
 * sensitive to the loop around the stores: 352 G for tools/store_rate.hip's loop on the same box), i.e. the ceiling bench.py
 * reports next to the roofline.  d_flags may be NULL (quads only).  Leaves the arrays zeroed.
 * options (ABI 5): 0, or OC_OPT_FLAGS_TILED8 — the flags array in the tiled layout ([n_steps / 8][n_envs][8]: per 8-step block
 * one 8-byte store per lane into the block's tile row, as the kernels serving that layout write it; n_steps a multiple of 8,
 * d_flags 8-byte aligned and not NULL), so that the ceiling is reported in the layout the rollout was timed in.
 */
int oc_output_stores_only(int64_t n_envs, int n_steps, float* d_rewards, uint8_t* d_flags, uint32_t options, void* stream);

/*
 * oc_rollout_plan (ABI 6) — which kernel instance oc_rollout_random would launch for this batch and launch shape, as text
 * (e.g. "k_rollout5<LAY_LDS=true, FT8=true, OLD=false, BIG=false, EV=false> mover + interact wavefronts, 1 round(s), 130864 B LDS";
 * "> one pot slot, mover + ..." where max_pots == 1 selects the instance compiled for one pot).
 * oc_rollout_random plans every call before it launches anything (its argument checks, then the choice of kernels); this is that
 * plan, put into words instead of launched: every check applies, every choice is the one a real call gets, and the code that answers
 * holds no launch and no device pointer — so it also runs on a host without a GPU
 * (the device's SIMD count then defaults to MI355X's 1 024).  docs/DISPATCH.md is generated from it (tools/gen_dispatch_table.py)
 * and tests/test_dispatch_table.py keeps that file equal to what the library answers.
 *   with_outputs  1: d_rewards and d_flags are given; 0: both NULL
 *   event_sink    0 none, 1 per-episode counters (OcEventSink.d_counts), 2 per-step masks as well (d_events)
 *   start         NULL or the start-state description the call would carry
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_rollout_plan(const OcBatch* batch, int horizon, uint32_t options, int64_t t0, int n_steps, int with_outputs,
                    int event_sink, const OcStartSpec* start, char* out, size_t out_size);

/*
 * oc_multi_agent_plan (ABI 6: an entry point added beside the others; no existing signature, struct or option changes, so the
 * version stays, and a binding that wants it on an older ABI 6 library looks the symbol up) — which path, and which kernel instance of it, oc_multi_agent_step would run for this batch and these
 * arrays, as text: "k_train_step_obs<MAXP=1, T=u8, NWV=16> unit=1, G=7, 142096 B LDS",
 * "k_train_step1<UNIFORM=false, MAXP=2, LAY_LDS=true> + oc_encode_lossless", "k_train_step<UNIFORM=true, EV=true> + oc_encode_lossless",
 * "sequence: oc_step, oc_potential, oc_shape_rewards, copy of the episode returns, oc_reset, oc_encode_lossless"; up to and
 * including '>' the text is the instance's name and stable.  oc_multi_agent_step plans every call before it launches anything (its
 * argument checks, then the choice of path and instance) and launches from that plan; this is the same plan put into words: every
 * check applies (refusals carry oc_multi_agent_step's name), the code that answers is told which arrays a call has, not where they
 * are, and holds no launch — so it also runs on a host without a GPU (the device's SIMD count then defaults to MI355X's 1 024).
 * The call described has every required array (aligned) and both episode-return arrays, and
 *   with_obs      1: d_obs is given (16-byte aligned), of obs_dtype; 0: NULL
 *   use_phi       1: the phi tables, the plan tables and the three phi buffers are given; 0: d_phi_tables is NULL
 *   event_sink    0 none, 1 per-episode counters (OcEventSink.d_counts)
 *   start         NULL or the start-state description the call would carry
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_multi_agent_plan(const OcBatch* batch, int horizon, int with_obs, int obs_dtype, int use_phi, int event_sink,
                        const OcStartSpec* start, char* out, size_t out_size);

/*
 * oc_observation_plan (ABI 6: an entry point added beside the others, as oc_multi_agent_plan was) — which kernel instance
 * oc_encode_lossless (n_steps == 0) or oc_rollout_encode (n_steps >= 1) would launch for this batch, as text; up to and including
 * '>' the text is the instance's name and stable:
 *   "k_encode_uniform<T=u8> unit=4, upg=4, grid=768, 47824 B LDS"       one layout, u8: envs per template, templates per group
 *   "k_encode<T=f32, LAY_LDS=true> epb=4, grid=16384, 37696 B LDS"       any table, u8 or f32: envs per workgroup
 *   "k_rollout_encode<MAXP=2, FAST=3, T=u8, NW=8> unit=4, G=4, 120336 B LDS, budget 158528 B (queried)"
 *                                                  one layout, at most two pots and 48 cells, u8 or f32, a batch that gives every
 *                                                  CU a workgroup (or OC_OPT_ONE_KERNEL): envs per template and per LDS image
 *   "step by step: oc_rollout_random + k_encode_uniform<T=u8> ..."       every other oc_rollout_encode call: per step the one-step
 *   "step by step: oc_step + k_encode<T=f32, LAY_LDS=true> ..."          entry point (oc_step with caller actions), then
 *                                                                       oc_encode_lossless, whose instance follows
 *   "nothing to launch (no envs)" / "nothing to launch (no steps)"
 * Both entry points plan a call before they launch anything (their argument checks, then every choice) and launch from that
 * plan; this is the same plan put into words: every check applies (a refusal returns its code, with the entry point's own
 * message in oc_last_error), the code that answers is told which arrays a call has, not where they are, and holds no launch.
 * The LDS budget k_rollout_encode's shape is chosen within is asked of the runtime ("queried"); on a host without a GPU the plan
 * assumes 144 KiB and says so ("fallback"; the device's SIMD count then defaults to MI355X's 1 024).
 * The call described has a state and a 16-byte aligned observation array (obs_step_stride a multiple of 16), env_offset equal
 * to the start spec's, and
 *   with_actions  1: d_actions is given; 0: NULL (the random policy)
 *   with_outputs  1: d_rewards and d_flags are given; 0: both NULL
 *   start         NULL or the start-state description the call would carry
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 * horizon, options, with_actions, with_outputs and start are not read when n_steps == 0.
 */
int oc_observation_plan(const OcBatch* batch, int obs_dtype, int horizon, uint32_t options, int n_steps, int with_actions,
                        int with_outputs, const OcStartSpec* start, char* out, size_t out_size);

/*
 * oc_step_plan (ABI 6: an entry point added beside the others, as oc_multi_agent_plan was) — which kernel instance oc_step
 * (entry 0), oc_step_many (entry 1) or oc_step_server_open (entry 2) would launch for this batch, as text; up to and including
 * '>' the text is the instance's name and stable:
 *   "k_step1<UNIFORM=true, MAXP=1, LAY_LDS=true, EVENTS=false> grid=10, 8192 B LDS"    one step on a grid of at most 64 cells, in
 *                                                                       place or out of place, with or without an event sink
 *   "k_step3<UNIFORM=false, MAXP=2, LAY_LDS=true, FAST=false, EVENTS=true> grid=..."   oc_step_many's K steps in one launch, and
 *                                                                       one step on 65..128 cells
 *   "k_step<UNIFORM=true, MAXP=2, LAY_LDS=true, EVENTS=false> grid=..."                OC_OPT_PREDICATE_INTERACT
 *   "k_step_server<UNIFORM=false, MAXP=8, LAY_LDS=false> grid=..."                     the resident step
 *   "step by step: oc_step + k_step<...> ..."                           oc_step_many with OC_OPT_PREDICATE_INTERACT: n_steps calls
 *   "nothing to launch (no envs)" / "nothing to launch (no steps)"
 * The three entry points plan a call before they launch anything (their argument checks, then the choice of the instance, the grid
 * and the dynamic LDS bytes) and launch from that plan; this is the same plan put into words: every check applies (a refusal
 * returns its code, with the entry point's own name in front of the message in oc_last_error), the code that answers is told which
 * arrays a call has, not where they are, and holds no launch — so it also runs on a host without a GPU.  One check is not made:
 * whether the GPU keeps every workgroup of the resident kernel resident at once is asked of the runtime when
 * oc_step_server_open launches, and refused there.  idle_ms and life_s are not part of the plan either.
 * The call described has every required array, and
 *   horizon, options   as the entry point takes them
 *   n_steps            oc_step_many's; not read for entries 0 and 2
 *   with_masks         1: per-step event masks are asked for (oc_step's d_events or OcEventSink.d_events); 0: not
 *   with_counts        1: per-episode counters (OcEventSink.d_counts); 0: not.  Neither is read for entry 2 (no event sink)
 *   start              NULL or the start-state description the call would carry
 *   out, out_size      caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_step_plan(const OcBatch* batch, int entry, int horizon, uint32_t options, int n_steps, int with_masks, int with_counts,
                 const OcStartSpec* start, char* out, size_t out_size);

/*
 * oc_potential_plan, oc_featurize_plan (ABI 6: entry points added beside the others, as oc_multi_agent_plan was) — which kernel
 * instance oc_potential / oc_featurize would launch for this batch (and this num_pots), as text; up to and including the
 * instance's name ('>' for k_featurize) the text is stable:
 *   "k_potential2 grid=10"                              every layout of the table has one or two pots (batch.max_pots 1 or 2)
 *   "k_potential grid=10"                               any other table, and withheld hints (batch.max_pots == 0: unknown)
 *   "k_featurize<LAY_LDS=true> grid=19, 78848 B LDS"    a table of at most 32 layouts, staged in LDS
 *   "k_featurize<LAY_LDS=false> grid=..."               a larger table, read through L2
 *   "nothing to launch (no envs)"
 * grid: oc_potential runs one lane per env, 256 envs per workgroup: ceil(n_envs / 256); oc_featurize two lanes per env, 128 envs
 * per workgroup: ceil(n_envs / 128), with 128 * (16 * state planes + 4 * (2 * (num_pots * 10 + 26) + 6)) bytes of dynamic LDS
 * (the envs' states and their int16 feature rows; oc_potential asks for none).
 * Both entry points plan a call before they launch anything (their argument checks, then the choice of the instance, the grid and
 * the dynamic LDS bytes) and launch from that plan; this is the same plan put into words: every check applies (num_pots in 0..4,
 * two-player layouts for oc_featurize, the batch; a refusal returns its code, with the entry point's own message in
 * oc_last_error), the code that answers is told which arrays a call has, not where they are, and holds no launch — so it also runs
 * on a host without a GPU.  Whether the device grants the dynamic LDS is asked when oc_featurize launches, and refused there.
 * The call described has every required array, aligned.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_potential_plan(const OcBatch* batch, char* out, size_t out_size);
int oc_featurize_plan(const OcBatch* batch, int num_pots, char* out, size_t out_size);

/*
 * oc_rollout_featurize_plan (ABI 6: an entry point added beside the others) — what oc_rollout_featurize would launch for this
 * batch, as text; up to and including '>' the text is the instance's name and stable:
 *   "k_rollout_featurize<MAXP=2, FAST=3> G=32, grid=256, 70656 B LDS"    one two-player layout of at most 64 cells with one or two
 *                                                  pots, a batch of at least 64 envs per CU and n_steps >= 2 (or
 *                                                  OC_OPT_ONE_KERNEL): envs per LDS image (always 32), workgroups, dynamic LDS
 *   "step by step: oc_rollout_random + k_featurize<LAY_LDS=true> ..."    every other call: per step the one-step entry point
 *   "step by step: oc_step + k_featurize<LAY_LDS=false> ..."             (oc_step with caller actions), then oc_featurize, whose
 *                                                                       instance, grid and LDS bytes follow
 *   "nothing to launch (no envs)" / "nothing to launch (no steps)"
 * oc_rollout_featurize plans a call before it launches anything and launches from that plan; this is the same plan put into
 * words: every check applies (a refusal returns its code, with the entry point's own message in oc_last_error), the code that
 * answers is told which arrays a call has, not where they are, and holds no launch — so it also runs on a host without a GPU
 * (the device's SIMD count then defaults to MI355X's 1 024).  The call described has the plan blob, a state and a 16-byte
 * aligned feature array, env_offset equal to the start spec's, and with_actions / with_outputs / start as for oc_observation_plan.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_rollout_featurize_plan(const OcBatch* batch, int num_pots, int horizon, uint32_t options, int n_steps,
                              int with_actions, int with_outputs, const OcStartSpec* start, char* out, size_t out_size);

/*
 * oc_multi_agent_step_featurize (ABI 6: an entry point added beside the others; no existing signature, struct or option changes,
 * so the version stays) — oc_multi_agent_step with featurize_state (mdp.py:2579-2898, the observation of behaviour-cloning
 * agents) of the states the next step starts from: what a training or evaluation loop with a "bc" partner needs every decision.
 * Every argument of oc_multi_agent_step, in its order, up to and including d_obs, obs_dtype, horizon; then
 *   d_feat_plan_blob, d_feat_plan_off   oc_featurize's motion-cost tables (planner.pack_plan_tables).  A pair of its own beside
 *               d_plan_blob / d_plan_off: phi always uses the counter_goals = "none" tables, features may be asked with "all";
 *               the two pairs may be the same pointers.  Required whenever d_features != NULL, also with d_phi_tables == NULL.
 *   d_features  float32 [n_envs][2][2 * (num_pots * 10 + 26) + 4], 16-byte aligned: featurize_state of the state the NEXT step
 *               starts from — after a restart the standard or drawn start state, on a re-drawn layout that layout's: exactly
 *               what oc_featurize of d_state gives after the call, the convention of d_obs.  NULL: the call IS
 *               oc_multi_agent_step, argument for argument.
 *   num_pots    0..4, as for oc_featurize;  options: 0 or OC_OPT_ONE_KERNEL (any other bit: OC_EINVAL)
 * All of oc_multi_agent_step's and all of oc_featurize's checks apply (two-player layouts), every one before any device call;
 * refusals carry this entry point's name.  The paths, chosen by one planner (oc_multi_agent_step_featurize_plan says which):
 *   k_train_step_feat<MAXP> (csrc/train_feat.hpp)   the whole call in ONE kernel — d_features without d_obs, one two-player
 *               layout of at most 64 cells with one or two pots, no event sink, and a batch that gives at least a quarter of
 *               the CUs a workgroup of 256 envs (>= 16 384 envs on MI355X; profiles/train_step_feat.txt) or OC_OPT_ONE_KERNEL:
 *               eight wavefronts per 256 envs — four step and restart, four compute phi and the shaped rewards, all eight
 *               featurize and stream the rows.  65 536 cramped_room envs, num_pots = 2: 15.4-15.5 us per call against 21.9-22.3 us
 *               for the two launches
 *   oc_multi_agent_step's own planned path, then k_featurize   every other call with features (d_obs as well, an event sink,
 *               65..128 cells, several layouts, more than two pots, small batches), with identical results.
 */
int oc_multi_agent_step_featurize(const OcBatch* batch, void* d_state, const uint8_t* d_actions, float* d_rewards,
                                  uint8_t* d_flags, float* d_ep_returns, float* d_ep_returns_out,
                                  const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const uint8_t* d_phi_tables,
                                  double* d_phi_next, double* d_phi_cur, const double* d_phi_start,
                                  double reward_shaping_factor, double* d_shaped, uint8_t* d_done, void* d_obs, int obs_dtype,
                                  int horizon, const uint8_t* d_feat_plan_blob, const uint32_t* d_feat_plan_off,
                                  float* d_features, int num_pots, uint32_t options, const OcStartSpec* start,
                                  const OcEventSink* events, void* stream);

/*
 * oc_multi_agent_step_featurize_plan (ABI 6: an entry point added beside the others) — what oc_multi_agent_step_featurize would
 * launch for this batch, as text; up to and including '>' the text is the instance's name and stable:
 *   "k_train_step_feat<MAXP=1> G=32, grid=256, 124928 B LDS"     the one-kernel path: envs per private LDS image (32, 16 or 8: the
 *                                                  largest whose eight images fit the LDS budget), workgroups, dynamic LDS
 *   "k_train_step1<UNIFORM=true, MAXP=1, LAY_LDS=true> + k_featurize<LAY_LDS=true> grid=512, 56320 B LDS"
 *                                                  every other call with features: oc_multi_agent_plan's text of the call, then
 *                                                  oc_featurize_plan's
 *   "nothing to launch (no envs)"
 * with_features = 0: oc_multi_agent_plan's answer, word for word.  The same plan the entry point launches from, put into words:
 * every check applies (refusals carry oc_multi_agent_step_featurize's name), the code that answers is told which arrays a call
 * has, not where they are, and holds no launch — so it also runs on a host without a GPU (the device's SIMD count then defaults
 * to MI355X's 1 024).  The call described has every required array (aligned), both episode-return arrays, the feature tables and,
 * as named, d_obs, the phi tables and buffers, an event sink with per-episode counters.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_multi_agent_step_featurize_plan(const OcBatch* batch, int horizon, int with_obs, int obs_dtype, int with_features,
                                       int num_pots, uint32_t options, int use_phi, int event_sink, const OcStartSpec* start,
                                       char* out, size_t out_size);

/*
 * The action sampler (ABI 6: entry points added beside the others; no existing signature, struct or option changes, so the
 * version stays) — both players' actions of every env drawn from a policy's logits on the library's counter-based stream, with
 * their log-probabilities (what PPO stores).  Everything between the policy's forward pass and the next observation is then one
 * call (oc_multi_agent_step_sample), and the draws are a function of (seed, global env, step): a sharded batch draws what the
 * whole batch draws, and any draw can be replayed.
 *
 * Stream.  For global env g = env_offset + e and the caller's 64-bit step counter t = step:
 *   r[0..3] = philox4x32_10(counter = {t_lo, g_lo, g_hi, t_hi}, key = {seed_lo, seed_hi ^ 0x53414D50 ("SAMP")})
 *   player p uses u_p = (float)(r[p] >> 8) * 2^-24, which is exact in f32 (0 <= u_p < 1); words 2 and 3 are reserved.
 * All counters are used in full 64-bit width, with a carry from g_lo into g_hi inside a batch, as for the other streams.
 *
 * Arithmetic, per player, on its six logits l_0..l_5.  All steps are f32, in this order, with no contraction and the
 * full-precision expf / logf (not the fast intrinsics):
 *   m = max_i l_i;  w_i = expf(l_i - m);  c_i = c_{i-1} + w_i, summed left to right;  S = c_5
 *   OC_SAMPLE_CATEGORICAL: x = u_p * S; the action is the number of i with c_i <= x, clamped to 5.  A -inf logit has w = 0 and
 *                          is never drawn.
 *   OC_SAMPLE_ARGMAX:      the lowest index holding m (u_p is not used).
 *   logp = (l_a - m) - logf(S)
 * Invalid rows.  If any of the six logits is NaN, or S is not finite and greater than 0 (all -inf, or a +inf), the action is 255
 * and logp is NaN.  Every step kernel flags an action above 5 as OC_F_BAD_ACTION and leaves the env untouched; so here.
 */
#define OC_SAMPLE_CATEGORICAL 0u
#define OC_SAMPLE_ARGMAX      1u
typedef struct OcActionSampler {
    const float* d_logits;   /* [n_envs][2][6] f32 (player, action index), 16-byte aligned */
    uint8_t* d_actions_out;  /* [n_envs][2] u8, 2-byte aligned; required */
    float* d_logp_out;       /* [n_envs][2] f32, 8-byte aligned; or NULL */
    uint64_t seed;
    int64_t env_offset;
    int64_t step;
    uint32_t mode;           /* OC_SAMPLE_CATEGORICAL / OC_SAMPLE_ARGMAX */
} OcActionSampler;

/*
 * oc_sample_actions — the sampler alone (k_sample_actions, csrc/sample.hpp): one lane per env draws both players' actions from
 * three 16-byte loads and one Philox block.  Of the batch only n_envs is read.  A NULL sampler, NULL d_logits or d_actions_out, a
 * misaligned array or an unknown mode is OC_EINVAL, before any device call.
 */
int oc_sample_actions(const OcBatch* batch, const OcActionSampler* sampler, void* stream);

/*
 * oc_multi_agent_step_sample — oc_multi_agent_step_featurize whose actions are drawn from policy logits inside the call: every
 * argument of oc_multi_agent_step_featurize, in its order, with `sampler` in the place of d_actions.  The drawn actions go to
 * sampler->d_actions_out (they are the step's d_actions) and their log-probabilities to sampler->d_logp_out.  d_features == NULL
 * gives the plain step's paths.  All checks of the step, of oc_featurize and of the sampler (as for oc_sample_actions) run before
 * any device call; refusals carry this entry point's name.  The paths (oc_multi_agent_step_sample_plan says which):
 *   fused      wherever the same call with an actions array is planned as k_train_step_obs, k_train_step_feat or k_train_step1, the
 *              SAMPLE = true instance of that kernel runs: its owner lanes draw where the others read the actions, store the draws
 *              and step — one launch (followed by what follows that kernel in the step's plan: oc_encode_lossless, k_featurize)
 *   otherwise  k_sample_actions into d_actions_out, then the step's own planned path reading it: k_train_step<.., EV>, 65..128
 *              cells, more than two pots (the sequence)
 * Both paths call one device function, so their results are bit-equal (profiles/train_step_sample.txt: what each costs).
 */
int oc_multi_agent_step_sample(const OcBatch* batch, void* d_state, const OcActionSampler* sampler, float* d_rewards,
                               uint8_t* d_flags, float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                               const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next, double* d_phi_cur,
                               const double* d_phi_start, double reward_shaping_factor, double* d_shaped, uint8_t* d_done,
                               void* d_obs, int obs_dtype, int horizon, const uint8_t* d_feat_plan_blob,
                               const uint32_t* d_feat_plan_off, float* d_features, int num_pots, uint32_t options,
                               const OcStartSpec* start, const OcEventSink* events, void* stream);

/*
 * oc_multi_agent_step_sample_plan — what oc_multi_agent_step_sample would launch, as text: oc_multi_agent_step_featurize_plan's
 * arguments (a whole, aligned sampler is assumed) and its words, changed in one of two ways:
 *   "k_train_step_obs<MAXP=1, T=u8, NWV=16, SAMPLE=true> unit=..."     the fused path: SAMPLE=true as the step kernel's last parameter
 *   "k_sample_actions + k_train_step<UNIFORM=true, EV=true> + ..."      every other plan
 *   "nothing to launch (no envs)"
 * Usable without a GPU, like the other plan calls; refusals carry oc_multi_agent_step_sample's name.
 *   out, out_size caller's text buffer (>= 320 bytes holds every answer)
 */
int oc_multi_agent_step_sample_plan(const OcBatch* batch, int horizon, int with_obs, int obs_dtype, int with_features,
                                    int num_pots, uint32_t options, int use_phi, int event_sink, const OcStartSpec* start,
                                    char* out, size_t out_size);

/*
 * The behaviour-cloning partner (ABI 6: entry points added beside the others; no existing signature, struct or option changes, so the
 * version stays) — the "bc" agent of the reference's PPO-with-BC-partner training (human_aware_rl/rllib/rllib.py:262-281: per
 * episode a bc_factor coin decides whether the env has a partner, a shuffle decides which player it plays) and its model, the small
 * dense network on featurize_state of human_aware_rl/imitation/behavior_cloning_tf2.py (in_dim -> h1 -> h2 -> 6 logits, ReLU).
 * oc_partner_logits seats the partners and writes their logits INTO the learner's logits array, so that the sampler that follows
 * (oc_multi_agent_step_sample, oc_sample_actions) draws the partner's action from its own policy and the learner's from the
 * learner's: one launch (k_partner_logits, csrc/partner.hpp; its MFMA tile: csrc/mlp_tile.hpp) in front of the step, whose kernels stay as they are.
 *
 * Seating stream.  For global env g = env_offset + e and the caller's 64-bit step counter t = step:
 *   r[0..3] = philox4x32_10(counter = {t_lo, g_lo, g_hi, t_hi}, key = {seed_lo, seed_hi ^ 0x53454154 ("SEAT")})
 *   an env is reseated when d_done == NULL or d_done[e] != 0;
 *   a reseated env gets a partner iff (float)(r[0] >> 8) * 2^-24 < bc_factor (the product is exact in f32, 0 <= u < 1: bc_factor 0
 *   seats nobody, 1 everybody); the partner plays player r[1] & 1: d_seat[e] = r[1] & 1, and d_seat[e] = 255 without a partner;
 *   every other env keeps its seat (any value above 1 reads as "no partner").  Words 2 and 3 are reserved.
 * All counters are used in full 64-bit width, with a carry from g_lo into g_hi inside a batch, as for the other streams.
 *
 * Logits.  For every env with a seat p (0 or 1) AFTER the reseat of this same call, d_logits[e][p][0..5] receives the network's
 * output on d_features[e][p][:].  Nothing else is written: the other player's six logits and an unseated env's twelve keep the
 * caller's bytes.
 *
 * Arithmetic.  All f32.  With x the feature row, every unit is an fmaf chain over its inputs in ascending index that starts from
 * the bias, every hidden unit followed by max(., 0):
 *   a1_j = max(fmaf(x_{in_dim-1}, w1[in_dim-1][j], ... fmaf(x_1, w1[1][j], fmaf(x_0, w1[0][j], b1_j)) ...), 0)      j < h1
 *   a2_j = max(the same chain over a1_0 .. a1_{h1-1} with w2, from b2_j, 0)                                         j < h2
 *   logit_j = the same chain over a2_0 .. a2_{h2-1} with w3, from b3_j                                              j < 6
 * one rounding per step, no wider accumulator.  This is what gfx950's f32-input MFMA computes bit for bit when the K steps are issued
 * in order with the bias as the initial accumulator (v_mfma_f32_32x32x2_f32; csrc/mlp_tile.hpp states the scheme); the kernel pads the hidden widths to its tile of 32
 * units with zero weights and zero biases, which add exact zeros to a chain.  (max(., 0) of a NaN is 0, as v_max_f32 gives it; a
 * chain whose value is exactly -0 may come out as +0, since a padded step adds +0 to it.)
 */
typedef struct OcDensePolicy {     /* two hidden ReLU layers, 6 logits; all f32, row-major [in][out] (the Keras Dense layout) */
    const float *d_w1, *d_b1;      /* [in_dim][h1], [h1] */
    const float *d_w2, *d_b2;      /* [h1][h2], [h2] */
    const float *d_w3, *d_b3;      /* [h2][6], [6] */
    int in_dim, h1, h2;            /* in_dim = 2*(num_pots*10+26)+4 of the call; 1 <= h1, h2 <= 64 */
} OcDensePolicy;

typedef struct OcPartnerSeats {
    uint8_t* d_seat;               /* [n_envs] in/out: 0 or 1 = the player the partner plays, 255 = no partner */
    const uint8_t* d_done;         /* [n_envs] done mask of the previous step; NULL: every env is reseated */
    float bc_factor;               /* in [0, 1] */
    uint64_t seed; int64_t env_offset; int64_t step;
} OcPartnerSeats;

/*
 * oc_partner_logits — the reseat and the partners' forward pass, one launch.  Of the batch only n_envs is read.
 *   d_features  [n_envs][2][2 * (num_pots * 10 + 26) + 4] f32 as oc_featurize writes it (of the CURRENT states), 16-byte aligned
 *   d_logits    [n_envs][2][6] f32, 8-byte aligned (a row of six is written as 8-byte stores; OcActionSampler, which reads the
 *               array next, asks 16 of it); in/out as described under "Logits"
 *   the six weight and bias arrays: 4-byte aligned; d_seat and d_done at any address
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL batch, policy, seats, d_features,
 * d_logits, weight or bias array or d_seat; a misaligned array; policy.in_dim different from the call's feature length; h1 or h2
 * outside 1..64; bc_factor outside [0, 1] or NaN; num_pots outside 0..4; n_envs < 0.
 */
int oc_partner_logits(const OcBatch* batch, const OcDensePolicy* policy, const OcPartnerSeats* seats, const float* d_features,
                      int num_pots, float* d_logits, void* stream);

/*
 * oc_partner_logits_plan — what oc_partner_logits would launch, as text:
 *   "k_partner_logits grid=256, 256 lanes (4 wavefronts x 64 envs), 32 x 32 x 2 f32 MFMA, K 96 -> 64 -> 64 -> 32 (h1 = 64, h2 = 64, 6 logits, zero-padded), 100224 B LDS"
 *   "nothing to launch (no envs)"
 * The checks that need no array apply (batch, policy: in_dim, h1, h2; num_pots); usable without a GPU, like the other plan calls;
 * refusals carry oc_partner_logits's name.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_partner_logits_plan(const OcBatch* batch, const OcDensePolicy* policy, int num_pots, char* out, size_t out_size);

/*
 * The partner pool (ABI 6: entry points added beside the others; no existing signature or struct changes, so the version stays) —
 * one of up to 16 frozen policies per episode: a league of the learner's past snapshots, BC models of several data splits,
 * fictitious co-play.  oc_partner_pool_logits is oc_partner_logits with a pool in the policy's place: it seats the partners, draws
 * each new partner's member, and writes every partner's logits from ITS member's network (csrc/partner_pool.hpp: the seated envs are
 * bucketed by member on the device, without atomics, and the network runs over the buckets — four launches, the step's kernels
 * stay as they are).
 *
 * Member draw.  The seating block is unchanged — the same counter and the same "SEAT" key — and so are the seats: d_seat is byte-equal
 * to what oc_partner_logits draws from the same OcPartnerSeats.  A reseated env that gets a partner also draws
 *   member = #{ m < n_members - 1 : r[2] >= thresholds[m] }
 * from word 2 of that block, with non-decreasing thresholds (two equal ones give the member between them probability 0).
 * thresholds == NULL is the uniform pool, thresholds[m] = ceil((m + 1) * 2^32 / n_members) formed in 64-bit integers, which makes
 * member = (r[2] * n_members) >> 32.  d_member[e] = the draw, and 255 where the reseated env has no partner; an env that is not
 * reseated keeps both its seat and its member (a kept member that is not below n_members reads as "no partner": no logits).  Word 3
 * stays reserved.
 *
 * Logits.  For every env with a seat p and a member m after the reseat of this same call, d_logits[e][p][0..5] receives the network
 * of members[m] on d_features[e][p][:], by OcDensePolicy's fmaf chain above: the six floats are bit-equal to what oc_partner_logits
 * writes for that env with members[m] as the only policy.  Nothing else of d_logits is written.  No atomics, no spin flags, no
 * look-back: a call repeats byte for byte.
 *
 * Scratch.  d_scratch is the caller's, 16-byte aligned, of the size in bytes that oc_partner_pool_plan states ("scratch ... B":
 * 1092 + 4 * n_members * ceil(n_envs / 256) + 4 * n_envs); its contents after a call are unspecified.
 */
#define OC_MAX_POOL 16
typedef struct OcPartnerPool {
    const OcDensePolicy* members;  /* HOST array [n_members]; device weight pointers; the same in_dim, h1 / h2 may differ per member */
    int n_members;                 /* 1..OC_MAX_POOL */
    const uint32_t* thresholds;    /* HOST array [n_members - 1], non-decreasing, or NULL = uniform */
    uint8_t* d_member;             /* [n_envs] in/out: the member an env's partner is, 255 = no partner */
} OcPartnerPool;

/*
 * oc_partner_pool_logits — the reseat, the member draw and the partners' forward passes; the other arguments as oc_partner_logits'.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL pool, members or d_member, or a
 * NULL or misaligned d_scratch where there are envs; n_members outside 1..16; a member whose in_dim differs from the call's
 * feature length, whose h1 or h2 lies outside 1..64, or that has a NULL or misaligned array (from the second member on the message
 * ends in "(members[m])"); decreasing thresholds; n_envs of 2^31 or more; whatever oc_partner_logits refuses.
 */
int oc_partner_pool_logits(const OcBatch* batch, const OcPartnerPool* pool, const OcPartnerSeats* seats, const float* d_features,
                           int num_pots, float* d_logits, void* d_scratch, void* stream);

/*
 * oc_partner_pool_plan — what oc_partner_pool_logits would launch, every launch with its grid, and the scratch bytes, as text:
 *   "k_pool_seat grid=256, 256 lanes + k_sample_scan grid=1, 256 lanes, 5 pass(es) of 256 counts + k_pool_write grid=256, 256 lanes + k_pool_logits grid=260 (256 blocks of envs + 4 members), 256 lanes (128 j rows of one member), 32 x 32 x 2 f32 MFMA, K 96 -> 64 -> 64 -> 32, 101248 B LDS; scratch 267332 B"
 *   "nothing to launch (no envs)"
 * (j is 2 unless the seated envs' chunks of 256 rows outnumber the device's CUs; then the kernel takes the least j for which chunks
 * of 128 j rows fit, from the scanned counts: a workgroup stages its member once and makes j passes.  No row's arithmetic depends
 * on it.)
 * The checks that need no device array apply (batch, pool: members' in_dim, h1, h2, n_members, thresholds; num_pots); usable without
 * a GPU, like the other plan calls; refusals carry oc_partner_pool_logits's name.
 *   out, out_size caller's text buffer (>= 512 bytes holds every answer)
 */
int oc_partner_pool_plan(const OcBatch* batch, const OcPartnerPool* pool, int num_pots, char* out, size_t out_size);

/*
 * Advantages and value targets of a collected batch (ABI 6: entry points added beside the others; no existing signature, struct or
 * option changes, so the version stays) — what PPO makes of the T steps it has collected: per-agent GAE(gamma, lambda) advantages
 * and the value targets A + V, as the reference's PPO computes them (use_gae; gamma 0.99, lambda 0.98; the end of the horizon is a
 * terminal done), in one launch (k_gae, csrc/gae.hpp) where a learner would run a reverse loop of small kernels over T.
 *
 * Layout.  Every array is time-major: row t is what step t of the collection left — T calls of oc_multi_agent_step_sample whose
 * d_shaped, d_done, d_actions_out and d_logp_out point at row t of [T][n_envs]... arrays write exactly these.  d_values[t] is the
 * policy's value estimate of the observation step t started from, d_last_values that of the observation after step T - 1.  A done
 * step is followed, in the same row, by the first observation of the restarted episode: d_values[t + 1] belongs to ANOTHER episode
 * then, and the chain does not reach across.  With a behaviour-cloning partner (oc_partner_logits) d_seat[t] is the seat array as
 * it stood during step t: the partner's samples are no learner samples.
 *
 * Arithmetic.  Per env e and player p, for t = T - 1 down to 0; every operation is f32 with one rounding, in this order, with no
 * contraction; the chain over t is sequential and is not re-associated:
 *   g = gamma;  gl = gamma * lambda (one f32 product, formed on the host);  the carried A starts as 0
 *   r = (float)d_rewards[t][e][p] (round to nearest);  v = d_values[t][e][p]
 *   if d_done[t][e] != 0:  delta = r - v;  A = delta
 *       (a select, not a multiplication by 0: neither d_values[t + 1][e] nor the carried A enters, so a NaN or a sentinel there
 *        cannot reach step t)
 *   otherwise:             vn = d_values[t + 1][e][p], at t = T - 1 d_last_values[e][p] (0 when that is NULL);
 *                          delta = (r + g * vn) - v;  A = delta + gl * A_carried
 *   target = A + v;  A is carried to t - 1
 *   if d_seat != NULL and d_seat[t][e] == p, the sample is the partner's: d_advantages[t][e][p] = d_targets[t][e][p] = +0.0f, the
 *   value carried on is 0, and the entry is left out of the moments; the other player's chain is unaffected.  (A seat that changes
 *   inside an episode is read as it stands, step by step.)
 * Moments (for the batch standardisation of the advantages).  d_partials[k] = {count, sum A, sum A^2} over the learner samples of
 * envs [256 k, 256 k + 256), all steps and both players, accumulated in f64 with A widened before it is squared; d_moments is the
 * sum of the partials in ascending k.  No floating-point atomics: the same call on the same inputs gives the same bits.
 */
typedef struct OcGaeBatch {
    const double*  d_rewards;      /* [T][n_envs][2] f64: the step's d_shaped rows; 16-byte aligned; required */
    const float*   d_values;       /* [T][n_envs][2] f32: V(observation step t started from); 8-byte aligned; required */
    const float*   d_last_values;  /* [n_envs][2] f32: V(observation after step T-1); 8-byte aligned; NULL = 0 */
    const uint8_t* d_done;         /* [T][n_envs] u8: the step's d_done rows; any address; required */
    const uint8_t* d_seat;         /* [T][n_envs] u8: the partner's player during step t (0 / 1), else no partner; NULL = none */
    float*         d_advantages;   /* [T][n_envs][2] f32 out; 8-byte aligned; required */
    float*         d_targets;      /* [T][n_envs][2] f32 out; 8-byte aligned; required */
    double*        d_partials;     /* [ceil(n_envs / 256)][3] f64 out, or NULL (then d_moments must be NULL too) */
    double*        d_moments;      /* [3] f64 out: count, sum A, sum A^2 over learner samples; or NULL */
    int64_t n_steps;               /* T >= 0 */
    float gamma, lambda;
} OcGaeBatch;

/*
 * oc_gae — the reverse pass: k_gae, one lane per env, and, with d_moments, k_gae_moments behind it (one wavefront adding the
 * partials).  Of the batch only n_envs is read.  n_steps == 0 or n_envs == 0 launches nothing and returns 0; the moments asked for
 * are then set to zeros.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL batch, struct or required array;
 * a misaligned array (d_partials and d_moments: 8 bytes); n_steps < 0 or n_envs < 0; gamma or lambda outside [0, 1] or NaN;
 * d_moments without d_partials.
 */
int oc_gae(const OcBatch* batch, const OcGaeBatch* g, void* stream);

/*
 * oc_gae_plan — what oc_gae would launch, as text (with_seat: d_seat given; with_moments: d_partials and d_moments given):
 *   "k_gae<SEAT=true, MOM=true> grid=256, 256 lanes (one per env, both players), 8 steps per prefetch block, 50 block(s) + k_gae_moments grid=1, 64 lanes"
 *   "nothing to launch (no envs)"     "nothing to launch (no steps)"
 * A prefetch block is the run of steps whose loads a lane issues before it needs the first of them.  The checks that need no array
 * apply (batch, n_envs, n_steps); usable without a GPU, like the other plan calls; refusals carry oc_gae's name.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_gae_plan(const OcBatch* batch, int64_t n_steps, int with_seat, int with_moments, char* out, size_t out_size);

/*
 * The PPO loss head (ABI 6: entry points added beside the others) — the learner's call behind oc_gae: the clipped-surrogate loss of
 * a minibatch, as the reference's trainer (RLlib's PPO) states it, and its gradients with respect to the policy's logits and
 * values, in one launch (k_ppo_loss, csrc/ppo_loss.hpp) where a learner would run some 25 elementwise and reduction kernels forward
 * and as many backward.
 *
 * Layout.  A sample is s = (t * n_envs + e) * 2 + p, the flat index into the time-major [T][n_envs][2] arrays of OcGaeBatch and of
 * the collection; S = T * n_envs * 2.  The batch side is the whole buffer; the minibatch side — the policy's logits and values of
 * M samples, in the order of its forward pass — names its samples through d_index, or is samples first_sample .. first_sample +
 * M - 1.
 *
 * Arithmetic.  Per minibatch row, with a = d_actions[s], l = the row's logits, v its value; every operation is f32 with one
 * rounding, in this order, with no contraction, expf and logf in full precision:
 *   m = max l_i;  d_i = l_i - m;  w_i = expf(d_i);  S = ((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5
 *   lp_i = d_i - logf(S);  p_i = w_i / S;  logp = lp_a;  ratio = expf(logp - d_logp_old[s])
 *   A^ = d_advantages[s], or with d_moments = {n, s1, s2} and n >= 1, in f64: mean = s1 / n;
 *        std = max(sqrt(max(s2 / n - mean * mean, 0)), 1e-4);  A^ = (float)(((double)A - mean) / std)
 *        (the moments of the whole batch, as RLlib standardises the train batch)
 *   s1 = ratio * A^;  s2 = min(max(ratio, lo), hi) * A^ with lo = 1 - clip_param, hi = 1 + clip_param (one f32 operation each);
 *   surr = min(s1, s2)
 *   H = -(((((t_0 + t_1) + t_2) + t_3) + t_4) + t_5), t_i = p_i * lp_i, and t_i = 0 where p_i == 0
 *   dv = v - d_targets[s];  vf = dv * dv;  vfc = min(vf, vf_clip_param)
 *   kl, with d_logits_old (lq_i, q_i: the same softmax of the old row): the sum of u_i = q_i * (lq_i - lp_i), u_i = 0 where
 *       q_i == 0, from u_0 on; without: the sample estimate d_logp_old[s] - logp, reported only (kl_coeff must be 0)
 * Gradients of -surr + vf_loss_coeff * vfc - entropy_coeff * H + kl_coeff * kl, per sample, not divided by the count:
 *   g = (s1 <= s2) ? -s1 : 0
 *   d/dl_i = g * ([i == a] - p_i) + (entropy_coeff * p_i) * (lp_i + H), the second product 0 where p_i == 0,
 *            and with d_logits_old + kl_coeff * (p_i - q_i)
 *   d/dv = vf_loss_coeff * ((vf <= vf_clip_param) ? 2 * dv : 0)
 * Left-out samples.  A row is left out when its index is outside 0 .. S - 1, when d_actions[s] > 5 (255: the sampler's invalid
 * row, whose logp is NaN) or when d_seat[s >> 1] == (s & 1) (the partner's sample).  Its seven gradients and its terms are +0.0f,
 * by a select, so that a NaN anywhere in its inputs reaches nothing, and it enters no sum.
 * Sums.  d_partials[k] = {count, sum -surr, sum vfc, sum H, sum kl, number of ratios outside [lo, hi]} over the learner samples
 * of minibatch rows [P k, P k + P), P = 1024 (oc_ppo_loss_plan states it): each term widened to f64 before it is added, in a fixed
 * tree.  d_stats = {count, total, policy, vf, entropy, kl, clip_frac, 1 / count}: the partials added in ascending k, each of the
 * five sums divided by count, total = ((policy + vf_loss_coeff * vf) - entropy_coeff * entropy) + kl_coeff * kl in f64 with
 * the coefficients widened; all zeros when count == 0.  No floating-point atomics: the same call on the same inputs gives the same bits.
 */
typedef struct OcPpoLoss {
    const uint8_t* d_actions;      /* [S] u8: the collection's actions; any address; required */
    const float*   d_logp_old;     /* [S] f32: their log-probabilities under the collecting policy; 4-byte aligned; required */
    const float*   d_advantages;   /* [S] f32: oc_gae's; 4-byte aligned; required */
    const float*   d_targets;      /* [S] f32: oc_gae's; 4-byte aligned; required */
    const uint8_t* d_seat;         /* [S / 2] u8: the partner's player of (t, e), else no partner; any address; NULL = none */
    const float*   d_logits_old;   /* [S][6] f32: the collecting policy's logits, for the exact KL; 8-byte aligned; or NULL */
    const double*  d_moments;      /* [3] f64: oc_gae's d_moments, for standardising the advantages; 8-byte aligned; or NULL */
    int64_t n_samples;             /* S >= 0 */
    const float*   d_logits;       /* [M][6] f32: the policy's logits of the minibatch; 16-byte aligned; required */
    const float*   d_values;       /* [M] f32: its values; 4-byte aligned; required */
    const int32_t* d_index;        /* [M] i32: the sample of every row; 4-byte aligned; NULL = first_sample + row */
    int64_t first_sample;          /* read without d_index only */
    int64_t n_minibatch;           /* M >= 0 */
    float*         d_grad_logits;  /* [M][6] f32 out; 16-byte aligned; required */
    float*         d_grad_values;  /* [M] f32 out; 4-byte aligned; required */
    double*        d_partials;     /* [ceil(M / P)][6] f64 out; 8-byte aligned; or NULL (then d_stats must be NULL too) */
    double*        d_stats;        /* [8] f64 out; 8-byte aligned; or NULL */
    float*         d_terms_out;    /* [M][4] f32 out: surr, vfc, H, kl of every row; 16-byte aligned; or NULL */
    float clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff;
} OcPpoLoss;

/*
 * oc_ppo_loss — k_ppo_loss, one lane per minibatch row and four rows per lane, and, with d_stats, k_ppo_loss_stats behind it (one wavefront adding the
 * partials).  n_minibatch == 0 launches nothing and returns 0; d_stats is then set to zeros.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL struct or required array; a
 * misaligned array; n_minibatch < 0 or n_samples < 0; an odd n_samples with d_seat; n_samples >= 2^31 with d_index; without d_index a first_sample < 0 or
 * first_sample + n_minibatch > n_samples; clip_param or vf_clip_param not finite and positive; a negative or NaN coefficient;
 * kl_coeff > 0 without d_logits_old; d_stats without d_partials.
 */
int oc_ppo_loss(const OcPpoLoss* q, void* stream);

/*
 * oc_ppo_loss_plan — what oc_ppo_loss would launch, as text (with_...: the optional array is given):
 *   "k_ppo_loss<OLD=true> grid=4096, 256 lanes (one per sample, 4 tiles of 256), 1024 samples per partial, index=yes seat=yes moments=yes terms=no + k_ppo_loss_stats grid=1, 64 lanes, 4096 partial(s) (with d_stats)"
 *   "nothing to launch (no samples)"
 * Usable without a GPU, like the other plan calls; refusals carry oc_ppo_loss's name.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_ppo_loss_plan(int64_t n_minibatch, int with_index, int with_seat, int with_moments, int with_old_logits, int with_terms, char* out, size_t out_size);

/*
 * The learner's actor-critic on featurize_state rows (ABI 6: entry points added beside the others; no existing signature, struct or
 * option changes, so the version stays) — the one stage of a PPO iteration that was still a torch module: the policy that is called
 * once per collected step and, forward and backward, once per minibatch.  It is the partner's small dense network with a value
 * output, a shared trunk:
 *   a1 = relu(x W1 + b1),  a2 = relu(a1 W2 + b2),  logits = a2 Wp + bp (six),  value = a2 wv + bv (one)
 * all f32, row-major [in][out] (the Keras Dense layout), in_dim = 2 * (num_pots * 10 + 26) + 4 for num_pots in 0..4 (56, 76, 96, 116
 * or 136), 1 <= h1, h2 <= 64.  oc_policy_forward evaluates it for every row of a call in one launch, oc_policy_backward turns the
 * gradients with respect to logits and values (oc_ppo_loss writes them) into the gradients of the eight weight arrays, in two
 * launches and without saved activations: it reads the 4 * in_dim bytes of features per row again rather than 512 bytes of
 * activations (csrc/policy.hpp).
 *
 * Forward arithmetic.  All f32.  With x the feature row, every unit is an fmaf chain over its inputs in ascending index that starts
 * from the bias, every hidden unit followed by max(., 0) — OcDensePolicy's chain, so that the six logits equal oc_partner_logits'
 * bit for bit on the same weights and row:
 *   pre1_j = fmaf(x_{in_dim-1}, w1[in_dim-1][j], ... fmaf(x_1, w1[1][j], fmaf(x_0, w1[0][j], b1_j)) ...),  a1_j = max(pre1_j, 0)     j < h1
 *   pre2_j = the same chain over a1_0 .. a1_{h1-1} with w2, from b2_j,  a2_j = max(pre2_j, 0)                                      j < h2
 *   logit_j = the same chain over a2_0 .. a2_{h2-1} with wp, from bp_j (j < 6);  value = the same chain with wv, from bv
 * one rounding per step, no wider accumulator (v_mfma_f32_32x32x2_f32, K steps in order from the bias; the value head is the seventh
 * row of the last layer's tile).  (max(., 0) of a NaN is 0; a chain whose value is exactly -0 may come out as +0.)
 *
 * Backward arithmetic.  All f32.  With gl_0..5 and gv the row's upstream gradients (delta3_j = gl_j for j < 6, delta3_6 = gv):
 *   delta2_u = pre2_u > 0 ? fmaf(wv[u], gv, fmaf(wp[u][5], gl_5, ... fmaf(wp[u][0], gl_0, +0) ...)) : 0          u < h2
 *   delta1_i = pre1_i > 0 ? the fmaf chain over u = 0 .. h2-1 of w2[i][u] * delta2_u, from +0 : 0                   i < h1
 * The ReLU derivative is 1 where the f32 pre-activation is > 0 and 0 elsewhere (0 at exactly 0 and at a NaN): torch's convention.
 * Every weight gradient is the sum over the call's rows of input_i * delta_j — gw1[i][j] of x_i * delta1_j, gw2[i][j] of
 * a1_i * delta2_j, gwp[i][j] of a2_i * delta3_j, gwv[i] of a2_i * gv — and every bias gradient the sum of delta_j.  The order of
 * summation is fixed:
 *   rows are taken in tiles of 32 consecutive rows of the call; tile k belongs to wavefront k % W of workgroup (k / W) % G, where W
 *   is the number of wavefronts of a workgroup and G the grid (oc_policy_plan states both);
 *   a wavefront adds its tiles in ascending order and the rows of a tile in ascending order into ONE f32 accumulator per element, by
 *   fmaf for the weights (one rounding per row) and by addition for the biases, from +0;
 *   a workgroup adds its wavefronts' accumulators in ascending order, ((w0 + w1) + w2) + w3, into d_partials[workgroup];
 *   the gradient is d_partials[0] + d_partials[1] + ... in ascending order (k_policy_grad_sum).
 * No floating-point atomics: a call repeats bit for bit.  A tile whose 32 rows have only zero upstream gradients is not computed (it
 * would add +-0 to accumulators that are never -0); its features are not read.
 *
 * Rows.  Without d_index the call's row r is feature row first_row + r.  With d_index it is feature row d_index[r]; first_row is
 * not read; an entry outside 0 .. n_feature_rows - 1 is an out-of-range row: nothing is read for it, oc_policy_forward writes
 * +0.0f logits and value for it, and it contributes nothing to oc_policy_backward whatever its upstream gradients hold
 * (oc_ppo_loss leaves such entries out too).  An index may name a row more than once.
 */
typedef struct OcActorCritic {     /* all f32, row-major [in][out]; read at every call: an optimiser may update them in place */
    const float *d_w1, *d_b1;      /* [in_dim][h1], [h1] */
    const float *d_w2, *d_b2;      /* [h1][h2], [h2] */
    const float *d_wp, *d_bp;      /* [h2][6], [6] */
    const float *d_wv, *d_bv;      /* [h2], [1] */
    int in_dim, h1, h2;
} OcActorCritic;

typedef struct OcPolicyRows {
    const float* d_features;       /* [n_feature_rows][in_dim] f32, 16-byte aligned (oc_featurize's [n_envs][2][in_dim] is 2 n_envs rows) */
    int64_t n_feature_rows;
    const int32_t* d_index;        /* [n_rows] or NULL; 4-byte aligned; needs n_feature_rows < 2^31 */
    int64_t first_row;             /* without d_index: the first feature row of the call */
    int64_t n_rows;
} OcPolicyRows;

typedef struct OcPolicyGrads {     /* the gradients of OcActorCritic's arrays, same shapes; 4-byte aligned; OVERWRITTEN */
    float *d_w1, *d_b1, *d_w2, *d_b2, *d_wp, *d_bp, *d_wv, *d_bv;
} OcPolicyGrads;

/*
 * oc_policy_forward — k_policy_forward, one launch: a persistent grid whose wavefronts take 32-row tiles.
 *   d_logits [n_rows][6] f32, 8-byte aligned;  d_values [n_rows] f32, 4-byte aligned; the weight and bias arrays 4-byte aligned
 * n_rows == 0 launches nothing.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL policy, rows, array of either,
 * d_logits or d_values (d_index may be NULL); a misaligned array; an in_dim that is no feature length; h1 or h2 outside 1..64;
 * n_rows < 0 or above 2^40; n_feature_rows < 0; n_feature_rows >= 2^31 with d_index; without d_index a first_row < 0 or
 * first_row + n_rows > n_feature_rows.
 */
int oc_policy_forward(const OcActorCritic* policy, const OcPolicyRows* rows, float* d_logits, float* d_values, void* stream);

/*
 * oc_policy_backward — k_policy_backward, which recomputes the hidden layers of every tile, and k_policy_grad_sum behind it.
 *   d_grad_logits [n_rows][6] f32, 8-byte aligned;  d_grad_values [n_rows] f32, 4-byte aligned
 *   grads         the eight gradient arrays: OVERWRITTEN, not accumulated into
 *   d_partials    f32 scratch of the caller, 4-byte aligned: as many rows of as many floats as oc_policy_plan states for the call
 *                 ("256 partial(s) of 10823 floats"; a row is the eight gradient arrays one behind the other, w1 b1 w2 b2 wp bp wv bv)
 * n_rows == 0 launches k_policy_grad_sum alone, which zeroes the gradients.
 * OC_EINVAL as oc_policy_forward, and for a NULL or misaligned d_grad_logits, d_grad_values, grads, gradient array or d_partials.
 */
int oc_policy_backward(const OcActorCritic* policy, const OcPolicyRows* rows, const float* d_grad_logits, const float* d_grad_values,
                       const OcPolicyGrads* grads, float* d_partials, void* stream);

/*
 * oc_policy_plan — what oc_policy_forward (backward == 0) or oc_policy_backward would launch, as text:
 *   "k_policy_forward grid=256, 256 lanes (4 wavefronts x 32-row tiles), 128 rows per workgroup per pass, 32 x 32 x 2 f32 MFMA, K 96 -> 64 -> 64 -> 32 (h1 = 64, h2 = 64, 6 logits + value, zero-padded), index=no, 99968 B LDS"
 *   "k_policy_backward<F0=0,NF=3,REST> grid=256, 256 lanes (4 wavefronts x 32-row tiles), 128 rows per workgroup per pass, 32 x 32 x 2 f32 MFMA, 12 accumulator tiles per wavefront, index=yes, 147456 B LDS + k_policy_grad_sum grid=43, 256 lanes, 256 partial(s) of 10823 floats"
 *   "nothing to launch (no rows)"
 *   "k_policy_grad_sum grid=43, 256 lanes, 0 partial(s) of 10823 floats (no rows: the gradients are zeroed)"
 * The grid is the number of workgroups, at most 256.  With 136 inputs a backward workgroup has three wavefronts (its LDS
 * holds no more; at 116 inputs four still fit) and with 116 and 136 inputs a second k_policy_backward launch
 * ("+ k_policy_backward<F0=3,NF=2> grid=256 (feature rows 96.. of gw1)") accumulates the rows of gw1 that the first one's registers do not hold; the order of summation is the same.  The checks that need no array apply; usable without a GPU, like the other plan calls; refusals carry the name of the entry
 * point the plan is for.
 *   out, out_size caller's text buffer (>= 384 bytes holds every answer)
 */
int oc_policy_plan(int64_t n_rows, int with_index, int in_dim, int h1, int h2, int backward, char* out, size_t out_size);

/*
 * The learner's optimiser step (ABI 6: entry points added beside the others; no existing signature, struct or option changes, so the
 * version stays) — gradient clipping by global norm (torch's clip_grad_norm_) and Adam on the eight arrays of an OcActorCritic in
 * ONE launch of one workgroup (k_adam_step, csrc/adam.hpp), where a learner would run clip_grad_norm_ and torch.optim.Adam: a
 * dozen small launches.
 *
 * Flat order.  Element i runs over the concatenation w1, b1, w2, b2, wp, bp, wv, bv — the order of a partial row of
 * oc_policy_backward; n = in_dim * h1 + h1 + h1 * h2 + h2 + h2 * 6 + 6 + h2 + 1 (73 for 56/1/1, 10 823 for 96/64/64, 13 383 for 136/64/64).
 * Gradient scale.  gs = (float)*d_grad_scale where that f64 pointer is given (oc_ppo_loss's d_stats[7], 1 / count), else 1.0f;
 *   g_i = graw_i * gs, one f32 rounding (with gs == 1 the product is exact).
 * Norm.  q_i = (double)g_i * (double)g_i (exact).  Lane l of the ONE workgroup of 256 lanes adds the q_i with i % 256 == l in
 *   ascending i, from +0, in f64; the 256 lane sums are added by the fixed tree s[l] += s[l + k] for k = 128, 64, ..., 1;
 *   norm = (float)sqrt(s[0]).  The order of summation is part of the interface, which is why there is one workgroup.
 * Clip.  With max_grad_norm finite and > 0: c = min(max_grad_norm / (norm + 1e-6f), 1.0f) in f32 and g_i = g_i * c (torch's
 *   clip_grad_norm_); otherwise c = 1 and there is no multiply.
 * Skipped steps.  The step is skipped if norm is not finite (a NaN or an infinity among the gradients, or a sum of squares beyond
 *   f32), and if d_grad_scale is given and is 0 (oc_ppo_loss's count == 0: no learner sample in the minibatch).  A skipped step
 *   writes nothing to parameters or moments, leaves steps and the beta powers alone and increments skipped: a NaN must not reach
 *   the weights, and an empty minibatch must not move them by momentum.
 * Clock.  d_clock = {steps, beta1^steps, beta2^steps, skipped} in f64; the caller initialises it to {0, 1, 1, 0}.  A step taken
 *   sets steps += 1, p1 *= (double)beta1, p2 *= (double)beta2 — running products, not pow — and then, in f64,
 *   bc1 = 1 - p1;  bc2s = sqrt(1 - p2);  step_size = (float)((double)lr / bc1);  rbc2s = (float)bc2s
 * Update.  Every operation f32 with one rounding, in this order, with no contraction, sqrtf and / correctly rounded; 1 - beta is
 *   computed once in f32:
 *   m_i = m_i + (g_i - m_i) * (1 - beta1)
 *   v_i = v_i * beta2 + (g_i * g_i) * (1 - beta2)
 *   den = sqrtf(v_i) / rbc2s + eps
 *   p_i = p_i - step_size * (m_i / den)
 *   (torch.optim.Adam's update — bias-corrected, eps added to sqrt(v) / sqrt(1 - beta2^t) — in another order of operations)
 * Info.  d_info = {norm before clipping, c, gs, 1 if skipped else 0} in f64; on a skipped step c is reported as 0, and a norm that
 *   is a NaN is reported as a NaN (its sign and payload are not specified).
 * No atomics: a call on the same inputs gives the same bits.  The gradients are read only.
 */
typedef struct OcAdam {
    float *d_m[8], *d_v[8];      /* first and second moments, OcActorCritic's shapes and order; 4-byte aligned; updated in place */
    double* d_clock;             /* [4] f64, 8-byte aligned */
    const double* d_grad_scale;  /* f64 scalar on the device, or NULL */
    double* d_info;              /* [4] f64 out, or NULL */
    float lr, beta1, beta2, eps, max_grad_norm;
} OcAdam;

/*
 * oc_adam_step — k_adam_step, one launch of one workgroup.  params' eight arrays are WRITTEN THROUGH (the struct declares them
 * const for the forward and backward calls); grads' are read.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL struct or array (d_grad_scale
 * and d_info may be NULL); a misaligned array (weights, gradients and moments 4 bytes; d_clock, d_grad_scale, d_info 8); an in_dim
 * that is no feature length; h1 or h2 outside 1..64; lr negative or not finite; a beta outside [0, 1); eps not positive;
 * max_grad_norm NaN (an infinity, 0 or a negative number: no clipping).
 */
int oc_adam_step(const OcActorCritic* params, const OcPolicyGrads* grads, const OcAdam* adam, void* stream);

/*
 * oc_adam_plan — what oc_adam_step would launch, as text:
 *   "k_adam_step grid=1, 256 lanes, 10823 elements (43 per lane), flat order w1 b1 w2 b2 wp bp wv bv, f64 norm in a fixed tree, 55580 B LDS"
 * The checks of the shape apply; usable without a GPU, like the other plan calls; refusals carry oc_adam_step's name.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_adam_plan(int in_dim, int h1, int h2, char* out, size_t out_size);

/*
 * The learner's update (ABI 6: entry points added beside the others) — a run of minibatches in ONE C call: for minibatch k of the
 * index, entries k M .. min((k + 1) M, n_index) - 1 (the last may be shorter), it enqueues on the caller's stream, with no host
 * synchronisation, exactly what these four calls enqueue:
 *   oc_policy_forward  rows d_index + k M of d_features -> d_logits, d_values
 *   oc_ppo_loss        the batch side and the five coefficients of `loss`, the same index entries as samples (an entry names both
 *                      the sample and its feature row) -> d_grad_logits, d_grad_values, d_loss_partials, d_stats[k]
 *   oc_policy_backward on those RAW gradients (not divided by the count) -> grads, through d_policy_partials
 *   oc_adam_step       with d_grad_scale = &d_stats[k][7] (1 / count; 0: the step is skipped) and d_info[k]
 * (csrc/update_chain.hpp: host code; the existing launch code, no kernel of its own).  The results are bit for bit those of the four
 * calls made one by one.  The scratch is one minibatch's and is reused from minibatch to minibatch: the stream orders them.
 * Of `loss`, d_logits, d_values, d_index, first_sample, n_minibatch, d_grad_logits, d_grad_values, d_partials, d_stats and d_terms_out
 * are not read; of `adam`, d_grad_scale and d_info are not.
 */
typedef struct OcPpoUpdate {
    const float*   d_features;         /* [n_feature_rows][in_dim] f32, 16-byte aligned (OcPolicyRows') */
    int64_t n_feature_rows;
    const int32_t* d_index;            /* [n_index] i32, 4-byte aligned; required */
    int64_t n_index;                   /* >= 0, below 2^31 */
    int64_t minibatch;                 /* M >= 1 */
    float*         d_logits;           /* scratch [min(M, n_index)][6] f32, 16-byte aligned */
    float*         d_values;           /* scratch [min(M, n_index)] f32, 4-byte aligned */
    float*         d_grad_logits;      /* scratch [min(M, n_index)][6] f32, 16-byte aligned */
    float*         d_grad_values;      /* scratch [min(M, n_index)] f32, 4-byte aligned */
    double*        d_loss_partials;    /* scratch f64, 8-byte aligned: the rows oc_ppo_update_plan states */
    float*         d_policy_partials;  /* scratch f32, 4-byte aligned: the rows oc_ppo_update_plan states */
    OcPolicyGrads  grads;              /* scratch: the eight gradient arrays; they hold the last minibatch's raw gradients afterwards */
    double*        d_stats;            /* [K][8] f64 out: oc_ppo_loss's d_stats of every minibatch; 8-byte aligned */
    double*        d_info;             /* [K][4] f64 out: oc_adam_step's d_info of every minibatch; 8-byte aligned */
} OcPpoUpdate;

/*
 * oc_ppo_update — K = ceil(n_index / M) minibatches.  n_index == 0 launches nothing.
 * OC_EINVAL, before the FIRST launch of the call, with this entry point's name in front of the message: a NULL policy, loss, adam
 * or update; n_index < 0 or >= 2^31; minibatch < 1; a NULL d_index, d_stats, d_info or d_loss_partials; and every refusal of the
 * four calls above for every minibatch, in their words.
 */
int oc_ppo_update(const OcActorCritic* policy, const OcPpoLoss* loss, const OcAdam* adam, const OcPpoUpdate* update, void* stream);

/*
 * oc_ppo_update_plan — what oc_ppo_update would launch, as text: K, the kernels of one (the first, longest) minibatch in the words
 * of oc_policy_plan, oc_ppo_loss_plan and oc_adam_plan, and the sizes of the scratch and of the outputs:
 *   "16 minibatch(es) of 4096 rows (the last 4096), no host synchronisation, each: [k_policy_forward grid=32, ...] + [k_ppo_loss<OLD=false> grid=4, ...] + [k_policy_backward<F0=0,NF=3,REST> grid=32, ... + k_policy_grad_sum grid=43, ...] + [k_adam_step grid=1, ...]; scratch: logits 4096 x 6 f32, values 4096 f32, grad_logits 4096 x 6 f32, grad_values 4096 f32, loss partials 4 x 6 f64, policy partials 32 x 10823 f32, gradients 10823 f32; out: stats 16 x 8 f64, info 16 x 4 f64"
 *   "nothing to launch (no index); scratch: ..."
 * The checks that need no array apply; usable without a GPU, like the other plan calls; refusals carry oc_ppo_update's name.
 *   out, out_size caller's text buffer (>= 2048 bytes holds every answer)
 */
int oc_ppo_update_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_seat, int with_moments, int with_old_logits,
                       char* out, size_t out_size);

/*
 * The behaviour-cloning loss head (ABI 6: entry points added beside the others; no existing signature, struct or option changes, so
 * the version stays) — the objective of the reference's BC partner (human_aware_rl/imitation/behavior_cloning_tf2.py: Keras's
 * SparseCategoricalCrossentropy(from_logits=True) with optional class_weight and the sparse categorical accuracy metric) on the
 * logits of a minibatch, with its gradients, in one launch (k_bc_loss, csrc/bc_loss.hpp).
 *
 * Layout.  The batch side is S samples: an action byte each (and, for oc_bc_update, a feature row each).  The minibatch side — the
 * policy's logits of M samples, in the order of its forward pass — names its samples through d_index, or is samples first_sample ..
 * first_sample + M - 1.
 *
 * Arithmetic.  Per minibatch row, with l = the row's logits; every operation is f32 with one rounding, in this order, with no
 * contraction, expf and logf in full precision.  The softmax is OcPpoLoss's:
 *   m = max l_i;  d_i = l_i - m;  w_i = expf(d_i);  S = ((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5
 *   lp_i = d_i - logf(S);  p_i = w_i / S
 *   a = d_actions[s];  c = d_class_weights[a], or 1.0f without d_class_weights;  ce = -lp_a;  the row's loss is c * ce
 *   correct = (a == the lowest i with l_i == m)     (ties go to the lowest index, as argmax does; a row with a NaN logit is never correct)
 * Gradients of c * ce, per sample, not divided by the count:
 *   d/dl_i = c * (p_i - [i == a])     (one subtraction, one multiply)
 *   d/dv   = +0.0f     (d_grad_values is written so that oc_policy_backward runs unchanged: the value head gets zero gradients)
 * A -inf logit at the taken action gives lp_a = -inf, ce = +inf and p_a = 0: the row's loss, the sum and d_stats[1] are +inf (with a zero
 * class weight, 0 * inf: a NaN) while its gradient c * (p_i - [i == a]) stays finite.  A -inf logit elsewhere gives p_i = 0 there and
 * changes nothing else.  Neither is hidden.
 * Left-out rows.  A row is left out when its index is outside 0 .. S - 1 or when d_actions[s] > 5 (255: the sampler's invalid row).
 * Its gradients and its loss are +0.0f, by a select, so that a NaN anywhere in its inputs reaches nothing, and it enters no sum.
 * Class weights.  d_class_weights holds six f32 that must be finite and >= 0.  They are read on the device: the host checks the
 * pointer's alignment and nothing else.
 * Sums.  d_partials[k] = {count, sum c * ce, number correct, sum c} over the kept rows of minibatch rows [P k, P k + P), P = 1024
 * (oc_bc_loss_plan states it): each term widened to f64 before it is added, in a fixed tree.  d_stats = {count, loss = sum c * ce /
 * count, accuracy = number correct / count, mean weight = sum c / count, 0, 0, 0, 1 / count}: the partials added in ascending k; all zeros
 * when count == 0.  Slot 7 is where oc_adam_step reads d_grad_scale, as it does behind oc_ppo_loss.  The loss divides by the count,
 * not by the sum of the weights: Keras's class_weight convention.  No floating-point atomics: the same call on the same inputs gives
 * the same bits.
 */
typedef struct OcBcLoss {
    const uint8_t* d_actions;        /* [S] u8: the demonstrated actions; any address; required */
    const float*   d_class_weights;  /* [6] f32: the weight of every action, finite and >= 0 (not checked); 4-byte aligned; NULL = all 1 */
    int64_t n_samples;               /* S >= 0 */
    const float*   d_logits;         /* [M][6] f32: the policy's logits of the minibatch; 8-byte aligned; required */
    const int32_t* d_index;          /* [M] i32: the sample of every row; 4-byte aligned; NULL = first_sample + row */
    int64_t first_sample;            /* read without d_index only */
    int64_t n_minibatch;             /* M >= 0 */
    float*         d_grad_logits;    /* [M][6] f32 out; 8-byte aligned; NULL together with d_grad_values: evaluation, no gradient stores */
    float*         d_grad_values;    /* [M] f32 out: +0.0f everywhere; 4-byte aligned; NULL together with d_grad_logits */
    float*         d_loss_out;       /* [M] f32 out: c * ce of every row; 4-byte aligned; or NULL */
    double*        d_partials;       /* [ceil(M / P)][4] f64 out; 8-byte aligned; or NULL (then d_stats must be NULL too) */
    double*        d_stats;          /* [8] f64 out; 8-byte aligned; or NULL */
} OcBcLoss;

/*
 * oc_bc_loss — k_bc_loss, one lane per minibatch row and four rows per lane, and, with d_stats, k_bc_loss_stats behind it (one
 * wavefront adding the partials).  n_minibatch == 0 launches nothing and returns 0; d_stats is then set to zeros.  With d_grad_logits
 * and d_grad_values both NULL the call evaluates: sums, stats and d_loss_out only.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL struct, d_actions or d_logits; one
 * of d_grad_logits and d_grad_values without the other; a misaligned array; n_minibatch < 0 or n_samples < 0; n_samples >= 2^31 with
 * d_index; without d_index a first_sample < 0 or first_sample + n_minibatch > n_samples; d_stats without d_partials.
 */
int oc_bc_loss(const OcBcLoss* q, void* stream);

/*
 * oc_bc_loss_plan — what oc_bc_loss would launch, as text (with_...: the optional array is given; with_gradients: d_grad_logits and d_grad_values are):
 *   "k_bc_loss<GRAD=true> grid=4096, 256 lanes (one per sample, 4 tiles of 256), 1024 samples per partial, index=yes class_weights=yes loss_out=no + k_bc_loss_stats grid=1, 64 lanes, 4096 partial(s) (with d_stats)"
 *   "nothing to launch (no samples)"
 * Usable without a GPU, like the other plan calls; refusals carry oc_bc_loss's name.
 *   out, out_size caller's text buffer (>= 256 bytes holds every answer)
 */
int oc_bc_loss_plan(int64_t n_minibatch, int with_index, int with_class_weights, int with_gradients, int with_loss_out, char* out, size_t out_size);

/*
 * The behaviour-cloning update (ABI 6: entry points added beside the others) — OcPpoUpdate's chain with the cross-entropy head: for
 * minibatch k of the index, entries k M .. min((k + 1) M, n_index) - 1 (the last may be shorter), it enqueues on the caller's stream,
 * with no host synchronisation, exactly what these four calls enqueue:
 *   oc_policy_forward  rows d_index + k M of d_features -> d_logits, d_values
 *   oc_bc_loss         the actions, n_samples and class weights of `loss`, the same index entries as samples (an entry names both the
 *                      sample and its feature row) -> d_grad_logits, d_grad_values (zeros), d_loss_partials, d_stats[k]
 *   oc_policy_backward on those RAW gradients (not divided by the count) -> grads, through d_policy_partials
 *   oc_adam_step       with d_grad_scale = &d_stats[k][7] (1 / count; 0: the step is skipped) and d_info[k]
 * (csrc/update_chain.hpp: host code; the existing launch code, no kernel of its own).  The results are bit for bit those of the four
 * calls made one by one.  The scratch is one minibatch's and is reused from minibatch to minibatch: the stream orders them.
 * Of `loss`, d_logits, d_index, first_sample, n_minibatch, d_grad_logits, d_grad_values, d_loss_out, d_partials and d_stats are not
 * read; of `adam`, d_grad_scale and d_info are not.
 */
typedef struct OcBcUpdate {
    const float*   d_features;         /* [n_feature_rows][in_dim] f32, 16-byte aligned (OcPolicyRows') */
    int64_t n_feature_rows;
    const int32_t* d_index;            /* [n_index] i32, 4-byte aligned; required */
    int64_t n_index;                   /* >= 0, below 2^31 */
    int64_t minibatch;                 /* M >= 1 */
    float*         d_logits;           /* scratch [min(M, n_index)][6] f32, 8-byte aligned */
    float*         d_values;           /* scratch [min(M, n_index)] f32, 4-byte aligned */
    float*         d_grad_logits;      /* scratch [min(M, n_index)][6] f32, 8-byte aligned */
    float*         d_grad_values;      /* scratch [min(M, n_index)] f32, 4-byte aligned */
    double*        d_loss_partials;    /* scratch f64, 8-byte aligned: the rows oc_bc_update_plan states */
    float*         d_policy_partials;  /* scratch f32, 4-byte aligned: the rows oc_bc_update_plan states */
    OcPolicyGrads  grads;              /* scratch: the eight gradient arrays; they hold the last minibatch's raw gradients afterwards */
    double*        d_stats;            /* [K][8] f64 out: oc_bc_loss's d_stats of every minibatch; 8-byte aligned */
    double*        d_info;             /* [K][4] f64 out: oc_adam_step's d_info of every minibatch; 8-byte aligned */
} OcBcUpdate;

/*
 * oc_bc_update — K = ceil(n_index / M) minibatches.  n_index == 0 launches nothing.
 * OC_EINVAL, before the FIRST launch of the call, with this entry point's name in front of the message: a NULL policy, loss, adam
 * or update; n_index < 0 or >= 2^31; minibatch < 1; a NULL d_index, d_stats, d_info or d_loss_partials; and every refusal of the
 * four calls above for every minibatch, in their words (a NULL d_grad_logits or d_grad_values is oc_policy_backward's refusal here,
 * not an evaluation).
 */
int oc_bc_update(const OcActorCritic* policy, const OcBcLoss* loss, const OcAdam* adam, const OcBcUpdate* update, void* stream);

/*
 * oc_bc_update_plan — what oc_bc_update would launch, as text: K, the kernels of one (the first, longest) minibatch in the words of
 * oc_policy_plan, oc_bc_loss_plan and oc_adam_plan, and the sizes of the scratch and of the outputs:
 *   "16 minibatch(es) of 4096 rows (the last 4096), no host synchronisation, each: [k_policy_forward grid=32, ...] + [k_bc_loss<GRAD=true> grid=4, ...] + [k_policy_backward<F0=0,NF=3,REST> grid=32, ... + k_policy_grad_sum grid=43, ...] + [k_adam_step grid=1, ...]; scratch: logits 4096 x 6 f32, values 4096 f32, grad_logits 4096 x 6 f32, grad_values 4096 f32, loss partials 4 x 4 f64, policy partials 32 x 10823 f32, gradients 10823 f32; out: stats 16 x 8 f64, info 16 x 4 f64"
 *   "nothing to launch (no index); scratch: ..."
 * The checks that need no array apply; usable without a GPU, like the other plan calls; refusals carry oc_bc_update's name.
 *   out, out_size caller's text buffer (>= 2048 bytes holds every answer)
 */
int oc_bc_update_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_class_weights, char* out, size_t out_size);

/*
 * The behaviour-cloning update of small minibatches in ONE kernel (ABI 6: entry points added beside the others) — what oc_bc_update
 * computes, for the shapes in which every stage of its chain is one workgroup, by k_bc_epoch_fused (csrc/bc_fused.hpp): ONE workgroup
 * of 256 lanes that walks the minibatches of the index in order, each from the weights the one before left, with no intermediate
 * array — logits, upstream gradients, partial sums and weight gradients stay in LDS and registers.
 * Shapes served: minibatch 1..128; in_dim 56, 76 or 96; h1 and h2 in 1..64.  For these the parameters, the moments, the clock,
 * d_stats and d_info after the call are oc_bc_update's BIT FOR BIT: the arithmetic and every order of summation are those stated for
 * OcActorCritic, OcBcLoss and OcAdam above.  (A NaN norm in d_info is "a NaN" in both, its payload unspecified.)
 * Its own argument block rather than OcBcUpdate with six members ignored: the call takes NO scratch, and a block without scratch
 * members cannot be handed a stale or missing one.  Of `loss`, d_actions, d_class_weights and n_samples are read (an index entry names
 * both the sample and its feature row); of `adam`, d_grad_scale and d_info are not read.
 * Launches: the epoch is cut into launches of at most 64 minibatches (oc_bc_epoch_fused_plan states the number), chained on the
 * caller's stream without synchronising.
 */
typedef struct OcBcEpochFused {
    const float*   d_features;      /* [n_feature_rows][in_dim] f32, 16-byte aligned (OcPolicyRows') */
    int64_t n_feature_rows;
    const int32_t* d_index;         /* [n_index] i32, 4-byte aligned; required */
    int64_t n_index;                /* >= 0, below 2^31 */
    int64_t minibatch;              /* M in 1..128 */
    double*        d_stats;         /* [K][8] f64 out: oc_bc_loss's d_stats of every minibatch; 8-byte aligned */
    double*        d_info;          /* [K][4] f64 out: oc_adam_step's d_info of every minibatch; 8-byte aligned */
} OcBcEpochFused;

/*
 * oc_bc_epoch_fused — K = ceil(n_index / M) minibatches, the last one shorter.  n_index == 0 launches nothing.  params' eight arrays
 * and the moments are WRITTEN THROUGH, as by oc_adam_step.
 * OC_EINVAL, before the FIRST launch of the call, with this entry point's name in front of the message: a NULL policy, loss, adam or
 * epoch; n_index < 0 or >= 2^31; a minibatch outside 1..128 and an in_dim other than 56, 76 or 96 (the messages say what is served
 * and that oc_bc_update serves the rest); h1 or h2 outside 1..64; a NULL d_index, d_stats or d_info; misaligned d_stats or d_info;
 * oc_policy_forward's refusals of the weights, the feature rows and the index; a NULL d_actions, a misaligned d_class_weights,
 * n_samples < 0 or >= 2^31; oc_adam_step's refusals of the moments, the clock and the hyperparameters.
 */
int oc_bc_epoch_fused(const OcActorCritic* policy, const OcBcLoss* loss, const OcAdam* adam, const OcBcEpochFused* epoch, void* stream);

/*
 * oc_bc_epoch_fused_plan — what oc_bc_epoch_fused would launch, as text:
 *   "k_bc_epoch_fused<NF=3> grid=1, 256 lanes (4 wavefronts x one 32-row tile), 400 minibatch(es) of 64 rows (the last 64), at most 64 minibatches per launch: 7 launch(es), no host synchronisation, 32 x 32 x 2 f32 MFMA, 12 accumulator tiles per wavefront, 10823 elements (43 per lane) in Adam's phases, class_weights=no, 158016 B LDS; no scratch; out: stats 400 x 8 f64, info 400 x 4 f64"
 *   "nothing to launch (no index); no scratch; out: stats 0 x 8 f64, info 0 x 4 f64"
 * The checks that need no array apply; usable without a GPU, like the other plan calls; refusals carry oc_bc_epoch_fused's name.
 *   out, out_size caller's text buffer (>= 1024 bytes holds every answer)
 */
int oc_bc_epoch_fused_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_class_weights, char* out, size_t out_size);

/*
 * The learner's sample index (ABI 6: entry points added beside the others; no existing signature, struct or option changes, so the
 * version stays) — the d_index of oc_ppo_update and oc_bc_update, made on the device (csrc/sample_index.hpp): first the samples of a
 * collected batch that the loss uses, then a permutation of them that is a stated function of (seed, epoch), like every other random
 * stream of the library.  With a behaviour-cloning partner about half of a batch's samples are the partner's: oc_ppo_loss leaves
 * them out, but a minibatch cut from a permutation of all S samples still carries them through the policy's forward and backward
 * pass, and its count of learner samples is about half its size.  A minibatch cut from this index holds learner samples only, as the
 * reference's train batch does, whose sgd_minibatch_size counts learner samples.
 *
 * Selection.  Sample s of 0 .. S - 1 (s = (t * n_envs + e) * 2 + p, as for OcPpoLoss) is selected when both hold:
 *   d_seat == NULL or d_seat[s >> 1] != (s & 1)        (not the partner's sample)
 *   d_actions == NULL or d_actions[s] <= 5             (not the sampler's invalid row)
 * — oc_ppo_loss's left-out rules without the one on the index range.  With L the number of selected samples, d_ids[0 .. L) holds
 * them in ascending order, d_ids[L .. S) holds -1 and *d_count = L.
 *
 * Permutation.  d_index[i] = d_ids[pi(i)] for i < min(L, n_out) and -1 for L <= i < n_out, with L = *d_count READ ON THE DEVICE (the
 * host need not know it) and pi a bijection of 0 .. L - 1, in u32 arithmetic that wraps:
 *   keys: for j = 0, 1:  k[4j .. 4j+3] = philox4x32_10(counter = {epoch_lo, epoch_hi, j, 0}, key = {seed_lo, seed_hi ^ 0x53485546})
 *         ("SHUF"): eight round keys, the same for every i
 *   L <= 1:  pi(0) = 0
 *   otherwise:  w = max(1, bit length of L - 1),  a = w >> 1,  c = w - a
 *     mix(v):  v *= 0x9E3779B1;  v ^= v >> 16;  v *= 0x85EBCA6B;  v ^= v >> 13
 *     top(v, q) = q ? v >> (32 - q) : 0
 *     x = i;  repeat {  l = x >> c,  r = x & (2^c - 1);
 *                       for j = 0 .. 7:  even j:  l ^= top(mix(r + k[j]), a),   odd j:  r ^= top(mix(l + k[j]), c);
 *                       x = (l << c) | r  }  until x < L;   pi(i) = x
 * Each of the eight rounds changes one half by a function of the other, so together they are a bijection of 0 .. 2^w - 1, and
 * 2^w < 2 L.  The repeat ("cycle walking") follows that bijection's cycle from a point below L until it is below L again: it ends
 * by construction (the cycle returns to i), pi is a bijection of 0 .. L - 1, and it evaluates the rounds fewer than 2 times per
 * element on average.  Every lane walks alone: nothing waits for another lane.  It is a shuffle for SGD, not a cipher: nothing
 * here is meant to withstand someone who wants to predict it.
 * No atomics in either call: the same call on the same inputs gives the same bytes.
 */

/*
 * oc_sample_select — three launches on the caller's stream, in none of which a workgroup waits for another (no look-back, no spin
 * flags): k_sample_count writes the number of selected samples of every block of P = 1024 consecutive samples (a wavefront's count
 * is the popcount of a __ballot), k_sample_scan, one workgroup, turns the counts into exclusive offsets and writes *d_count,
 * k_sample_write evaluates the rule again, ranks a sample inside its block (ballot prefix, an LDS prefix across wavefronts) and
 * stores it at the block's offset; position s >= L gets its -1 from the lane of sample s.  n_samples == 0 launches only what sets
 * *d_count = 0.
 *   n_samples        S, 0 .. 2^31 - 1; even when d_seat is given
 *   d_seat           [S / 2] u8: the partner's player of (t, e), else no partner; any address; NULL = no partner anywhere
 *   d_actions        [S] u8; any address; NULL = every action valid
 *   d_ids            [S] i32 out; 4-byte aligned; required
 *   d_count          [1] i64 out; 8-byte aligned; required
 *   d_block_offsets  [max(1, ceil(S / P))] u32 scratch (oc_sample_index_plan states its bytes); 4-byte aligned; required
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL d_ids, d_count or
 * d_block_offsets; a misaligned one; n_samples < 0 or >= 2^31; an odd n_samples with d_seat.
 */
int oc_sample_select(int64_t n_samples, const uint8_t* d_seat, const uint8_t* d_actions, int32_t* d_ids, int64_t* d_count,
                     uint32_t* d_block_offsets, void* stream);

/*
 * oc_sample_permute — one launch (k_sample_permute): one lane per output, at most 1024 workgroups, outputs beyond them by grid
 * stride.  n_out == 0 launches nothing.
 *   d_ids    [>= *d_count] i32: oc_sample_select's; 4-byte aligned; NULL = the identity (ids[j] = j): a plain permutation of
 *            0 .. L - 1, for a learner whose every sample counts (oc_bc_update)
 *   d_count  [1] i64: L, 0 .. 2^31 - 1, read on the device; 8-byte aligned; required
 *   n_out    how many entries of d_index to write, 0 .. 2^31 - 1: L where the host knows it; S without reading L back, the
 *            entries from L on are then -1, which oc_ppo_loss and the policy's passes leave out
 *   seed, epoch   the stream's key and counter, all 64 bits of both
 *   d_index  [n_out] i32 out; 4-byte aligned; required
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL d_count or d_index; a misaligned
 * d_ids, d_count or d_index; n_out < 0 or >= 2^31.
 */
int oc_sample_permute(const int32_t* d_ids, const int64_t* d_count, int64_t n_out, uint64_t seed, uint64_t epoch, int32_t* d_index,
                      void* stream);

/*
 * oc_sample_index_plan — what the two calls would launch, as text (with_seat, with_actions, with_ids: the optional array is
 * given; n_learner: L, for the permutation's w, a and c):
 *   "select: k_sample_count<SEAT=true, ACT=true> grid=51200, 256 lanes + k_sample_scan grid=1, 256 lanes, 200 pass(es) of 256 blocks, 8 passes in flight + k_sample_write<SEAT=true, ACT=true> grid=51200, 256 lanes; P = 1024 samples per block, scratch 204800 B; permute: k_sample_permute<IDS=true> grid=1024, 256 lanes (one per output, 100 output(s) per lane at most); L = 26214400: w = 25, a = 12, c = 13"
 *   "select: k_sample_scan grid=1, 256 lanes, 0 pass(es) (no samples: *d_count = 0); P = 1024 samples per block, scratch 4 B; permute: nothing to launch (no output); L = 0: w = 1, a = 0, c = 1"
 * Usable without a GPU, like the other plan calls.  The checks that need no array apply, under the name of the call they belong
 * to; n_learner outside 0 .. 2^31 - 1 is refused under this call's name.
 *   out, out_size caller's text buffer (>= 640 bytes holds every answer)
 */
int oc_sample_index_plan(int64_t n_samples, int with_seat, int with_actions, int with_ids, int64_t n_out, int64_t n_learner, char* out,
                         size_t out_size);

/*
 * Episode outcomes of a collected batch by partner member and seat (additive to ABI version 6: two new entry points, the version
 * stays) — how well anyone played, from the arrays the step calls already write (csrc/outcomes.hpp).  oc_multi_agent_step_sample
 * copies the episode totals of every env to d_ep_returns_out at every step; they are final where the done mask is set.  Kept per
 * step, time-major like OcGaeBatch, next to the done mask, the seats and the members of a partner pool, one reduction gives the
 * table cross-play tables and prioritised partner sampling are built from.
 *
 * Episodes.  An episode ends at (t, e) iff d_done[t][e] != 0.  Its row is d_ep_returns[t][e][0..3] = (sparse p0, sparse p1, shaped
 * p0, shaped p1), and R = (double) sparse p0 + (double) sparse p1.  d_ep_returns is READ ONLY WHERE d_done IS SET: nothing else the
 * array holds, a NaN included, reaches the result.
 *
 * Groups.  G = 1 without d_seat, else 1 + 2 K (K = n_members).  With s = d_seat[t][e] and m = d_member[t][e] (0 without d_member):
 *   no d_seat, or s == 255      group 0, "no partner" (m is not looked at)
 *   s <= 1 and m < K            group 1 + 2 m + s, "member m plays seat s"
 *   anything else               no group: the episode adds 1 to d_table[G][0], "unattributed", and nothing else anywhere in d_table
 *
 * d_table, f64 [G + 1][8].  Row g < G, over the episodes of group g:
 *   [0] episodes   [1] sum R   [2] sum R * R   [3] min R (+inf: no episode)   [4] max R (-inf: no episode)
 *   [5] sum shaped p0   [6] sum shaped p1   [7] sum sparse p0
 * Row G holds the unattributed count in [0] and 0, 0, +inf, -inf, 0, 0, 0 behind it.
 * d_env_table, f64 [n_envs][4], optional: episodes, sum R, sum R * R, sum ((double) shaped p0 + (double) shaped p1) of env e over
 * ALL its episodes, attributed or not, added in ascending t.  A caller groups it by anything constant per env (the layout of a mixed
 * batch) with one index_add.
 *
 * Order of summation — a function of (n_steps, n_envs, the block of envs B = 256 the plan names) and of nothing else.  Every sum
 * starts at +0.0, every min at +inf, every max at -inf; a product R * R is rounded to f64 before it is added; min and max are fmin
 * and fmax.  "Adding" a table to another adds columns 0, 1, 2, 5, 6, 7, takes the min of column 3 and the max of column 4, entry by
 * entry, the running table on the left.
 *   1. Wavefront q of block b holds the envs b * B + 64 q .. b * B + 64 q + 63 (those below n_envs).  Its table starts empty and
 *      takes its episodes one at a time, in ascending t and, within a step, in ascending e.
 *   2. The partial of block b (d_scratch[b]) is the empty table plus the tables of its wavefronts q = 0, 1, 2, 3, in that order.
 *   3. d_table is the empty table plus the partials b = 0, 1, ..., ceil(n_envs / B) - 1, in that order.
 * No atomics on floating-point data, no look-back, no spin flags: the same call on the same inputs gives the same bytes.  Counts, min
 * and max are exact whatever the order, and so is every sum of the env's own returns (multiples of 20, sums of 3s and 5s).
 * Cost: the done lanes of a wavefront take turns.  64 envs of a wavefront finishing on one step (equal horizons) are 64 short turns
 * on that step, once per horizon; a batch that is done on every step takes a turn per env and step: slow, and correct.
 */
typedef struct OcOutcomeBatch {
    const uint8_t* d_done;        /* [n_steps][n_envs] u8; any address */
    const float* d_ep_returns;    /* [n_steps][n_envs][4] f32; 16-byte aligned; read only where d_done is set */
    const uint8_t* d_seat;        /* [n_steps][n_envs] u8 or NULL (no partner anywhere: G = 1); any address */
    const uint8_t* d_member;      /* [n_steps][n_envs] u8 or NULL (one partner policy: n_members == 1); any address; needs d_seat */
    double* d_table;              /* [G + 1][8] f64 out; 8-byte aligned; required */
    double* d_env_table;          /* [n_envs][4] f64 out or NULL; 8-byte aligned */
    double* d_scratch;            /* the bytes oc_outcome_plan states (ceil(n_envs / 256) * (G + 1) * 64); 8-byte aligned; what it held does not matter */
    int64_t n_envs;               /* N >= 0; 0 writes the empty table */
    int64_t n_steps;              /* T >= 1; T * N < 2^31 */
    int n_members;                /* K, 1..16; 1 when d_member is NULL */
} OcOutcomeBatch;

/*
 * oc_outcome_table — two launches on the caller's stream: k_outcomes, a lane per env walking t upwards with the bytes of the next 16
 * steps in flight, writes one partial per block of 256 envs (and d_env_table); k_outcome_sum, one wavefront, adds the partials.
 * n_envs == 0 launches k_outcome_sum alone, which writes the empty table.
 * OC_EINVAL, before any device call, with this entry point's name in front of the message: a NULL batch or d_table; a NULL d_done,
 * d_ep_returns or d_scratch where n_envs > 0; a d_ep_returns that is not 16-byte aligned; a d_table, d_env_table or d_scratch that is
 * not 8-byte aligned; d_member without d_seat; n_members outside 1..16, or not 1 without d_member; n_steps < 1; n_envs < 0;
 * n_steps * n_envs >= 2^31.
 */
int oc_outcome_table(const OcOutcomeBatch* q, void* stream);

/*
 * oc_outcome_plan — what a call would launch, as text (with_seat, with_member, with_env_table: the optional array is given):
 *   "k_outcomes<SEAT=true, MEMBER=true, ENV=false> grid=256, 256 lanes (one per env; one partial per block of 256 envs), 16 steps per prefetch block, 25 block(s) + k_outcome_sum grid=1, 64 lanes; G = 7 group(s), table 512 B, scratch 131072 B"
 *   "k_outcome_sum grid=1, 64 lanes (no envs: the empty table); G = 1 group(s), table 128 B, scratch 0 B"
 * Usable without a GPU, like the other plan calls.  The checks that need no array apply, under oc_outcome_table's name.
 *   out, out_size caller's text buffer (>= 384 bytes holds every answer)
 */
int oc_outcome_plan(int64_t n_envs, int64_t n_steps, int with_seat, int with_member, int n_members, int with_env_table, char* out,
                    size_t out_size);

#ifdef __cplusplus
}
#endif
#endif /* OC_AMD_H */
