// shared.hpp — what the translation units of liboc_amd.so share (everything else is internal to a unit: the kernels and
// their helpers live in headers that each unit includes inside its own anonymous namespace).
// Units: oc_amd.hip (the C-ABI and every kernel family but k_rollout4) and rollout4.hip, compiled three times with
// -DOC_R4_PART=0/1/2 (k_rollout4's instances: joint-table + event-logging / per-env-terrain MODE 2 / arithmetic MODE 0), so
// that a clean build compiles them in parallel (overcooked_ai_amd/build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/oc_amd.h"

#define OC_HIDDEN __attribute__((visibility("hidden")))

namespace oc_detail {

// (__thread, not thread_local: a C++ thread_local referenced from another translation unit goes through a "TLS init function"
//  hook that is weak-undefined for these constant-initialised variables; with hidden visibility the null test is folded away and
//  the first access from rollout4.hip jumped to the library's base address — found in round 6 by oc_rollout_plan, latent since
//  round 4 on the error paths of the rollout4 units)
extern __thread char g_err[256] OC_HIDDEN;       // oc_last_error()
extern __thread bool g_lds_refused OC_HIDDEN;    // a dynamic-LDS request was refused: nothing was launched

// Launch-time description of the start_state_fn (include/oc_amd.h, OcStartSpec), by value in kernel arguments.
struct StartArgs {
    uint32_t enabled, seed_lo, seed_hi, epoch;
    int64_t env_offset;
    uint64_t thresh;  // floor(rnd_obj_prob_thresh * 2^32)
    int32_t random_start_pos;
    uint32_t regen_first, regen_count;  // regen_count > 0: a restarted env moves to layout regen_first + draw % regen_count
    uint16_t* layout_ids;               // the batch's layout ids, writable (regen_count > 0)
};

// Where the event_infos of a launch go (include/oc_amd.h, OcEventSink), by value in kernel arguments.
struct EvArgs {
    uint64_t* events;       // [n_steps][n_envs] masks, or NULL
    uint32_t* counts;       // [n_envs][25] running counts of the current episode (player 0: bits 0..15, player 1: 16..31), or NULL
    uint32_t* counts_done;  // [n_envs][25] counts of the last finished episode, or NULL
    uint32_t clear_on_done; // the caller restarts finished envs itself right after this launch (oc_multi_agent_step)
};

// Where a recorded launch (oc_rollout_record / oc_rollout_record_ex) writes each step's pre-step state, actions and layout id,
// by value in kernel arguments; all NULL in every other launch.
struct RecArgs {
    uint8_t* actions;       // [n_steps][n_envs][2] u8, or NULL
    void* states;           // [n_steps][n_planes][n_envs][16] wire-format states, 16-byte aligned, or NULL
    uint16_t* layout_ids;   // [n_steps][n_envs]: the layout id of the state of slice k (after re-draws), or NULL
};

// ---- The instances of k_rollout4 (step_lut4.hpp).  Each is a traits struct: R4Base's members, overridden by name.  The base
//      is the instance that serves any table (arithmetic movement, up to 8 pot slots, records read through L2, either dynamics).
template <class D>  // D: the instance (its choices are read by the derived values below)
struct R4Base {
    static constexpr bool UNIFORM = false;  // one layout: its tables and cook times are staged once per workgroup
    static constexpr int MAXP = 8;          // pot slots per env
    static constexpr bool LAY_LDS = false;  // the layout records are staged in LDS (<= LDS_LAYOUT_MAX layouts)
    static constexpr int MODE = 0;          // 0 arithmetic movement, 1 JOINT move table, 2 per-env terrain, pose one step ahead
    static constexpr bool OUT = false;      // both output arrays are present: no per-step NULL tests
    static constexpr bool OLD = true;       // some layout may use old dynamics
    static constexpr bool EV = false;       // event_infos are logged (EvArgs)
    static constexpr bool PIPE = true;      // MODE 1 / 2: the next step's faced cells are read one step ahead
    static constexpr bool RU = false;       // one set of shaping rewards and one dynamics flag for the whole table
    static constexpr int CW = 2;            // bytes of a cell word
    static constexpr bool NOCONF = false;   // the two players can never face the same cell (OC_BATCH_NO_SHARED_FACES)
    static constexpr bool FT8 = false;      // the flags array is tiled by 8 steps (OC_OPT_FLAGS_TILED8)
    static constexpr bool REC = false;      // every step's pre-step state, actions and layout id are stored too (oc_rollout_record*)
    // derived
    static constexpr bool RUX = D::UNIFORM || D::RU;  // one LUT variant, patched with the reward floats
    static constexpr int NF = D::MODE == 1 ? 6 : 0;   // free cells the move table has room for
    static constexpr int PART = D::EV || D::MODE == 1 ? 0 : D::MODE == 2 ? 1 : 2;  // the rollout4.hip unit (OC_R4_PART) that compiles it
    static constexpr bool legal() {
        static_assert(D::CW == 2 || D::CW == 4, "cell words are u16 or u32");
        static_assert(!D::REC || (D::MODE == 0 && D::CW == 2 && !D::FT8), "recording is served by the arithmetic-movement instances");
        static_assert(!D::FT8 || ((D::MODE == 1 || D::MODE == 2) && D::OUT && !D::EV),
                      "the tiled flags array is served by joint-table and per-env-terrain instances");
        return true;
    }
};

// Every instance, with the batches choose_rollout (oc_amd.hip) gives it.  "Pipelined": <= ~1.5 wavefronts per SIMD (PIPE with
// 32-bit cell words); "lean": bigger batches.
// -- event logging (arithmetic movement, either dynamics)
struct R4EvUniform : R4Base<R4EvUniform> {  // one layout, <= 2 pots
    static constexpr bool UNIFORM = true, LAY_LDS = true, EV = true; static constexpr int MAXP = 2;
};
struct R4EvSmall : R4Base<R4EvSmall> { static constexpr bool EV = true; static constexpr int MAXP = 2; };  // mixed tables, <= 2 pots
struct R4EvGeneral : R4Base<R4EvGeneral> { static constexpr bool EV = true; };  // more than 2 pots
// -- JOINT move table: one two-player, one-pot, new-dynamics layout with 2..6 free cells, launches of >= 8 steps ("pipelined": also
//    <= 64 cells and no shared faced cells)
struct R4JointTiled : R4Base<R4JointTiled> {  // pipelined, tiled flags
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false, NOCONF = true, FT8 = true;
    static constexpr int MAXP = 1, MODE = 1, CW = 4;
};
struct R4JointPipe : R4Base<R4JointPipe> {  // pipelined
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false, NOCONF = true;
    static constexpr int MAXP = 1, MODE = 1, CW = 4;
};
struct R4JointLean : R4Base<R4JointLean> {  // big batches, shared faced cells or more than 64 cells
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false, PIPE = false; static constexpr int MAXP = 1, MODE = 1;
};
// -- MODE 2, per-env terrain: two players everywhere, <= 2 pots, <= 64 cells, one set of shaping rewards, new dynamics, both output
//    arrays, no event log (what k_rollout5 does not take of these: ragged batches, above 8 rounds, < 8 steps, ONE_WAVEFRONT)
struct R4TerrainUniform1 : R4Base<R4TerrainUniform1> {  // one one-pot layout, pipelined
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false; static constexpr int MAXP = 1, MODE = 2, CW = 4;
};
struct R4TerrainUniform : R4Base<R4TerrainUniform> {  // one layout, pipelined
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false; static constexpr int MAXP = 2, MODE = 2, CW = 4;
};
struct R4TerrainUniformLean : R4Base<R4TerrainUniformLean> {  // one layout, lean
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false, PIPE = false; static constexpr int MAXP = 2, MODE = 2;
};
struct R4TerrainLdsTiled : R4Base<R4TerrainLdsTiled> {  // table in LDS, pipelined, tiled flags
    static constexpr bool LAY_LDS = true, OUT = true, OLD = false, RU = true, FT8 = true; static constexpr int MAXP = 2, MODE = 2, CW = 4;
};
struct R4TerrainLds : R4Base<R4TerrainLds> {  // table in LDS, pipelined
    static constexpr bool LAY_LDS = true, OUT = true, OLD = false, RU = true; static constexpr int MAXP = 2, MODE = 2, CW = 4;
};
struct R4TerrainLdsLean : R4Base<R4TerrainLdsLean> {  // table in LDS, lean
    static constexpr bool LAY_LDS = true, OUT = true, OLD = false, RU = true, PIPE = false; static constexpr int MAXP = 2, MODE = 2;
};
struct R4TerrainL2OnePotTiled : R4Base<R4TerrainL2OnePotTiled> {  // one-pot table through L2, pipelined, tiled flags
    static constexpr bool OUT = true, OLD = false, RU = true, FT8 = true; static constexpr int MAXP = 1, MODE = 2, CW = 4;
};
struct R4TerrainL2OnePotLeanTiled : R4Base<R4TerrainL2OnePotLeanTiled> {  // one-pot table through L2, lean, tiled flags
    static constexpr bool OUT = true, OLD = false, RU = true, PIPE = false, FT8 = true; static constexpr int MAXP = 1, MODE = 2;
};
struct R4TerrainL2OnePot : R4Base<R4TerrainL2OnePot> {  // one-pot table through L2, pipelined
    static constexpr bool OUT = true, OLD = false, RU = true; static constexpr int MAXP = 1, MODE = 2, CW = 4;
};
struct R4TerrainL2OnePotLean : R4Base<R4TerrainL2OnePotLean> {  // one-pot table through L2, lean
    static constexpr bool OUT = true, OLD = false, RU = true, PIPE = false; static constexpr int MAXP = 1, MODE = 2;
};
struct R4TerrainL2 : R4Base<R4TerrainL2> {  // two-pot table through L2, pipelined
    static constexpr bool OUT = true, OLD = false, RU = true; static constexpr int MAXP = 2, MODE = 2, CW = 4;
};
struct R4TerrainL2Lean : R4Base<R4TerrainL2Lean> {  // two-pot table through L2, lean
    static constexpr bool OUT = true, OLD = false, RU = true, PIPE = false; static constexpr int MAXP = 2, MODE = 2;
};
// -- arithmetic movement (MODE 0): every other batch
struct R4ArithUniformOut : R4Base<R4ArithUniformOut> {  // one new-dynamics layout, <= 2 pots, both output arrays
    static constexpr bool UNIFORM = true, LAY_LDS = true, OUT = true, OLD = false; static constexpr int MAXP = 2;
};
struct R4ArithLdsOut : R4Base<R4ArithLdsOut> {  // new-dynamics table in LDS, <= 2 pots, both output arrays
    static constexpr bool LAY_LDS = true, OUT = true, OLD = false; static constexpr int MAXP = 2;
};
struct R4ArithL2Out : R4Base<R4ArithL2Out> {  // new-dynamics table through L2, <= 2 pots, both output arrays
    static constexpr bool OUT = true, OLD = false; static constexpr int MAXP = 2;
};
struct R4ArithUniform : R4Base<R4ArithUniform> {  // other single layouts with <= 2 pots
    static constexpr bool UNIFORM = true, LAY_LDS = true; static constexpr int MAXP = 2;
};
struct R4ArithSmall : R4Base<R4ArithSmall> { static constexpr int MAXP = 2; };  // other tables with <= 2 pots (records through L2)
struct R4ArithGeneral : R4Base<R4ArithGeneral> {};  // more than 2 pots
// -- oc_rollout_record: the three general arithmetic-movement instances with REC
struct R4RecUniform : R4Base<R4RecUniform> {  // one layout, <= 2 pots
    static constexpr bool UNIFORM = true, LAY_LDS = true, REC = true; static constexpr int MAXP = 2;
};
struct R4RecSmall : R4Base<R4RecSmall> { static constexpr bool REC = true; static constexpr int MAXP = 2; };  // mixed tables, <= 2 pots
struct R4RecGeneral : R4Base<R4RecGeneral> { static constexpr bool REC = true; };  // more than 2 pots
// -- oc_rollout_record_ex with an event sink: the same three with the event log as well (compiled beside the R4Ev* instances)
struct R4RecEvUniform : R4Base<R4RecEvUniform> {  // one layout, <= 2 pots
    static constexpr bool UNIFORM = true, LAY_LDS = true, EV = true, REC = true; static constexpr int MAXP = 2;
};
struct R4RecEvSmall : R4Base<R4RecEvSmall> {  // mixed tables, <= 2 pots
    static constexpr bool EV = true, REC = true; static constexpr int MAXP = 2;
};
struct R4RecEvGeneral : R4Base<R4RecEvGeneral> { static constexpr bool EV = true, REC = true; };  // more than 2 pots

template <class... P>
struct R4List {
    static_assert((P::legal() && ...), "");
    static constexpr int PART[] = {P::PART...};
    static constexpr bool FT8[] = {P::FT8...};
    template <class Q> static constexpr int id() {  // index of instance Q, -1 when it is not listed
        constexpr bool same[] = {std::is_same<Q, P>::value...};
        for (int i = 0; i < (int)sizeof...(P); ++i)
            if (same[i]) return i;
        return -1;
    }
};
using R4Instances = R4List<R4EvUniform, R4EvSmall, R4EvGeneral, R4JointTiled, R4JointPipe, R4JointLean, R4TerrainUniform1,
                           R4TerrainUniform, R4TerrainUniformLean, R4TerrainLdsTiled, R4TerrainLds, R4TerrainLdsLean,
                           R4TerrainL2OnePotTiled, R4TerrainL2OnePotLeanTiled, R4TerrainL2OnePot, R4TerrainL2OnePotLean, R4TerrainL2,
                           R4TerrainL2Lean, R4ArithUniformOut, R4ArithUniform, R4ArithLdsOut, R4ArithL2Out, R4ArithSmall, R4ArithGeneral,
                           R4RecUniform, R4RecSmall, R4RecGeneral, R4RecEvUniform, R4RecEvSmall, R4RecEvGeneral>;

// k_rollout5<LAY_LDS, FT8, OLD, BIG, EV, NOOUT, MAXP> (step_duo5.hpp): the mover / interact kernel, chosen by its own six flags;
// one_pot: every layout of the table has one pot (OcBatch.max_pots == 1) and the instance exists with one pot slot (new
// dynamics, not big, no event log): MAXP = 1
struct R5Sel {
    bool lay_lds, ft8, old, big, ev, noout, one_pot;
};

// One oc_rollout_random / oc_rollout_record(_ex) launch, as oc_amd.hip hands it to the unit that compiles the chosen instance.
struct Rollout4Call {
    const OcBatch* b;
    int n_obj;
    void* d_state;
    float* d_rewards;
    uint8_t* d_flags;
    float* d_ep_returns;
    int horizon;
    uint32_t options;
    uint64_t seed;
    int64_t env_offset, t0;
    int n_steps;
    StartArgs sa;
    EvArgs ea;
    hipStream_t stream;
    int r4;     // the chosen k_rollout4 instance: its index in R4Instances; -1: k_rollout5, r5
    R5Sel r5;
    RecArgs ra = {nullptr, nullptr, nullptr};  // oc_rollout_record / oc_rollout_record_ex: the recording outputs
};
// rollout4.hip, compiled with -DOC_R4_PART=UNIT (one explicit instantiation of each per unit): launches c's instance, which that
// unit compiles ...
template <int UNIT> OC_HIDDEN void launch_rollout(const Rollout4Call& c);
// ... or names it and its dynamic LDS in out (oc_rollout_plan: only the unit knows Lds4<P> / Lds5<>).  Reads c.b, c.n_obj, c.r4 and
// c.r5; launches nothing.
template <int UNIT> OC_HIDDEN void describe_rollout(const Rollout4Call& c, char* out, size_t out_size);
OC_HIDDEN size_t rollout5_lds_bytes(bool lay_lds, bool big, bool ev, int n_obj);  // rollout4.hip, OC_R4_PART 1

}  // namespace oc_detail
