// step_dispatch.hpp — host only: the caller-actions family.  oc_step and oc_step_many fill one call record (StepCall); one planner
// (plan_step: every check of the entry point, then the choice, choose_step; no launch, no device address) serves them and
// oc_step_server_open; launch_step_from launches the chosen instance from the record, describe_step puts the choice into words
// (oc_step_plan).  The instances of k_step1, k_step3, k_step and k_step_server stand once, as the rows below; the resident step's
// host side (step_server_host.hpp: sv_launch) walks its rows the same way.
// Part of liboc_amd.so: included by oc_amd.hip at file scope.  The kernels are step_one.hpp (k_step1), step_table.hpp (k_step3),
// step_predicate.hpp (k_step) and step_server.hpp (k_step_server).
#pragma once

namespace {
// ---- the call is planned first (every check, every choice; no launch, no device address), then launched from the plan — or, by
//      oc_step_plan, described
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

// ---- the kernel instances of the family, each once: a row is the (UNIFORM, MAXP, LAY_LDS, FAST) of an instance, a list of rows
//      launches the one equal to a choice.  EVENTS is no part of a row: launch_step_from picks it from the choice
template <bool U, int MP, bool LL, bool F = false>
struct StepRow {
    static constexpr bool UNIFORM = U, LAY_LDS = LL, FAST = F;
    static constexpr int MAXP = MP;
    static bool is(const StepChoice& c) { return c.uniform == U && c.maxp == MP && c.lay_lds == LL && c.fast == F; }
};
template <class... Row> struct StepRows {};
// go(row) for the row equal to the choice, and for no other; false: the choice has no row
template <class... Row, class Go>
auto launch_row(StepRows<Row...>, const StepChoice& c, Go go) { return (... || (Row::is(c) && (go(Row()), true))); }
using Step1Rows = StepRows<  // k_step1<UNIFORM, MAXP, LAY_LDS, EVENTS>
    StepRow<true, 1, true>,
    StepRow<true, 2, true>,
    StepRow<true, 8, true>,
    StepRow<false, 2, true>,
    StepRow<false, 2, false>,
    StepRow<false, 8, false>>;
using Step3Rows = StepRows<  // k_step3<UNIFORM, MAXP, LAY_LDS, FAST, EVENTS>
    StepRow<true, 1, true, true>,
    StepRow<true, 2, true, true>,
    StepRow<false, 2, true, false>,
    StepRow<false, 8, false, false>>;
using PredicateRows = StepRows<  // k_step<UNIFORM, MAXP, LAY_LDS, EVENTS>
    StepRow<true, 2, true>,
    StepRow<true, 8, true>,
    StepRow<false, 8, false>>;
using ServerRows = StepRows<  // k_step_server<UNIFORM, MAXP, LAY_LDS>
    StepRow<true, 2, true>,
    StepRow<false, 2, true>,
    StepRow<false, 8, false>>;
const char* const NO_STEP_INSTANCE = "no kernel instance for the planned step (internal error)";

// The arrays and scalars of one launch of k_step1, k_step3 or k_step
struct StepCall {
    const OcBatch* b;
    int n_obj;
    const void* d_state_in;
    void* d_state_out;
    const uint8_t* d_actions;
    float* d_rewards;
    uint8_t* d_flags;
    float* d_ep_returns;
    int horizon;
    uint32_t options;
    int n_steps;
    StartArgs sa;
    EvArgs ea;
    hipStream_t stream;
};

// launch what choose_step chose (EVENTS: the event-logging instances)
template <bool EVENTS>
int launch_step_as(const StepChoice& ch, const StepCall& c) {
    const OcBatch* b = c.b;
    // the launch shape and the arguments every kernel of the family begins with, then the kernel's own
    const auto launch = [&](auto kernel, auto... own) {
        hipLaunchKernelGGL(kernel, dim3(ch.grid), dim3(BLOCK), ch.lds, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id, (uint4*)c.d_state_in,
                           (uint4*)c.d_state_out, c.d_actions, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, own...);
    };
    const auto step1 = [&](auto row) {
        launch(k_step1<row.UNIFORM, row.MAXP, row.LAY_LDS, EVENTS>, b->n_envs, b->width, c.n_obj, c.horizon, c.options, c.sa, c.ea);
    };
    const auto step3 = [&](auto row) {
        const auto kernel = k_step3<row.UNIFORM, row.MAXP, row.LAY_LDS, row.FAST, EVENTS>;
        if (want_lds(kernel, ch.lds)) launch(kernel, b->n_envs, b->width, c.n_obj, c.horizon, c.options, c.n_steps, c.sa, c.ea);
    };
    const auto predicate = [&](auto row) {
        const auto kernel = k_step<row.UNIFORM, row.MAXP, row.LAY_LDS, EVENTS>;
        if (want_lds(kernel, ch.lds)) launch(kernel, c.ea.events, b->n_envs, b->width, c.n_obj, c.horizon, c.options);
    };
    const bool found = ch.family == StepChoice::STEP1 ? launch_row(Step1Rows(), ch, step1)
                     : ch.family == StepChoice::STEP3 ? launch_row(Step3Rows(), ch, step3)
                     : ch.family == StepChoice::PREDICATE && launch_row(PredicateRows(), ch, predicate);
    return found ? OC_OK : fail(OC_ELAUNCH, NO_STEP_INSTANCE);  // (a missing kernel is an error, never another kernel)
}
// (a refused LDS request is no failure here: check_launch reports it, as it reports a failed launch)
int launch_step_from(const StepChoice& ch, const StepCall& c) {
    return (ch.events ? launch_step_as<true> : launch_step_as<false>)(ch, c);
}
// one step of a batch that another entry point has checked (the training step's sequence)
void launch_step(const StepCall& c) { (void)launch_step_from(choose_step(c.b, c.n_obj, c.options, 1, ev_on(c.ea), false), c); }

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
}  // namespace

extern "C" {

int oc_step(const OcBatch* b, const void* d_state_in, void* d_state_out, const uint8_t* d_actions, float* d_rewards,
            uint8_t* d_flags, float* d_ep_returns, uint64_t* d_events, int horizon, uint32_t options,
            const OcStartSpec* start, const OcEventSink* events, void* stream) {
    const EvArgs ea = ev_args(events, d_events);
    const StepArrays have = {d_state_in && d_state_out && d_actions && d_rewards && d_flags, ea.events != nullptr, ea.counts != nullptr,
                             aligned16(d_rewards), aligned16(d_ep_returns)};
    const StepPlan p = plan_step(b, ENTRY_STEP, have, horizon, options, 1, start);
    if (p.rc != OC_OK || p.ch.family == StepChoice::NOTHING) return p.rc;
    const StepCall c = {b, p.n_obj, d_state_in, d_state_out, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options, 1, p.sa, ea,
                        (hipStream_t)stream};
    if (int rc = launch_step_from(p.ch, c)) return rc;
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
        const StepCall c = {b, p.n_obj, d_state, d_state, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options, n_steps, p.sa, ea,
                            (hipStream_t)stream};
        if (int rc = launch_step_from(p.ch, c)) return rc;
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

}  // extern "C"
