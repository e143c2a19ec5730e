// train_dispatch.hpp — host only: the training-step family.  oc_multi_agent_step, oc_multi_agent_step_featurize and
// oc_multi_agent_step_sample fill one call record (TrainCall); one planner (plan_train: every check, then every choice; no launch,
// no device memory) turns what the record holds into one flat plan (TrainPlan: what the call enqueues, in stream order); one
// function launches from that plan (launch_train) and one puts it into words (describe_train_plan: oc_multi_agent_plan,
// oc_multi_agent_step_featurize_plan, oc_multi_agent_step_sample_plan).  oc_sample_actions, the sampler alone, is here too.
// Part of liboc_amd.so: included by oc_amd.hip at file scope.  The kernels are shaping.hpp (k_train_step, k_train_step1),
// train_obs.hpp, train_feat.hpp and sample.hpp; each instance of them is named once, in the select_* functions below.
#pragma once

namespace {
// ---- the step of a call is one of:
//        k_train_step_obs<MAXP, T, NWV>          the step and its observation in one kernel
//        k_train_step_feat<MAXP>                 the step and its featurize_state features in one kernel
//        k_train_step1<UNIFORM, MAXP, LAY_LDS>   the step in one kernel on the wire format
//        k_train_step<UNIFORM, EV>               the same with event counters or on 65..128 cells
//        the sequence of entry points            any other table (train_sequence)
//      then oc_encode_lossless where an observation is wanted and the step kernel has not written it, then k_featurize<LAY_LDS>
//      where features are wanted and the step kernel has not written them.  A call with a sampler draws its actions in the
//      SAMPLE = true instance of k_train_step_obs, k_train_step_feat or k_train_step1 wherever the step is that kernel (its
//      owner lanes draw where the others read the actions), and with k_sample_actions in front of every other step.

// Everything the widest entry point (oc_multi_agent_step_sample) receives; the narrower ones leave the rest zero
struct TrainCall {
    const char* who;  // the entry point, as messages name it
    const OcBatch* b;
    void* d_state;
    const uint8_t* d_actions;  // (with a sampler: its d_actions_out)
    float* d_rewards;
    uint8_t* d_flags;
    float *d_ep_returns, *d_ep_returns_out;
    const uint8_t* d_plan_blob;  // the potential: plan tables, phi tables, phi(s'), phi(s), phi(start)
    const uint32_t* d_plan_off;
    const uint8_t* d_phi_tables;
    double *d_phi_next, *d_phi_cur;
    const double* d_phi_start;
    double reward_shaping_factor, *d_shaped;
    uint8_t* d_done;
    void* d_obs;
    int obs_dtype, horizon;
    const uint8_t* d_feat_plan_blob;  // featurize_state of the states the next step starts from
    const uint32_t* d_feat_plan_off;
    float* d_features;
    int num_pots;
    uint32_t options;
    const OcActionSampler* sampler;  // NULL: the actions are d_actions
    const OcStartSpec* start;
    EvArgs ea;
    hipStream_t stream;
};

// How k_train_step_obs (train_obs.hpp) would run a call: envs per template, wavefronts per workgroup, envs per private image,
// dynamic LDS.  nwv = 0: it does not apply.
struct TrainObsShape {
    int unit = 0, nwv = 0, gmax = 0;
    size_t smem = 0;
};
// What a plan needs to know of a call's arrays: which ones are there, never where (the *_plan entry points have no more than
// that to give)
struct TrainArrays {
    bool state, actions, rewards, flags, shaped, shaped_aligned16, done;
    bool phi_tables, phi_rest;  // use_phi: the phi tables / the plan tables and the three phi buffers
    bool ep_returns, ep_returns_out;  // (no choice depends on them: read by describe_train_plan only, for the sequence's copy)
    bool quads_aligned16 = true;      // d_rewards, d_ep_returns and d_ep_returns_out
    bool obs, obs_aligned16;
    bool events;  // an event sink with counters or masks
    bool features, feat_tables, features_aligned16;  // d_features / both feature plan pointers
    bool sampler;  // the actions are drawn
};
// The plan of one call: every check, every choice; no launch, no device memory
struct TrainPlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    int n_obj = 0;
    StartArgs sa = {};
    // what the call enqueues, in stream order
    bool sample_first = false;  // k_sample_actions
    enum Step { NOTHING, OBS, FEAT, STEP1, STEP, SEQUENCE } step = NOTHING;  // a kernel instance (below) / the sequence of entry points
    bool encode = false;     // oc_encode_lossless
    bool featurize = false;  // k_featurize<feat.lay_lds>
    FeaturizePlan feat;
    // the step kernel's instance and launch
    bool sample = false;  // OBS, FEAT, STEP1: SAMPLE
    int maxp = 2;         // OBS, FEAT, STEP1: MAXP
    bool obs_u8 = false;  // OBS: T
    bool uniform = false, lay_lds = false, ev = false;  // STEP1, STEP: UNIFORM; LAY_LDS (STEP1), EV (STEP)
    TrainObsShape sh;     // OBS: NWV, unit, envs per private image
    int g = 0;            // FEAT: envs per private image
    unsigned grid = 0, block = 0;
    size_t lds = 0;
};

const char* const STEP_WHO = "oc_multi_agent_step";
const char* const FEAT_WHO = "oc_multi_agent_step_featurize";
const char* const SAMPLE_WHO = "oc_multi_agent_step_sample";

// Round 5: the step AND its observation in one kernel for single-layout batches (at most two pots, two players, 64 cells, no
// event sink) that give at least half of the CUs a workgroup of 256 envs (smaller batches: the observation kernel spreads
// over all CUs)
bool train_obs_wanted(const OcBatch* b, int n_obj, const TrainArrays& have, int obs_dtype) {
    static const bool no_fused_obs = tuning_set("OC_TRAIN_NO_FUSED_OBS");
    return have.obs && b->n_layouts == 1 && b->width * b->height <= 64 && !have.events && n_obj <= STEP1_MAX_PLANES && !step_no_lean() &&
           !no_fused_obs && obs_dtype_ok(obs_dtype) && have.obs_aligned16 && b->n_envs >= (simd_count() / 8) * BLOCK;
}
TrainObsShape train_obs_shape(const OcBatch* b, int n_obj, const TrainArrays& have, int obs_dtype) {
    TrainObsShape sh;
    if (!train_obs_wanted(b, n_obj, have, obs_dtype)) return sh;
    const ObsGeometry geo(b->width, b->height, obs_dtype);
    const int unit = geo.unit;
    const size_t fixed = (size_t)n_obj * BLOCK * 16 + geo.env_bytes * unit + (size_t)4 * BLOCK * 16;
    const size_t budget = 150 * 1024;
    // wavefronts per workgroup: 16 (4 owners, 4 helpers, 8 encoders; round 6) for u8 observations whose private images
    // still hold >= 6 envs then (cramped_room-sized grids: the encode loop there is bound by what the wavefronts of a
    // CU can issue, not by bytes), else 8
    static const int forced_w = tuning_int("OC_TRAIN_OBS_WAVES", 0), forced_g = tuning_int("OC_TRAIN_OBS_G", 0);
    for (int w : {16, 8}) {
        if (forced_w && w != forced_w) continue;
        if (!forced_w && w == 16 && obs_dtype != OC_OBS_U8) continue;
        int g = geo.envs_per_image(fixed, budget, w);
        if (forced_g > 0 && forced_g < g) g = forced_g;
        g = geo.whole_units(g);
        if (w == 16 && g < 6 && !forced_w) continue;  // (measured: 7-env images 22.0 -> 19.5 us, 3-env images 31.8 -> 37.6)
        if (g >= unit && g >= 2) {  // (one env per image — 9x5 f32 — measured slower than the two kernels: 123-127 vs 116-122 us)
            sh.unit = unit; sh.nwv = w; sh.gmax = g;
            sh.smem = fixed + (size_t)w * g * geo.env_bytes;
            break;
        }
    }
    return sh;
}

// The batch size from which k_train_step_feat is taken without OC_OPT_ONE_KERNEL: a quarter of the CUs get a workgroup of 256 envs
// (16 384 envs on MI355X).  It started from k_train_step_obs's rule (half of the CUs) and was settled by run 1 of
// profiles/train_step_feat.txt (tools/time_train_step_feat.py): at 16 384 envs, the smallest batch measured, a call takes 11.9 us
// with the one kernel against 17.5 us for k_train_step1 + k_featurize on cramped_room and 12.1 against 17.4 us on
// asymmetric_advantages (65 536 envs: 15.4 against 22.3 and 16.8 against 23.3 us).  Smaller batches are not measured and stay
// with the two launches, whose k_featurize spreads over twice as many CUs.
inline int64_t train_feat_fill() { return (simd_count() / 16) * BLOCK; }

// What a call enqueues: the one place that reads the batch and the call for it.  launch_train launches what it returns; the
// *_plan entry points put it into words.  who: the entry point a refusal names
TrainPlan plan_train(const OcBatch* b, const TrainArrays& have, int obs_dtype, int horizon, int num_pots, uint32_t options,
                     const OcStartSpec* start, const char* who) {
    TrainPlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    if (!have.done) return refused(refuse(who, "d_done is required (it is the reset mask)"));
    if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
    if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
    // at most two pots and two players: the whole step in one kernel
    const bool fused = b->max_pots >= 1 && b->max_pots <= 2 && (b->batch_flags & OC_BATCH_TWO_PLAYERS) != 0;
    if (!have.state || !have.actions || !have.rewards || !have.flags || (fused && !have.shaped))
        return refused(refuse(who, fused ? "NULL state/actions/rewards/flags/shaped pointer" : "NULL state/actions/rewards/flags pointer"));
    if (fused && have.phi_tables && !have.phi_rest) return refused(refuse(who, "use_phi needs the plan tables and the three phi buffers"));
    if (int rc = check_horizon(who, horizon)) return refused(rc);
    if (fused && !have.shaped_aligned16) return refused(refuse(who, "d_shaped must be 16-byte aligned"));
    if (!have.quads_aligned16) return refused(refuse(who, "d_rewards, d_ep_returns and d_ep_returns_out must be 16-byte aligned"));
    if (have.features) {
        if (!have.feat_tables) return refused(refuse(who, "d_features needs the feature plan tables (d_feat_plan_blob, d_feat_plan_off)"));
        if (num_pots < 0 || num_pots > 4) return refused(refuse(who, "num_pots must be in 0..4"));
        if (!(b->batch_flags & OC_BATCH_TWO_PLAYERS)) return refused(refuse(who, "d_features needs 2-player layouts"));
        if (!have.features_aligned16) return refused(refuse(who, "d_features must be 16-byte aligned"));
        if (b->n_envs == 0) return p;  // nothing at all: not the sequence either
        p.feat = plan_featurize(b, true, true, num_pots);  // (its checks were made above, under this entry point's name)
        if (p.feat.rc != OC_OK) return refused(p.feat.rc);
        p.featurize = true;
    }
    // ---- the step
    p.encode = have.obs;
    p.grid = grid_for(b->n_envs);
    p.block = BLOCK;
    p.uniform = b->n_layouts == 1;
    if (!fused) {
        p.step = TrainPlan::SEQUENCE;  // (no envs: its entry points find nothing to launch)
        p.sample_first = have.sampler && b->n_envs > 0;
        return p;
    }
    if (b->n_envs == 0) return p;
    p.sh = train_obs_shape(b, p.n_obj, have, obs_dtype);
    if (p.sh.nwv) {
        p.step = TrainPlan::OBS;
        p.encode = false;
        p.maxp = b->max_pots == 1 ? 1 : 2;
        p.obs_u8 = obs_dtype == OC_OBS_U8;
        p.block = p.sh.nwv * 64;
        p.lds = p.sh.smem;
    } else if (!have.events && p.n_obj <= STEP1_MAX_PLANES && !step_no_lean()) {  // the transition on the wire format itself (step_one.hpp)
        p.step = TrainPlan::STEP1;
        p.maxp = p.uniform && b->max_pots == 1 ? 1 : 2;
        p.lay_lds = b->n_layouts <= LDS_LAYOUT_MAX;
        p.lds = (size_t)p.n_obj * BLOCK * sizeof(uint4);
    } else {
        p.step = TrainPlan::STEP;
        p.ev = have.events;
        p.lds = (size_t)p.n_obj * 16 * BLOCK * sizeof(uint16_t);
    }
    // the step and its features in one kernel: no observation array, one layout of at most 64 cells with one or two pots on the
    // wire-format step (no event sink), a batch that fills the device (or OC_OPT_ONE_KERNEL), and private images of at least 8
    // envs within the LDS budget
    if (p.featurize && !have.obs && p.step == TrainPlan::STEP1 && p.uniform && b->width * b->height <= 64 &&
        (b->n_envs >= train_feat_fill() || (options & OC_OPT_ONE_KERNEL))) {
        const size_t budget = 150 * 1024;
        for (int g : {32, 16, 8}) {
            if (train_feat_lds(p.n_obj, g, num_pots) > budget) continue;
            p.step = TrainPlan::FEAT;
            p.featurize = false;
            p.maxp = b->max_pots == 1 ? 1 : 2;
            p.g = g;
            p.block = TF_WAVES * 64;
            p.lds = train_feat_lds(p.n_obj, g, num_pots);
            break;
        }
    }
    if (have.sampler) {
        p.sample = p.step == TrainPlan::OBS || p.step == TrainPlan::FEAT || p.step == TrainPlan::STEP1;
        p.sample_first = !p.sample;
    }
    return p;
}

TrainArrays train_arrays_of(const TrainCall& c) {
    TrainArrays have = {};
    have.state = c.d_state != nullptr; have.actions = c.d_actions != nullptr; have.rewards = c.d_rewards != nullptr; have.flags = c.d_flags != nullptr;
    have.shaped = c.d_shaped != nullptr; have.shaped_aligned16 = aligned16(c.d_shaped); have.done = c.d_done != nullptr;
    have.phi_tables = c.d_phi_tables != nullptr;
    have.phi_rest = c.d_plan_blob && c.d_plan_off && c.d_phi_next && c.d_phi_cur && c.d_phi_start;
    have.ep_returns = c.d_ep_returns != nullptr; have.ep_returns_out = c.d_ep_returns_out != nullptr;
    have.quads_aligned16 = aligned16(c.d_rewards) && aligned16(c.d_ep_returns) && aligned16(c.d_ep_returns_out);
    have.obs = c.d_obs != nullptr; have.obs_aligned16 = aligned16(c.d_obs);
    have.events = ev_on(c.ea);
    have.features = c.d_features != nullptr; have.feat_tables = c.d_feat_plan_blob && c.d_feat_plan_off;
    have.features_aligned16 = aligned16(c.d_features);
    have.sampler = c.sampler != nullptr;
    return have;
}
// the call VecOvercookedMultiAgent.step (step_sampled) makes: every required array (aligned), the named optional ones; the *_plan
// entry points add the features and the sampler they are asked about
TrainArrays train_arrays_planned(bool with_obs, bool use_phi, bool event_sink) {
    TrainArrays have = {};
    have.state = have.actions = have.rewards = have.flags = have.shaped = have.shaped_aligned16 = have.done = true;
    have.phi_tables = have.phi_rest = use_phi;
    have.ep_returns = have.ep_returns_out = true;
    have.obs = with_obs;
    have.obs_aligned16 = true;
    have.events = event_sink;
    have.feat_tables = have.features_aligned16 = true;
    return have;
}

// A plan in words (the *_plan entry points): up to and including '>' the step's kernel instance, as tests match it; a call
// with a sampler has SAMPLE=true as that kernel's last parameter, or "k_sample_actions + " in front
void describe_train_plan(const OcBatch* b, const TrainPlan& p, const TrainArrays& have, const OcStartSpec* start, char* out, size_t out_size) {
    const auto tf = [](bool v) { return v ? "true" : "false"; };
    const char* const smp = p.sample ? ", SAMPLE=true" : "";
    const char* const then_obs = p.encode ? " + oc_encode_lossless" : "";
    char step[320], feat[96] = "";
    if (p.step == TrainPlan::NOTHING) {
        snprintf(step, sizeof(step), "nothing to launch (no envs)");
    } else if (p.step == TrainPlan::SEQUENCE) {  // what train_sequence enqueues, in its order, and the observation
        const bool regen = start && start->regen_count && b->n_layouts > 1;
        snprintf(step, sizeof(step), "sequence: oc_step%s, oc_shape_rewards%s%s, %s%s%s", have.phi_tables ? ", oc_potential" : "",
                 have.ep_returns && have.ep_returns_out ? ", copy of the episode returns" : "", regen ? ", oc_regen_layouts" : "",
                 start ? "oc_reset_random" : "oc_reset", start && have.phi_tables ? ", oc_potential" : "", p.encode ? ", oc_encode_lossless" : "");
    } else if (p.step == TrainPlan::OBS) {
        snprintf(step, sizeof(step), "k_train_step_obs<MAXP=%d, T=%s, NWV=%d%s> unit=%d, G=%d, %zu B LDS", p.maxp, p.obs_u8 ? "u8" : "f32",
                 p.sh.nwv, smp, p.sh.unit, p.sh.gmax, p.lds);
    } else if (p.step == TrainPlan::FEAT) {
        snprintf(step, sizeof(step), "k_train_step_feat<MAXP=%d%s> G=%d, grid=%u, %zu B LDS", p.maxp, smp, p.g, p.grid, p.lds);
    } else if (p.step == TrainPlan::STEP1) {
        snprintf(step, sizeof(step), "k_train_step1<UNIFORM=%s, MAXP=%d, LAY_LDS=%s%s>%s", tf(p.uniform), p.maxp, tf(p.lay_lds), smp, then_obs);
    } else {
        snprintf(step, sizeof(step), "k_train_step<UNIFORM=%s, EV=%s>%s", tf(p.uniform), tf(p.ev), then_obs);
    }
    if (p.featurize) snprintf(feat, sizeof(feat), " + k_featurize<LAY_LDS=%s> grid=%u, %zu B LDS", tf(p.feat.lay_lds), p.feat.grid, p.feat.smem);
    snprintf(out, out_size, "%s%s%s", p.sample_first ? "k_sample_actions + " : "", step, feat);
}

int check_train_options(const char* who, uint32_t options) {
    return options & ~(uint32_t)OC_OPT_ONE_KERNEL ? refuse(who, "options other than OC_OPT_ONE_KERNEL") : OC_OK;
}

int check_sampler(const char* who, const OcActionSampler* s) {
    if (!s) return refuse(who, "sampler is NULL");
    if (!s->d_logits || !s->d_actions_out) return refuse(who, "NULL sampler.d_logits or sampler.d_actions_out");
    if (!aligned16(s->d_logits)) return refuse(who, "sampler.d_logits must be 16-byte aligned");
    if ((uintptr_t)s->d_actions_out & 1u) return refuse(who, "sampler.d_actions_out must be 2-byte aligned");
    if ((uintptr_t)s->d_logp_out & 7u) return refuse(who, "sampler.d_logp_out must be 8-byte aligned");
    if (s->mode != OC_SAMPLE_CATEGORICAL && s->mode != OC_SAMPLE_ARGMAX) return refuse(who, "unknown sampler.mode");
    return OC_OK;
}

SampleArgs sample_args(const OcActionSampler* s) {
    SampleArgs sm;
    sm.logits = s->d_logits; sm.actions_out = s->d_actions_out; sm.logp_out = s->d_logp_out;
    sm.seed_lo = (uint32_t)s->seed; sm.seed_hi = (uint32_t)(s->seed >> 32);
    sm.t_lo = (uint32_t)(uint64_t)s->step; sm.t_hi = (uint32_t)((uint64_t)s->step >> 32);
    sm.env_offset = s->env_offset;
    sm.mode = s->mode;
    return sm;
}

void launch_sample_actions(const OcBatch* b, const SampleArgs& sm, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_actions, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, stream, sm, b->n_envs);
}

// ---- the launches.  Per kernel one launch_* template over the kernel's template parameters (the arguments, type-checked against
//      the kernel's signature; SAMPLE = true: the instance with a trailing SampleArgs) and one select_* that turns the plan's
//      values into template arguments: one line per instance, read by the census tests (tests/test_host_train_*.py).

// The 15 arguments every training-step kernel takes from st to done, in the kernels' order
template <typename F>
void with_step_arrays(const TrainCall& c, F f) {
    f((uint4*)c.d_state, c.d_actions, (float4*)c.d_rewards, c.d_flags, (float4*)c.d_ep_returns, (float4*)c.d_ep_returns_out, c.d_plan_blob,
      c.d_plan_off, c.d_phi_tables, c.d_phi_next, c.d_phi_cur, c.d_phi_start, c.reward_shaping_factor, c.d_shaped, c.d_done);
}

template <int MP, typename T, int NW, bool SAMPLE>
void launch_train_obs(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    const auto go = [&](auto kernel, auto... smp) {
        if (!want_lds(kernel, p.lds)) return;
        with_step_arrays(c, [&](auto... arrays) {
            hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, c.stream, b->d_layouts, arrays..., (uint8_t*)c.d_obs, b->n_envs,
                               b->width, b->height, p.n_obj, c.horizon, p.sh.unit, p.sh.gmax, p.sa, smp...);
        });
    };
    if constexpr (SAMPLE) go(k_train_step_obs<MP, T, NW, true, SampleArgs>, sample_args(c.sampler));
    else go(k_train_step_obs<MP, T, NW>);
}
template <bool SAMPLE>
void select_train_obs(const TrainCall& c, const TrainPlan& p) {
    const bool u8 = p.obs_u8, one = p.maxp == 1, w16 = p.sh.nwv == 16;
    if (u8 && one && w16) return launch_train_obs<1, uint8_t, 16, SAMPLE>(c, p);
    if (u8 && one) return launch_train_obs<1, uint8_t, 8, SAMPLE>(c, p);
    if (u8 && w16) return launch_train_obs<2, uint8_t, 16, SAMPLE>(c, p);
    if (u8) return launch_train_obs<2, uint8_t, 8, SAMPLE>(c, p);
    if (one && w16) return launch_train_obs<1, float, 16, SAMPLE>(c, p);
    if (one) return launch_train_obs<1, float, 8, SAMPLE>(c, p);
    if (w16) return launch_train_obs<2, float, 16, SAMPLE>(c, p);
    return launch_train_obs<2, float, 8, SAMPLE>(c, p);
}

template <int MP, bool SAMPLE>
void launch_train_feat(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    const auto go = [&](auto kernel, auto... smp) {
        if (!want_lds(kernel, p.lds)) return;
        with_step_arrays(c, [&](auto... arrays) {
            hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, c.stream, b->d_layouts, arrays..., c.d_feat_plan_blob,
                               c.d_feat_plan_off, c.d_features, b->n_envs, b->width, b->height, p.n_obj, c.num_pots, c.horizon, p.g, p.sa,
                               smp...);
        });
    };
    if constexpr (SAMPLE) go(k_train_step_feat<MP, true, SampleArgs>, sample_args(c.sampler));
    else go(k_train_step_feat<MP>);
}
template <bool SAMPLE>
void select_train_feat(const TrainCall& c, const TrainPlan& p) {
    if (p.maxp == 1) return launch_train_feat<1, SAMPLE>(c, p);
    return launch_train_feat<2, SAMPLE>(c, p);
}

template <bool U, int MP, bool LL, bool SAMPLE>
void launch_train_step1(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    const auto go = [&](auto kernel, auto... smp) {
        with_step_arrays(c, [&](auto... arrays) {
            hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id, arrays...,
                               b->n_envs, b->width, b->height, p.n_obj, c.horizon, p.sa, smp...);
        });
    };
    if constexpr (SAMPLE) go(k_train_step1<U, MP, LL, true, SampleArgs>, sample_args(c.sampler));
    else go(k_train_step1<U, MP, LL>);
}
template <bool SAMPLE>
void select_train_step1(const TrainCall& c, const TrainPlan& p) {
    if (p.uniform && p.maxp == 1) return launch_train_step1<true, 1, true, SAMPLE>(c, p);
    if (p.uniform) return launch_train_step1<true, 2, true, SAMPLE>(c, p);
    if (p.lay_lds) return launch_train_step1<false, 2, true, SAMPLE>(c, p);
    return launch_train_step1<false, 2, false, SAMPLE>(c, p);
}

// (no SAMPLE instance: k_sample_actions runs in front)
template <bool U, bool EV>
void launch_train_step(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    const auto kernel = k_train_step<U, 2, U, false, EV>;
    if (!want_lds(kernel, p.lds)) return;
    with_step_arrays(c, [&](auto... arrays) {
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, c.stream, b->d_layouts, b->n_layouts, b->d_layout_id, arrays...,
                           b->n_envs, b->width, b->height, p.n_obj, c.horizon, p.sa, c.ea);
    });
}
void select_train_step(const TrainCall& c, const TrainPlan& p) {
    if (p.uniform && p.ev) return launch_train_step<true, true>(c, p);
    if (p.uniform) return launch_train_step<true, false>(c, p);
    if (p.ev) return launch_train_step<false, true>(c, p);
    return launch_train_step<false, false>(c, p);
}

// any table: oc_step (finished envs are restarted below: their counters clear at the DONE step), potential, shaping, restart
int train_sequence(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    if (b->n_envs > 0) {
        StartArgs none;
        start_args(nullptr, &none);
        launch_step(StepCall{b, p.n_obj, c.d_state, c.d_state, c.d_actions, c.d_rewards, c.d_flags, c.d_ep_returns, c.horizon, 0u, 1, none, c.ea, c.stream});
        if (int rc = check_launch(c.who)) return rc;
    }
    if (c.d_phi_tables) {
        if (int rc = oc_potential(b, c.d_plan_blob, c.d_plan_off, c.d_phi_tables, c.d_state, c.d_phi_next, c.stream)) return rc;
    }
    if (int rc = oc_shape_rewards(b, c.d_rewards, c.d_flags, c.d_phi_tables ? c.d_phi_next : nullptr, c.d_phi_cur, c.d_phi_start,
                                  c.reward_shaping_factor, c.d_shaped, c.d_done, c.stream))
        return rc;
    if (c.d_ep_returns && c.d_ep_returns_out && b->n_envs > 0) {
        if (hipMemcpyAsync(c.d_ep_returns_out, c.d_ep_returns, (size_t)b->n_envs * 4 * sizeof(float), hipMemcpyDeviceToDevice,
                           c.stream) != hipSuccess)
            return fail(OC_ELAUNCH, "oc_multi_agent_step: copy of the episode returns failed");
    }
    if (const OcStartSpec* start = c.start) {  // finished envs restart from drawn states; d_phi_cur = the potential of what every env starts the next step from
        if (start->regen_count && b->n_layouts > 1) {  // ... on layouts drawn for their new episodes
            if (int rc = oc_regen_layouts(b, const_cast<uint16_t*>(b->d_layout_id), c.d_done, 0xFF, start, c.stream)) return rc;
        }
        if (int rc = oc_reset_random(b, c.d_state, c.d_done, c.d_ep_returns, start->seed, start->env_offset, start->epoch,
                                     start->random_start_pos, start->rnd_obj_prob_thresh, c.stream))
            return rc;
        if (c.d_phi_tables) {
            if (int rc = oc_potential(b, c.d_plan_blob, c.d_plan_off, c.d_phi_tables, c.d_state, c.d_phi_cur, c.stream)) return rc;
        }
        return OC_OK;
    }
    return oc_reset(b, c.d_state, c.d_done, c.d_ep_returns, c.stream);
}

// the step kernel of a plan; SAMPLE: p.sample
template <bool SAMPLE>
void launch_train_kernel(const TrainCall& c, const TrainPlan& p) {
    if (p.step == TrainPlan::OBS) select_train_obs<SAMPLE>(c, p);
    else if (p.step == TrainPlan::STEP1) select_train_step1<SAMPLE>(c, p);
    else if (p.step == TrainPlan::STEP) select_train_step(c, p);
    else select_train_feat<SAMPLE>(c, p);
}

// the launches of a planned call: the plan's list, in its order
int launch_train(const TrainCall& c, const TrainPlan& p) {
    const OcBatch* b = c.b;
    if (p.sample_first) {
        launch_sample_actions(b, sample_args(c.sampler), c.stream);
        if (int rc = check_launch(c.who)) return rc;
    }
    if (p.step == TrainPlan::SEQUENCE) {
        if (int rc = train_sequence(c, p)) return rc;
    } else if (p.step != TrainPlan::NOTHING) {
        if (!p.sample) launch_train_kernel<false>(c, p);
        else launch_train_kernel<true>(c, p);
        if (int rc = check_launch(c.who)) return rc;
    }
    if (p.encode) {
        if (int rc = oc_encode_lossless(b, c.d_state, c.d_obs, c.obs_dtype, c.horizon, c.stream)) return rc;
    }
    if (p.featurize) {
        if (p.feat.lay_lds) launch_featurize<true>(p.feat, b, c.d_feat_plan_blob, c.d_feat_plan_off, c.d_state, c.d_features, c.num_pots, c.stream);
        else launch_featurize<false>(p.feat, b, c.d_feat_plan_blob, c.d_feat_plan_off, c.d_state, c.d_features, c.num_pots, c.stream);
        return check_launch(c.who);
    }
    return OC_OK;
}

int train_call(const TrainCall& c) {
    const TrainPlan p = plan_train(c.b, train_arrays_of(c), c.obs_dtype, c.horizon, c.num_pots, c.options, c.start, c.who);
    return p.rc != OC_OK ? p.rc : launch_train(c, p);
}
// a *_plan entry point's answer; have: train_arrays_planned with the features and the sampler asked about
int train_plan_text(const OcBatch* b, const TrainArrays& have, const TrainPlan& p, const OcStartSpec* start, char* out, size_t out_size) {
    if (p.rc != OC_OK) return p.rc;
    describe_train_plan(b, p, have, start, out, out_size);
    return OC_OK;
}
}  // namespace

extern "C" {

int oc_sample_actions(const OcBatch* b, const OcActionSampler* sampler, void* stream) {
    if (!b) return refuse("oc_sample_actions", "batch is NULL");
    if (b->n_envs < 0) return refuse("oc_sample_actions", "batch.n_envs < 0");
    if (int rc = check_sampler("oc_sample_actions", sampler)) return rc;
    if (b->n_envs == 0) return OC_OK;
    launch_sample_actions(b, sample_args(sampler), (hipStream_t)stream);
    return check_launch("oc_sample_actions");
}

// oc_multi_agent_step_featurize whose actions are drawn from the sampler's logits
int oc_multi_agent_step_sample(const OcBatch* b, void* d_state, const OcActionSampler* sampler, float* d_rewards, uint8_t* d_flags,
                               float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                               const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next, double* d_phi_cur,
                               const double* d_phi_start, double reward_shaping_factor, double* d_shaped, uint8_t* d_done,
                               void* d_obs, int obs_dtype, int horizon, const uint8_t* d_feat_plan_blob,
                               const uint32_t* d_feat_plan_off, float* d_features, int num_pots, uint32_t options,
                               const OcStartSpec* start, const OcEventSink* events, void* stream) {
    if (int rc = check_train_options(SAMPLE_WHO, options)) return rc;
    if (int rc = check_sampler(SAMPLE_WHO, sampler)) return rc;
    TrainCall c = {};
    c.who = SAMPLE_WHO; c.b = b; c.d_state = d_state; c.d_actions = sampler->d_actions_out; c.sampler = sampler;
    c.d_rewards = d_rewards; c.d_flags = d_flags; c.d_ep_returns = d_ep_returns; c.d_ep_returns_out = d_ep_returns_out;
    c.d_plan_blob = d_plan_blob; c.d_plan_off = d_plan_off; c.d_phi_tables = d_phi_tables; c.d_phi_next = d_phi_next; c.d_phi_cur = d_phi_cur;
    c.d_phi_start = d_phi_start; c.reward_shaping_factor = reward_shaping_factor; c.d_shaped = d_shaped; c.d_done = d_done;
    c.d_obs = d_obs; c.obs_dtype = obs_dtype; c.horizon = horizon; c.start = start; c.ea = ev_args(events, nullptr, 1u); c.stream = (hipStream_t)stream;
    c.d_feat_plan_blob = d_feat_plan_blob; c.d_feat_plan_off = d_feat_plan_off; c.d_features = d_features; c.num_pots = num_pots; c.options = options;
    return train_call(c);
}

int oc_multi_agent_step_sample_plan(const OcBatch* b, int horizon, int with_obs, int obs_dtype, int with_features, int num_pots,
                                    uint32_t options, int use_phi, int event_sink, const OcStartSpec* start, char* out,
                                    size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_multi_agent_step_sample_plan: no output buffer");
    out[0] = 0;
    if (int rc = check_train_options(SAMPLE_WHO, options)) return rc;
    TrainArrays have = train_arrays_planned(with_obs != 0, use_phi != 0, event_sink != 0);
    have.features = with_features != 0;
    have.sampler = true;  // (a whole one)
    return train_plan_text(b, have, plan_train(b, have, obs_dtype, horizon, num_pots, options, start, SAMPLE_WHO), start, out, out_size);
}

int oc_multi_agent_step(const OcBatch* b, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                        float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                        const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next, double* d_phi_cur,
                        const double* d_phi_start, double reward_shaping_factor, double* d_shaped, uint8_t* d_done,
                        void* d_obs, int obs_dtype, int horizon, const OcStartSpec* start, const OcEventSink* events,
                        void* stream) {
    TrainCall c = {};
    c.who = STEP_WHO; c.b = b; c.d_state = d_state; c.d_actions = d_actions;
    c.d_rewards = d_rewards; c.d_flags = d_flags; c.d_ep_returns = d_ep_returns; c.d_ep_returns_out = d_ep_returns_out;
    c.d_plan_blob = d_plan_blob; c.d_plan_off = d_plan_off; c.d_phi_tables = d_phi_tables; c.d_phi_next = d_phi_next; c.d_phi_cur = d_phi_cur;
    c.d_phi_start = d_phi_start; c.reward_shaping_factor = reward_shaping_factor; c.d_shaped = d_shaped; c.d_done = d_done;
    c.d_obs = d_obs; c.obs_dtype = obs_dtype; c.horizon = horizon; c.start = start; c.ea = ev_args(events, nullptr, 1u); c.stream = (hipStream_t)stream;
    return train_call(c);
}

int oc_multi_agent_plan(const OcBatch* b, int horizon, int with_obs, int obs_dtype, int use_phi, int event_sink, const OcStartSpec* start,
                        char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_multi_agent_plan: no output buffer");
    out[0] = 0;
    const TrainArrays have = train_arrays_planned(with_obs != 0, use_phi != 0, event_sink != 0);
    return train_plan_text(b, have, plan_train(b, have, obs_dtype, horizon, 0, 0u, start, STEP_WHO), start, out, out_size);
}

// oc_multi_agent_step with featurize_state of the states the next step starts from
int oc_multi_agent_step_featurize(const OcBatch* b, void* d_state, const uint8_t* d_actions, float* d_rewards, uint8_t* d_flags,
                                  float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                                  const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next, double* d_phi_cur,
                                  const double* d_phi_start, double reward_shaping_factor, double* d_shaped, uint8_t* d_done,
                                  void* d_obs, int obs_dtype, int horizon, const uint8_t* d_feat_plan_blob,
                                  const uint32_t* d_feat_plan_off, float* d_features, int num_pots, uint32_t options,
                                  const OcStartSpec* start, const OcEventSink* events, void* stream) {
    if (int rc = check_train_options(FEAT_WHO, options)) return rc;
    TrainCall c = {};
    c.who = d_features ? FEAT_WHO : STEP_WHO;  // no features: the call is oc_multi_agent_step
    c.b = b; c.d_state = d_state; c.d_actions = d_actions;
    c.d_rewards = d_rewards; c.d_flags = d_flags; c.d_ep_returns = d_ep_returns; c.d_ep_returns_out = d_ep_returns_out;
    c.d_plan_blob = d_plan_blob; c.d_plan_off = d_plan_off; c.d_phi_tables = d_phi_tables; c.d_phi_next = d_phi_next; c.d_phi_cur = d_phi_cur;
    c.d_phi_start = d_phi_start; c.reward_shaping_factor = reward_shaping_factor; c.d_shaped = d_shaped; c.d_done = d_done;
    c.d_obs = d_obs; c.obs_dtype = obs_dtype; c.horizon = horizon; c.start = start; c.ea = ev_args(events, nullptr, 1u); c.stream = (hipStream_t)stream;
    c.d_feat_plan_blob = d_feat_plan_blob; c.d_feat_plan_off = d_feat_plan_off; c.d_features = d_features; c.num_pots = num_pots; c.options = options;
    return train_call(c);
}

int oc_multi_agent_step_featurize_plan(const OcBatch* b, int horizon, int with_obs, int obs_dtype, int with_features, int num_pots,
                                       uint32_t options, int use_phi, int event_sink, const OcStartSpec* start, char* out,
                                       size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_multi_agent_step_featurize_plan: no output buffer");
    out[0] = 0;
    if (int rc = check_train_options(FEAT_WHO, options)) return rc;
    TrainArrays have = train_arrays_planned(with_obs != 0, use_phi != 0, event_sink != 0);
    have.features = with_features != 0;  // no features: oc_multi_agent_plan, word for word
    return train_plan_text(b, have, plan_train(b, have, obs_dtype, horizon, num_pots, options, start, with_features ? FEAT_WHO : STEP_WHO), start,
                           out, out_size);
}

}  // extern "C"
