// train_sample.hpp — the training step that draws its actions from policy logits: oc_sample_actions, oc_multi_agent_step_sample,
// oc_multi_agent_step_sample_plan (include/oc_amd.h)
// Part of liboc_amd.so: included by oc_amd.hip at file scope behind the planners of oc_multi_agent_step and
// oc_multi_agent_step_featurize (plan_train_step, plan_train_step_featurize, their descriptions and launches), which this file
// asks and leaves as they are.  The sampler itself (sample_env, k_sample_actions) is sample.hpp.
#pragma once

namespace {
// ---- oc_multi_agent_step_sample: oc_multi_agent_step_featurize whose actions are drawn from the sampler's logits.  Planned first
//      (plan_train_step_sample: the sampler's checks, then the plan the same call would get with an actions array; no launch, no
//      device memory), then launched from that plan — or, by oc_multi_agent_step_sample_plan, described.  The paths:
//        the SAMPLE = true instance of k_train_step_obs, k_train_step_feat or k_train_step1   wherever the step's own plan is that
//                                              kernel: its owner lanes draw where the others read the actions — one launch
//                                              (then whatever follows that kernel in the step's plan: the observation, k_featurize)
//        k_sample_actions, then the step's own path    every other plan: k_train_step<.., EV>, 65..128 cells, the sequence
struct TrainSamplePlan {
    int rc = OC_OK;
    bool features = false;  // the call has a feature array: `feat` is its plan, else `step`
    bool fused = false;     // the step kernel draws the actions itself
    TrainFeatPlan feat;
    TrainPlan step;
    const TrainPlan& step_plan() const { return features ? feat.step : step; }
};

const char* const SAMPLE_WHO = "oc_multi_agent_step_sample";

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

// features: the call has a feature array (feat_tables, feat_aligned: as for plan_train_step_featurize)
TrainSamplePlan plan_train_step_sample(const OcBatch* b, const TrainArrays& have, bool features, bool feat_tables, bool feat_aligned,
                                       int obs_dtype, int horizon, int num_pots, uint32_t options, const OcStartSpec* start) {
    TrainSamplePlan p;
    p.features = features;
    if (features) {
        p.feat = plan_train_step_featurize(b, have, feat_tables, feat_aligned, obs_dtype, horizon, num_pots, options, start, SAMPLE_WHO);
        p.rc = p.feat.rc;
    } else {
        p.step = plan_train_step(b, have, obs_dtype, horizon, start, SAMPLE_WHO);
        p.rc = p.step.rc;
    }
    if (p.rc != OC_OK || b->n_envs == 0) return p;
    const TrainPlan& s = p.step_plan();
    p.fused = (features && p.feat.path == TrainFeatPlan::ONE_KERNEL) || s.path == TrainPlan::OBS || (s.path == TrainPlan::FUSED && s.lean);
    return p;
}

// A plan in words (oc_multi_agent_step_sample_plan): the words of the same call with an actions array, with SAMPLE=true as the
// step kernel's last parameter, or behind "k_sample_actions + "
void describe_train_sample_plan(const OcBatch* b, const TrainSamplePlan& p, const TrainArrays& have, int obs_dtype, const OcStartSpec* start,
                                char* out, size_t out_size) {
    char base[320];
    if (p.features) describe_train_feat_plan(b, p.feat, have, obs_dtype, start, base, sizeof(base));
    else describe_train_plan(b, p.step, have, obs_dtype, start, base, sizeof(base));
    const char* gt = strchr(base, '>');
    if (b->n_envs == 0) snprintf(out, out_size, "%s", base);
    else if (p.fused && gt) snprintf(out, out_size, "%.*s, SAMPLE=true%s", (int)(gt - base), base, gt);
    else snprintf(out, out_size, "k_sample_actions + %s", base);
}

void launch_sample_actions(const OcBatch* b, const SampleArgs& sm, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_actions, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, stream, sm, b->n_envs);
}

// the SAMPLE = true instance of the step kernel p names (k_train_step_obs or k_train_step1), then the observation as
// train_step_fused enqueues it; a.d_actions is the sampler's d_actions_out
int train_step_sampled(const TrainStep& a, const TrainPlan& p, const SampleArgs& sm) {
    const OcBatch* b = a.b;
    if (b->n_envs == 0) return OC_OK;
    const dim3 grid(grid_for(b->n_envs));
    if (p.path == TrainPlan::OBS) {
        const TrainObsShape& sh = p.sh;
#define SAMPLE_OBS(MP, T, NW)                                                                                              \
    do {                                                                                                                   \
        if (!want_lds(k_train_step_obs<MP, T, NW, true, SampleArgs>, sh.smem)) break;                                      \
        hipLaunchKernelGGL((k_train_step_obs<MP, T, NW, true, SampleArgs>), grid, dim3(NW * 64), sh.smem, a.stream,        \
                           b->d_layouts, (uint4*)a.d_state, a.d_actions, (float4*)a.d_rewards, a.d_flags,                  \
                           (float4*)a.d_ep_returns, (float4*)a.d_ep_returns_out, a.d_plan_blob, a.d_plan_off,              \
                           a.d_phi_tables, a.d_phi_next, a.d_phi_cur, a.d_phi_start, a.reward_shaping_factor, a.d_shaped,  \
                           a.d_done, (uint8_t*)a.d_obs, b->n_envs, b->width, b->height, a.n_obj, a.horizon, sh.unit,       \
                           sh.gmax, a.sa, sm);                                                                             \
    } while (0)
#define SAMPLE_OBSW(MP, T) do { if (sh.nwv == 16) SAMPLE_OBS(MP, T, 16); else SAMPLE_OBS(MP, T, 8); } while (0)
        if (a.obs_dtype == OC_OBS_U8) { if (p.maxp == 1) SAMPLE_OBSW(1, uint8_t); else SAMPLE_OBSW(2, uint8_t); }
        else { if (p.maxp == 1) SAMPLE_OBSW(1, float); else SAMPLE_OBSW(2, float); }
#undef SAMPLE_OBSW
#undef SAMPLE_OBS
        return check_launch(SAMPLE_WHO);
    }
    const size_t smem1 = (size_t)a.n_obj * BLOCK * sizeof(uint4);
#define SAMPLE_STEP1(U, MP, LL)                                                                                            \
    hipLaunchKernelGGL((k_train_step1<U, MP, LL, true, SampleArgs>), grid, dim3(BLOCK), smem1, a.stream, b->d_layouts,     \
                       b->n_layouts, b->d_layout_id, (uint4*)a.d_state, a.d_actions, (float4*)a.d_rewards, a.d_flags,      \
                       (float4*)a.d_ep_returns, (float4*)a.d_ep_returns_out, a.d_plan_blob, a.d_plan_off, a.d_phi_tables,  \
                       a.d_phi_next, a.d_phi_cur, a.d_phi_start, a.reward_shaping_factor, a.d_shaped, a.d_done, b->n_envs, \
                       b->width, b->height, a.n_obj, a.horizon, a.sa, sm)
    if (p.uniform && p.maxp == 1) SAMPLE_STEP1(true, 1, true);
    else if (p.uniform) SAMPLE_STEP1(true, 2, true);
    else if (p.lay_lds) SAMPLE_STEP1(false, 2, true);
    else SAMPLE_STEP1(false, 2, false);
#undef SAMPLE_STEP1
    if (int rc = check_launch(SAMPLE_WHO)) return rc;
    if (a.d_obs) return oc_encode_lossless(b, a.d_state, a.d_obs, a.obs_dtype, a.horizon, a.stream);
    return OC_OK;
}

// the SAMPLE = true instance of k_train_step_feat
int train_step_feat_sampled(const TrainStep& a, const TrainFeatPlan& p, const uint8_t* d_feat_plan_blob, const uint32_t* d_feat_plan_off,
                            float* d_features, int num_pots, const SampleArgs& sm) {
    const OcBatch* b = a.b;
    const dim3 grid(grid_for(b->n_envs));
#define SAMPLE_FEAT(MP)                                                                                                    \
    do {                                                                                                                   \
        if (!want_lds(k_train_step_feat<MP, true, SampleArgs>, p.smem)) break;                                             \
        hipLaunchKernelGGL((k_train_step_feat<MP, true, SampleArgs>), grid, dim3(TF_WAVES * 64), p.smem, a.stream,         \
                           b->d_layouts, (uint4*)a.d_state, a.d_actions, (float4*)a.d_rewards, a.d_flags,                  \
                           (float4*)a.d_ep_returns, (float4*)a.d_ep_returns_out, a.d_plan_blob, a.d_plan_off,              \
                           a.d_phi_tables, a.d_phi_next, a.d_phi_cur, a.d_phi_start, a.reward_shaping_factor, a.d_shaped,  \
                           a.d_done, d_feat_plan_blob, d_feat_plan_off, d_features, b->n_envs, b->width, b->height,        \
                           a.n_obj, num_pots, a.horizon, p.g, a.sa, sm);                                                   \
    } while (0)
    if (p.maxp == 1) SAMPLE_FEAT(1);
    else SAMPLE_FEAT(2);
#undef SAMPLE_FEAT
    return check_launch(SAMPLE_WHO);
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

int oc_multi_agent_step_sample(const OcBatch* b, void* d_state, const OcActionSampler* sampler, float* d_rewards, uint8_t* d_flags,
                               float* d_ep_returns, float* d_ep_returns_out, const uint8_t* d_plan_blob,
                               const uint32_t* d_plan_off, const uint8_t* d_phi_tables, double* d_phi_next, double* d_phi_cur,
                               const double* d_phi_start, double reward_shaping_factor, double* d_shaped, uint8_t* d_done,
                               void* d_obs, int obs_dtype, int horizon, const uint8_t* d_feat_plan_blob,
                               const uint32_t* d_feat_plan_off, float* d_features, int num_pots, uint32_t options,
                               const OcStartSpec* start, const OcEventSink* events, void* stream) {
    if (options & ~(uint32_t)OC_OPT_ONE_KERNEL) return refuse(SAMPLE_WHO, "options other than OC_OPT_ONE_KERNEL");
    if (int rc = check_sampler(SAMPLE_WHO, sampler)) return rc;
    const uint8_t* d_actions = sampler->d_actions_out;
    const EvArgs ea = ev_args(events, nullptr, 1u);
    const TrainArrays have = train_arrays_of(d_state, d_actions, d_rewards, d_flags, d_ep_returns, d_ep_returns_out, d_plan_blob, d_plan_off,
                                             d_phi_tables, d_phi_next, d_phi_cur, d_phi_start, d_shaped, d_done, d_obs, ev_on(ea));
    const bool features = d_features != nullptr;
    const TrainSamplePlan p = plan_train_step_sample(b, have, features, d_feat_plan_blob && d_feat_plan_off, aligned16(d_features), obs_dtype,
                                                     horizon, num_pots, options, start);
    if (p.rc != OC_OK || (features && p.feat.path == TrainFeatPlan::NOTHING)) return p.rc;
    const TrainPlan& sp = p.step_plan();
    const TrainStep a = {b, sp.n_obj, d_state, d_actions, d_rewards, d_flags, d_ep_returns, d_ep_returns_out, d_plan_blob, d_plan_off,
                         d_phi_tables, d_phi_next, d_phi_cur, d_phi_start, reward_shaping_factor, d_shaped, d_done, d_obs, obs_dtype,
                         horizon, start, sp.sa, ea, (hipStream_t)stream};
    const SampleArgs sm = sample_args(sampler);
    if (!p.fused && b->n_envs > 0) {
        launch_sample_actions(b, sm, a.stream);
        if (int rc = check_launch(SAMPLE_WHO)) return rc;
    }
    if (features && p.feat.path == TrainFeatPlan::ONE_KERNEL)
        return train_step_feat_sampled(a, p.feat, d_feat_plan_blob, d_feat_plan_off, d_features, num_pots, sm);
    if (int rc = p.fused ? train_step_sampled(a, sp, sm) : launch_train_step(a, sp)) return rc;
    if (!features) return OC_OK;
    if (p.feat.feat.lay_lds) launch_featurize<true>(p.feat.feat, b, d_feat_plan_blob, d_feat_plan_off, d_state, d_features, num_pots, a.stream);
    else launch_featurize<false>(p.feat.feat, b, d_feat_plan_blob, d_feat_plan_off, d_state, d_features, num_pots, a.stream);
    return check_launch(SAMPLE_WHO);
}

int oc_multi_agent_step_sample_plan(const OcBatch* b, int horizon, int with_obs, int obs_dtype, int with_features, int num_pots,
                                    uint32_t options, int use_phi, int event_sink, const OcStartSpec* start, char* out,
                                    size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_multi_agent_step_sample_plan: no output buffer");
    out[0] = 0;
    if (options & ~(uint32_t)OC_OPT_ONE_KERNEL) return refuse(SAMPLE_WHO, "options other than OC_OPT_ONE_KERNEL");
    // the call VecOvercookedMultiAgent.step_sampled makes: every required array (aligned), the named optional ones, a whole sampler
    TrainArrays have = {};
    have.state = have.actions = have.rewards = have.flags = have.shaped = have.shaped_aligned16 = have.done = true;
    have.phi_tables = have.phi_rest = use_phi != 0;
    have.ep_returns = have.ep_returns_out = true;
    have.obs = with_obs != 0;
    have.obs_aligned16 = true;
    have.events = event_sink != 0;
    const TrainSamplePlan p = plan_train_step_sample(b, have, with_features != 0, true, true, obs_dtype, horizon, num_pots, options, start);
    if (p.rc != OC_OK) return p.rc;
    describe_train_sample_plan(b, p, have, obs_dtype, start, out, out_size);
    return OC_OK;
}

}  // extern "C"
