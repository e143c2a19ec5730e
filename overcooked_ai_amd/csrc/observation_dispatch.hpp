// observation_dispatch.hpp — host only: the launches of the observation paths.  oc_encode_lossless, oc_rollout_encode and
// oc_rollout_featurize plan a call first (observation_plan.hpp: every check, every choice; no launch, no device memory), then launch
// from that plan — or, by oc_observation_plan / oc_rollout_featurize_plan, describe it.  The two rollouts with an observation of every
// step share the head of their call record (RolloutObsCall) and their step-by-step path (rollout_step_by_step).
// Part of liboc_amd.so: included by oc_amd.hip at file scope, after derived_dispatch.hpp (plan_featurize).  The kernels are encode.hpp,
// rollout_encode.hpp and rollout_featurize.hpp.
#pragma once

namespace {
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

// The arrays and scalars every rollout with an observation of each step receives (oc_rollout_encode, oc_rollout_featurize)
struct RolloutObsCall {
    const OcBatch* b;
    void* d_state;
    const uint8_t* d_actions;
    float* d_rewards;
    uint8_t* d_flags;
    float* d_ep_returns;
    int horizon;
    uint32_t step_options;  // OC_OPT_AUTO_RESET or nothing
    uint64_t seed;
    int64_t env_offset, t0;
    int n_steps;
    const OcStartSpec* start;
    hipStream_t stream;
};

// every table the single kernels do not take: the same result from the one-step entry points, step by step.  observe(k): the
// observation call of step k, made on the state that step leaves
template <class Observe>
int rollout_step_by_step(const RolloutObsCall& c, Observe observe) {
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
        if ((rc = observe(k))) return rc;
    }
    return OC_OK;
}

// One oc_rollout_encode call
struct RolloutEncodeCall : RolloutObsCall {
    void* d_obs;
    int obs_dtype;
    int64_t obs_step_stride;
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

// every other table: oc_encode_lossless into step k's part of the trajectory buffer
int rollout_encode_step_by_step(const RolloutEncodeCall& c) {
    return rollout_step_by_step(c, [&c](int k) {
        return oc_encode_lossless(c.b, c.d_state, (uint8_t*)c.d_obs + (int64_t)k * c.obs_step_stride, c.obs_dtype, c.horizon, c.stream);
    });
}

// ---- oc_rollout_featurize: planned first (observation_plan.hpp: plan_rollout_featurize), then launched from that plan — or, by
//      oc_rollout_featurize_plan, described
// One oc_rollout_featurize call
struct RolloutFeaturizeCall : RolloutObsCall {
    const uint8_t* d_plan_blob;
    const uint32_t* d_plan_off;
    float* d_features;
    int64_t feat_step_stride;
    int num_pots;
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

// every other table: oc_featurize into step k's part of the feature buffer
int rollout_featurize_step_by_step(const RolloutFeaturizeCall& c) {
    return rollout_step_by_step(c, [&c](int k) {
        float* feat_k = (float*)((uint8_t*)c.d_features + (int64_t)k * c.feat_step_stride);
        return oc_featurize(c.b, c.d_plan_blob, c.d_plan_off, c.d_state, feat_k, c.num_pots, c.stream);
    });
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
    const RolloutEncodeCall c = {{b, d_state, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options & (uint32_t)OC_OPT_AUTO_RESET, seed, env_offset,
                                  t0, n_steps, start, (hipStream_t)stream}, d_obs, obs_dtype, obs_step_stride};
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
    const RolloutFeaturizeCall c = {{b, d_state, d_actions, d_rewards, d_flags, d_ep_returns, horizon, options & (uint32_t)OC_OPT_AUTO_RESET, seed, env_offset,
                                     t0, n_steps, start, (hipStream_t)stream}, d_plan_blob, d_plan_off, d_features, feat_step_stride, num_pots};
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

}  // extern "C"
