// sample.hpp — both players' actions of an env drawn from policy logits: sample_env, k_sample_actions
// Part of liboc_amd.so: included by oc_amd.hip inside its anonymous namespace after common.hpp (philox4x32_10) and before the
// training-step kernels (shaping.hpp, train_obs.hpp, train_feat.hpp), whose SAMPLE = true instances call sample_env where the
// others read the caller's actions.
#pragma once

// ------------------------------------------------------------------------------------------
// The sampler of include/oc_amd.h (OcActionSampler), by value in kernel arguments.  A policy leaves logits [n_envs][2][6]; the
// caller of a training step used to turn them into the u8 actions with half a dozen small torch kernels on torch's global
// generator.  Here the draw is a function of (seed, global env, step) on the library's counter-based stream, like every other
// random stream of the library: r = philox4x32_10({t_lo, g_lo, g_hi, t_hi}, {seed_lo, seed_hi ^ "SAMP"}), player p takes
// u_p = (r[p] >> 8) * 2^-24 (words 2 and 3 are reserved).  The arithmetic is f32, in the header's order, without contraction,
// with the full-precision expf / logf: anyone can restate it (tests/sample_cases.py does, in numpy).
// ------------------------------------------------------------------------------------------
constexpr uint32_t SAMPLE_KEY_TWEAK = 0x53414D50u;  // "SAMP"

struct SampleArgs {
    const float* logits;   // [n_envs][2][6] f32, 16-byte aligned
    uint8_t* actions_out;  // [n_envs][2] u8, 2-byte aligned
    float* logp_out;       // [n_envs][2] f32, 8-byte aligned, or NULL
    uint32_t seed_lo, seed_hi, t_lo, t_hi;
    int64_t env_offset;
    uint32_t mode;         // OC_SAMPLE_CATEGORICAL / OC_SAMPLE_ARGMAX
};

// the first (only) argument of a kernel's trailing parameter pack: the SAMPLE = true instances carry their SampleArgs there, so
// that the others keep their argument lists
template <class A>
__device__ __forceinline__ const A& first_of(const A& a) { return a; }

// one player's row of six logits -> action (255: invalid row) and its log-probability
__device__ __forceinline__ void sample_row(const float (&l)[6], float u, uint32_t mode, uint32_t& a, float& logp) {
#pragma clang fp contract(off)
    bool nan = false;
    float m = l[0];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        nan |= l[i] != l[i];
        m = l[i] > m ? l[i] : m;
    }
    float c[6], S = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        S = S + expf(l[i] - m);  // (a -inf logit: w = 0; m = +-inf: NaN, an invalid row)
        c[i] = S;
    }
    if (nan || !(S > 0.f) || !(S < __builtin_inff())) {
        a = 255u;
        logp = __builtin_nanf("");
        return;
    }
    uint32_t k = 0;
    if (mode == OC_SAMPLE_ARGMAX) {
        k = 5u;
#pragma unroll
        for (int i = 4; i >= 0; --i) k = l[i] == m ? (uint32_t)i : k;  // the lowest index holding m
    } else {
        const float x = u * S;
#pragma unroll
        for (int i = 0; i < 6; ++i) k += c[i] <= x ? 1u : 0u;
        k = min(k, 5u);
    }
    float la = l[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) la = k == (uint32_t)i ? l[i] : la;
    a = k;
    logp = (la - m) - logf(S);
}

// Both players of local env `el` (global env sm.env_offset + el): three 16-byte loads, one Philox block.  Returns a0 | a1 << 8, as
// the step kernels read it from the actions array; write: store the actions and, when asked for, the log-probabilities.
__device__ __forceinline__ uint32_t sample_env(const SampleArgs& sm, int64_t el, bool write) {
    const float4* src = reinterpret_cast<const float4*>(sm.logits) + 3 * el;
    const float4 q0 = src[0], q1 = src[1], q2 = src[2];
    const float l0[6] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y}, l1[6] = {q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    const uint64_t g = (uint64_t)(sm.env_offset + el);
    uint32_t r[4];
    philox4x32_10(sm.t_lo, (uint32_t)g, (uint32_t)(g >> 32), sm.t_hi, sm.seed_lo, sm.seed_hi ^ SAMPLE_KEY_TWEAK, r);
    uint32_t a0, a1;
    float p0, p1;
    sample_row(l0, (float)(r[0] >> 8) * 0x1p-24f, sm.mode, a0, p0);
    sample_row(l1, (float)(r[1] >> 8) * 0x1p-24f, sm.mode, a1, p1);
    const uint32_t a01 = a0 | (a1 << 8);
    if (write) {
        reinterpret_cast<uint16_t*>(sm.actions_out)[el] = (uint16_t)a01;
        if (sm.logp_out) reinterpret_cast<float2*>(sm.logp_out)[el] = make_float2(p0, p1);
    }
    return a01;
}

// k_sample_actions: the sampler alone, one lane per env (oc_sample_actions, and in front of every training-step path that has no
// SAMPLE instance)
__global__ __launch_bounds__(BLOCK) void k_sample_actions(SampleArgs sm, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e < n) sample_env(sm, e, true);
}
