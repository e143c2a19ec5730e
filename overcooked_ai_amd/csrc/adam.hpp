// adam.hpp — the learner's optimiser step: gradient clipping by global norm and Adam on the eight parameter arrays of an
// OcActorCritic in ONE launch: k_adam_step, oc_adam_step, oc_adam_plan (include/oc_amd.h: OcAdam)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind policy.hpp, whose PolicyLayout
// (the flat order w1 b1 w2 b2 wp bp wv bv of a partial row), pol_refuse and pol_check_shape it uses; after common.hpp and
// host_util.hpp (fail, check_launch).  No other kernel knows of this file.
//
// k_adam_step is ONE workgroup of ADAM_LANES lanes: the order in which the squares of the gradients are added is part of the
// interface (the header states it), and the arrays are at most 13 383 floats.  Lane l owns the flat elements i with i % 256 == l.
// The eight arrays are walked one after the other, each as its own loop with the array's pointers in scalar registers (no select
// of a pointer per element): the lane's first element of array k is start_k + ((l - start_k) mod 256), then every 256th.
//   pass 1  g_i = graw_i * gs into LDS, q_i = (double)g_i * (double)g_i added to the lane's f64 sum in ascending i; eight loads in
//           flight per lane
//   tree    the 256 sums through LDS, s[l] += s[l + k] for k = 128 .. 1; norm = (float)sqrt(s[0]); every lane derives c, the skip
//           and the step's scalars from it and from the clock it read before the first barrier
//   pass 2  p, m, v of four elements in flight per lane, g from LDS, the header's f32 operations one by one, three stores
// sqrtf and / are the correctly rounded ones: the build states hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt, for this
// unit (build.py).  Plain C++, vector stores only, no atomics: a call on the same inputs gives the same bits.
#pragma once

#include <type_traits>

namespace {

constexpr int ADAM_LANES = 256;
constexpr int ADAM_B1 = 8;  // loads in flight per lane in pass 1 (16 and 8 in the two passes measured no faster: docs/NOTEBOOK.md)
constexpr int ADAM_B2 = 4;  // elements in flight per lane in pass 2 (three loads each)
constexpr int ADAM_MAX = 136 * PL_HID + PL_HID + PL_HID * PL_HID + PL_HID + PL_HID * OC_NUM_ACTIONS + OC_NUM_ACTIONS + PL_HID + 1;  // 13 383

struct AdamArgs {
    float* p[8];
    const float* g[8];
    float* m[8];
    float* v[8];
    int start[9];  // flat index of the first element of every array, and n
    double* clock;
    const double* grad_scale;
    double* info;
    float lr, beta1, beta2, eps, max_grad_norm;
};

// f(K) for K = 0 .. 7 as compile-time constants: the arrays' pointers stay kernel arguments in scalar registers
template <int K = 0, class F>
__device__ __forceinline__ void adam_arrays(F f) {
    if constexpr (K < 8) {
        f(std::integral_constant<int, K>());
        adam_arrays<K + 1>(f);
    }
}

// what every lane derives from the norm, the clock's beta powers and the hyperparameters: the clip factor and the scalars of a step taken
struct AdamStep {
    bool clip;
    float c, step_size, rbc2s, omb1, omb2, beta2, eps;
    double p1n, p2n;
};
__device__ __forceinline__ AdamStep adam_step_of(float norm, double p1, double p2, float lr, float beta1, float beta2, float eps, float max_grad_norm) {
#pragma clang fp contract(off)
    AdamStep st;
    st.clip = max_grad_norm > 0.f && max_grad_norm < __builtin_inff();
    st.c = 1.f;
    if (st.clip) {
        const float q = max_grad_norm / (norm + 1e-6f);
        st.c = q < 1.f ? q : 1.f;
    }
    st.p1n = p1 * (double)beta1, st.p2n = p2 * (double)beta2;
    const double bc1 = 1.0 - st.p1n, bc2s = sqrt(1.0 - st.p2n);
    st.step_size = (float)((double)lr / bc1), st.rbc2s = (float)bc2s;
    st.omb1 = 1.f - beta1, st.omb2 = 1.f - beta2;
    st.beta2 = beta2, st.eps = eps;
    return st;
}

// the header's update of one element from its scaled gradient g
__device__ __forceinline__ void adam_element(float g, float m, float v, float p, const AdamStep& st, float& mn, float& vn, float& pn) {
#pragma clang fp contract(off)
    if (st.clip) g = g * st.c;
    mn = m + (g - m) * st.omb1;
    vn = v * st.beta2 + (g * g) * st.omb2;
    const float den = sqrtf(vn) / st.rbc2s + st.eps;
    pn = p - st.step_size * (mn / den);
}

__global__ __launch_bounds__(ADAM_LANES) void k_adam_step(AdamArgs a) {
#pragma clang fp contract(off)
    __shared__ float sg[ADAM_MAX];
    __shared__ double red[ADAM_LANES];
    const int tid = threadIdx.x;
    const bool scaled = a.grad_scale != nullptr;
    const double gs64 = scaled ? *a.grad_scale : 1.0;
    const float gs = (float)gs64;
    const double steps = a.clock[0], p1 = a.clock[1], p2 = a.clock[2], skipped = a.clock[3];  // (read before the first barrier, written behind the last)

    // ---- pass 1: the scaled gradients into LDS, their squares into the lane's sum
    double acc = 0.0;
    adam_arrays([&](auto K) {
        constexpr int k = decltype(K)::value;
        const int s = a.start[k], len = a.start[k + 1] - s;
        const float* const g = a.g[k];
        for (int off = (tid - s) & (ADAM_LANES - 1); off < len; off += ADAM_B1 * ADAM_LANES) {
            float x[ADAM_B1];
#pragma unroll
            for (int j = 0; j < ADAM_B1; ++j) x[j] = off + j * ADAM_LANES < len ? g[off + j * ADAM_LANES] : 0.f;
#pragma unroll
            for (int j = 0; j < ADAM_B1; ++j)
                if (off + j * ADAM_LANES < len) {
                    const float gi = x[j] * gs;
                    sg[s + off + j * ADAM_LANES] = gi;
                    acc += (double)gi * (double)gi;
                }
        }
    });
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int k = ADAM_LANES / 2; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    const float norm = (float)sqrt(red[0]);

    // ---- what every lane derives from the norm and the clock (uniform)
    const bool finite = norm - norm == 0.f;  // neither NaN nor an infinity
    const bool skip = !finite || (scaled && gs64 == 0.0);
    const AdamStep st = adam_step_of(norm, p1, p2, a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm);
    const float c = st.c;
    if (skip) {  // nothing is written to parameters or moments; steps and the powers stay
        if (tid == 0) {
            a.clock[3] = skipped + 1.0;
            if (a.info) a.info[0] = (double)norm, a.info[1] = 0.0, a.info[2] = (double)gs, a.info[3] = 1.0;
        }
        return;
    }
    const double p1n = st.p1n, p2n = st.p2n;

    // ---- pass 2: the update
    adam_arrays([&](auto K) {
        constexpr int k = decltype(K)::value;
        const int s = a.start[k], len = a.start[k + 1] - s;
        float* const P = a.p[k];
        float* const M = a.m[k];
        float* const V = a.v[k];
        for (int off = (tid - s) & (ADAM_LANES - 1); off < len; off += ADAM_B2 * ADAM_LANES) {
            float pi[ADAM_B2], mi[ADAM_B2], vi[ADAM_B2];
#pragma unroll
            for (int j = 0; j < ADAM_B2; ++j) {
                const int at = off + j * ADAM_LANES;
                const bool in = at < len;
                pi[j] = in ? P[at] : 0.f;
                mi[j] = in ? M[at] : 0.f;
                vi[j] = in ? V[at] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < ADAM_B2; ++j) {
                const int at = off + j * ADAM_LANES;
                if (at < len) {
                    float mn, vn, pn;
                    adam_element(sg[s + at], mi[j], vi[j], pi[j], st, mn, vn, pn);
                    M[at] = mn;
                    V[at] = vn;
                    P[at] = pn;
                }
            }
        }
    });
    if (tid == 0) {
        a.clock[0] = steps + 1.0;
        a.clock[1] = p1n;
        a.clock[2] = p2n;
        if (a.info) a.info[0] = (double)norm, a.info[1] = (double)c, a.info[2] = (double)gs, a.info[3] = 0.0;
    }
}

const char* const ADAM_WHO = "oc_adam_step";

// the checks of the shape alone (oc_adam_plan makes these)
int adam_check_shape(const char* who, int in_dim, int h1, int h2) { return pol_check_shape(who, 0, in_dim, h1, h2); }

// the moments and the clock
int adam_check_arrays(const char* who, const OcAdam* ad) {
    uintptr_t bits = 0;
    for (int k = 0; k < 8; ++k) {
        if (!ad->d_m[k] || !ad->d_v[k]) return pol_refuse(who, "NULL moment array");
        bits |= (uintptr_t)ad->d_m[k] | (uintptr_t)ad->d_v[k];
    }
    if (bits & 3u) return pol_refuse(who, "moment arrays must be 4-byte aligned");
    if (!ad->d_clock) return pol_refuse(who, "adam.d_clock is NULL");
    if (((uintptr_t)ad->d_clock | (uintptr_t)ad->d_grad_scale | (uintptr_t)ad->d_info) & 7u)
        return pol_refuse(who, "adam.d_clock, adam.d_grad_scale and adam.d_info must be 8-byte aligned");
    return OC_OK;
}

// the hyperparameters
int adam_check_hyper(const char* who, const OcAdam* ad) {
    if (!(ad->lr >= 0.f) || !(ad->lr < __builtin_inff())) return pol_refuse(who, "adam.lr must be finite and >= 0");
    if (!(ad->beta1 >= 0.f && ad->beta1 < 1.f) || !(ad->beta2 >= 0.f && ad->beta2 < 1.f)) return pol_refuse(who, "adam.beta1 and adam.beta2 must be in [0, 1)");
    if (!(ad->eps > 0.f)) return pol_refuse(who, "adam.eps must be positive");
    if (ad->max_grad_norm != ad->max_grad_norm) return pol_refuse(who, "adam.max_grad_norm is NaN");
    return OC_OK;
}

// every refusal of oc_adam_step; no device call
int adam_check(const char* who, const OcActorCritic* pol, const OcPolicyGrads* grads, const OcAdam* ad) {
    if (!pol) return pol_refuse(who, "params is NULL");
    if (!grads) return pol_refuse(who, "grads is NULL");
    if (!ad) return pol_refuse(who, "adam is NULL");
    if (!pol->d_w1 || !pol->d_b1 || !pol->d_w2 || !pol->d_b2 || !pol->d_wp || !pol->d_bp || !pol->d_wv || !pol->d_bv)
        return pol_refuse(who, "NULL weight or bias array");
    if (((uintptr_t)pol->d_w1 | (uintptr_t)pol->d_b1 | (uintptr_t)pol->d_w2 | (uintptr_t)pol->d_b2 | (uintptr_t)pol->d_wp | (uintptr_t)pol->d_bp |
         (uintptr_t)pol->d_wv | (uintptr_t)pol->d_bv) & 3u)
        return pol_refuse(who, "weight and bias arrays must be 4-byte aligned");
    if (!grads->d_w1 || !grads->d_b1 || !grads->d_w2 || !grads->d_b2 || !grads->d_wp || !grads->d_bp || !grads->d_wv || !grads->d_bv)
        return pol_refuse(who, "NULL gradient array");
    if (((uintptr_t)grads->d_w1 | (uintptr_t)grads->d_b1 | (uintptr_t)grads->d_w2 | (uintptr_t)grads->d_b2 | (uintptr_t)grads->d_wp |
         (uintptr_t)grads->d_bp | (uintptr_t)grads->d_wv | (uintptr_t)grads->d_bv) & 3u)
        return pol_refuse(who, "gradient arrays must be 4-byte aligned");
    if (int rc = adam_check_arrays(who, ad)) return rc;
    if (int rc = adam_check_shape(who, pol->in_dim, pol->h1, pol->h2)) return rc;
    return adam_check_hyper(who, ad);
}

// the optimiser's own arrays and numbers, for a caller that has checked the weights and the shape itself (bc_fused.hpp)
int adam_check_state(const char* who, const OcAdam* ad) {
    if (int rc = adam_check_arrays(who, ad)) return rc;
    return adam_check_hyper(who, ad);
}

// the launch of a call that adam_check has passed
int adam_run(const char* who, const OcActorCritic* pol, const OcPolicyGrads* grads, const OcAdam* ad, hipStream_t stream) {
    AdamArgs a;
    const float* const p[8] = {pol->d_w1, pol->d_b1, pol->d_w2, pol->d_b2, pol->d_wp, pol->d_bp, pol->d_wv, pol->d_bv};
    const float* const g[8] = {grads->d_w1, grads->d_b1, grads->d_w2, grads->d_b2, grads->d_wp, grads->d_bp, grads->d_wv, grads->d_bv};
    for (int k = 0; k < 8; ++k) {
        a.p[k] = const_cast<float*>(p[k]);  // (written through: the header says so)
        a.g[k] = g[k];
        a.m[k] = ad->d_m[k];
        a.v[k] = ad->d_v[k];
    }
    const PolicyLayout o = pol_layout(pol->in_dim, pol->h1, pol->h2);
    const int start[9] = {o.w1, o.b1, o.w2, o.b2, o.wp, o.bp, o.wv, o.bv, o.size};
    for (int k = 0; k < 9; ++k) a.start[k] = start[k];
    a.clock = ad->d_clock; a.grad_scale = ad->d_grad_scale; a.info = ad->d_info;
    a.lr = ad->lr; a.beta1 = ad->beta1; a.beta2 = ad->beta2; a.eps = ad->eps; a.max_grad_norm = ad->max_grad_norm;
    hipLaunchKernelGGL(k_adam_step, dim3(1), dim3(ADAM_LANES), 0, stream, a);
    return check_launch(who);
}

// the plan's words (oc_ppo_update_plan quotes them)
void adam_describe(int in_dim, int h1, int h2, char* out, size_t out_size) {
    const int n = pol_layout(in_dim, h1, h2).size;
    snprintf(out, out_size, "k_adam_step grid=1, %d lanes, %d elements (%d per lane), flat order w1 b1 w2 b2 wp bp wv bv, f64 norm in a fixed tree, "
             "%zu B LDS", ADAM_LANES, n, (n + ADAM_LANES - 1) / ADAM_LANES, sizeof(float) * ADAM_MAX + sizeof(double) * ADAM_LANES);
}

}  // namespace

extern "C" {

int oc_adam_step(const OcActorCritic* params, const OcPolicyGrads* grads, const OcAdam* adam, void* stream) {
    if (int rc = adam_check(ADAM_WHO, params, grads, adam)) return rc;
    return adam_run(ADAM_WHO, params, grads, adam, (hipStream_t)stream);
}

int oc_adam_plan(int in_dim, int h1, int h2, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_adam_plan: no output buffer");
    out[0] = 0;
    if (int rc = adam_check_shape(ADAM_WHO, in_dim, h1, h2)) return rc;
    adam_describe(in_dim, h1, h2, out, out_size);
    return OC_OK;
}

}  // extern "C"
