// gae.hpp — advantages and value targets of a collected batch: k_gae, k_gae_moments, oc_gae, oc_gae_plan (include/oc_amd.h: OcGaeBatch)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind partner.hpp, after common.hpp
// (BLOCK) and host_util.hpp (fail, check_launch, grid_for).  Nothing else of the library is used, and no other kernel or entry point
// knows of this file.
//
// k_gae: one lane per env, both players in it, so that a lane's accesses are the widest the header's alignments allow — one 16-byte
// load of the reward pair, 8-byte loads and stores of the value, advantage and target pairs (MI355X: an 8-byte access moves bytes
// at 0.54-0.70 of the 16-byte rate, a 4-byte one lower still, which a lane per (env, player) would make of every access) — and
// adjacent lanes read adjacent addresses of every [n_envs][2] row.  The chain runs from t = T - 1 down to 0 in the header's order:
// it is sequential by definition and is not re-associated.  What does not depend on the chain is every load: the arrays are walked
// in blocks of GAE_B steps, and the loads of the block below are issued before the chain of the current block runs, so that a
// wavefront has GAE_B * 4 loads (26 bytes per lane and step) in flight while it computes — at 65 536 envs a CU holds four
// wavefronts, one per SIMD, and nothing else hides the latency.  Loads and stores are plain: every byte is touched once, and a
// non-temporal load differs from a plain one by 0-3 % on this chip, a non-temporal store keeps its line in L2 like a plain one.
// Moments: a lane sums count, A and A^2 of its learner samples in f64 in the order it meets them, the 256 lanes of a workgroup are
// summed in a fixed tree (shuffles inside a wavefront, then the four wavefronts in order) into d_partials[blockIdx.x]: no atomics,
// the same bits every time.  k_gae_moments, one wavefront behind it on the stream, adds the partials in ascending order.
#pragma once

namespace {

constexpr int GAE_B = 8;  // steps per prefetch block

struct GaeArgs {
    const double* rewards;     // [T][n][2]
    const float* values;       // [T][n][2]
    const float* last_values;  // [n][2] or NULL
    const uint8_t* done;       // [T][n]
    const uint8_t* seat;       // [T][n] or NULL
    float* advantages;         // [T][n][2]
    float* targets;            // [T][n][2]
    double* partials;          // [gridDim.x][3] or NULL
    int64_t n_steps;
    float g, gl;
};

// the inputs of GAE_B steps of one env
struct GaeBlock {
    double2 r[GAE_B];
    float2 v[GAE_B];
    uint32_t d[GAE_B], s[GAE_B];
};

// steps [t0, t0 + GAE_B) of env e; a step at or beyond T reads step T - 1 in its place (an address inside the arrays; never used)
template <bool SEAT>
__device__ __forceinline__ void gae_load(GaeBlock& b, const GaeArgs& a, int64_t t0, int64_t e, int64_t n) {
#pragma unroll
    for (int j = 0; j < GAE_B; ++j) {
        const int64_t t = t0 + j < a.n_steps ? t0 + j : a.n_steps - 1;
        const int64_t at = t * n + e;
        b.r[j] = reinterpret_cast<const double2*>(a.rewards)[at];
        b.v[j] = reinterpret_cast<const float2*>(a.values)[at];
        b.d[j] = a.done[at];
        b.s[j] = SEAT ? a.seat[at] : 255u;
    }
}

// one player's step of the header's recurrence: A (carried in and out), the target
__device__ __forceinline__ void gae_step(float r, float v, float vn, bool done, bool partner, float g, float gl, float& A, float& target) {
#pragma clang fp contract(off)
    const float d_end = r - v;
    const float d_run = (r + g * vn) - v;
    const float a_run = d_run + gl * A;
    A = done ? d_end : a_run;  // a select: neither vn nor the carried A reaches a done step
    target = A + v;
    A = partner ? 0.f : A;
    target = partner ? 0.f : target;
}

template <bool SEAT, bool MOM>
__global__ __launch_bounds__(BLOCK) void k_gae(GaeArgs a, int64_t n) {
    const int64_t e_lane = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = e_lane < n;
    const int64_t e = live ? e_lane : n - 1;  // (a lane beyond the batch reads the last env and stores nothing)
    const int64_t T = a.n_steps;
    float2 vn = a.last_values ? reinterpret_cast<const float2*>(a.last_values)[e] : make_float2(0.f, 0.f);
    float A0 = 0.f, A1 = 0.f;
    double cnt = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t blocks = (T + GAE_B - 1) / GAE_B;
    GaeBlock cur;
    gae_load<SEAT>(cur, a, (blocks - 1) * GAE_B, e, n);
    for (int64_t k = blocks - 1; k >= 0; --k) {
        const int64_t t0 = k * GAE_B;
        GaeBlock nxt = cur;
        if (k > 0) gae_load<SEAT>(nxt, a, t0 - GAE_B, e, n);  // in flight while this block's chain runs
#pragma unroll
        for (int j = GAE_B - 1; j >= 0; --j) {
            if (t0 + j < T) {  // (uniform: only the block at the horizon end is short)
                const bool done = cur.d[j] != 0;
                const bool p0 = SEAT && cur.s[j] == 0u, p1 = SEAT && cur.s[j] == 1u;
                float tg0, tg1;
                gae_step((float)cur.r[j].x, cur.v[j].x, vn.x, done, p0, a.g, a.gl, A0, tg0);
                gae_step((float)cur.r[j].y, cur.v[j].y, vn.y, done, p1, a.g, a.gl, A1, tg1);
                vn = cur.v[j];
                if (live) {
                    const int64_t at = (t0 + j) * n + e;
                    reinterpret_cast<float2*>(a.advantages)[at] = make_float2(A0, A1);
                    reinterpret_cast<float2*>(a.targets)[at] = make_float2(tg0, tg1);
                }
                if constexpr (MOM) {
                    const double x0 = (double)A0, x1 = (double)A1;
                    if (!p0) {
                        cnt += 1.0;
                        s1 += x0;
                        s2 += x0 * x0;
                    }
                    if (!p1) {
                        cnt += 1.0;
                        s1 += x1;
                        s2 += x1 * x1;
                    }
                }
            }
        }
        cur = nxt;
    }
    if constexpr (MOM) {
        __shared__ double red[3][BLOCK / 64];
        if (!live) cnt = s1 = s2 = 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_down(cnt, off, 64);
            s1 += __shfl_down(s1, off, 64);
            s2 += __shfl_down(s2, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = cnt;
            red[1][threadIdx.x >> 6] = s1;
            red[2][threadIdx.x >> 6] = s2;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            double sum = red[threadIdx.x][0];
#pragma unroll
            for (int w = 1; w < BLOCK / 64; ++w) sum += red[threadIdx.x][w];
            a.partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = sum;
        }
    }
}

// d_moments[c] = partials[0][c] + partials[1][c] + ... in ascending order: lane c of one wavefront, eight loads at a time
__global__ __launch_bounds__(64) void k_gae_moments(const double* __restrict__ partials, int64_t count, double* __restrict__ moments) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    double sum = 0.0;
    for (int64_t k0 = 0; k0 < count; k0 += 8) {
        double x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = k0 + j < count ? partials[(k0 + j) * 3 + c] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k0 + j < count) sum += x[j];
    }
    moments[c] = sum;
}

const char* const GAE_WHO = "oc_gae";

int gae_refuse(const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", GAE_WHO, why);
    return fail(OC_EINVAL, msg);
}

// the checks that need no array (oc_gae_plan makes these alone)
int gae_check_shape(const OcBatch* b, int64_t n_steps) {
    if (!b) return gae_refuse("batch is NULL");
    if (b->n_envs < 0) return gae_refuse("batch.n_envs < 0");
    if (n_steps < 0) return gae_refuse("n_steps < 0");
    return OC_OK;
}

int gae_check(const OcBatch* b, const OcGaeBatch* g) {
    if (!b) return gae_refuse("batch is NULL");
    if (!g) return gae_refuse("gae batch is NULL");
    if (!g->d_rewards || !g->d_values || !g->d_done || !g->d_advantages || !g->d_targets)
        return gae_refuse("NULL d_rewards, d_values, d_done, d_advantages or d_targets");
    if ((uintptr_t)g->d_rewards & 15u) return gae_refuse("d_rewards must be 16-byte aligned");
    if (((uintptr_t)g->d_values | (uintptr_t)g->d_last_values | (uintptr_t)g->d_advantages | (uintptr_t)g->d_targets) & 7u)
        return gae_refuse("d_values, d_last_values, d_advantages and d_targets must be 8-byte aligned");
    if (((uintptr_t)g->d_partials | (uintptr_t)g->d_moments) & 7u) return gae_refuse("d_partials and d_moments must be 8-byte aligned");
    if (int rc = gae_check_shape(b, g->n_steps)) return rc;
    if (!(g->gamma >= 0.f && g->gamma <= 1.f)) return gae_refuse("gamma must be in [0, 1]");
    if (!(g->lambda >= 0.f && g->lambda <= 1.f)) return gae_refuse("lambda must be in [0, 1]");
    if (g->d_moments && !g->d_partials) return gae_refuse("d_moments needs d_partials");
    return OC_OK;
}

template <bool SEAT>
void gae_go(const GaeArgs& a, int64_t n, hipStream_t stream) {
    if (a.partials) hipLaunchKernelGGL((k_gae<SEAT, true>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, a, n);
    else hipLaunchKernelGGL((k_gae<SEAT, false>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, a, n);
}

}  // namespace

extern "C" {

int oc_gae(const OcBatch* b, const OcGaeBatch* g, void* stream) {
    if (int rc = gae_check(b, g)) return rc;
    const int64_t n = b->n_envs;
    if (n == 0 || g->n_steps == 0) {  // no sample: nothing to launch; the moments of no sample are zeros
        hipError_t err = hipSuccess;
        if (g->d_partials && n > 0) err = hipMemsetAsync(g->d_partials, 0, (size_t)grid_for(n) * 3 * sizeof(double), (hipStream_t)stream);
        if (g->d_moments && err == hipSuccess) err = hipMemsetAsync(g->d_moments, 0, 3 * sizeof(double), (hipStream_t)stream);
        if (err != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "%s: %s", GAE_WHO, hipGetErrorString(err));
            return OC_ELAUNCH;
        }
        return OC_OK;
    }
    GaeArgs a;
    a.rewards = g->d_rewards; a.values = g->d_values; a.last_values = g->d_last_values; a.done = g->d_done; a.seat = g->d_seat;
    a.advantages = g->d_advantages; a.targets = g->d_targets; a.partials = g->d_partials;
    a.n_steps = g->n_steps;
    a.g = g->gamma;
    a.gl = g->gamma * g->lambda;  // one f32 product
    if (a.seat) gae_go<true>(a, n, (hipStream_t)stream);
    else gae_go<false>(a, n, (hipStream_t)stream);
    if (g->d_moments)
        hipLaunchKernelGGL(k_gae_moments, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)g->d_partials, (int64_t)grid_for(n), g->d_moments);
    return check_launch(GAE_WHO);
}

int oc_gae_plan(const OcBatch* b, int64_t n_steps, int with_seat, int with_moments, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_gae_plan: no output buffer");
    out[0] = 0;
    if (int rc = gae_check_shape(b, n_steps)) return rc;
    if (b->n_envs == 0) snprintf(out, out_size, "nothing to launch (no envs)");
    else if (n_steps == 0) snprintf(out, out_size, "nothing to launch (no steps)");
    else
        snprintf(out, out_size, "k_gae<SEAT=%s, MOM=%s> grid=%u, %d lanes (one per env, both players), %d steps per prefetch block, %lld block(s)%s",
                 with_seat ? "true" : "false", with_moments ? "true" : "false", grid_for(b->n_envs), BLOCK, GAE_B,
                 (long long)((n_steps + GAE_B - 1) / GAE_B), with_moments ? " + k_gae_moments grid=1, 64 lanes" : "");
    return OC_OK;
}

}  // extern "C"
