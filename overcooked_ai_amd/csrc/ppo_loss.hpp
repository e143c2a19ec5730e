// ppo_loss.hpp — the clipped-surrogate loss of a minibatch and its gradients with respect to the policy's logits and values:
// k_ppo_loss, k_ppo_loss_stats, oc_ppo_loss, oc_ppo_loss_plan (include/oc_amd.h: OcPpoLoss)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind gae.hpp, after common.hpp (BLOCK)
// and host_util.hpp (fail, check_launch, grid_for).  Nothing else of the library is used, and no other kernel or entry point knows
// of this file.
//
// k_ppo_loss: one lane per minibatch row; a workgroup walks PPO_TILES tiles of BLOCK consecutive rows — PPO_P rows, one partial: the
// finishing kernel's chain of additions is as long as there are partials, and the reduction tree is paid once per PPO_TILES rows of
// a lane.  The rows of the policy's logits and of their gradients are 24 bytes: a lane loads and stores its own row as three 8-byte
// accesses.  Moving a tile's 6 144 contiguous bytes as 384 coalesced 16-byte accesses through LDS instead was measured and lost
// (106 against 94 us at 2^22 rows; two more barriers per tile, and the kernel is not bound by those accesses).  What is
// read through the index — the action, logp_old, the advantage, the target, the seat byte, the old logits row — are 1- to 8-byte
// accesses at random addresses: all of a lane's are issued before the first is used.
// Instances: OLD (the old logits row: six more loads and a second softmax, the one option that moves the register count) is a
// template parameter; index, seat, moments and terms are wavefront-uniform branches on a pointer of the argument block, a scalar
// compare each.  Two instances.
// The six sums of a workgroup's learner samples: each term widened to f64 and added to the lane's own sum, tile after tile, then
// the 64 lanes of a wavefront in a fixed shuffle tree, then the four wavefronts in order, into d_partials[blockIdx.x]: no atomics,
// the same bits every time.  k_ppo_loss_stats, one wavefront behind it on the stream, adds the partials in ascending order — 64
// rows at a time through LDS, so that the loads are coalesced and only the additions are sequential — and derives the stats.
#pragma once

namespace {

constexpr int PPO_TILES = 4;              // tiles of BLOCK rows a workgroup walks
constexpr int PPO_P = BLOCK * PPO_TILES;  // minibatch rows per partial: one workgroup

struct PpoArgs {
    const uint8_t* actions;    // [S]
    const float* logp_old;     // [S]
    const float* advantages;   // [S]
    const float* targets;      // [S]
    const uint8_t* seat;       // [S / 2] or NULL
    const float* logits_old;   // [S][6] or NULL (OLD)
    const double* moments;     // [3] or NULL
    const float* logits;       // [M][6]
    const float* values;       // [M]
    const int32_t* index;      // [M] or NULL
    float* grad_logits;        // [M][6]
    float* grad_values;        // [M]
    double* partials;          // [gridDim.x][6] or NULL
    float* terms;              // [M][4] or NULL
    int64_t n_samples, first, m;
    float clip_lo, clip_hi, vf_clip, vf_coeff, ent_coeff, kl_coeff;
};

// the header's softmax of one row: lp_i and p_i
__device__ __forceinline__ void ppo_softmax(const float (&l)[6], float (&lp)[6], float (&p)[6]) {
#pragma clang fp contract(off)
    float m = l[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) m = l[i] > m ? l[i] : m;
    float d[6], w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        d[i] = l[i] - m;
        w[i] = expf(d[i]);
    }
    float S = w[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) S = S + w[i];
    const float log_s = logf(S);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        lp[i] = d[i] - log_s;
        p[i] = w[i] / S;
    }
}

template <bool OLD>
__global__ __launch_bounds__(BLOCK) void k_ppo_loss(PpoArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[6][BLOCK / 64];
    const int tid = threadIdx.x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the lane's sums over its rows, one per tile, in the order of the tiles
    for (int tile = 0; tile < PPO_TILES; ++tile) {
        const int64_t row0 = ((int64_t)blockIdx.x * PPO_TILES + tile) * BLOCK, row = row0 + tid;
        if (row0 >= a.m) break;  // (uniform)
        const bool live = row < a.m;
        // ---- which sample, and everything that is read through it, before anything is used
        int64_t s = a.first + row;
        bool in = live;
        if (a.index) {
            const int32_t ix = live ? a.index[row] : -1;
            s = ix;
            in = ix >= 0 && (int64_t)ix < a.n_samples;
        }
        uint32_t act = 255u, st = 255u;
        float lpo = 0.f, A = 0.f, tg = 0.f, v = 0.f;
        float2 o0 = make_float2(0.f, 0.f), o1 = o0, o2 = o0, x0 = o0, x1 = o0, x2 = o0;
        if (in) {
            act = a.actions[s];
            lpo = a.logp_old[s];
            A = a.advantages[s];
            tg = a.targets[s];
            if (a.seat) st = a.seat[s >> 1];
            if constexpr (OLD) {
                const float2* src = reinterpret_cast<const float2*>(a.logits_old) + 3 * s;
                o0 = src[0], o1 = src[1], o2 = src[2];
            }
        }
        if (live) {
            v = a.values[row];
            const float2* src = reinterpret_cast<const float2*>(a.logits) + 3 * row;
            x0 = src[0], x1 = src[1], x2 = src[2];
        }
        const bool left_out = !in || act > 5u || st == (uint32_t)(s & 1);
        // ---- the header's arithmetic
        const float l[6] = {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y};
        float lp[6], p[6], lq[6], q[6];
        ppo_softmax(l, lp, p);
        if constexpr (OLD) {
            const float lo[6] = {o0.x, o0.y, o1.x, o1.y, o2.x, o2.y};
            ppo_softmax(lo, lq, q);
        }
        float logp = lp[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) logp = act == (uint32_t)i ? lp[i] : logp;
        const float ratio = expf(logp - lpo);
        float Ah = A;
        if (a.moments) {
            const double n = a.moments[0], m1 = a.moments[1], m2 = a.moments[2];
            if (n >= 1.0) {
                const double mean = m1 / n;
                double var = m2 / n - mean * mean;
                var = var > 0.0 ? var : 0.0;
                double sd = sqrt(var);
                sd = sd > 1e-4 ? sd : 1e-4;
                Ah = (float)(((double)A - mean) / sd);
            }
        }
        const float s1 = ratio * Ah;
        float rc = ratio < a.clip_lo ? a.clip_lo : ratio;
        rc = rc > a.clip_hi ? a.clip_hi : rc;
        const float s2 = rc * Ah;
        const bool unclipped = s1 <= s2;
        const float surr = unclipped ? s1 : s2;
        float h_acc = 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float t = p[i] * lp[i];
            t = p[i] == 0.f ? 0.f : t;
            h_acc = i == 0 ? t : h_acc + t;
        }
        const float H = -h_acc;
        const float dv = v - tg;
        const float vf = dv * dv;
        const bool vf_inside = vf <= a.vf_clip;
        const float vfc = vf_inside ? vf : a.vf_clip;
        float kl = lpo - logp;
        if constexpr (OLD) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                float t = q[i] * (lq[i] - lp[i]);
                t = q[i] == 0.f ? 0.f : t;
                kl = i == 0 ? t : kl + t;
            }
        }
        const float g = unclipped ? -s1 : 0.f;
        float gl[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float t1 = g * ((act == (uint32_t)i ? 1.f : 0.f) - p[i]);
            float t2 = (a.ent_coeff * p[i]) * (lp[i] + H);
            t2 = p[i] == 0.f ? 0.f : t2;
            float gi = t1 + t2;
            if constexpr (OLD) gi = gi + a.kl_coeff * (p[i] - q[i]);
            gl[i] = left_out ? 0.f : gi;  // a select: a NaN of a left-out sample reaches nothing
        }
        float gv = vf_inside ? 2.f * dv : 0.f;
        gv = a.vf_coeff * gv;
        gv = left_out ? 0.f : gv;
        const bool outside = ratio < a.clip_lo || ratio > a.clip_hi;
        // ---- the stores
        if (live) {
            a.grad_values[row] = gv;
            if (a.terms)
                reinterpret_cast<float4*>(a.terms)[row] = left_out ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(surr, vfc, H, kl);
            float2* dst = reinterpret_cast<float2*>(a.grad_logits) + 3 * row;
            dst[0] = make_float2(gl[0], gl[1]), dst[1] = make_float2(gl[2], gl[3]), dst[2] = make_float2(gl[4], gl[5]);
        }
        const double x[6] = {1.0, (double)(-surr), (double)vfc, (double)H, (double)kl, outside ? 1.0 : 0.0};  // each term widened first
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += left_out ? 0.0 : x[c];
    }
    // ---- the six sums of the workgroup's learner samples
    if (a.partials) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double x = acc[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if ((tid & 63) == 0) red[c][tid >> 6] = x;
        }
        __syncthreads();
        if (tid < 6) {
            double sum = red[tid][0];
#pragma unroll
            for (int w = 1; w < BLOCK / 64; ++w) sum += red[tid][w];
            a.partials[(int64_t)blockIdx.x * 6 + tid] = sum;
        }
    }
}

// d_stats of the partials: sums[c] = partials[0][c] + partials[1][c] + ... in ascending order, by lane c of one wavefront.  The 64
// lanes load 64 rows of partials at a time (384 consecutive doubles, coalesced; the next 64 rows are in flight while these are
// added) and hand them over through LDS; a lane reads its 64 numbers before it adds the first, so that what is sequential is the 64
// additions and nothing else.
__global__ __launch_bounds__(64) void k_ppo_loss_stats(const double* __restrict__ partials, int64_t count, double* __restrict__ stats,
                                                        float vf_coeff, float ent_coeff, float kl_coeff) {
#pragma clang fp contract(off)
    __shared__ double chunk[64 * 6];
    const int lane = threadIdx.x;
    const int64_t total = count * 6;
    double nxt[6], sum = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) nxt[q] = lane + 64 * q < total ? partials[lane + 64 * q] : 0.0;
    for (int64_t k0 = 0; k0 < count; k0 += 64) {
        __syncthreads();  // (the rows of the chunk before are read)
#pragma unroll
        for (int q = 0; q < 6; ++q) chunk[lane + 64 * q] = nxt[q];
        __syncthreads();
        if (k0 + 64 < count) {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int64_t at = (k0 + 64) * 6 + lane + 64 * q;
                nxt[q] = at < total ? partials[at] : 0.0;
            }
        }
        if (lane < 6) {  // (rows beyond the last partial hold +0.0, which changes no sum: the chain needs no bound)
            double x[64];
#pragma unroll
            for (int r = 0; r < 64; ++r) x[r] = chunk[r * 6 + lane];
#pragma unroll
            for (int r = 0; r < 64; ++r) sum += x[r];
        }
    }
    __syncthreads();
    if (lane < 6) chunk[lane] = sum;
    __syncthreads();
    if (lane == 0) {
        const double n = chunk[0];
        double out[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (n > 0.0) {
            const double policy = chunk[1] / n, vf = chunk[2] / n, H = chunk[3] / n, kl = chunk[4] / n;
            out[0] = n;
            out[1] = ((policy + (double)vf_coeff * vf) - (double)ent_coeff * H) + (double)kl_coeff * kl;
            out[2] = policy, out[3] = vf, out[4] = H, out[5] = kl;
            out[6] = chunk[5] / n;
            out[7] = 1.0 / n;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) stats[i] = out[i];
    }
}

const char* const PPO_WHO = "oc_ppo_loss";

int ppo_refuse_as(const char* who, const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail(OC_EINVAL, msg);
}

// the check that needs no array (oc_ppo_loss_plan makes this one alone)
int ppo_check_shape(int64_t n_minibatch, const char* who = PPO_WHO) {
    auto ppo_refuse = [who](const char* why) { return ppo_refuse_as(who, why); };
    if (n_minibatch < 0) return ppo_refuse("n_minibatch < 0");
    if (n_minibatch > ((int64_t)1 << 38)) return ppo_refuse("n_minibatch above 2^38");
    return OC_OK;
}

bool ppo_positive(float x) { return x > 0.f && x < __builtin_inff(); }

// (who: the entry point the refusals name — oc_ppo_loss, or the caller of several stages that makes them ahead of its launches)
int ppo_check(const OcPpoLoss* q, const char* who = PPO_WHO) {
    auto ppo_refuse = [who](const char* why) { return ppo_refuse_as(who, why); };
    if (!q) return ppo_refuse("loss is NULL");
    if (!q->d_actions || !q->d_logp_old || !q->d_advantages || !q->d_targets || !q->d_logits || !q->d_values || !q->d_grad_logits ||
        !q->d_grad_values)
        return ppo_refuse("NULL d_actions, d_logp_old, d_advantages, d_targets, d_logits, d_values, d_grad_logits or d_grad_values");
    if (((uintptr_t)q->d_logp_old | (uintptr_t)q->d_advantages | (uintptr_t)q->d_targets | (uintptr_t)q->d_values | (uintptr_t)q->d_index |
         (uintptr_t)q->d_grad_values) & 3u)
        return ppo_refuse("d_logp_old, d_advantages, d_targets, d_values, d_index and d_grad_values must be 4-byte aligned");
    if (((uintptr_t)q->d_logits_old | (uintptr_t)q->d_moments | (uintptr_t)q->d_partials | (uintptr_t)q->d_stats) & 7u)
        return ppo_refuse("d_logits_old, d_moments, d_partials and d_stats must be 8-byte aligned");
    if (((uintptr_t)q->d_logits | (uintptr_t)q->d_grad_logits | (uintptr_t)q->d_terms_out) & 15u)
        return ppo_refuse("d_logits, d_grad_logits and d_terms_out must be 16-byte aligned");
    if (int rc = ppo_check_shape(q->n_minibatch, who)) return rc;
    if (q->n_samples < 0) return ppo_refuse("n_samples < 0");
    if (q->d_seat && (q->n_samples & 1)) return ppo_refuse("n_samples must be even with d_seat");
    if (q->d_index) {
        if (q->n_samples >= ((int64_t)1 << 31)) return ppo_refuse("n_samples must be below 2^31 with d_index");
    } else if (q->first_sample < 0 || q->first_sample > q->n_samples || q->n_minibatch > q->n_samples - q->first_sample) {
        return ppo_refuse("first_sample .. first_sample + n_minibatch must lie inside 0 .. n_samples without d_index");
    }
    if (!ppo_positive(q->clip_param)) return ppo_refuse("clip_param must be finite and positive");
    if (!ppo_positive(q->vf_clip_param)) return ppo_refuse("vf_clip_param must be finite and positive");
    if (!(q->vf_loss_coeff >= 0.f) || !(q->entropy_coeff >= 0.f) || !(q->kl_coeff >= 0.f))
        return ppo_refuse("vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0");
    if (q->kl_coeff > 0.f && !q->d_logits_old) return ppo_refuse("kl_coeff > 0 needs d_logits_old");
    if (q->d_stats && !q->d_partials) return ppo_refuse("d_stats needs d_partials");
    return OC_OK;
}

// the launches of a call that ppo_check has passed
int ppo_run(const OcPpoLoss* q, hipStream_t stream, const char* who = PPO_WHO) {
    const int64_t m = q->n_minibatch;
    if (m == 0) {  // no row: nothing to launch; the stats of no sample are zeros
        if (q->d_stats && hipMemsetAsync(q->d_stats, 0, 8 * sizeof(double), stream) != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "%s: %s", who, hipGetErrorString(hipGetLastError()));
            return OC_ELAUNCH;
        }
        return OC_OK;
    }
    PpoArgs a;
    a.actions = q->d_actions; a.logp_old = q->d_logp_old; a.advantages = q->d_advantages; a.targets = q->d_targets; a.seat = q->d_seat;
    a.logits_old = q->d_logits_old; a.moments = q->d_moments; a.logits = q->d_logits; a.values = q->d_values; a.index = q->d_index;
    a.grad_logits = q->d_grad_logits; a.grad_values = q->d_grad_values; a.partials = q->d_partials; a.terms = q->d_terms_out;
    a.n_samples = q->n_samples; a.first = q->first_sample; a.m = m;
    a.clip_lo = 1.f - q->clip_param;  // one f32 operation each
    a.clip_hi = 1.f + q->clip_param;
    a.vf_clip = q->vf_clip_param; a.vf_coeff = q->vf_loss_coeff; a.ent_coeff = q->entropy_coeff; a.kl_coeff = q->kl_coeff;
    const unsigned grid = (unsigned)((m + PPO_P - 1) / PPO_P);
    if (a.logits_old) hipLaunchKernelGGL((k_ppo_loss<true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((k_ppo_loss<false>), dim3(grid), dim3(BLOCK), 0, stream, a);
    if (q->d_stats)
        hipLaunchKernelGGL(k_ppo_loss_stats, dim3(1), dim3(64), 0, stream, (const double*)q->d_partials, (int64_t)grid, q->d_stats,
                           a.vf_coeff, a.ent_coeff, a.kl_coeff);
    return check_launch(who);
}

}  // namespace

extern "C" {

int oc_ppo_loss(const OcPpoLoss* q, void* stream) {
    if (int rc = ppo_check(q)) return rc;
    return ppo_run(q, (hipStream_t)stream);
}

int oc_ppo_loss_plan(int64_t n_minibatch, int with_index, int with_seat, int with_moments, int with_old_logits, int with_terms, char* out,
                     size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_ppo_loss_plan: no output buffer");
    out[0] = 0;
    if (int rc = ppo_check_shape(n_minibatch)) return rc;
    if (n_minibatch == 0) {
        snprintf(out, out_size, "nothing to launch (no samples)");
        return OC_OK;
    }
    const long long grid = (long long)((n_minibatch + PPO_P - 1) / PPO_P);
    snprintf(out, out_size,
             "k_ppo_loss<OLD=%s> grid=%lld, %d lanes (one per sample, %d tiles of %d), %d samples per partial, index=%s seat=%s moments=%s terms=%s"
             " + k_ppo_loss_stats grid=1, 64 lanes, %lld partial(s) (with d_stats)",
             with_old_logits ? "true" : "false", grid, BLOCK, PPO_TILES, BLOCK, PPO_P, with_index ? "yes" : "no", with_seat ? "yes" : "no",
             with_moments ? "yes" : "no", with_terms ? "yes" : "no", grid);
    return OC_OK;
}

}  // extern "C"
