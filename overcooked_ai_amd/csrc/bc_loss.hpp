// bc_loss.hpp — the behaviour-cloning loss of a minibatch, sparse categorical cross-entropy from logits with optional class weights,
// its gradients with respect to the policy's logits and its accuracy: k_bc_loss, k_bc_loss_stats, oc_bc_loss, oc_bc_loss_plan
// (include/oc_amd.h: OcBcLoss)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind adam.hpp.  Of ppo_loss.hpp
// it calls ppo_softmax (the header's softmax of a row), PPO_TILES / PPO_P (the shape of a workgroup's walk), ppo_refuse_as and
// ppo_check_shape; no kernel or entry point there knows of this file.
//
// k_bc_loss is k_ppo_loss's shape with less to read: one lane per minibatch row; a workgroup walks PPO_TILES tiles of BLOCK consecutive
// rows — PPO_P rows, one partial.  A lane loads its 24-byte row of logits and stores its row of gradients as three 8-byte accesses.
// The one thing read through the index is the action byte; it is issued beside the row's logits, before either is used.  The six
// class weights are wavefront-uniform: they are read once, ahead of the tiles, and a row's weight is a select on its action, not a
// load behind it.  Gradient stores (training) or none (evaluation) is a template parameter; index, class weights, per-row losses and
// partials are wavefront-uniform branches on a pointer of the argument block.  Two instances.
// The four sums of a workgroup's kept rows: each term widened to f64 and added to the lane's own sum, tile after tile, then the 64
// lanes of a wavefront in a fixed shuffle tree, then the four wavefronts in order, into d_partials[blockIdx.x]: no atomics, the same
// bits every time.  k_bc_loss_stats, one wavefront behind it on the stream, adds the partials in ascending order — 64 rows at a time
// through LDS, as k_ppo_loss_stats does — and derives the stats.
#pragma once

namespace {

struct BcArgs {
    const uint8_t* actions;       // [S]
    const float* class_weights;   // [6] or NULL
    const float* logits;          // [M][6]
    const int32_t* index;         // [M] or NULL
    float* grad_logits;           // [M][6] (GRAD)
    float* grad_values;           // [M] (GRAD)
    float* loss_out;              // [M] or NULL
    double* partials;             // [gridDim.x][4] or NULL
    int64_t n_samples, first, m;
};

template <bool GRAD>
__global__ __launch_bounds__(BLOCK) void k_bc_loss(BcArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[4][BLOCK / 64];
    const int tid = threadIdx.x;
    float cw[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};  // (uniform: six loads per wavefront, ahead of the tiles)
    if (a.class_weights) {
#pragma unroll
        for (int i = 0; i < 6; ++i) cw[i] = a.class_weights[i];
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // the lane's sums over its rows, one per tile, in the order of the tiles
    for (int tile = 0; tile < PPO_TILES; ++tile) {
        const int64_t row0 = ((int64_t)blockIdx.x * PPO_TILES + tile) * BLOCK, row = row0 + tid;
        if (row0 >= a.m) break;  // (uniform)
        const bool live = row < a.m;
        // ---- which sample, its action and the row's logits, before anything is used
        int64_t s = a.first + row;
        bool in = live;
        if (a.index) {
            const int32_t ix = live ? a.index[row] : -1;
            s = ix;
            in = ix >= 0 && (int64_t)ix < a.n_samples;
        }
        uint32_t act = 255u;
        float2 x0 = make_float2(0.f, 0.f), x1 = x0, x2 = x0;
        if (in) act = a.actions[s];
        if (live) {
            const float2* src = reinterpret_cast<const float2*>(a.logits) + 3 * row;
            x0 = src[0], x1 = src[1], x2 = src[2];
        }
        const bool left_out = !in || act > 5u;
        // ---- the header's arithmetic
        const float l[6] = {x0.x, x0.y, x1.x, x1.y, x2.x, x2.y};
        float lp[6], p[6];
        ppo_softmax(l, lp, p);
        float m = l[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) m = l[i] > m ? l[i] : m;
        uint32_t best = 6u;  // the lowest i with l_i == m (none where the row holds a NaN)
#pragma unroll
        for (int i = 5; i >= 0; --i) best = l[i] == m ? (uint32_t)i : best;
        float lpa = lp[0], c = cw[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) {
            lpa = act == (uint32_t)i ? lp[i] : lpa;
            c = act == (uint32_t)i ? cw[i] : c;
        }
        const float ce = -lpa;
        const float loss = c * ce;
        const bool correct = act == best;
        // ---- the stores
        if (live) {
            if constexpr (GRAD) {
                float gl[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const float gi = c * (p[i] - (act == (uint32_t)i ? 1.f : 0.f));
                    gl[i] = left_out ? 0.f : gi;  // a select: a NaN of a left-out row reaches nothing
                }
                a.grad_values[row] = 0.f;
                float2* dst = reinterpret_cast<float2*>(a.grad_logits) + 3 * row;
                dst[0] = make_float2(gl[0], gl[1]), dst[1] = make_float2(gl[2], gl[3]), dst[2] = make_float2(gl[4], gl[5]);
            }
            if (a.loss_out) a.loss_out[row] = left_out ? 0.f : loss;
        }
        const double x[4] = {1.0, (double)loss, correct ? 1.0 : 0.0, (double)c};  // each term widened first
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += left_out ? 0.0 : x[k];
    }
    // ---- the four sums of the workgroup's kept rows
    if (a.partials) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double x = acc[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if ((tid & 63) == 0) red[k][tid >> 6] = x;
        }
        __syncthreads();
        if (tid < 4) {
            double sum = red[tid][0];
#pragma unroll
            for (int w = 1; w < BLOCK / 64; ++w) sum += red[tid][w];
            a.partials[(int64_t)blockIdx.x * 4 + tid] = sum;
        }
    }
}

// d_stats of the partials: sums[c] = partials[0][c] + partials[1][c] + ... in ascending order, by lane c of one wavefront.  The 64
// lanes load 64 rows of partials at a time (256 consecutive doubles, coalesced; the next 64 rows are in flight while these are added)
// and hand them over through LDS; a lane reads its 64 numbers before it adds the first.
__global__ __launch_bounds__(64) void k_bc_loss_stats(const double* __restrict__ partials, int64_t count, double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double chunk[64 * 4];
    const int lane = threadIdx.x;
    const int64_t total = count * 4;
    double nxt[4], sum = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) nxt[q] = lane + 64 * q < total ? partials[lane + 64 * q] : 0.0;
    for (int64_t k0 = 0; k0 < count; k0 += 64) {
        __syncthreads();  // (the rows of the chunk before are read)
#pragma unroll
        for (int q = 0; q < 4; ++q) chunk[lane + 64 * q] = nxt[q];
        __syncthreads();
        if (k0 + 64 < count) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t at = (k0 + 64) * 4 + lane + 64 * q;
                nxt[q] = at < total ? partials[at] : 0.0;
            }
        }
        if (lane < 4) {  // (rows beyond the last partial hold +0.0, which changes no sum: the chain needs no bound)
            double x[64];
#pragma unroll
            for (int r = 0; r < 64; ++r) x[r] = chunk[r * 4 + lane];
#pragma unroll
            for (int r = 0; r < 64; ++r) sum += x[r];
        }
    }
    __syncthreads();
    if (lane < 4) chunk[lane] = sum;
    __syncthreads();
    if (lane == 0) {
        const double n = chunk[0];
        double out[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (n > 0.0) {
            out[0] = n;
            out[1] = chunk[1] / n;
            out[2] = chunk[2] / n;
            out[3] = chunk[3] / n;
            out[7] = 1.0 / n;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) stats[i] = out[i];
    }
}

const char* const BC_WHO = "oc_bc_loss";

// (who: the entry point the refusals name — oc_bc_loss, or the caller of several stages that makes them ahead of its launches)
int bc_check(const OcBcLoss* q, const char* who = BC_WHO) {
    auto refuse = [who](const char* why) { return ppo_refuse_as(who, why); };
    if (!q) return refuse("loss is NULL");
    if (!q->d_actions || !q->d_logits) return refuse("NULL d_actions or d_logits");
    if (!q->d_grad_logits != !q->d_grad_values) return refuse("d_grad_logits and d_grad_values must be given together (both NULL: evaluation)");
    if (((uintptr_t)q->d_class_weights | (uintptr_t)q->d_index | (uintptr_t)q->d_grad_values | (uintptr_t)q->d_loss_out) & 3u)
        return refuse("d_class_weights, d_index, d_grad_values and d_loss_out must be 4-byte aligned");
    if (((uintptr_t)q->d_logits | (uintptr_t)q->d_grad_logits | (uintptr_t)q->d_partials | (uintptr_t)q->d_stats) & 7u)
        return refuse("d_logits, d_grad_logits, d_partials and d_stats must be 8-byte aligned");
    if (int rc = ppo_check_shape(q->n_minibatch, who)) return rc;
    if (q->n_samples < 0) return refuse("n_samples < 0");
    if (q->d_index) {
        if (q->n_samples >= ((int64_t)1 << 31)) return refuse("n_samples must be below 2^31 with d_index");
    } else if (q->first_sample < 0 || q->first_sample > q->n_samples || q->n_minibatch > q->n_samples - q->first_sample) {
        return refuse("first_sample .. first_sample + n_minibatch must lie inside 0 .. n_samples without d_index");
    }
    if (q->d_stats && !q->d_partials) return refuse("d_stats needs d_partials");
    return OC_OK;
}

// the launches of a call that bc_check has passed
int bc_run(const OcBcLoss* q, hipStream_t stream, const char* who = BC_WHO) {
    const int64_t m = q->n_minibatch;
    if (m == 0) {  // no row: nothing to launch; the stats of no sample are zeros
        if (q->d_stats && hipMemsetAsync(q->d_stats, 0, 8 * sizeof(double), stream) != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "%s: %s", who, hipGetErrorString(hipGetLastError()));
            return OC_ELAUNCH;
        }
        return OC_OK;
    }
    BcArgs a;
    a.actions = q->d_actions; a.class_weights = q->d_class_weights; a.logits = q->d_logits; a.index = q->d_index;
    a.grad_logits = q->d_grad_logits; a.grad_values = q->d_grad_values; a.loss_out = q->d_loss_out; a.partials = q->d_partials;
    a.n_samples = q->n_samples; a.first = q->first_sample; a.m = m;
    const unsigned grid = (unsigned)((m + PPO_P - 1) / PPO_P);
    if (a.grad_logits) hipLaunchKernelGGL((k_bc_loss<true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((k_bc_loss<false>), dim3(grid), dim3(BLOCK), 0, stream, a);
    if (q->d_stats) hipLaunchKernelGGL(k_bc_loss_stats, dim3(1), dim3(64), 0, stream, (const double*)q->d_partials, (int64_t)grid, q->d_stats);
    return check_launch(who);
}

}  // namespace

extern "C" {

int oc_bc_loss(const OcBcLoss* q, void* stream) {
    if (int rc = bc_check(q)) return rc;
    return bc_run(q, (hipStream_t)stream);
}

int oc_bc_loss_plan(int64_t n_minibatch, int with_index, int with_class_weights, int with_gradients, int with_loss_out, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_bc_loss_plan: no output buffer");
    out[0] = 0;
    if (int rc = ppo_check_shape(n_minibatch, BC_WHO)) return rc;
    if (n_minibatch == 0) {
        snprintf(out, out_size, "nothing to launch (no samples)");
        return OC_OK;
    }
    const long long grid = (long long)((n_minibatch + PPO_P - 1) / PPO_P);
    snprintf(out, out_size,
             "k_bc_loss<GRAD=%s> grid=%lld, %d lanes (one per sample, %d tiles of %d), %d samples per partial, index=%s class_weights=%s loss_out=%s"
             " + k_bc_loss_stats grid=1, 64 lanes, %lld partial(s) (with d_stats)",
             with_gradients ? "true" : "false", grid, BLOCK, PPO_TILES, BLOCK, PPO_P, with_index ? "yes" : "no", with_class_weights ? "yes" : "no",
             with_loss_out ? "yes" : "no", grid);
    return OC_OK;
}

}  // extern "C"
