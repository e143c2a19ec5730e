// bc_fused.hpp — a run of behaviour-cloning minibatches of at most 128 rows in ONE kernel of ONE workgroup: k_bc_epoch_fused,
// oc_bc_epoch_fused, oc_bc_epoch_fused_plan (include/oc_amd.h: OcBcEpochFused)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind update_chain.hpp.  It computes what
// oc_bc_update computes, bit for bit, for the shapes in which every stage of that chain is itself one workgroup — a minibatch of at
// most BCF_ROWS = 128 rows (pol_grid returns 1, k_policy_grad_sum is the identity over one partial, k_bc_loss writes one partial) and
// in_dim 56, 76 or 96 (two or three feature tiles: the instances NF = 2 and NF = 3) — without the six dependent launches of a minibatch
// and without an intermediate array: logits, upstream gradients, partials and weight gradients stay in LDS and registers.
//
// The workgroup is BLOCK = 256 lanes, launched once for up to BCF_PER_LAUNCH = 64 minibatches (a launch then runs a few milliseconds
// at the tens of microseconds a minibatch takes; docs/NOTEBOOK.md); the host chains the launches of an epoch on the caller's stream.
// Per minibatch k, from the weights minibatch k - 1 left:
//   stage     W1, W2, W2 transposed, (Wp|wv) both ways and the biases from global memory into LDS, as k_policy_forward and
//             k_policy_backward stage them (mlp_tile.hpp: pol_stage_dealt, pol_stage_biases; policy.hpp: pol_stage_w2_back and
//             pol_stage_head_back, which k_policy_backward holds as its own lambdas, pol_stage_head_forward, pol_stage_head_bias)
//   forward   wavefront w gathers tile w (rows 32 w .. 32 w + 31) through the index (pol_source, pol_load_rows: a row out of range is a
//             row of zeros), runs pol_hidden (mlp_tile.hpp) and k_policy_forward's last layer, and leaves the logits in its [row][8] image (zeros
//             for a row without a source, as k_policy_forward stores them)
//   head      lane r of the workgroup takes row r (row r on lane r % 64 of wavefront r / 64, k_bc_loss's dealing): bc_loss.hpp's
//             arithmetic, the gradients back into the [row][8] image, the four f64 sums in k_bc_loss's order (the shuffle tree 32 .. 1,
//             then the wavefronts in ascending order), the stats as k_bc_loss_stats derives them
//   backward  k_policy_backward's tile body on the pre-activations the forward pass left in registers (that kernel recomputes them
//             with the same instructions), including the skip of a tile whose 32 upstream rows are all zero; the wavefronts'
//             2 NF + 6 accumulator tiles are added ((w0 + w1) + w2) + w3 through LDS over the weights
//   adam      k_adam_step's three phases on that sum with grad_scale = stats[7]: lane l owns the flat elements i % 256 == l, the f64
//             tree 128 .. 1, the same skip rules and clock; the scaled gradients' image lies over the row images, which are dead
// Shared with the policy kernels: the stager and every staging function named above, pol_hidden, pol_source, pol_load_rows.
// The bodies of k_policy_backward's tile, of its wavefront sum and of k_bc_loss's row stand here a second time (bcf_tile_back,
// bcf_sum_waves, bcf_partial_element, bcf_row, bcf_row_grads, bcf_sum_lanes, bcf_stats_of): moved into functions that those kernels
// call too, they changed the register counts of k_policy_backward and the order of k_bc_loss's loads (docs/NOTEBOOK.md).  The last
// forward layer and the LDS carve-up stand here a second time too (mlp_tile.hpp: pol_head, pl_operands): with either, this kernel's
// ds_ instruction count moved by one or two (read pairs of the bias loads split); as it stands the kernel is the assembly it was
// before mlp_tile.hpp existed.
// Adam's scalars and element update are shared (adam.hpp: adam_step_of, adam_element; k_adam_step compiles to the same instructions).
//
// Visibility.  Adam's stores to the parameters are plain vector stores by the lanes that own the elements; the staging loads of
// minibatch k + 1 are plain vector loads by other lanes of the SAME workgroup.  Between them stands the __syncthreads() at the top of
// the loop: HIP lowers it to a workgroup-scope release fence (s_waitcnt vmcnt(0): every store of the wavefront has left for the
// CU's vector L1, which is write-through), s_barrier, and a workgroup-scope acquire fence.  All wavefronts of a workgroup run on one
// CU and (the kernel is not built for threadgroup-split mode) share its vector L1, so a load behind the barrier finds the stored
// bytes there or below it; no agent-scope fence, which is what ANOTHER CU would need, is called for.  Nothing that is written in the
// kernel is read again through the scalar cache: the clock is read once, ahead of the loop, and kept in registers (every lane keeps
// the same four doubles; lane 0 stores them), and the class weights are never written.
// Plain C++ and MFMA builtins, vector stores only, no atomics: a call on the same inputs gives the same bits.
#pragma once

namespace {

constexpr int BCF_ROWS = 128;        // rows of a minibatch, at most: one 32-row tile per wavefront
constexpr int BCF_PER_LAUNCH = 64;   // minibatches of one launch, at most
constexpr int BCF_F64 = ADAM_LANES + 4 * (BLOCK / 64) + 8;  // f64 of LDS: Adam's tree, the head's wavefront sums, its four sums and the gradient scale
constexpr size_t BCF_LDS_MAX = 160 * 1024;

struct BcFusedArgs {
    float* p[8];             // the parameters, Keras layout, [in][out]: w1 b1 w2 b2 wp bp wv bv
    float* m[8];
    float* v[8];
    int start[9];            // flat index of the first element of every array, and their sum
    int in_dim, h1, h2;
    const float* features;   // [n_feature_rows][in_dim]
    int64_t n_feature_rows;
    const int32_t* index;    // the entries of this launch's minibatches
    int64_t n;               // their number
    int minibatch, count;    // rows of a minibatch (the last may be shorter); minibatches of this launch
    const uint8_t* actions;  // [n_samples]
    const float* class_weights;  // [6] or NULL
    int64_t n_samples;
    double* clock;           // [4]
    double* stats;           // [count][8]
    double* info;            // [count][4]
    float lr, beta1, beta2, eps, max_grad_norm;
    unsigned long long* stamps;  // OC_AMD_TUNING: [count][BCF_STAMPS] cycle counts of lane 0, or NULL
};

constexpr int BCF_STAMPS = 6;  // start, staged, forward done, head done, backward and sum done, Adam done
#ifdef OC_AMD_TUNING
unsigned long long* g_bcf_stamps = nullptr;
#define BCF_STAMP(j)                                                                                          \
    do {                                                                                                      \
        if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)k * BCF_STAMPS + (j)] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define BCF_STAMP(j) \
    do {             \
    } while (0)
#endif

// x, behind a statement the optimiser cannot see through: the staging loops and Adam's walk are the same for every minibatch, and with
// their counts known the compiler unrolls them and keeps a register per address alive across the whole loop over the minibatches
// (116 bytes of scratch per lane); with an opaque count the addresses are computed where they are used
__device__ __forceinline__ int bcf_opaque(int x) {
    asm volatile("" : "+s"(x));
    return x;
}

__host__ __device__ constexpr int bcf_wave_floats(int in_dim) { return pol_image_floats(in_dim) + POL_BUF + POL_D3; }
__host__ __device__ constexpr int bcf_weight_floats(int in_dim) { return pl_w1_floats(in_dim) + 2 * PL_W2 + POL_WPT + 2 * PL_HID; }
// dynamic LDS: the f64 words, k_policy_backward's operands and images, the last forward layer's operand and bias
__host__ __device__ constexpr size_t bcf_lds(int in_dim) {
    return sizeof(double) * BCF_F64 + sizeof(float) * (size_t)(bcf_weight_floats(in_dim) + PL_WAVES * bcf_wave_floats(in_dim) + PL_W3 + 32);
}

// ---- k_policy_backward's tile body behind pol_hidden (policy.hpp), word for word: delta2 and delta1 from the row's seven upstream
// gradients (u0, u1, u2: the logits', uv: the value's) and the pre-activations (c: layer 1, d: layer 2), and the tile's terms of the
// weight and bias gradients added to the wavefront's accumulators.  sx holds the tile's feature rows and is overwritten by a1.
template <int NF>
__device__ __forceinline__ void bcf_tile_back(const float* swpt, const float* sw2t, float* sx, float* sd, float* sg, int S, int lane, float2 u0, float2 u1,
                                              float2 u2, float uv, const pl_f32x16& c0, const pl_f32x16& c1, const pl_f32x16& d0, const pl_f32x16& d1,
                                              pl_f32x16 (&g1)[NF][2], pl_f32x16 (&g2)[2][2], pl_f32x16 (&g3)[2], float& gb1, float& gb2, float& gb3) {
    const int col = lane & 31, h = lane >> 5;
    const pl_f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ---- delta2 = [pre2 > 0] (Wp|wv) delta3: lane half h supplies outputs 2 s + h
    pl_f32x16 e0 = zero16, e1 = zero16;
    {
        const float b3[4] = {h ? u0.y : u0.x, h ? u1.y : u1.x, h ? u2.y : u2.x, h ? 0.f : uv};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            e0 = __builtin_amdgcn_mfma_f32_32x32x2f32(swpt[(2 * s) * 64 + lane], b3[s], e0, 0, 0, 0);
            e1 = __builtin_amdgcn_mfma_f32_32x32x2f32(swpt[(2 * s + 1) * 64 + lane], b3[s], e1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        e0[reg] = d0[reg] > 0.f ? e0[reg] : 0.f;
        e1[reg] = d1[reg] > 0.f ? e1[reg] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- gbp|gbv, gWp|gwv += a2t delta3: K = the tile's rows, two at a step; a2 as [row][unit], delta3 as [row][8]
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        sd[col * POL_P + 2 * reg + h] = fmaxf(d0[reg], 0.f);
        sd[col * POL_P + 32 + 2 * reg + h] = fmaxf(d1[reg], 0.f);
    }
    if (h == 0) {
        float4* const dst = reinterpret_cast<float4*>(sg + col * 8);
        dst[0] = make_float4(u0.x, u0.y, u1.x, u1.y);
        dst[1] = make_float4(u2.x, u2.y, uv, 0.f);
    }
    pl_wave_fence();
    if (lane < 8) {
#pragma unroll 8
        for (int r = 0; r < 32; ++r) gb3 += sg[r * 8 + lane];
    }
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
        const int at = (2 * s + h) * POL_P + col;
        const float x0 = sd[at], x1 = sd[at + 32];
        float b = sg[(2 * s + h) * 8 + (col & 7)];
        b = col < 8 ? b : 0.f;
        g3[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, b, g3[0], 0, 0, 0);
        g3[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, b, g3[1], 0, 0, 0);
    }
    pl_wave_fence();
    __builtin_amdgcn_sched_barrier(0);
    // ---- delta1 = [pre1 > 0] W2 delta2, into the delta buffer [row][unit]
    {
        pl_f32x16 f0 = zero16, f1 = zero16;
#pragma unroll
        for (int s = 0; s < PL_STEPS; ++s) {
            const float b = s < 16 ? e0[s & 15] : e1[s & 15];
            f0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw2t[(2 * s) * 64 + lane], b, f0, 0, 0, 0);
            f1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw2t[(2 * s + 1) * 64 + lane], b, f1, 0, 0, 0);
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            sd[col * POL_P + 2 * reg + h] = c0[reg] > 0.f ? f0[reg] : 0.f;
            sd[col * POL_P + 32 + 2 * reg + h] = c1[reg] > 0.f ? f1[reg] : 0.f;
        }
    }
    pl_wave_fence();
    __builtin_amdgcn_sched_barrier(0);
    // ---- gb1, gW1 += Xt delta1
#pragma unroll 8
    for (int r = 0; r < 32; ++r) gb1 += sd[r * POL_P + lane];
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
        const float b0 = sd[(2 * s + h) * POL_P + col], b1 = sd[(2 * s + h) * POL_P + 32 + col];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float x = sx[(2 * s + h) * S + 32 * f + col];
            g1[f][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, b0, g1[f][0], 0, 0, 0);
            g1[f][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, b1, g1[f][1], 0, 0, 0);
        }
    }
    pl_wave_fence();
    __builtin_amdgcn_sched_barrier(0);
    // ---- gb2, gW2 += a1t delta2: a1 over the features' image
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        sx[col * POL_P + 2 * reg + h] = fmaxf(c0[reg], 0.f);
        sx[col * POL_P + 32 + 2 * reg + h] = fmaxf(c1[reg], 0.f);
        sd[col * POL_P + 2 * reg + h] = e0[reg];
        sd[col * POL_P + 32 + 2 * reg + h] = e1[reg];
    }
    pl_wave_fence();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) gb2 += sd[r * POL_P + lane];
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
        const int at = (2 * s + h) * POL_P + col;
        const float x0 = sx[at], x1 = sx[at + 32], b0 = sd[at], b1 = sd[at + 32];
        g2[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, b0, g2[0][0], 0, 0, 0);
        g2[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, b1, g2[0][1], 0, 0, 0);
        g2[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, b0, g2[1][0], 0, 0, 0);
        g2[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, b1, g2[1][1], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// ---- k_policy_backward's wavefront sum, word for word: ((w0 + w1) + w2) + w3, each element by the lane that owns it; the tiles into
// red (tile k's register reg of lane l at (k * 16 + reg) * 64 + l), the bias sums into redb.  The caller's barrier follows.
template <int NF>
__device__ __forceinline__ void bcf_sum_waves(float* red, float* redb, int wave, int lane, const pl_f32x16 (&g1)[NF][2], const pl_f32x16 (&g2)[2][2],
                                              const pl_f32x16 (&g3)[2], float gb1, float gb2, float gb3) {
    for (int w = 0; w < PL_WAVES; ++w) {
        __syncthreads();
        if (wave != w) continue;
        auto put = [&](int k, const pl_f32x16& v) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                float* const p = red + (k * 16 + reg) * 64 + lane;
                *p = w == 0 ? v[reg] : *p + v[reg];
            }
        };
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            put(2 * f, g1[f][0]);
            put(2 * f + 1, g1[f][1]);
        }
        put(2 * NF, g2[0][0]);
        put(2 * NF + 1, g2[0][1]);
        put(2 * NF + 2, g2[1][0]);
        put(2 * NF + 3, g2[1][1]);
        put(2 * NF + 4, g3[0]);
        put(2 * NF + 5, g3[1]);
        redb[lane] = w == 0 ? gb1 : redb[lane] + gb1;
        redb[64 + lane] = w == 0 ? gb2 : redb[64 + lane] + gb2;
        redb[128 + lane] = w == 0 ? gb3 : redb[128 + lane] + gb3;
    }
}

// ---- element i of the gradient (pol_layout's flat order) from the reduction image: what k_policy_backward writes to its partial
template <int NF>
__device__ __forceinline__ float bcf_partial_element(const float* red, const float* redb, const PolicyLayout& o, int h1, int h2, int i) {
    if (i < o.b1) {  // gW1[f][u]: tile (f >> 5, u >> 5)
        const int f = i / h1, u = i - f * h1;
        return red[pol_slot(2 * (f >> 5) + (u >> 5), f & 31, u & 31)];
    } else if (i < o.w2) {
        return redb[i - o.b1];
    } else if (i < o.b2) {  // gW2[u][j]
        const int u = (i - o.w2) / h2, j = (i - o.w2) - u * h2;
        return red[pol_slot(2 * NF + 2 * (u >> 5) + (j >> 5), u & 31, j & 31)];
    } else if (i < o.wp) {
        return redb[64 + i - o.b2];
    } else if (i < o.bp) {  // gWp[u][j]
        const int u = (i - o.wp) / OC_NUM_ACTIONS, j = (i - o.wp) - u * OC_NUM_ACTIONS;
        return red[pol_slot(2 * NF + 4 + (u >> 5), u & 31, j)];
    } else if (i < o.wv) {
        return redb[128 + i - o.bp];
    } else if (i < o.bv) {  // gwv[u]: column 6
        const int u = i - o.wv;
        return red[pol_slot(2 * NF + 4 + (u >> 5), u & 31, OC_NUM_ACTIONS)];
    }
    return redb[128 + OC_NUM_ACTIONS];
}

// ---- k_bc_loss's arithmetic of one row, word for word: its softmax p, the class weight c of its action, its loss c * ce and whether
// its action is the argmax
__device__ __forceinline__ void bcf_row(const float (&l)[6], uint32_t act, const float (&cw)[6], float (&p)[6], float& c, float& loss, bool& correct) {
#pragma clang fp contract(off)
    float lp[6];
    ppo_softmax(l, lp, p);
    float m = l[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) m = l[i] > m ? l[i] : m;
    uint32_t best = 6u;  // the lowest i with l_i == m (none where the row holds a NaN)
#pragma unroll
    for (int i = 5; i >= 0; --i) best = l[i] == m ? (uint32_t)i : best;
    float lpa = lp[0];
    c = cw[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) {
        lpa = act == (uint32_t)i ? lp[i] : lpa;
        c = act == (uint32_t)i ? cw[i] : c;
    }
    const float ce = -lpa;
    loss = c * ce;
    correct = act == best;
}

// the row's gradients with respect to its logits, +0.0f for a row that is left out
__device__ __forceinline__ void bcf_row_grads(const float (&p)[6], uint32_t act, float c, bool left_out, float (&gl)[6]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float gi = c * (p[i] - (act == (uint32_t)i ? 1.f : 0.f));
        gl[i] = left_out ? 0.f : gi;  // a select: a NaN of a left-out row reaches nothing
    }
}

// ---- k_bc_loss's four f64 sums of the workgroup's lanes: the 64 lanes of a wavefront in the shuffle tree 32 .. 1, then the wavefronts in
// ascending order; red: [4][BLOCK / 64] f64 of LDS; the sum of term k is lane k's, k < 4
__device__ __forceinline__ double bcf_sum_lanes(const double (&acc)[4], double (*red)[BLOCK / 64], int tid) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double x = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((tid & 63) == 0) red[k][tid >> 6] = x;
    }
    __syncthreads();
    double sum = 0.0;
    if (tid < 4) {
        sum = red[tid][0];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) sum += red[tid][w];
    }
    return sum;
}

// ---- k_bc_loss_stats's eight stats of the four sums {count, sum c * ce, number correct, sum c}
__device__ __forceinline__ void bcf_stats_of(const double* sums, double (&out)[8]) {
#pragma clang fp contract(off)
    const double n = sums[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    if (n > 0.0) {
        out[0] = n;
        out[1] = sums[1] / n;
        out[2] = sums[2] / n;
        out[3] = sums[3] / n;
        out[7] = 1.0 / n;
    }
}

template <int NF>
__global__ __launch_bounds__(BLOCK) void k_bc_epoch_fused(BcFusedArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float pol_lds[];  // (the policy kernels' declaration; this kernel has no static LDS, so the f64 words in front are aligned)
    double* const red64 = reinterpret_cast<double*>(pol_lds);                                       // [ADAM_LANES]: Adam's tree
    double(*const hred)[BLOCK / 64] = reinterpret_cast<double(*)[BLOCK / 64]>(red64 + ADAM_LANES);  // [4][4]: the head's wavefront sums
    double* const hsum = red64 + ADAM_LANES + 4 * (BLOCK / 64);                                     // [4]: the head's sums; [4]: the gradient scale
    float* const sw1 = reinterpret_cast<float*>(red64 + BCF_F64);
    float* const sw2 = sw1 + pl_w1_floats(a.in_dim);
    float* const sw2t = sw2 + PL_W2;
    float* const swpt = sw2t + PL_W2;
    float* const sb1 = swpt + POL_WPT;
    float* const sb2 = sb1 + PL_HID;
    float* const images = sb2 + PL_HID;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, per_wave = bcf_wave_floats(a.in_dim);
    float* const sx = images + wave * per_wave;           // x, then a1
    float* const sd = sx + pol_image_floats(a.in_dim);    // a2, then delta1, then delta2
    float* const sg = sd + POL_BUF;                       // the logits, then delta3
    float* const sw3 = images + PL_WAVES * per_wave;
    float* const sb3 = sw3 + PL_W3;
    constexpr int NT = 2 * NF + 6;
    float* const red = sw1;              // the wavefronts' sum, over the weights
    float* const redb = red + NT * 1024;
    float* const gimg = images;          // Adam's scaled gradients, over the row images

    PolicyArgs pa = {};
    pa.w1 = a.p[0]; pa.b1 = a.p[1]; pa.w2 = a.p[2]; pa.b2 = a.p[3]; pa.wp = a.p[4]; pa.bp = a.p[5]; pa.wv = a.p[6]; pa.bv = a.p[7];
    pa.in_dim = a.in_dim; pa.h1 = a.h1; pa.h2 = a.h2;
    pa.features = a.features; pa.n_feature_rows = a.n_feature_rows;
    const PolicyLayout o = pol_layout(a.in_dim, a.h1, a.h2);
    const int col = lane & 31, h = lane >> 5, S = a.in_dim + 2;
    const pl_f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    float cw[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};  // (uniform, never written: read once)
    if (a.class_weights) {
#pragma unroll
        for (int i = 0; i < 6; ++i) cw[i] = a.class_weights[i];
    }
    // the clock lives in registers from here on: every lane keeps the same four numbers, lane 0 stores them
    double steps = a.clock[0], p1 = a.clock[1], p2 = a.clock[2], skipped = a.clock[3];

    for (int k = 0; k < a.count; ++k) {
        const int64_t lo = (int64_t)k * a.minibatch;
        const int m = (int)(a.n - lo < a.minibatch ? a.n - lo : a.minibatch);
        pa.index = a.index + lo;
        pa.n = m;
        // ---- the operands, from the weights the minibatch before left: its stores are visible behind this barrier (see the top)
        __syncthreads();
        BCF_STAMP(0);
        pol_stage_dealt(sw1, pa.w1, pa.in_dim, pa.h1, pa.in_dim / 2);
        pol_stage_dealt(sw2, pa.w2, pa.h1, pa.h2, bcf_opaque(PL_STEPS));
        pol_stage_w2_back(sw2t, bcf_opaque(PL_W2), pa);
        pol_stage_head_back(swpt, bcf_opaque(POL_WPT), pa);
        pol_stage_head_forward(sw3, bcf_opaque(PL_W3), pa);
        pol_stage_biases(sb1, sb2, pa.b1, pa.b2, pa.h1, pa.h2);
        pol_stage_head_bias(sb3, pa);
        __syncthreads();
        BCF_STAMP(1);

        // ---- forward: wavefront `wave` owns tile `wave`
        const bool has = 32 * wave < m;  // (uniform in the wavefront)
        pl_f32x16 c0 = zero16, c1 = zero16, d0 = zero16, d1 = zero16;
        int rel = -1;
        if (has) {
            int64_t base;
            rel = pol_source(pa, 32 * wave, col, base);
            pl_wave_fence();
            pol_load_rows(sx, pa.features, base, rel, pa.in_dim, lane);
            pl_wave_fence();
            __builtin_amdgcn_sched_barrier(0);
            pol_hidden<true>(sw1, sw2, sb1, sb2, sx, pa.in_dim, lane, c0, c1, d0, d1);
            __builtin_amdgcn_sched_barrier(0);
            pl_f32x16 out;  // (pol_head of mlp_tile.hpp, word for word: called here it splits two ds_read2_b32 of the bias reads, + 2 ds_)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) out[reg] = sb3[(reg & 3) + 8 * (reg >> 2) + 4 * h];
#pragma unroll
            for (int s = 0; s < PL_STEPS; ++s) {
                const float b = fmaxf(s < 16 ? d0[s & 15] : d1[s & 15], 0.f);
                out = __builtin_amdgcn_mfma_f32_32x32x2f32(sw3[s * 64 + lane], b, out, 0, 0, 0);
            }
            // rows 0..3 sit in registers 0..3 of lane half 0, rows 4..6 in registers 0..2 of half 1: the row's logits, as
            // k_policy_forward stores them, into the [row][8] image
            const bool ok = rel >= 0;
            if (h == 0) *reinterpret_cast<float4*>(sg + col * 8) = ok ? make_float4(out[0], out[1], out[2], out[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            else *reinterpret_cast<float2*>(sg + col * 8 + 4) = ok ? make_float2(out[0], out[1]) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        BCF_STAMP(2);

        // ---- the head: lane tid takes minibatch row tid
        {
            const bool live = tid < m;
            const int32_t ix = live ? pa.index[tid] : -1;
            const bool in = ix >= 0 && (int64_t)ix < a.n_samples;
            uint32_t act = 255u;
            if (in) act = a.actions[ix];
            float* const lrow = images + (tid >> 5) * per_wave + pol_image_floats(a.in_dim) + POL_BUF + (tid & 31) * 8;  // (inside the images where live)
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f);
            float2 x1 = make_float2(0.f, 0.f);
            if (live) x0 = *reinterpret_cast<const float4*>(lrow), x1 = *reinterpret_cast<const float2*>(lrow + 4);
            const bool left_out = !in || act > 5u;
            const float l[6] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y};
            float p[6], c, loss;
            bool correct;
            bcf_row(l, act, cw, p, c, loss, correct);
            if (live) {  // delta3 of the row: the six gradients, +0.0f for the value
                float gl[6];
                bcf_row_grads(p, act, c, left_out, gl);
                reinterpret_cast<float4*>(lrow)[0] = make_float4(gl[0], gl[1], gl[2], gl[3]);
                reinterpret_cast<float4*>(lrow)[1] = make_float4(gl[4], gl[5], 0.f, 0.f);
            }
            const double x[4] = {1.0, (double)loss, correct ? 1.0 : 0.0, (double)c};  // each term widened first
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] += left_out ? 0.0 : x[t];
            const double part = bcf_sum_lanes(acc, hred, tid);
            if (tid < 4) {  // k_bc_loss_stats's chain over the one partial: from +0.0
                double sum = 0.0;
                sum += part;
                hsum[tid] = sum;
            }
            __syncthreads();
            if (tid == 0) {
                double st[8];
                bcf_stats_of(hsum, st);
#pragma unroll
                for (int i = 0; i < 8; ++i) a.stats[(size_t)k * 8 + i] = st[i];
                hsum[4] = st[7];
            }
        }
        BCF_STAMP(3);

        // ---- backward: k_policy_backward's tile on the registers the forward pass left
        pl_f32x16 g1[NF][2], g2[2][2], g3[2];
#pragma unroll
        for (int f = 0; f < NF; ++f) g1[f][0] = g1[f][1] = zero16;
        g2[0][0] = g2[0][1] = g2[1][0] = g2[1][1] = g3[0] = g3[1] = zero16;
        float gb1 = 0.f, gb2 = 0.f, gb3 = 0.f;  // lane = unit (gb3: lane = output)
        if (has) {
            float2 u0 = make_float2(0.f, 0.f), u1 = u0, u2 = u0;
            float uv = 0.f;
            if (rel >= 0) {  // (zeros for a row without a source)
                const float4 lo4 = *reinterpret_cast<const float4*>(sg + col * 8), hi4 = *reinterpret_cast<const float4*>(sg + col * 8 + 4);
                u0 = make_float2(lo4.x, lo4.y), u1 = make_float2(lo4.z, lo4.w), u2 = make_float2(hi4.x, hi4.y);
                uv = hi4.z;
            }
            const bool any = u0.x != 0.f || u0.y != 0.f || u1.x != 0.f || u1.y != 0.f || u2.x != 0.f || u2.y != 0.f || uv != 0.f;
            if (__ballot(any) != 0) {  // (32 rows of zeros: nothing to add)
                pl_wave_fence();  // (every lane has read its delta3 before the image is written again)
                __builtin_amdgcn_sched_barrier(0);
                bcf_tile_back<NF>(swpt, sw2t, sx, sd, sg, S, lane, u0, u1, u2, uv, c0, c1, d0, d1, g1, g2, g3, gb1, gb2, gb3);
            }
        }
        bcf_sum_waves<NF>(red, redb, wave, lane, g1, g2, g3, gb1, gb2, gb3);
        __syncthreads();
        BCF_STAMP(4);

        // ---- k_adam_step's pass 1: the scaled gradients into LDS, their squares into the lane's sum in ascending i
        const double gs64 = hsum[4];
        const float gs = (float)gs64;
        double sq = 0.0;
        for (int i = tid; i < o.size; i += ADAM_LANES) {
            const float gi = bcf_partial_element<NF>(red, redb, o, a.h1, a.h2, i) * gs;
            gimg[i] = gi;
            sq += (double)gi * (double)gi;
        }
        red64[tid] = sq;
        __syncthreads();
#pragma unroll
        for (int t = ADAM_LANES / 2; t > 0; t >>= 1) {
            if (tid < t) red64[tid] += red64[tid + t];
            __syncthreads();
        }
        const float norm = (float)sqrt(red64[0]);
        const bool finite = norm - norm == 0.f;  // neither NaN nor an infinity
        const bool skip = !finite || gs64 == 0.0;
        const AdamStep st = adam_step_of(norm, p1, p2, a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm);
        double* const info = a.info + (size_t)k * 4;
        if (skip) {  // nothing is written to parameters or moments; steps and the powers stay
            skipped = skipped + 1.0;
            if (tid == 0) {
                a.clock[3] = skipped;
                info[0] = (double)norm, info[1] = 0.0, info[2] = (double)gs, info[3] = 1.0;
            }
        } else {
            // ---- pass 2: the update, the arrays one after the other with their pointers in scalar registers
            adam_arrays([&](auto KK) {
                constexpr int kk = decltype(KK)::value;
                const int s = bcf_opaque(a.start[kk]), len = a.start[kk + 1] - s;
                float* const P = a.p[kk];
                float* const M = a.m[kk];
                float* const V = a.v[kk];
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
                            adam_element(gimg[s + at], mi[j], vi[j], pi[j], st, mn, vn, pn);
                            M[at] = mn;
                            V[at] = vn;
                            P[at] = pn;
                        }
                    }
                }
            });
            steps = steps + 1.0, p1 = st.p1n, p2 = st.p2n;
            if (tid == 0) {
                a.clock[0] = steps, a.clock[1] = p1, a.clock[2] = p2;
                info[0] = (double)norm, info[1] = (double)st.c, info[2] = (double)gs, info[3] = 0.0;
            }
        }
        BCF_STAMP(5);
    }
}

const char* const BCF_WHO = "oc_bc_epoch_fused";

// the checks that need no array (oc_bc_epoch_fused_plan makes these alone)
int bcf_check_shape(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2) {
    const char* const who = BCF_WHO;
    if (int rc = upd_check_index(who, n_index)) return rc;  // (update_chain.hpp)
    if (minibatch < 1 || minibatch > BCF_ROWS)
        return pol_refuse(who, "minibatch must be in 1..128: a 32-row tile for each of the workgroup's four wavefronts (oc_bc_update serves every size)");
    if (in_dim != 56 && in_dim != 76 && in_dim != 96)
        return pol_refuse(who, "policy.in_dim must be 56, 76 or 96: two or three feature tiles (oc_bc_update serves 116 and 136 too)");
    if (h1 < 1 || h1 > PL_HID || h2 < 1 || h2 > PL_HID) return pol_refuse(who, "policy.h1 and policy.h2 must be in 1..64");
    return OC_OK;
}

int64_t bcf_launches(int64_t K) { return (K + BCF_PER_LAUNCH - 1) / BCF_PER_LAUNCH; }

template <int NF>
void bcf_launch(const BcFusedArgs& a, size_t smem, hipStream_t stream) {
    if (want_lds(k_bc_epoch_fused<NF>, smem)) hipLaunchKernelGGL((k_bc_epoch_fused<NF>), dim3(1), dim3(BLOCK), smem, stream, a);
}

}  // namespace

extern "C" {

int oc_bc_epoch_fused(const OcActorCritic* pol, const OcBcLoss* loss, const OcAdam* adam, const OcBcEpochFused* e, void* stream) {
    const char* const who = BCF_WHO;
    if (!pol) return pol_refuse(who, "policy is NULL");
    if (!loss) return pol_refuse(who, "loss is NULL");
    if (!adam) return pol_refuse(who, "adam is NULL");
    if (!e) return pol_refuse(who, "epoch is NULL");
    if (int rc = bcf_check_shape(e->n_index, e->minibatch, pol->in_dim, pol->h1, pol->h2)) return rc;
    if (!e->d_index) return pol_refuse(who, "epoch.d_index is NULL");
    if (!e->d_stats || !e->d_info) return pol_refuse(who, "NULL epoch.d_stats or epoch.d_info");
    if (((uintptr_t)e->d_stats | (uintptr_t)e->d_info) & 7u) return pol_refuse(who, "epoch.d_stats and epoch.d_info must be 8-byte aligned");
    // the weights, the feature rows and the index: oc_policy_forward's checks of the longest minibatch (the others differ in an
    // offset that keeps the alignment)
    OcPolicyRows rows = {};
    rows.d_features = e->d_features; rows.n_feature_rows = e->n_feature_rows; rows.d_index = e->d_index;
    rows.n_rows = e->n_index < e->minibatch ? e->n_index : e->minibatch;
    if (int rc = pol_check(who, pol, &rows)) return rc;
    // the batch side of the head: oc_bc_loss's checks of what is read here
    if (!loss->d_actions) return pol_refuse(who, "loss.d_actions is NULL");
    if ((uintptr_t)loss->d_class_weights & 3u) return pol_refuse(who, "loss.d_class_weights must be 4-byte aligned");
    if (loss->n_samples < 0) return pol_refuse(who, "n_samples < 0");
    if (loss->n_samples >= ((int64_t)1 << 31)) return pol_refuse(who, "n_samples must be below 2^31 with d_index");
    if (int rc = adam_check_state(who, adam)) return rc;
    const PolicyLayout o = pol_layout(pol->in_dim, pol->h1, pol->h2);
    const size_t smem = bcf_lds(pol->in_dim);
    const int nf = pol_nf(pol->in_dim);
    if (smem > BCF_LDS_MAX || (size_t)(2 * nf + 6) * 1024 + 192 > (size_t)bcf_weight_floats(pol->in_dim) || o.size > PL_WAVES * bcf_wave_floats(pol->in_dim))
        return fail(OC_EINVAL, "oc_bc_epoch_fused: the LDS layout does not hold this shape");  // (no served shape comes here)

    BcFusedArgs a = {};
    const float* const p[8] = {pol->d_w1, pol->d_b1, pol->d_w2, pol->d_b2, pol->d_wp, pol->d_bp, pol->d_wv, pol->d_bv};
    for (int k = 0; k < 8; ++k) {
        a.p[k] = const_cast<float*>(p[k]);  // (written through: the header says so)
        a.m[k] = adam->d_m[k];
        a.v[k] = adam->d_v[k];
    }
    const int start[9] = {o.w1, o.b1, o.w2, o.b2, o.wp, o.bp, o.wv, o.bv, o.size};
    for (int k = 0; k < 9; ++k) a.start[k] = start[k];
    a.in_dim = pol->in_dim; a.h1 = pol->h1; a.h2 = pol->h2;
    a.features = e->d_features; a.n_feature_rows = e->n_feature_rows;
    a.minibatch = (int)e->minibatch;
    a.actions = loss->d_actions; a.class_weights = loss->d_class_weights; a.n_samples = loss->n_samples;
    a.clock = adam->d_clock;
    a.lr = adam->lr; a.beta1 = adam->beta1; a.beta2 = adam->beta2; a.eps = adam->eps; a.max_grad_norm = adam->max_grad_norm;
    const int64_t K = upd_count(e->n_index, e->minibatch);
    for (int64_t k0 = 0; k0 < K; k0 += BCF_PER_LAUNCH) {
        const int64_t lo = k0 * e->minibatch, rest = e->n_index - lo, most = (int64_t)BCF_PER_LAUNCH * e->minibatch;
        a.index = e->d_index + lo;
        a.n = rest < most ? rest : most;
        a.count = (int)(K - k0 < BCF_PER_LAUNCH ? K - k0 : BCF_PER_LAUNCH);
        a.stats = e->d_stats + 8 * k0;
        a.info = e->d_info + 4 * k0;
#ifdef OC_AMD_TUNING
        a.stamps = g_bcf_stamps ? g_bcf_stamps + BCF_STAMPS * k0 : nullptr;
#endif
        if (nf == 2) bcf_launch<2>(a, smem, (hipStream_t)stream);
        else bcf_launch<3>(a, smem, (hipStream_t)stream);
        if (int rc = check_launch(who)) return rc;
    }
    return OC_OK;
}

int oc_bc_epoch_fused_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_class_weights, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_bc_epoch_fused_plan: no output buffer");
    out[0] = 0;
    if (int rc = bcf_check_shape(n_index, minibatch, in_dim, h1, h2)) return rc;
    const auto [K, m, last] = upd_split(n_index, minibatch);  // (update_chain.hpp)
    if (K == 0) {
        snprintf(out, out_size, "nothing to launch (no index); no scratch; out: stats 0 x 8 f64, info 0 x 4 f64");
        return OC_OK;
    }
    const int nf = pol_nf(in_dim);
    snprintf(out, out_size, "k_bc_epoch_fused<NF=%d> grid=1, %d lanes (%d wavefronts x one 32-row tile), %lld minibatch(es) of %lld rows (the last %lld), "
             "at most %d minibatches per launch: %lld launch(es), no host synchronisation, 32 x 32 x 2 f32 MFMA, %d accumulator tiles per wavefront, "
             "%d elements (%d per lane) in Adam's phases, class_weights=%s, %zu B LDS; no scratch; out: stats %lld x 8 f64, info %lld x 4 f64",
             nf, BLOCK, PL_WAVES, (long long)K, (long long)m, (long long)last, BCF_PER_LAUNCH, (long long)bcf_launches(K), 2 * nf + 6,
             pol_layout(in_dim, h1, h2).size, (pol_layout(in_dim, h1, h2).size + ADAM_LANES - 1) / ADAM_LANES, with_class_weights ? "yes" : "no",
             bcf_lds(in_dim), (long long)K, (long long)K);
    return OC_OK;
}

#ifdef OC_AMD_TUNING
// measurement builds only: where lane 0 leaves BCF_STAMPS cycle counts per minibatch of the calls that follow (NULL: nowhere)
void oc_bc_epoch_fused_stamps(unsigned long long* d_stamps) { g_bcf_stamps = d_stamps; }
#endif

}  // extern "C"
