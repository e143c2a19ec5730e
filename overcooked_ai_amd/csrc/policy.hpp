// policy.hpp — the learner's actor-critic on featurize_state rows, forward and backward to the weights: k_policy_forward,
// k_policy_backward, k_policy_grad_sum, oc_policy_forward, oc_policy_backward, oc_policy_plan
// (include/oc_amd.h: OcActorCritic, OcPolicyRows, OcPolicyGrads)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind mlp_tile.hpp (the MFMA tile of the
// dense network: scheme, stager, pol_hidden, pol_head); after common.hpp (BLOCK) and host_util.hpp (fail, check_launch, want_lds).
//
// Both kernels run a persistent grid of at most POL_GRID workgroups.  A wavefront takes 32-row tiles
//   tile = (pass * gridDim.x + blockIdx.x) * wavefronts + wavefront,   pass = 0, 1, ...
// and computes them as mlp_tile.hpp says, a tile's 32 columns the rows of the call.  Rows may be gathered through an index; a row
// that is out of range is a row of zeros in the image (nothing is read for it) and its outputs are +0.0f.  The last layer's tile
// carries the value head as its seventh row.
//
// k_policy_backward recomputes layers 1 and 2 of a tile (the logits themselves are not needed), then
//   delta3 = the seven upstream gradients of the row (zeros for a row out of range),
//   delta2 = [pre2 > 0] (Wp|wv) delta3         4 K steps (7 outputs padded to 8) x 2 unit tiles, A = (Wp|wv) staged [unit][output]
//   delta1 = [pre1 > 0] W2 delta2              32 K steps x 2 unit tiles, A = W2 staged [unit of layer 1][unit of layer 2];
//                                              delta2 is B straight from the registers, as the activations are going forward
//   gW1 += Xt delta1, gW2 += a1t delta2, gWp|gwv += a2t delta3
// In the three weight products K is the ROW of the call, which the registers hold on the lane: both operands are turned through
// LDS as [row][unit] images (stride 65; the features' own image is the A operand of gW1) and read lane = unit, k = row pair.  The
// order keeps few registers alive beside the accumulators: a2 and delta3 first (the pre-activations of layer 2 die there), then
// delta1 against x, then a1 — over the features' image — against delta2; the second image holds a2, delta1, delta2 in turn.  The
// bias gradients are column sums of the delta images: lane = unit, rows in ascending order.
// A wavefront keeps all 2 NF + 6 accumulator tiles (NF = ceil(in_dim / 32) feature tiles; 12 tiles = 192 registers at 96 inputs;
// with 116 and 136 inputs the rows 96.. of gW1 are left to a second launch, which repeats the way there for 2 or 4 tiles more)
// across its tiles: a workgroup is one wavefront per SIMD, which on gfx950's unified file may hold 512 registers (the alternative,
// dealing the twelve tiles to the four wavefronts of ONE row tile, makes every wavefront repeat or wait for the tile's forward
// pass; docs/NOTEBOOK.md).  A tile whose 32 upstream rows are all zero is skipped before its features are read (the partner's
// samples after oc_ppo_loss): it would add +-0 to accumulators that are never -0.
// At the end the wavefronts add their accumulators in ascending order through LDS — ((w0 + w1) + w2) + w3, each element by the
// lane that owns it — and the workgroup writes ONE partial in the layout of the eight gradient arrays, one behind the other.
// k_policy_grad_sum then adds the partials in ascending workgroup order, one lane per element.  No atomics anywhere.
#pragma once

namespace {

constexpr int POL_GRID = 256;          // workgroups of the persistent grid, at most (one per CU of an MI355X)
constexpr int POL_P = PL_HID + 1;      // row stride of the [row][unit] images of the weight products
constexpr int POL_BUF = 32 * POL_P;    // floats of such an image
constexpr int POL_D3 = 32 * 8;         // floats of the [row][8] image of delta3
constexpr int POL_WPT = 4 * 2 * 64;    // (Wp|wv) transposed: 4 K steps x 2 unit tiles x 64 lanes
constexpr size_t POL_LDS_MAX = 160 * 1024;
constexpr int POL_OUT = OC_NUM_ACTIONS + 1;  // six logits and the value

struct PolicyArgs {
    const float *w1, *b1, *w2, *b2, *wp, *bp, *wv, *bv;  // Keras layout, [in][out]
    int in_dim, h1, h2;
    const float* features;  // [n_feature_rows][in_dim]
    int64_t n_feature_rows;
    const int32_t* index;   // [n] or NULL
    int64_t first, n;
    float* logits;          // forward: [n][6]
    float* values;          // forward: [n]
    const float* grad_logits;  // backward: [n][6]
    const float* grad_values;  // backward: [n]
    float* partials;           // backward: [gridDim.x][size]
    int size;                  // floats of a partial
};

__host__ __device__ constexpr int pol_nf(int in_dim) { return (in_dim + 31) / 32; }
// floats of a wavefront's image in the backward kernel: the feature rows, read 32 NF columns wide from every row, or a [row][unit] image
__host__ __device__ constexpr int pol_image_floats(int in_dim) {
    int need = 31 * (in_dim + 2) + 32 * pol_nf(in_dim);
    need = need < 32 * (in_dim + 2) ? 32 * (in_dim + 2) : need;
    need = need < POL_BUF ? POL_BUF : need;
    return (need + 3) & ~3;
}
__host__ __device__ constexpr size_t pol_forward_lds(int in_dim) {
    return sizeof(float) * (size_t)(pl_w1_floats(in_dim) + PL_W2 + PL_W3 + PL_BIAS + PL_WAVES * pl_image_floats(in_dim));
}
__host__ __device__ constexpr size_t pol_backward_lds(int in_dim, int waves) {
    return sizeof(float) * (size_t)(pl_w1_floats(in_dim) + 2 * PL_W2 + POL_WPT + 2 * PL_HID + waves * (pol_image_floats(in_dim) + POL_BUF + POL_D3));
}
// wavefronts of a backward workgroup: four where the LDS holds their images (up to 116 inputs: 163 008 of 163 840 bytes), else three (136 inputs)
__host__ __device__ constexpr int pol_backward_waves(int in_dim) { return pol_backward_lds(in_dim, PL_WAVES) <= POL_LDS_MAX ? PL_WAVES : PL_WAVES - 1; }

struct PolicyLayout {  // offsets (floats) of the eight gradient arrays inside a partial
    int w1, b1, w2, b2, wp, bp, wv, bv, size;
};
__host__ __device__ inline PolicyLayout pol_layout(int in_dim, int h1, int h2) {
    PolicyLayout o;
    o.w1 = 0;
    o.b1 = in_dim * h1;
    o.w2 = o.b1 + h1;
    o.b2 = o.w2 + h1 * h2;
    o.wp = o.b2 + h2;
    o.bp = o.wp + h2 * OC_NUM_ACTIONS;
    o.wv = o.bp + OC_NUM_ACTIONS;
    o.bv = o.wv + h2;
    o.size = o.bv + 1;
    return o;
}

// ---- the operands that are the learner's own, each by the whole workgroup (pol_stage, mlp_tile.hpp); total: the floats of dst, which a
// caller may hide from the optimiser (bc_fused.hpp: bcf_opaque).  The two for the way back serve k_bc_epoch_fused; k_policy_backward
// keeps them as lambdas of its own (see there).

// W2 for the way back: A[unit i of layer 1, dealt][k = unit j of layer 2]
__device__ __forceinline__ void pol_stage_w2_back(float* dst, int total, const PolicyArgs& a) {
    pol_stage(dst, total, a.w1, [=](int i) -> const float* {
        const int ln = i & 63, tile = (i >> 6) & 1, s = i >> 7;
        const int u = 32 * tile + pl_unit_of_row(ln & 31), j = 2 * s + (ln >> 5);
        return u < a.h1 && j < a.h2 ? a.w2 + u * a.h2 + j : nullptr;
    });
}

// (Wp|wv) for the way back: A[unit of layer 2, dealt][k = output j], 7 outputs padded to 8
__device__ __forceinline__ void pol_stage_head_back(float* dst, int total, const PolicyArgs& a) {
    pol_stage(dst, total, a.w1, [=](int i) -> const float* {
        const int ln = i & 63, tile = (i >> 6) & 1, s = i >> 7;
        const int u = 32 * tile + pl_unit_of_row(ln & 31), j = 2 * s + (ln >> 5);
        if (u >= a.h2 || j >= POL_OUT) return nullptr;
        return j < OC_NUM_ACTIONS ? a.wp + u * OC_NUM_ACTIONS + j : a.wv + u;
    });
}

// (Wp|wv) going forward, the last layer, rows in their natural order: six logits and the value
__device__ __forceinline__ void pol_stage_head_forward(float* dst, int total, const PolicyArgs& a) {
    pol_stage(dst, total, a.w1, [=](int i) -> const float* {
        const int ln = i & 63, k = 2 * (i >> 6) + (ln >> 5), r = ln & 31;
        if (k >= a.h2 || r >= POL_OUT) return nullptr;
        return r < OC_NUM_ACTIONS ? a.wp + k * OC_NUM_ACTIONS + r : a.wv + k;
    });
}

// its bias: bp, bv, zeros
__device__ __forceinline__ void pol_stage_head_bias(float* sb3, const PolicyArgs& a) {
    if (threadIdx.x < 32) sb3[threadIdx.x] = threadIdx.x < OC_NUM_ACTIONS ? a.bp[threadIdx.x] : threadIdx.x == OC_NUM_ACTIONS ? a.bv[0] : 0.f;
}

// which feature row column `col` of tile `row0` reads, relative to `base`: -1 for a row beyond the call or out of range
__device__ __forceinline__ int pol_source(const PolicyArgs& a, int64_t row0, int col, int64_t& base) {
    const bool live = row0 + col < a.n;
    if (a.index) {
        base = 0;
        const int32_t ix = live ? a.index[row0 + col] : -1;
        return ix >= 0 && (int64_t)ix < a.n_feature_rows ? ix : -1;
    }
    base = a.first + row0;
    return live ? col : -1;
}

// the tile's 32 feature rows -> the wavefront's image, rows in_dim + 2 apart; a row without a source is zeros
__device__ __forceinline__ void pol_load_rows(float* sx, const float* __restrict__ features, int64_t base, int rel, int in_dim, int lane) {
    const int S = in_dim + 2, q = in_dim / 4;
    for (int i0 = lane; i0 < 32 * q; i0 += 4 * 64) {  // four 16-byte loads in flight per lane
        float4 v[4];
        int at[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * 64;
            const bool in = i < 32 * q;
            const int r = in ? i / q : 0, c = in ? i - r * q : 0;
            const int rr = __shfl(rel, r, 64);
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in && rr >= 0) v[j] = *reinterpret_cast<const float4*>(features + (base + rr) * in_dim + 4 * c);
            at[j] = in ? r * S + 4 * c : -1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (at[j] >= 0) {
                float2* const dst = reinterpret_cast<float2*>(sx + at[j]);
                dst[0] = make_float2(v[j].x, v[j].y);
                dst[1] = make_float2(v[j].z, v[j].w);
            }
    }
}

__global__ __launch_bounds__(BLOCK) void k_policy_forward(PolicyArgs a) {
    extern __shared__ float pol_lds[];
    const PlOperands w = pl_operands(pol_lds, a.in_dim);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const sx = w.end + wave * pl_image_floats(a.in_dim);

    pol_stage_dealt(w.sw1, a.w1, a.in_dim, a.h1, a.in_dim / 2);
    pol_stage_dealt(w.sw2, a.w2, a.h1, a.h2, PL_STEPS);
    pol_stage_head_forward(w.sw3, PL_W3, a);
    pol_stage_biases(w.sb1, w.sb2, a.b1, a.b2, a.h1, a.h2);
    pol_stage_head_bias(w.sb3, a);
    __syncthreads();

    const int col = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (a.n + 31) >> 5;
    for (int64_t t = (int64_t)blockIdx.x * PL_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PL_WAVES) {
        const int64_t row0 = t << 5;
        int64_t base;
        const int rel = pol_source(a, row0, col, base);
        pl_wave_fence();  // (the reads of the previous tile are done)
        pol_load_rows(sx, a.features, base, rel, a.in_dim, lane);
        pl_wave_fence();
        pl_f32x16 c0, c1, d0, d1;
        pol_hidden<false>(w.sw1, w.sw2, w.sb1, w.sb2, sx, a.in_dim, lane, c0, c1, d0, d1);
        const pl_f32x16 o = pol_head(w.sw3, w.sb3, lane, d0, d1);
        // ---- rows 0..3 sit in registers 0..3 of lane half 0, rows 4..6 in registers 0..2 of half 1
        if (row0 + col < a.n) {
            const bool ok = rel >= 0;
            float2* const out = reinterpret_cast<float2*>(a.logits + (row0 + col) * OC_NUM_ACTIONS);
            if (h == 0) {
                out[0] = ok ? make_float2(o[0], o[1]) : make_float2(0.f, 0.f);
                out[1] = ok ? make_float2(o[2], o[3]) : make_float2(0.f, 0.f);
            } else {
                out[2] = ok ? make_float2(o[0], o[1]) : make_float2(0.f, 0.f);
                a.values[row0 + col] = ok ? o[2] : 0.f;
            }
        }
    }
}

// where element (natural row m, column c) of accumulator tile k sits in the workgroup's reduction image
__device__ __forceinline__ int pol_slot(int k, int m, int c) {
    const int reg = (m & 3) + 4 * (m >> 3), hh = (m >> 2) & 1;
    return (k * 16 + reg) * 64 + hh * 32 + c;
}

// F0, NF: the feature tiles whose rows of gW1 this instance accumulates; REST: it also accumulates every other gradient.  A call
// is the instance <0, min(tiles, 3), true> and, with more than three feature tiles (116 and 136 inputs), <3, tiles - 3, false> behind
// it: 2 * 3 + 6 accumulator tiles are what a wavefront's registers hold beside the tile in flight.
template <int F0, int NF, bool REST>
__global__ __launch_bounds__(BLOCK) void k_policy_backward(PolicyArgs a) {
    extern __shared__ float pol_lds[];
    const int waves = blockDim.x >> 6;
    float* const sw1 = pol_lds;
    float* const sw2 = sw1 + pl_w1_floats(a.in_dim);
    float* const sw2t = sw2 + PL_W2;
    float* const swpt = sw2t + PL_W2;
    float* const sb1 = swpt + POL_WPT;
    float* const sb2 = sb1 + PL_HID;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const sx = sb2 + PL_HID + wave * (pol_image_floats(a.in_dim) + POL_BUF + POL_D3);  // x, then a1
    float* const sd = sx + pol_image_floats(a.in_dim);                                         // a2, then delta1, then delta2
    float* const sg = sd + POL_BUF;                                                            // delta3

    pol_stage_dealt(sw1, a.w1, a.in_dim, a.h1, a.in_dim / 2);
    pol_stage_dealt(sw2, a.w2, a.h1, a.h2, PL_STEPS);
    // (pol_stage_w2_back and pol_stage_head_back, word for word, as this kernel's own lambdas: through the functions its rows on a
    // grid of one wave of workgroups were 0.5-0.8 us of 80 slower on the device; docs/NOTEBOOK.md)
    // W2 for the way back: A[unit i of layer 1, dealt][k = unit j of layer 2]
    pol_stage(sw2t, PL_W2, a.w1, [=](int i) -> const float* {
        const int ln = i & 63, tile = (i >> 6) & 1, s = i >> 7;
        const int u = 32 * tile + pl_unit_of_row(ln & 31), j = 2 * s + (ln >> 5);
        return u < a.h1 && j < a.h2 ? a.w2 + u * a.h2 + j : nullptr;
    });
    // (Wp|wv) for the way back: A[unit of layer 2, dealt][k = output j], 7 outputs padded to 8
    pol_stage(swpt, POL_WPT, a.w1, [=](int i) -> const float* {
        const int ln = i & 63, tile = (i >> 6) & 1, s = i >> 7;
        const int u = 32 * tile + pl_unit_of_row(ln & 31), j = 2 * s + (ln >> 5);
        if (u >= a.h2 || j >= POL_OUT) return nullptr;
        return j < OC_NUM_ACTIONS ? a.wp + u * OC_NUM_ACTIONS + j : a.wv + u;
    });
    pol_stage_biases(sb1, sb2, a.b1, a.b2, a.h1, a.h2);
    __syncthreads();

    const int col = lane & 31, h = lane >> 5, S = a.in_dim + 2;
    const pl_f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    pl_f32x16 g1[NF][2], g2[2][2], g3[2];
#pragma unroll
    for (int f = 0; f < NF; ++f) g1[f][0] = g1[f][1] = zero16;
    g2[0][0] = g2[0][1] = g2[1][0] = g2[1][1] = g3[0] = g3[1] = zero16;
    float gb1 = 0.f, gb2 = 0.f, gb3 = 0.f;  // lane = unit (gb3: lane = output)

    const int64_t n_tiles = (a.n + 31) >> 5;
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < n_tiles; t += (int64_t)gridDim.x * waves) {
        const int64_t row0 = t << 5;
        int64_t base;
        const int rel = pol_source(a, row0, col, base);
        // ---- delta3: the row's seven upstream gradients; zeros for a row without a source
        float2 u0 = make_float2(0.f, 0.f), u1 = u0, u2 = u0;
        float uv = 0.f;
        if (rel >= 0) {
            const float2* const src = reinterpret_cast<const float2*>(a.grad_logits + (row0 + col) * OC_NUM_ACTIONS);
            u0 = src[0], u1 = src[1], u2 = src[2];
            uv = a.grad_values[row0 + col];
        }
        const bool any = u0.x != 0.f || u0.y != 0.f || u1.x != 0.f || u1.y != 0.f || u2.x != 0.f || u2.y != 0.f || uv != 0.f;
        if (__ballot(any) == 0) continue;  // 32 rows of zeros: nothing to add
        pl_wave_fence();  // (the reads of the previous tile are done)
        pol_load_rows(sx, a.features, base, rel, a.in_dim, lane);
        pl_wave_fence();
        pl_f32x16 c0, c1, d0, d1;
        __builtin_amdgcn_sched_barrier(0);
        pol_hidden<true>(sw1, sw2, sb1, sb2, sx, a.in_dim, lane, c0, c1, d0, d1);
        __builtin_amdgcn_sched_barrier(0);
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
        if constexpr (REST) {
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
        }
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
        for (int r = 0; r < 32; ++r) gb1 += REST ? sd[r * POL_P + lane] : 0.f;
#pragma unroll 2
        for (int s = 0; s < 16; ++s) {
            const float b0 = sd[(2 * s + h) * POL_P + col], b1 = sd[(2 * s + h) * POL_P + 32 + col];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float x = sx[(2 * s + h) * S + 32 * (F0 + f) + col];
                g1[f][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, b0, g1[f][0], 0, 0, 0);
                g1[f][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, b1, g1[f][1], 0, 0, 0);
            }
        }
        pl_wave_fence();
        __builtin_amdgcn_sched_barrier(0);
        // ---- gb2, gW2 += a1t delta2: a1 over the features' image
        if constexpr (REST) {
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
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- the wavefronts' accumulators, added in ascending order in the reduction image (over the weights, which are done with)
    constexpr int NT = 2 * NF + (REST ? 6 : 0);
    float* const red = pol_lds;
    float* const redb = red + NT * 1024;
    for (int w = 0; w < waves; ++w) {
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
        if constexpr (REST) {
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
    __syncthreads();
    // ---- the workgroup's partial, in the layout of the gradient arrays: the elements this instance owns
    const PolicyLayout o = pol_layout(a.in_dim, a.h1, a.h2);
    float* const out = a.partials + (size_t)blockIdx.x * a.size;
    const int i_first = F0 * 32 * a.h1, i_end = REST ? a.size : o.b1;
    for (int i = i_first + threadIdx.x; i < i_end; i += blockDim.x) {
        float v;
        if (i < o.b1) {  // gW1[f][u]: tile (f >> 5, u >> 5)
            const int f = i / a.h1, u = i - f * a.h1;
            if (f >= 32 * (F0 + NF)) continue;  // (the instance behind this one owns it)
            v = red[pol_slot(2 * ((f >> 5) - F0) + (u >> 5), f & 31, u & 31)];
        } else if (i < o.w2) {
            v = redb[i - o.b1];
        } else if (i < o.b2) {  // gW2[u][j]
            const int u = (i - o.w2) / a.h2, j = (i - o.w2) - u * a.h2;
            v = red[pol_slot(2 * NF + 2 * (u >> 5) + (j >> 5), u & 31, j & 31)];
        } else if (i < o.wp) {
            v = redb[64 + i - o.b2];
        } else if (i < o.bp) {  // gWp[u][j]
            const int u = (i - o.wp) / OC_NUM_ACTIONS, j = (i - o.wp) - u * OC_NUM_ACTIONS;
            v = red[pol_slot(2 * NF + 4 + (u >> 5), u & 31, j)];
        } else if (i < o.wv) {
            v = redb[128 + i - o.bp];
        } else if (i < o.bv) {  // gwv[u]: column 6
            const int u = i - o.wv;
            v = red[pol_slot(2 * NF + 4 + (u >> 5), u & 31, OC_NUM_ACTIONS)];
        } else {
            v = redb[128 + OC_NUM_ACTIONS];
        }
        out[i] = v;
    }
}

struct PolicyGradPointers {
    float* p[8];  // w1, b1, w2, b2, wp, bp, wv, bv
};

// gradient element i = partial 0's + partial 1's + ... in ascending order (no partial: +0.0f), one lane per element; eight loads in flight
__global__ __launch_bounds__(BLOCK) void k_policy_grad_sum(const float* __restrict__ partials, int count, PolicyLayout o, PolicyGradPointers g) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= o.size) return;
    float sum = 0.f;
    int p = 0;
    if (count > 0) sum = partials[i], p = 1;
    for (; p + 8 <= count; p += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = partials[(size_t)(p + j) * o.size + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[j];
    }
    for (; p < count; ++p) sum += partials[(size_t)p * o.size + i];
    const int start[9] = {o.w1, o.b1, o.w2, o.b2, o.wp, o.bp, o.wv, o.bv, o.size};
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (i >= start[k] && i < start[k + 1]) g.p[k][i - start[k]] = sum;
}

int pol_refuse(const char* who, const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail(OC_EINVAL, msg);
}

// the checks that need no array (oc_policy_plan makes these alone)
int pol_check_shape(const char* who, int64_t n_rows, int in_dim, int h1, int h2) {
    if (n_rows < 0) return pol_refuse(who, "n_rows < 0");
    if (n_rows > ((int64_t)1 << 40)) return pol_refuse(who, "n_rows above 2^40");
    if (in_dim < 56 || in_dim > 136 || (in_dim - 56) % 20) return pol_refuse(who, "policy.in_dim must be a feature length 2 * (num_pots * 10 + 26) + 4, num_pots in 0..4");
    if (h1 < 1 || h1 > PL_HID || h2 < 1 || h2 > PL_HID) return pol_refuse(who, "policy.h1 and policy.h2 must be in 1..64");
    return OC_OK;
}

int pol_check(const char* who, const OcActorCritic* pol, const OcPolicyRows* rows) {
    if (!pol) return pol_refuse(who, "policy is NULL");
    if (!rows) return pol_refuse(who, "rows is NULL");
    if (!pol->d_w1 || !pol->d_b1 || !pol->d_w2 || !pol->d_b2 || !pol->d_wp || !pol->d_bp || !pol->d_wv || !pol->d_bv)
        return pol_refuse(who, "NULL weight or bias array");
    if (((uintptr_t)pol->d_w1 | (uintptr_t)pol->d_b1 | (uintptr_t)pol->d_w2 | (uintptr_t)pol->d_b2 | (uintptr_t)pol->d_wp | (uintptr_t)pol->d_bp |
         (uintptr_t)pol->d_wv | (uintptr_t)pol->d_bv) & 3u)
        return pol_refuse(who, "weight and bias arrays must be 4-byte aligned");
    if (!rows->d_features) return pol_refuse(who, "rows.d_features is NULL");
    if ((uintptr_t)rows->d_features & 15u) return pol_refuse(who, "rows.d_features must be 16-byte aligned");
    if ((uintptr_t)rows->d_index & 3u) return pol_refuse(who, "rows.d_index must be 4-byte aligned");
    if (int rc = pol_check_shape(who, rows->n_rows, pol->in_dim, pol->h1, pol->h2)) return rc;
    if (rows->n_feature_rows < 0) return pol_refuse(who, "rows.n_feature_rows < 0");
    if (rows->d_index) {
        if (rows->n_feature_rows >= ((int64_t)1 << 31)) return pol_refuse(who, "rows.n_feature_rows must be below 2^31 with d_index");
    } else if (rows->first_row < 0 || rows->first_row > rows->n_feature_rows || rows->n_rows > rows->n_feature_rows - rows->first_row) {
        return pol_refuse(who, "first_row .. first_row + n_rows must lie inside 0 .. n_feature_rows without d_index");
    }
    return OC_OK;
}

PolicyArgs pol_args(const OcActorCritic* pol, const OcPolicyRows* rows) {
    PolicyArgs a = {};
    a.w1 = pol->d_w1; a.b1 = pol->d_b1; a.w2 = pol->d_w2; a.b2 = pol->d_b2; a.wp = pol->d_wp; a.bp = pol->d_bp; a.wv = pol->d_wv; a.bv = pol->d_bv;
    a.in_dim = pol->in_dim; a.h1 = pol->h1; a.h2 = pol->h2;
    a.features = rows->d_features; a.n_feature_rows = rows->n_feature_rows; a.index = rows->d_index; a.first = rows->first_row; a.n = rows->n_rows;
    return a;
}

unsigned pol_grid(int64_t n_rows, int waves) {
    const int64_t tiles = (n_rows + 31) / 32, groups = (tiles + waves - 1) / waves;
    return (unsigned)(groups < POL_GRID ? groups : POL_GRID);
}

template <int F0, int NF, bool REST>
void pol_launch_backward(const PolicyArgs& a, unsigned grid, int waves, size_t smem, hipStream_t stream) {
    if (want_lds(k_policy_backward<F0, NF, REST>, smem))
        hipLaunchKernelGGL((k_policy_backward<F0, NF, REST>), dim3(grid), dim3(64 * waves), smem, stream, a);
}

const char* const POL_FORWARD_WHO = "oc_policy_forward";
const char* const POL_BACKWARD_WHO = "oc_policy_backward";
const char* const POL_PLAN_WHO = "oc_policy_plan";

// ---- the two entry points in two halves each: every refusal (no device call), then the launches of a call that passed — so that a
// caller of several stages (update_chain.hpp) can make all its refusals before its first launch
int pol_check_forward(const char* who, const OcActorCritic* pol, const OcPolicyRows* rows, const float* d_logits, const float* d_values) {
    if (int rc = pol_check(who, pol, rows)) return rc;
    if (!d_logits || !d_values) return pol_refuse(who, "NULL d_logits or d_values");
    if ((uintptr_t)d_logits & 7u) return pol_refuse(who, "d_logits must be 8-byte aligned");
    if ((uintptr_t)d_values & 3u) return pol_refuse(who, "d_values must be 4-byte aligned");
    return OC_OK;
}

int pol_run_forward(const char* who, const OcActorCritic* pol, const OcPolicyRows* rows, float* d_logits, float* d_values, hipStream_t stream) {
    if (rows->n_rows == 0) return OC_OK;
    PolicyArgs a = pol_args(pol, rows);
    a.logits = d_logits; a.values = d_values;
    const size_t smem = pol_forward_lds(a.in_dim);
    if (want_lds(k_policy_forward, smem))
        hipLaunchKernelGGL(k_policy_forward, dim3(pol_grid(a.n, PL_WAVES)), dim3(BLOCK), smem, stream, a);
    return check_launch(who);
}

int pol_check_backward(const char* who, const OcActorCritic* pol, const OcPolicyRows* rows, const float* d_grad_logits, const float* d_grad_values,
                       const OcPolicyGrads* grads, const float* d_partials) {
    if (int rc = pol_check(who, pol, rows)) return rc;
    if (!d_grad_logits || !d_grad_values) return pol_refuse(who, "NULL d_grad_logits or d_grad_values");
    if ((uintptr_t)d_grad_logits & 7u) return pol_refuse(who, "d_grad_logits must be 8-byte aligned");
    if ((uintptr_t)d_grad_values & 3u) return pol_refuse(who, "d_grad_values must be 4-byte aligned");
    if (!grads) return pol_refuse(who, "grads is NULL");
    if (!grads->d_w1 || !grads->d_b1 || !grads->d_w2 || !grads->d_b2 || !grads->d_wp || !grads->d_bp || !grads->d_wv || !grads->d_bv)
        return pol_refuse(who, "NULL gradient array");
    if (((uintptr_t)grads->d_w1 | (uintptr_t)grads->d_b1 | (uintptr_t)grads->d_w2 | (uintptr_t)grads->d_b2 | (uintptr_t)grads->d_wp |
         (uintptr_t)grads->d_bp | (uintptr_t)grads->d_wv | (uintptr_t)grads->d_bv) & 3u)
        return pol_refuse(who, "gradient arrays must be 4-byte aligned");
    if (!d_partials) return pol_refuse(who, "d_partials is NULL");
    if ((uintptr_t)d_partials & 3u) return pol_refuse(who, "d_partials must be 4-byte aligned");
    return OC_OK;
}

int pol_run_backward(const char* who, const OcActorCritic* pol, const OcPolicyRows* rows, const float* d_grad_logits, const float* d_grad_values,
                     const OcPolicyGrads* grads, float* d_partials, hipStream_t stream) {
    PolicyArgs a = pol_args(pol, rows);
    a.grad_logits = d_grad_logits; a.grad_values = d_grad_values; a.partials = d_partials;
    const PolicyLayout o = pol_layout(a.in_dim, a.h1, a.h2);
    a.size = o.size;
    const int waves = pol_backward_waves(a.in_dim);
    const unsigned grid = pol_grid(a.n, waves);
    const size_t smem = pol_backward_lds(a.in_dim, waves);
    if (grid > 0) {
        const int nf = pol_nf(a.in_dim);
        if (nf == 2) pol_launch_backward<0, 2, true>(a, grid, waves, smem, stream);
        else pol_launch_backward<0, 3, true>(a, grid, waves, smem, stream);
        if (int rc = check_launch(who)) return rc;
        if (nf == 4) pol_launch_backward<3, 1, false>(a, grid, waves, smem, stream);
        if (nf == 5) pol_launch_backward<3, 2, false>(a, grid, waves, smem, stream);
        if (int rc = check_launch(who)) return rc;
    }
    PolicyGradPointers g = {{grads->d_w1, grads->d_b1, grads->d_w2, grads->d_b2, grads->d_wp, grads->d_bp, grads->d_wv, grads->d_bv}};
    hipLaunchKernelGGL(k_policy_grad_sum, dim3((o.size + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, (const float*)d_partials, (int)grid, o, g);
    return check_launch(who);
}

}  // namespace

extern "C" {

int oc_policy_forward(const OcActorCritic* pol, const OcPolicyRows* rows, float* d_logits, float* d_values, void* stream) {
    const char* const who = POL_FORWARD_WHO;
    if (int rc = pol_check_forward(who, pol, rows, d_logits, d_values)) return rc;
    return pol_run_forward(who, pol, rows, d_logits, d_values, (hipStream_t)stream);
}

int oc_policy_backward(const OcActorCritic* pol, const OcPolicyRows* rows, const float* d_grad_logits, const float* d_grad_values,
                       const OcPolicyGrads* grads, float* d_partials, void* stream) {
    const char* const who = POL_BACKWARD_WHO;
    if (int rc = pol_check_backward(who, pol, rows, d_grad_logits, d_grad_values, grads, d_partials)) return rc;
    return pol_run_backward(who, pol, rows, d_grad_logits, d_grad_values, grads, d_partials, (hipStream_t)stream);
}

int oc_policy_plan(int64_t n_rows, int with_index, int in_dim, int h1, int h2, int backward, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_policy_plan: no output buffer");
    out[0] = 0;
    const char* const who = backward ? POL_BACKWARD_WHO : POL_FORWARD_WHO;
    if (int rc = pol_check_shape(who, n_rows, in_dim, h1, h2)) return rc;
    const PolicyLayout o = pol_layout(in_dim, h1, h2);
    if (!backward) {
        if (n_rows == 0) snprintf(out, out_size, "nothing to launch (no rows)");
        else
            snprintf(out, out_size, "k_policy_forward grid=%u, %d lanes (%d wavefronts x 32-row tiles), %d rows per workgroup per pass, 32 x 32 x 2 f32 MFMA, "
                     "K %d -> %d -> %d -> 32 (h1 = %d, h2 = %d, 6 logits + value, zero-padded), index=%s, %zu B LDS", pol_grid(n_rows, PL_WAVES),
                     BLOCK, PL_WAVES, PL_WAVES * 32, in_dim, PL_HID, PL_HID, h1, h2, with_index ? "yes" : "no", pol_forward_lds(in_dim));
        return OC_OK;
    }
    const int waves = pol_backward_waves(in_dim), nf = pol_nf(in_dim);
    const unsigned grid = pol_grid(n_rows, waves);
    const int sum_grid = (o.size + BLOCK - 1) / BLOCK;
    if (n_rows == 0) {
        snprintf(out, out_size, "k_policy_grad_sum grid=%d, %d lanes, 0 partial(s) of %d floats (no rows: the gradients are zeroed)", sum_grid, BLOCK, o.size);
    } else {
        char more[96] = "";
        if (nf > 3) snprintf(more, sizeof(more), " + k_policy_backward<F0=3,NF=%d> grid=%u (feature rows 96.. of gw1)", nf - 3, grid);
        snprintf(out, out_size, "k_policy_backward<F0=0,NF=%d,REST> grid=%u, %d lanes (%d wavefronts x 32-row tiles), %d rows per workgroup per pass, 32 x 32 x 2 f32 MFMA, "
                 "%d accumulator tiles per wavefront, index=%s, %zu B LDS%s + k_policy_grad_sum grid=%d, %d lanes, %u partial(s) of %d floats",
                 nf < 3 ? nf : 3, grid, 64 * waves, waves, waves * 32, 2 * (nf < 3 ? nf : 3) + 6, with_index ? "yes" : "no", pol_backward_lds(in_dim, waves), more,
                 sum_grid, BLOCK, grid, o.size);
    }
    return OC_OK;
}

}  // extern "C"
