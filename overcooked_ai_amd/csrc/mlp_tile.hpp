// mlp_tile.hpp — the 32-row MFMA tile of the 64-wide dense network, once, for the five kernels that compute it: k_partner_logits
// (partner.hpp), k_pool_logits (partner_pool.hpp), k_policy_forward and k_policy_backward (policy.hpp) and k_bc_epoch_fused
// (bc_fused.hpp).  Device code and LDS arithmetic only: no kernel, no entry point.
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, in front of partner.hpp, after common.hpp
// (BLOCK).
//
// The scheme.  Dt = Wt * Xt on v_mfma_f32_32x32x2_f32.
//   The tile's 32 ROWS are units, its 32 COLUMNS rows of the call (envs, samples): lane l holds column l & 31 and, in its 16 accumulator
//   registers, rows (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5) — exactly the shape of the B operand of the next layer (lane l supplies
//   B[k = 2 s + (l >> 5)][column l & 31] at K step s) once the units are dealt to the rows so that register reg of lane half h holds
//   unit 2 * reg + h of its tile: then max(acc[reg], 0) IS the operand of step s = 16 * tile + reg, and activations pass from layer
//   to layer in registers — no LDS round trip, no lane permute.  The dealing costs nothing: it is the order in which the weights
//   (the A operand, lane l: A[row l & 31][k = 2 s + (l >> 5)]) are staged into LDS, once per workgroup, in operand order
//   [step][tile][lane] — one conflict-free ds_read_b32 per MFMA.  K steps are issued in ascending order with the bias as the
//   initial accumulator, which makes every unit the header's fmaf chain bit for bit (the hardware sums k = 2 s before 2 s + 1).
//   Hidden widths are padded to 64 (two tiles) and the outputs of the last layer to one tile with zero weights and biases; the last
//   layer's rows stay in their natural order.
//   Feature rows come through a per-wavefront LDS image, 32 rows at a time: coalesced 16-byte loads, rows in_dim + 2 floats apart so
//   that the 64 operand reads of a step (lane: row * (in_dim + 2) + 2 s + h) fall into 64 banks.
// What is NOT here: the wavefront fences, workgroup barriers and scheduling barriers around these pieces stay in the kernels, each
// where it stood; pol_load_rows (policy.hpp) writes ZEROS for a row without a source, pl_load_seated below leaves such a row as it
// was — both are needed (the backward pass reads the image as the A operand of gW1; the partner's image holds rows nobody names).
#pragma once

namespace {

constexpr int PL_WAVES = 4;           // wavefronts per workgroup (= BLOCK lanes)
constexpr int PL_HID = 64;            // hidden widths are padded to this: two tiles of 32 units
constexpr int PL_STEPS = PL_HID / 2;  // K steps of layers 2 and 3
static_assert(PL_WAVES * 64 == BLOCK, "one lane per env in the partner's seat pass");

typedef float pl_f32x16 __attribute__((ext_vector_type(16)));

// floats of LDS: the three weight matrices in operand order, the padded biases, a wavefront's feature image
__host__ __device__ constexpr int pl_w1_floats(int in_dim) { return (in_dim / 2) * 2 * 64; }
constexpr int PL_W2 = PL_STEPS * 2 * 64, PL_W3 = PL_STEPS * 64, PL_BIAS = PL_HID + PL_HID + 32;
__host__ __device__ constexpr int pl_image_floats(int in_dim) { return 32 * (in_dim + 2); }

// the forward operands of a workgroup, one behind the other from `base`; `end` is where the kernel's own words follow
struct PlOperands {
    float *sw1, *sw2, *sw3, *sb1, *sb2, *sb3, *end;
};
__device__ __forceinline__ PlOperands pl_operands(float* base, int in_dim) {
    PlOperands o;
    o.sw1 = base;
    o.sw2 = o.sw1 + pl_w1_floats(in_dim);
    o.sw3 = o.sw2 + PL_W2;
    o.sb1 = o.sw3 + PL_W3;
    o.sb2 = o.sb1 + PL_HID;
    o.sb3 = o.sb2 + PL_HID;
    o.end = o.sb3 + 32;
    return o;
}

// the unit (of its tile) that is dealt to tile row r: register reg = (r & 3) + 4 * (r >> 3) of lane half h = (r >> 2) & 1 holds row r,
// and must hold unit 2 * reg + h
__device__ __forceinline__ int pl_unit_of_row(int r) { return 2 * ((r & 3) + 4 * (r >> 3)) + ((r >> 2) & 1); }

__device__ __forceinline__ void pl_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the stager: dst[i] = *at(i), or 0 where at(i) is NULL, for i < total, by the whole workgroup.  PL_BATCH loads are issued before
// the first of them is stored: a lane's loads are round trips to L2, and one at a time they, not the MFMAs, were the partner
// kernel's time.  k_partner_logits and k_pool_logits keep a stager of their own (partner.hpp: pl_stage, an index in place of the
// pointer-or-NULL): with this one they were 0.85 us of 24 slower on the device (docs/NOTEBOOK.md).
constexpr int PL_BATCH = 8;
template <class F>
__device__ __forceinline__ void pol_stage(float* dst, int total, const float* inside, F at) {
    const int nt = blockDim.x;
    for (int i0 = threadIdx.x; i0 < total; i0 += PL_BATCH * nt) {
        float v[PL_BATCH];
#pragma unroll
        for (int j = 0; j < PL_BATCH; ++j) {
            const int i = i0 + j * nt;
            const float* p = i < total ? at(i) : nullptr;
            v[j] = *(p ? p : inside);  // (an address inside an array in any case)
            v[j] = p ? v[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < PL_BATCH; ++j)
            if (i0 + j * nt < total) dst[i0 + j * nt] = v[j];
    }
}

// the forward operands of layers 1 and 2, w [K][H] (Keras): dst[(s * 2 + tile) * 64 + lane] = w[2 s + (lane >> 5)][32 tile + unit of row lane & 31],
// 0 outside K x H
__device__ __forceinline__ void pol_stage_dealt(float* dst, const float* __restrict__ w, int K, int H, int steps) {
    pol_stage(dst, steps * 2 * 64, w, [=](int i) -> const float* {
        const int lane = i & 63, tile = (i >> 6) & 1, s = i >> 7;
        const int k = 2 * s + (lane >> 5), u = 32 * tile + pl_unit_of_row(lane & 31);
        return k < K && u < H ? w + (size_t)k * H + u : nullptr;
    });
}

// the biases of layers 1 and 2, zero-padded to PL_HID (the last layer's 32 are the kernel's own line: they differ)
__device__ __forceinline__ void pol_stage_biases(float* sb1, float* sb2, const float* b1, const float* b2, int h1, int h2) {
    if (threadIdx.x < PL_HID) {
        sb1[threadIdx.x] = (int)threadIdx.x < h1 ? b1[threadIdx.x] : 0.f;
        sb2[threadIdx.x] = (int)threadIdx.x < h2 ? b2[threadIdx.x] : 0.f;
    }
}

// ---- layers 1 and 2 of the tile in the image: the PRE-activations, register reg of lane half h of tile u = unit 32 u + 2 reg + h.
// TIGHT: the operand reads stay within four K steps of their MFMAs (the backward kernel's registers hold its accumulators; left to
// itself the scheduler lifts all 64 reads of layer 2 to the top)
template <bool TIGHT>
__device__ __forceinline__ void pol_hidden(const float* sw1, const float* sw2, const float* sb1, const float* sb2, const float* sx, int in_dim,
                                           int lane, pl_f32x16& c0, pl_f32x16& c1, pl_f32x16& d0, pl_f32x16& d1) {
    const int col = lane & 31, h = lane >> 5, S = in_dim + 2, steps1 = in_dim / 2;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        c0[reg] = sb1[2 * reg + h];
        c1[reg] = sb1[32 + 2 * reg + h];
    }
    const float* const xrow = sx + col * S + h;
#pragma unroll 4
    for (int s = 0; s < steps1; ++s) {
        const float b = xrow[2 * s];
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw1[(2 * s) * 64 + lane], b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw1[(2 * s + 1) * 64 + lane], b, c1, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        d0[reg] = sb2[2 * reg + h];
        d1[reg] = sb2[32 + 2 * reg + h];
    }
#pragma unroll
    for (int s = 0; s < PL_STEPS; ++s) {
        const float b = fmaxf(s < 16 ? c0[s & 15] : c1[s & 15], 0.f);
        d0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw2[(2 * s) * 64 + lane], b, d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sw2[(2 * s + 1) * 64 + lane], b, d1, 0, 0, 0);
        if (TIGHT && (s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- the last layer: 64 -> one tile, rows in their natural order (row m in register (m & 3) + 4 * (m >> 3) of lane half (m >> 2) & 1)
__device__ __forceinline__ pl_f32x16 pol_head(const float* sw3, const float* sb3, int lane, const pl_f32x16& d0, const pl_f32x16& d1) {
    const int h = lane >> 5;
    pl_f32x16 o;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) o[reg] = sb3[(reg & 3) + 8 * (reg >> 2) + 4 * h];
#pragma unroll
    for (int s = 0; s < PL_STEPS; ++s) {
        const float b = fmaxf(s < 16 ? d0[s & 15] : d1[s & 15], 0.f);
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(sw3[s * 64 + lane], b, o, 0, 0, 0);
    }
    return o;
}

// ---- the seated rows of a tile -> the wavefront's image: row r is player tseat[r]'s feature row of env env_of(r) where tseat[r] <= 1.
// Any other row is neither loaded nor written — the image keeps what it held, and the column is never stored.
template <class F>
__device__ __forceinline__ void pl_load_seated(float* sx, const float* features, const uint8_t* tseat, int in_dim, int lane, F env_of) {
    const int S = in_dim + 2, q = in_dim / 4;
    for (int i0 = lane; i0 < 32 * q; i0 += 4 * 64) {  // four 16-byte loads in flight per lane
        float4 v[4];
        int at[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * 64;
            const bool in = i < 32 * q;
            const int r = in ? i / q : 0, c = in ? i - r * q : 0;
            const uint32_t p = tseat[r];
            const bool load = in && p <= 1u;
            // (a lane without a row to fetch reads the array's first 16 bytes: no branch around the load, no traffic to speak of)
            v[j] = *reinterpret_cast<const float4*>(load ? features + ((int64_t)env_of(r) * 2 + p) * in_dim + 4 * c : features);
            at[j] = load ? r * S + 4 * c : -1;
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

// ---- the six logits of the lane's column out of the last layer's tile: rows 0..3 sit in registers 0..3 of lane half 0, rows 4..5 in
// registers 0..1 of half 1
__device__ __forceinline__ void pl_store_logits(float* row, int h, const pl_f32x16& o) {
    float2* const out = reinterpret_cast<float2*>(row);
    if (h == 0) {
        out[0] = make_float2(o[0], o[1]);
        out[1] = make_float2(o[2], o[3]);
    } else {
        out[2] = make_float2(o[0], o[1]);
    }
}

}  // namespace
