// partner.hpp — the behaviour-cloning partner of the training env: k_partner_logits, oc_partner_logits, oc_partner_logits_plan
// (include/oc_amd.h: OcDensePolicy, OcPartnerSeats)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit — the shortest of the four units of a
// clean build, so the longest stays as long as it was — after common.hpp (philox4x32_10) and host_util.hpp (fail, check_launch,
// want_lds).  Nothing else of the library is used, and no other kernel or entry point knows of this file.
//
// One launch per call does two things.
//   The seat pass: lane = env.  An env whose previous step was done (or every env, d_done == NULL) draws its seat from the
//   header's seating stream; the others read theirs.  A workgroup without a seated env leaves here (one barrier), so a self-play
//   phase (bc_factor = 0) costs a byte read per env.
//   The network, for the seated rows only — one feature row per env, the seated player's: Dt = Wt * Xt on v_mfma_f32_32x32x2_f32.
//   The tile's 32 ROWS are units, its 32 COLUMNS envs: lane l holds column l & 31 (an env) and, in its 16 accumulator registers,
//   rows (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5) — exactly the shape of the B operand of the next layer (lane l supplies
//   B[k = 2 s + (l >> 5)][column l & 31] at K step s) once the units are dealt to the rows so that register reg of lane half h holds
//   unit 2 * reg + h of its tile: then max(acc[reg], 0) IS the operand of step s = 16 * tile + reg, and activations pass from layer
//   to layer in registers — no LDS round trip, no lane permute.  The dealing costs nothing: it is the order in which the weights
//   (the A operand, lane l: A[row l & 31][k = 2 s + (l >> 5)]) are staged into LDS, once per workgroup, in operand order
//   [step][tile][lane] — one conflict-free ds_read_b32 per MFMA.  K steps are issued in ascending order with the bias as the
//   initial accumulator, which makes every unit the header's fmaf chain bit for bit (the hardware sums k = 2 s before 2 s + 1).
//   Hidden widths are padded to 64 (two tiles) and the six logits to one tile with zero weights and biases.
//   Feature rows come through a per-wavefront LDS image, 32 envs at a time: coalesced 16-byte loads of the seated rows, rows
//   in_dim + 2 floats apart so that the 64 operand reads of a step (lane: row * (in_dim + 2) + 2 s + h) fall into 64 banks.
//   A wavefront without a seated env leaves after the staging barrier, a 32-env tile without one is skipped.
#pragma once

namespace {

constexpr uint32_t SEAT_KEY_TWEAK = 0x53454154u;  // "SEAT"
constexpr int PL_WAVES = 4;                       // wavefronts per workgroup, 64 envs each (= BLOCK lanes)
constexpr int PL_HID = 64;                        // hidden widths are padded to this: two tiles of 32 units
constexpr int PL_STEPS = PL_HID / 2;              // K steps of layers 2 and 3
static_assert(PL_WAVES * 64 == BLOCK, "one lane per env in the seat pass");

struct PartnerArgs {
    const float *w1, *b1, *w2, *b2, *w3, *b3;  // Keras layout, [in][out]
    int in_dim, h1, h2;
    uint8_t* seat;
    const uint8_t* done;
    float bc_factor;
    uint32_t seed_lo, seed_hi, t_lo, t_hi;
    int64_t env_offset;
    const float* features;  // [n][2][in_dim]
    float* logits;          // [n][2][6]
};

typedef float pl_f32x16 __attribute__((ext_vector_type(16)));

// floats of dynamic LDS: the three weight matrices in operand order, the padded biases, the seats of the workgroup's envs (a byte
// each), the wavefronts' feature images
__host__ __device__ constexpr int pl_w1_floats(int in_dim) { return (in_dim / 2) * 2 * 64; }
constexpr int PL_W2 = PL_STEPS * 2 * 64, PL_W3 = PL_STEPS * 64, PL_BIAS = PL_HID + PL_HID + 32, PL_SEATS = BLOCK / 4;
__host__ __device__ constexpr int pl_image_floats(int in_dim) { return 32 * (in_dim + 2); }
__host__ __device__ constexpr size_t pl_lds_bytes(int in_dim) {
    return sizeof(float) * (size_t)(pl_w1_floats(in_dim) + PL_W2 + PL_W3 + PL_BIAS + PL_SEATS + PL_WAVES * pl_image_floats(in_dim));
}

// the unit (of its tile) that is dealt to tile row r: register reg = (r & 3) + 4 * (r >> 3) of lane half h = (r >> 2) & 1 holds row r,
// and must hold unit 2 * reg + h
__device__ __forceinline__ int pl_unit_of_row(int r) { return 2 * ((r & 3) + 4 * (r >> 3)) + ((r >> 2) & 1); }

// w [K][H] (Keras) -> dst[(s * T + tile) * 64 + lane] = w[2 s + (lane >> 5)][32 tile + unit of row lane & 31], 0 outside K x H.
// steps * T * 64 is a multiple of BLOCK.  PL_BATCH loads are issued before the first of them is stored: a lane's loads are
// round trips to L2, and one at a time they, not the MFMAs, were the kernel's time.
constexpr int PL_BATCH = 8;
template <int T, bool DEAL>
__device__ __forceinline__ void pl_stage(float* dst, const float* __restrict__ w, int K, int H, int steps) {
    const int total = steps * T * 64;
    for (int i0 = threadIdx.x; i0 < total; i0 += PL_BATCH * BLOCK) {
        float v[PL_BATCH];
#pragma unroll
        for (int j = 0; j < PL_BATCH; ++j) {
            const int i = i0 + j * BLOCK;
            const int lane = i & 63, tile = (i >> 6) % T, s = i / (64 * T);
            const int k = 2 * s + (lane >> 5), r = lane & 31;
            const int u = 32 * tile + (DEAL ? pl_unit_of_row(r) : r);
            const bool in = i < total && k < K && u < H;
            v[j] = w[in ? (size_t)k * H + u : 0];  // (an address inside the array in any case)
            v[j] = in ? v[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < PL_BATCH; ++j)
            if (i0 + j * BLOCK < total) dst[i0 + j * BLOCK] = v[j];
    }
}

__device__ __forceinline__ void pl_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(BLOCK) void k_partner_logits(PartnerArgs a, int64_t n) {
    extern __shared__ float pl_lds[];
    float* const sw1 = pl_lds;
    float* const sw2 = sw1 + pl_w1_floats(a.in_dim);
    float* const sw3 = sw2 + PL_W2;
    float* const sb1 = sw3 + PL_W3;
    float* const sb2 = sb1 + PL_HID;
    float* const sb3 = sb2 + PL_HID;
    uint8_t* const sseat = reinterpret_cast<uint8_t*>(sb3 + 32);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const sx = sb3 + 32 + PL_SEATS + wave * pl_image_floats(a.in_dim);

    // ---- the seat pass: lane = env
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t seat = 255u;
    if (e < n) {
        if (!a.done || a.done[e]) {
            const uint64_t g = (uint64_t)(a.env_offset + e);
            uint32_t r[4];
            philox4x32_10(a.t_lo, (uint32_t)g, (uint32_t)(g >> 32), a.t_hi, a.seed_lo, a.seed_hi ^ SEAT_KEY_TWEAK, r);
            seat = (float)(r[0] >> 8) * 0x1p-24f < a.bc_factor ? (r[1] & 1u) : 255u;
            a.seat[e] = (uint8_t)seat;
        } else {
            seat = a.seat[e];
        }
    }
    const bool seated = seat <= 1u;  // (never beyond the batch)
    sseat[threadIdx.x] = (uint8_t)(seated ? seat : 255u);
    if (!__syncthreads_or(seated)) return;  // no partner in this workgroup

    // ---- weights and biases, once per workgroup, in operand order
    pl_stage<2, true>(sw1, a.w1, a.in_dim, a.h1, a.in_dim / 2);
    pl_stage<2, true>(sw2, a.w2, a.h1, a.h2, PL_STEPS);
    pl_stage<1, false>(sw3, a.w3, a.h2, OC_NUM_ACTIONS, PL_STEPS);
    if (threadIdx.x < PL_HID) {
        sb1[threadIdx.x] = (int)threadIdx.x < a.h1 ? a.b1[threadIdx.x] : 0.f;
        sb2[threadIdx.x] = (int)threadIdx.x < a.h2 ? a.b2[threadIdx.x] : 0.f;
        if (threadIdx.x < 32) sb3[threadIdx.x] = threadIdx.x < OC_NUM_ACTIONS ? a.b3[threadIdx.x] : 0.f;
    }
    __syncthreads();
    const uint64_t seated_mask = __ballot(seated);
    if (seated_mask == 0) return;  // no partner in this wavefront

    const int col = lane & 31, h = lane >> 5;
    const int S = a.in_dim + 2, q = a.in_dim / 4, steps1 = a.in_dim / 2;
    for (int t = 0; t < 2; ++t) {
        if (((seated_mask >> (32 * t)) & 0xFFFFFFFFull) == 0) continue;  // no partner among these 32 envs
        const int64_t e0 = (int64_t)blockIdx.x * BLOCK + wave * 64 + 32 * t;  // the tile's first env
        const uint8_t* const tseat = sseat + wave * 64 + 32 * t;
        // ---- the seated rows of the tile -> the image (other rows keep what the image held: their columns are never stored)
        pl_wave_fence();  // (the reads of the previous tile are done)
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
                v[j] = *reinterpret_cast<const float4*>(load ? a.features + ((e0 + r) * 2 + p) * a.in_dim + 4 * c : a.features);
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
        pl_wave_fence();
        // ---- layer 1: in_dim -> 64, two unit tiles
        pl_f32x16 c0, c1;
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
        // ---- layer 2: 64 -> 64; register reg of unit tile u is the operand of step 16 u + reg
        pl_f32x16 d0, d1;
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
        }
        // ---- layer 3: 64 -> 6 logits in one tile, rows in their natural order
        pl_f32x16 o;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) o[reg] = sb3[(reg & 3) + 8 * (reg >> 2) + 4 * h];
#pragma unroll
        for (int s = 0; s < PL_STEPS; ++s) {
            const float b = fmaxf(s < 16 ? d0[s & 15] : d1[s & 15], 0.f);
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(sw3[s * 64 + lane], b, o, 0, 0, 0);
        }
        // ---- rows 0..3 sit in registers 0..3 of lane half 0, rows 4..5 in registers 0..1 of half 1
        const uint32_t p = tseat[col];
        if (p <= 1u) {
            float2* const out = reinterpret_cast<float2*>(a.logits + ((e0 + col) * 2 + p) * OC_NUM_ACTIONS);
            if (h == 0) {
                out[0] = make_float2(o[0], o[1]);
                out[1] = make_float2(o[2], o[3]);
            } else {
                out[2] = make_float2(o[0], o[1]);
            }
        }
    }
}

const char* const PARTNER_WHO = "oc_partner_logits";

// (who: the entry point a refusal names — oc_partner_pool_logits, csrc/partner_pool.hpp, makes the same checks under its own)
int pl_refuse(const char* why, const char* who = PARTNER_WHO) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail(OC_EINVAL, msg);
}

// the checks that need no array (oc_partner_logits_plan makes these alone)
int pl_check_shape(const OcBatch* b, const OcDensePolicy* pol, int num_pots, const char* who = PARTNER_WHO) {
    if (!b) return pl_refuse("batch is NULL", who);
    if (b->n_envs < 0) return pl_refuse("batch.n_envs < 0", who);
    if (!pol) return pl_refuse("policy is NULL", who);
    if (num_pots < 0 || num_pots > 4) return pl_refuse("num_pots must be in 0..4", who);
    if (pol->in_dim != 2 * (num_pots * 10 + 26) + 4) return pl_refuse("policy.in_dim must equal the feature length 2 * (num_pots * 10 + 26) + 4", who);
    if (pol->h1 < 1 || pol->h1 > PL_HID || pol->h2 < 1 || pol->h2 > PL_HID) return pl_refuse("policy.h1 and policy.h2 must be in 1..64", who);
    return OC_OK;
}

int pl_check(const OcBatch* b, const OcDensePolicy* pol, const OcPartnerSeats* seats, const float* d_features, int num_pots,
             const float* d_logits, const char* who = PARTNER_WHO) {
    if (!b) return pl_refuse("batch is NULL", who);
    if (!pol) return pl_refuse("policy is NULL", who);
    if (!seats) return pl_refuse("seats is NULL", who);
    if (!pol->d_w1 || !pol->d_b1 || !pol->d_w2 || !pol->d_b2 || !pol->d_w3 || !pol->d_b3) return pl_refuse("NULL weight or bias array", who);
    if (!seats->d_seat) return pl_refuse("seats.d_seat is NULL", who);
    if (!d_features || !d_logits) return pl_refuse("NULL d_features or d_logits", who);
    if ((uintptr_t)d_features & 15u) return pl_refuse("d_features must be 16-byte aligned", who);
    if ((uintptr_t)d_logits & 7u) return pl_refuse("d_logits must be 8-byte aligned", who);
    if (((uintptr_t)pol->d_w1 | (uintptr_t)pol->d_b1 | (uintptr_t)pol->d_w2 | (uintptr_t)pol->d_b2 | (uintptr_t)pol->d_w3 |
         (uintptr_t)pol->d_b3) & 3u)
        return pl_refuse("weight and bias arrays must be 4-byte aligned", who);
    if (int rc = pl_check_shape(b, pol, num_pots, who)) return rc;
    if (!(seats->bc_factor >= 0.f && seats->bc_factor <= 1.f)) return pl_refuse("seats.bc_factor must be in [0, 1]", who);
    return OC_OK;
}

}  // namespace

extern "C" {

int oc_partner_logits(const OcBatch* b, const OcDensePolicy* pol, const OcPartnerSeats* seats, const float* d_features, int num_pots,
                      float* d_logits, void* stream) {
    if (int rc = pl_check(b, pol, seats, d_features, num_pots, d_logits)) return rc;
    if (b->n_envs == 0) return OC_OK;
    PartnerArgs a;
    a.w1 = pol->d_w1; a.b1 = pol->d_b1; a.w2 = pol->d_w2; a.b2 = pol->d_b2; a.w3 = pol->d_w3; a.b3 = pol->d_b3;
    a.in_dim = pol->in_dim; a.h1 = pol->h1; a.h2 = pol->h2;
    a.seat = seats->d_seat; a.done = seats->d_done; a.bc_factor = seats->bc_factor;
    a.seed_lo = (uint32_t)seats->seed; a.seed_hi = (uint32_t)(seats->seed >> 32);
    a.t_lo = (uint32_t)(uint64_t)seats->step; a.t_hi = (uint32_t)((uint64_t)seats->step >> 32);
    a.env_offset = seats->env_offset;
    a.features = d_features; a.logits = d_logits;
    const size_t smem = pl_lds_bytes(a.in_dim);
    if (want_lds(k_partner_logits, smem))
        hipLaunchKernelGGL(k_partner_logits, dim3(grid_for(b->n_envs)), dim3(BLOCK), smem, (hipStream_t)stream, a, b->n_envs);
    return check_launch(PARTNER_WHO);
}

int oc_partner_logits_plan(const OcBatch* b, const OcDensePolicy* pol, int num_pots, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_partner_logits_plan: no output buffer");
    out[0] = 0;
    if (int rc = pl_check_shape(b, pol, num_pots)) return rc;
    if (b->n_envs == 0) snprintf(out, out_size, "nothing to launch (no envs)");
    else
        snprintf(out, out_size, "k_partner_logits grid=%u, %d lanes (%d wavefronts x 64 envs), 32 x 32 x 2 f32 MFMA, K %d -> %d -> %d -> 32 "
                 "(h1 = %d, h2 = %d, 6 logits, zero-padded), %zu B LDS", grid_for(b->n_envs), BLOCK, PL_WAVES, pol->in_dim, PL_HID, PL_HID,
                 pol->h1, pol->h2, pl_lds_bytes(pol->in_dim));
    return OC_OK;
}

}  // extern "C"
