// partner.hpp — the behaviour-cloning partner of the training env: k_partner_logits, oc_partner_logits, oc_partner_logits_plan
// (include/oc_amd.h: OcDensePolicy, OcPartnerSeats), and the seating stream that partner_pool.hpp draws from too
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit — the shortest of the four units of a
// clean build, so the longest stays as long as it was — after common.hpp (philox4x32_10), host_util.hpp (fail, check_launch,
// want_lds) and mlp_tile.hpp (the MFMA tile of the dense network: its scheme, operand order, layers and image are there).
//
// One launch per call does two things.
//   The seat pass: lane = env.  An env whose previous step was done (or every env, d_done == NULL) draws its seat from the
//   header's seating stream; the others read theirs.  A workgroup without a seated env leaves here (one barrier), so a self-play
//   phase (bc_factor = 0) costs a byte read per env.
//   The network, for the seated rows only — one feature row per env, the seated player's — as mlp_tile.hpp computes a tile: a
//   tile's 32 columns are envs, 32 at a time through the wavefront's image.  A wavefront without a seated env leaves after the
//   staging barrier, a 32-env tile without one is skipped.
#pragma once

namespace {

constexpr uint32_t SEAT_KEY_TWEAK = 0x53454154u;  // "SEAT"

// the seating stream of a call (include/oc_amd.h: OcPartnerSeats), as the kernels take it
struct SeatStream {
    uint8_t* seat;
    const uint8_t* done;
    float bc_factor;
    uint32_t seed_lo, seed_hi, t_lo, t_hi;
    int64_t env_offset;
};

SeatStream seat_stream_of(const OcPartnerSeats* seats) {
    SeatStream s;
    s.seat = seats->d_seat; s.done = seats->d_done; s.bc_factor = seats->bc_factor;
    s.seed_lo = (uint32_t)seats->seed; s.seed_hi = (uint32_t)(seats->seed >> 32);
    s.t_lo = (uint32_t)(uint64_t)seats->step; s.t_hi = (uint32_t)((uint64_t)seats->step >> 32);
    s.env_offset = seats->env_offset;
    return s;
}

// env e's block of the stream -> r, and the seat it draws: 0 or 1, or 255 for an env without a partner (r[2] draws the pool's member)
__device__ __forceinline__ uint32_t seat_draw(const SeatStream& s, int64_t e, uint32_t (&r)[4]) {
    const uint64_t g = (uint64_t)(s.env_offset + e);
    philox4x32_10(s.t_lo, (uint32_t)g, (uint32_t)(g >> 32), s.t_hi, s.seed_lo, s.seed_hi ^ SEAT_KEY_TWEAK, r);
    return (float)(r[0] >> 8) * 0x1p-24f < s.bc_factor ? (r[1] & 1u) : 255u;
}

struct PartnerArgs {
    const float *w1, *b1, *w2, *b2, *w3, *b3;  // Keras layout, [in][out]
    int in_dim, h1, h2;
    SeatStream s;
    const float* features;  // [n][2][in_dim]
    float* logits;          // [n][2][6]
};

// dynamic LDS: mlp_tile.hpp's operands and biases, the seats of the workgroup's envs (a byte each), the wavefronts' feature images
constexpr int PL_SEATS = BLOCK / 4;
__host__ __device__ constexpr size_t pl_lds_bytes(int in_dim) {
    return sizeof(float) * (size_t)(pl_w1_floats(in_dim) + PL_W2 + PL_W3 + PL_BIAS + PL_SEATS + PL_WAVES * pl_image_floats(in_dim));
}

// w [K][H] (Keras) -> dst[(s * T + tile) * 64 + lane] = w[2 s + (lane >> 5)][32 tile + unit of row lane & 31] (DEAL; else row lane & 31
// itself: the last layer), 0 outside K x H; steps * T * 64 is a multiple of BLOCK.  What pol_stage_dealt (mlp_tile.hpp) produces for
// T = 2, by a stager of this file's own: see there.
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

__global__ __launch_bounds__(BLOCK) void k_partner_logits(PartnerArgs a, int64_t n) {
    extern __shared__ float pl_lds[];
    const PlOperands w = pl_operands(pl_lds, a.in_dim);
    uint8_t* const sseat = reinterpret_cast<uint8_t*>(w.end);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const sx = w.end + PL_SEATS + wave * pl_image_floats(a.in_dim);

    // ---- the seat pass: lane = env
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t seat = 255u;
    if (e < n) {
        if (!a.s.done || a.s.done[e]) {
            uint32_t r[4];
            seat = seat_draw(a.s, e, r);
            a.s.seat[e] = (uint8_t)seat;
        } else {
            seat = a.s.seat[e];
        }
    }
    const bool seated = seat <= 1u;  // (never beyond the batch)
    sseat[threadIdx.x] = (uint8_t)(seated ? seat : 255u);
    if (!__syncthreads_or(seated)) return;  // no partner in this workgroup

    // ---- weights and biases, once per workgroup, in operand order
    pl_stage<2, true>(w.sw1, a.w1, a.in_dim, a.h1, a.in_dim / 2);
    pl_stage<2, true>(w.sw2, a.w2, a.h1, a.h2, PL_STEPS);
    pl_stage<1, false>(w.sw3, a.w3, a.h2, OC_NUM_ACTIONS, PL_STEPS);
    pol_stage_biases(w.sb1, w.sb2, a.b1, a.b2, a.h1, a.h2);
    if (threadIdx.x < 32) w.sb3[threadIdx.x] = threadIdx.x < OC_NUM_ACTIONS ? a.b3[threadIdx.x] : 0.f;
    __syncthreads();
    const uint64_t seated_mask = __ballot(seated);
    if (seated_mask == 0) return;  // no partner in this wavefront

    const int col = lane & 31, h = lane >> 5;
    for (int t = 0; t < 2; ++t) {
        if (((seated_mask >> (32 * t)) & 0xFFFFFFFFull) == 0) continue;  // no partner among these 32 envs
        const int64_t e0 = (int64_t)blockIdx.x * BLOCK + wave * 64 + 32 * t;  // the tile's first env
        const uint8_t* const tseat = sseat + wave * 64 + 32 * t;
        pl_wave_fence();  // (the reads of the previous tile are done)
        pl_load_seated(sx, a.features, tseat, a.in_dim, lane, [=](int r) { return e0 + r; });
        pl_wave_fence();
        pl_f32x16 c0, c1, d0, d1;
        pol_hidden<false>(w.sw1, w.sw2, w.sb1, w.sb2, sx, a.in_dim, lane, c0, c1, d0, d1);
        const pl_f32x16 o = pol_head(w.sw3, w.sb3, lane, d0, d1);
        const uint32_t p = tseat[col];
        if (p <= 1u) pl_store_logits(a.logits + ((e0 + col) * 2 + p) * OC_NUM_ACTIONS, h, o);
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
    a.s = seat_stream_of(seats);
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
