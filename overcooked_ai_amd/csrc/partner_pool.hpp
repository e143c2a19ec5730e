// partner_pool.hpp — a pool of frozen partner policies, one member per episode: k_pool_seat, k_pool_write, k_pool_logits,
// oc_partner_pool_logits, oc_partner_pool_plan (include/oc_amd.h: OcPartnerPool)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, after mlp_tile.hpp (the MFMA tile of
// the dense network), partner.hpp (the seating stream, the stager pl_stage, the LDS shape, the host checks) and sample_index.hpp (k_sample_scan, si_lanes_below).
//
// A 32-env MFMA tile shares one set of weights, and neighbouring envs draw different members: so the seated envs are bucketed by
// member first — over the whole batch, since a bucket of one workgroup's 256 envs would hold 256 / K rows and every workgroup would
// stage all K members' operands (about 42 KB each, the cost partner.hpp names as that kernel's time) — and the network runs over the
// buckets.  Four launches, none of which waits for another workgroup, and no atomics: a call repeats byte for byte.
//   k_pool_seat    lane = env: k_partner_logits' seat pass plus the member draw (word 2 of the same block); stores seat and member,
//                  and counts the seated envs of every member in its 256-env block (a ballot and a popcount per member and
//                  wavefront) into counts[member * n_blocks + block].  Block 0 also copies the member table into the scratch, from
//                  where k_pool_logits reads one row by a uniform index (indexing the by-value argument would need a stack object).
//   k_sample_scan  the exclusive scan of the counts in place (sample_index.hpp), one entry more than there are counts: the last
//                  entry becomes the number of seated envs, so that member m's bucket is [offsets[m * n_blocks], offsets[(m + 1) * n_blocks]).
//   k_pool_write   lane = env: order[offsets[member * n_blocks + block] + the wavefront counts before its own + the ballot bits below
//                  the lane] = env — every bucket ascending in env.
//   k_pool_logits  k_partner_logits' network over bucket rows: a workgroup serves 256 rows of ONE member (two passes of 128: a 32-row tile per wavefront) and stages that member's
//                  operands once.  The grid is the host-known bound ceil(n_envs / 256) + n_members (sum of ceil(c_m / 256) <=
//                  floor(sum c_m / 256) + K); a workgroup finds its (member, chunk) by a scalar walk over at most 16 bucket bounds and
//                  leaves when it lies beyond the last chunk.  Rows are gathered through order[] and the env's seat byte, logits
//                  scattered to d_logits[env][seat].  Same K steps in the same order from the same operands: the six floats of an env
//                  are k_partner_logits' with that member as the only policy, bit for bit.  Where the chunks of 256 rows outnumber
//                  the CUs (a workgroup's LDS image leaves room for one per CU) a workgroup takes 128 j rows in j > 2 passes instead of 256 in two.
#pragma once

namespace {

struct PoolMember {  // a row of the member table: 64 bytes
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int h1, h2;
    int pad[2];
};
static_assert(sizeof(PoolMember) == 64, "the scratch layout below counts on it");

// the caller's scratch: the number of seated envs (i64, k_sample_scan's), the member table, the counts / offsets, the bucket order
constexpr size_t PP_TABLE_AT = 64, PP_COUNTS_AT = PP_TABLE_AT + OC_MAX_POOL * sizeof(PoolMember);
inline size_t pp_counts(int64_t n, int n_members) { return (size_t)n_members * grid_for(n) + 1; }
inline size_t pp_scratch_bytes(int64_t n, int n_members) { return PP_COUNTS_AT + sizeof(uint32_t) * pp_counts(n, n_members) + sizeof(int32_t) * (size_t)n; }
__host__ __device__ constexpr size_t pp_lds_bytes(int in_dim) { return pl_lds_bytes(in_dim) + sizeof(int32_t) * BLOCK; }  // + the rows' envs

struct PoolSeatArgs {
    SeatStream s;  // (partner.hpp)
    uint8_t* member;
    int n_members;
    uint32_t thr[OC_MAX_POOL - 1];
    PoolMember members[OC_MAX_POOL];
};

// seat and member of env e after this call's reseat, as k_pool_seat left them; an env is bucketed when it has both
__device__ __forceinline__ bool pp_bucketed(uint32_t seat, uint32_t member, int n_members) { return seat <= 1u && member < (uint32_t)n_members; }

__global__ __launch_bounds__(BLOCK) void k_pool_seat(PoolSeatArgs a, int64_t n, uint32_t n_blocks, uint32_t* __restrict__ counts,
                                                     PoolMember* __restrict__ table) {
    __shared__ uint32_t s_cnt[OC_MAX_POOL][PL_WAVES];
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t seat = 255u, member = 255u;
    if (e < n) {
        if (!a.s.done || a.s.done[e]) {
            uint32_t r[4];
            seat = seat_draw(a.s, e, r);
            if (seat <= 1u) {
                member = 0u;
#pragma unroll
                for (int m = 0; m < OC_MAX_POOL - 1; ++m) member += (m < a.n_members - 1 && r[2] >= a.thr[m]) ? 1u : 0u;
            }
            a.s.seat[e] = (uint8_t)seat;
            a.member[e] = (uint8_t)member;
        } else {
            seat = a.s.seat[e];
            member = a.member[e];
        }
    }
    const bool in = pp_bucketed(seat, member, a.n_members);
#pragma unroll
    for (int m = 0; m < OC_MAX_POOL; ++m)
        if (m < a.n_members) {  // (uniform)
            const uint32_t c = (uint32_t)__popcll(__ballot(in && member == (uint32_t)m));
            if ((threadIdx.x & 63) == 0) s_cnt[m][threadIdx.x >> 6] = c;
        }
    __syncthreads();
    if ((int)threadIdx.x < a.n_members) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < PL_WAVES; ++w) sum += s_cnt[threadIdx.x][w];
        counts[(size_t)threadIdx.x * n_blocks + blockIdx.x] = sum;
    }
    if (blockIdx.x == 0) {
#pragma unroll
        for (int m = 0; m < OC_MAX_POOL; ++m)
            if ((int)threadIdx.x == m && m < a.n_members) table[m] = a.members[m];
        if (threadIdx.x == 0) counts[(size_t)a.n_members * n_blocks] = 0u;  // (scanned: the number of seated envs)
    }
}

__global__ __launch_bounds__(BLOCK) void k_pool_write(const uint8_t* __restrict__ d_seat, const uint8_t* __restrict__ d_member, int64_t n,
                                                      uint32_t n_blocks, int n_members, const uint32_t* __restrict__ offsets,
                                                      int32_t* __restrict__ order) {
    __shared__ uint32_t s_cnt[OC_MAX_POOL][PL_WAVES];
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t seat = 255u, member = 255u;
    if (e < n) {
        seat = d_seat[e];
        member = d_member[e];
    }
    const bool in = pp_bucketed(seat, member, n_members);
    uint32_t below = 0;
#pragma unroll
    for (int m = 0; m < OC_MAX_POOL; ++m)
        if (m < n_members) {  // (uniform)
            const uint64_t mask = __ballot(in && member == (uint32_t)m);
            if ((threadIdx.x & 63) == 0) s_cnt[m][wave] = (uint32_t)__popcll(mask);
            if (member == (uint32_t)m) below = si_lanes_below(mask);
        }
    __syncthreads();
    if (in) {
        uint32_t at = offsets[(size_t)member * n_blocks + blockIdx.x];
#pragma unroll
        for (int w = 0; w < PL_WAVES; ++w) at += (uint32_t)w < wave ? s_cnt[member][w] : 0u;
        order[at + below] = (int32_t)e;  // (below the number of seated envs, which is at most n)
    }
}

struct PoolArgs {
    const PoolMember* table;
    const uint32_t* offsets;
    const int32_t* order;
    const uint8_t* seat;
    int in_dim, n_members;
    uint32_t n_blocks;
    uint32_t n_cus;         // workgroups that run side by side (one per CU: the LDS image is above half a CU's)
    const float* features;  // [n][2][in_dim]
    float* logits;          // [n][2][6]
};

__global__ __launch_bounds__(BLOCK) void k_pool_logits(PoolArgs a) {
    // ---- rows per workgroup: 256 — two passes of 128, a 32-row tile per wavefront and pass —, unless the chunks of 256 outnumber
    //      the CUs: some CU would then run a second workgroup, for a few rows, after the first (65 536 seated envs of 4 members: 260
    //      chunks on 256 CUs took 2.4x the single-policy call).  Then chunks of 128 j rows, j the least for which floor(T / 128) / j + K
    //      (a bound of their number) fits the CUs: staged once, j passes.  Which rows a workgroup serves changes no row's arithmetic.
    constexpr uint32_t PASS = 4 * 32;
    uint32_t chunks = 0, passes = BLOCK / PASS;
    for (int m = 0; m < a.n_members; ++m)
        chunks += (a.offsets[(size_t)(m + 1) * a.n_blocks] - a.offsets[(size_t)m * a.n_blocks] + BLOCK - 1) / BLOCK;
    if (chunks > a.n_cus) {
        const uint32_t room = a.n_cus > (uint32_t)a.n_members ? a.n_cus - (uint32_t)a.n_members : 1u;
        passes = (a.offsets[(size_t)a.n_members * a.n_blocks] / PASS + room - 1) / room;  // (3 or more where K < n_cus: T / 256 >= chunks - K > room)
        passes = passes < BLOCK / PASS ? BLOCK / PASS : passes;  // (at least 256 rows: the grid counts on it)
    }
    const uint32_t rows = passes * PASS;
    // ---- this workgroup's member and its rows of that member's bucket
    uint32_t first = 0, last = 0;
    int member = -1;
    chunks = 0;
    for (int m = 0; m < a.n_members; ++m) {
        const uint32_t s = a.offsets[(size_t)m * a.n_blocks], t = a.offsets[(size_t)(m + 1) * a.n_blocks];
        const uint32_t c = (t - s + rows - 1) / rows;
        if (blockIdx.x < chunks + c) {
            member = m;
            first = s + (blockIdx.x - chunks) * rows;
            last = t < first + rows ? t : first + rows;
            break;
        }
        chunks += c;
    }
    if (member < 0) return;  // beyond the last chunk
    const PoolMember pm = a.table[__builtin_amdgcn_readfirstlane(member)];

    extern __shared__ float pp_lds[];
    const PlOperands w = pl_operands(pp_lds, a.in_dim);
    uint8_t* const sseat = reinterpret_cast<uint8_t*>(w.end);
    int32_t* const senv = reinterpret_cast<int32_t*>(w.end + PL_SEATS);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const sx = w.end + PL_SEATS + BLOCK + wave * pl_image_floats(a.in_dim);

    // (the rows of the first pass: their loads are in flight beside the staging)
    const int col = lane & 31, h = lane >> 5;
    uint32_t row = first + wave * 32 + col;  // (both halves of a wavefront hold the tile's 32 rows)
    int32_t env = row < last ? a.order[row] : 0;
    uint32_t seat = row < last ? a.seat[env] : 255u;

    // ---- the member's weights and biases, once per workgroup, in operand order
    pl_stage<2, true>(w.sw1, pm.w1, a.in_dim, pm.h1, a.in_dim / 2);
    pl_stage<2, true>(w.sw2, pm.w2, pm.h1, pm.h2, PL_STEPS);
    pl_stage<1, false>(w.sw3, pm.w3, pm.h2, OC_NUM_ACTIONS, PL_STEPS);
    pol_stage_biases(w.sb1, w.sb2, pm.b1, pm.b2, pm.h1, pm.h2);
    if (threadIdx.x < 32) w.sb3[threadIdx.x] = threadIdx.x < OC_NUM_ACTIONS ? pm.b3[threadIdx.x] : 0.f;
    __syncthreads();

    const uint8_t* const tseat = sseat + wave * 32;
    const int32_t* const tenv = senv + wave * 32;
    // ---- the passes of 128 rows; from here on a wavefront works alone, on rows [32 wave, 32 wave + 32) of every pass
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const bool seated = seat <= 1u;  // (255 beyond the workgroup's rows)
        if (__ballot(seated) == 0) break;  // the workgroup's rows end before this wavefront's: those of the later passes too
        pl_wave_fence();  // (the reads of the previous pass are done)
        sseat[wave * 32 + col] = (uint8_t)(seated ? seat : 255u);  // (twice, by both halves)
        senv[wave * 32 + col] = env;
        row += PASS;  // the next pass's rows, in flight beside the tile
        env = row < last ? a.order[row] : 0;
        seat = row < last ? a.seat[env] : 255u;
        // ---- the tile's rows -> the image (rows beyond the bucket keep what the image held: their columns are never stored)
        pl_wave_fence();  // (and the tile's rows are written)
        pl_load_seated(sx, a.features, tseat, a.in_dim, lane, [=](int r) { return tenv[r]; });
        pl_wave_fence();
        pl_f32x16 c0, c1, d0, d1;
        pol_hidden<false>(w.sw1, w.sw2, w.sb1, w.sb2, sx, a.in_dim, lane, c0, c1, d0, d1);
        const pl_f32x16 o = pol_head(w.sw3, w.sb3, lane, d0, d1);
        const uint32_t p = tseat[col];
        if (p <= 1u) pl_store_logits(a.logits + ((int64_t)tenv[col] * 2 + p) * OC_NUM_ACTIONS, h, o);
    }
}

const char* const POOL_WHO = "oc_partner_pool_logits";

// thresholds of a pool: the caller's, or the uniform ones ceil((m + 1) * 2^32 / K)
void pp_thresholds(const OcPartnerPool* pool, uint32_t* thr) {
    for (int m = 0; m < OC_MAX_POOL - 1; ++m) {
        if (m >= pool->n_members - 1) thr[m] = 0xFFFFFFFFu;  // (never read)
        else if (pool->thresholds) thr[m] = pool->thresholds[m];
        else thr[m] = (uint32_t)((((uint64_t)(m + 1) << 32) + (uint64_t)pool->n_members - 1) / (uint64_t)pool->n_members);
    }
}

// a refusal of member m >= 1 says which (member 0 has passed every check that is not a member's own)
int pp_member(int rc, int m) {
    if (m == 0) return rc;
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%.400s (members[%d])", g_err, m);
    return fail(rc, msg);
}

// the checks that need no device array (oc_partner_pool_plan makes these alone)
int pp_check_shape(const OcBatch* b, const OcPartnerPool* pool, int num_pots) {
    if (!pool) return pl_refuse("pool is NULL", POOL_WHO);
    if (!pool->members) return pl_refuse("pool.members is NULL", POOL_WHO);
    if (pool->n_members < 1 || pool->n_members > OC_MAX_POOL) return pl_refuse("pool.n_members must be in 1..16", POOL_WHO);
    for (int m = 0; m < pool->n_members; ++m)
        if (int rc = pl_check_shape(b, &pool->members[m], num_pots, POOL_WHO)) return pp_member(rc, m);
    if (b->n_envs > INT32_MAX) return pl_refuse("batch.n_envs must be below 2^31", POOL_WHO);
    if (pool->thresholds)
        for (int m = 1; m < pool->n_members - 1; ++m)
            if (pool->thresholds[m] < pool->thresholds[m - 1]) return pl_refuse("pool.thresholds must not decrease", POOL_WHO);
    return OC_OK;
}

}  // namespace

extern "C" {

int oc_partner_pool_logits(const OcBatch* b, const OcPartnerPool* pool, const OcPartnerSeats* seats, const float* d_features, int num_pots,
                           float* d_logits, void* d_scratch, void* stream) {
    if (int rc = pp_check_shape(b, pool, num_pots)) return rc;
    if (!pool->d_member) return pl_refuse("pool.d_member is NULL", POOL_WHO);
    for (int m = 0; m < pool->n_members; ++m)
        if (int rc = pl_check(b, &pool->members[m], seats, d_features, num_pots, d_logits, POOL_WHO)) return pp_member(rc, m);
    const int64_t n = b->n_envs;
    if (n == 0) return OC_OK;
    if (!d_scratch) return pl_refuse("d_scratch is NULL", POOL_WHO);
    if ((uintptr_t)d_scratch & 15u) return pl_refuse("d_scratch must be 16-byte aligned", POOL_WHO);
    const int K = pool->n_members;
    const unsigned blocks = grid_for(n);
    char* const scratch = static_cast<char*>(d_scratch);
    int64_t* const total = reinterpret_cast<int64_t*>(scratch);
    PoolMember* const table = reinterpret_cast<PoolMember*>(scratch + PP_TABLE_AT);
    uint32_t* const counts = reinterpret_cast<uint32_t*>(scratch + PP_COUNTS_AT);
    int32_t* const order = reinterpret_cast<int32_t*>(counts + pp_counts(n, K));
    PoolSeatArgs s = {};
    s.s = seat_stream_of(seats);
    s.member = pool->d_member;
    s.n_members = K;
    pp_thresholds(pool, s.thr);
    for (int m = 0; m < K; ++m) {
        const OcDensePolicy& p = pool->members[m];
        s.members[m] = PoolMember{p.d_w1, p.d_b1, p.d_w2, p.d_b2, p.d_w3, p.d_b3, p.h1, p.h2, {0, 0}};
    }
    PoolArgs a;
    a.table = table; a.offsets = counts; a.order = order; a.seat = seats->d_seat;
    a.in_dim = pool->members[0].in_dim; a.n_members = K; a.n_blocks = blocks;
    a.n_cus = (uint32_t)(simd_count() / 4);
    a.features = d_features; a.logits = d_logits;
    const size_t smem = pp_lds_bytes(a.in_dim);
    hipStream_t st = (hipStream_t)stream;
    if (want_lds(k_pool_logits, smem)) {
        hipLaunchKernelGGL(k_pool_seat, dim3(blocks), dim3(BLOCK), 0, st, s, n, (uint32_t)blocks, counts, table);
        hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(BLOCK), 0, st, counts, (uint32_t)pp_counts(n, K), total);
        hipLaunchKernelGGL(k_pool_write, dim3(blocks), dim3(BLOCK), 0, st, (const uint8_t*)seats->d_seat, (const uint8_t*)pool->d_member, n,
                           (uint32_t)blocks, K, (const uint32_t*)counts, order);
        hipLaunchKernelGGL(k_pool_logits, dim3(blocks + K), dim3(BLOCK), smem, st, a);
    }
    return check_launch(POOL_WHO);
}

int oc_partner_pool_plan(const OcBatch* b, const OcPartnerPool* pool, int num_pots, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_partner_pool_plan: no output buffer");
    out[0] = 0;
    if (int rc = pp_check_shape(b, pool, num_pots)) return rc;
    const int64_t n = b->n_envs;
    const int K = pool->n_members;
    if (n == 0) snprintf(out, out_size, "nothing to launch (no envs)");
    else
        snprintf(out, out_size, "k_pool_seat grid=%u, %d lanes + k_sample_scan grid=1, %d lanes, %u pass(es) of %d counts + k_pool_write grid=%u, %d lanes + "
                 "k_pool_logits grid=%u (%u blocks of envs + %d members), %d lanes (128 j rows of one member), 32 x 32 x 2 f32 MFMA, K %d -> %d -> %d -> 32, "
                 "%zu B LDS; scratch %zu B", grid_for(n), BLOCK, BLOCK, (unsigned)((pp_counts(n, K) + BLOCK - 1) / BLOCK), BLOCK, grid_for(n), BLOCK,
                 grid_for(n) + K, grid_for(n), K, BLOCK, pool->members[0].in_dim, PL_HID, PL_HID, pp_lds_bytes(pool->members[0].in_dim),
                 pp_scratch_bytes(n, K));
    return OC_OK;
}

}  // extern "C"
