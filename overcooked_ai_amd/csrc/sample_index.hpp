// sample_index.hpp — the learner's sample index on the device: k_sample_count, k_sample_scan, k_sample_write (oc_sample_select: the
// learner's samples of a collected batch, ascending) and k_sample_permute (oc_sample_permute: a keyed permutation of them), with
// oc_sample_index_plan (include/oc_amd.h: "The learner's sample index")
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, after common.hpp (BLOCK, philox4x32_10)
// and host_util.hpp (fail, check_launch).  Nothing else of the library is used, and no other kernel or entry point knows of this file.
//
// Selection: a stream compaction in three launches, none of which waits for another workgroup.  A block is SI_P = 1024 consecutive
// samples, tile k of it the 256 samples [256 k, 256 k + 256): lane l of the workgroup evaluates sample 256 k + l of every tile, so
// that a wavefront's byte loads are 64 adjacent bytes, and a wavefront's count of a tile is the popcount of one __ballot.
// k_sample_count adds the sixteen (tile, wavefront) counts of a block; k_sample_scan, ONE workgroup, turns the block counts into
// exclusive offsets in place, 256 blocks per pass (a shuffle scan inside each wavefront, the four wavefront totals through LDS, one
// barrier per pass: the LDS row alternates), with the counts of the next SI_SCAN_B passes loaded before the current ones are
// scanned — the passes are sequential, their loads are not; k_sample_write evaluates the predicate again, ranks a selected sample
// by the block's offset + the (tile, wavefront) counts before its own + the ballot bits below its lane, and stores its index there.
// The lane of sample s >= L stores -1 at position s: selected samples land below L, so the two sets of stores are disjoint.
// No atomics anywhere: the same inputs give the same bytes.
// Permutation: one lane per output.  The eight round keys are two Philox blocks of (seed, epoch), the same for every lane; the
// bijection is eight alternating xor-rounds on the two halves of a w-bit number, walked along its cycle until it is below L.
#pragma once

namespace {

constexpr int SI_TILES = 4;                    // samples per lane of a block
constexpr int SI_P = BLOCK * SI_TILES;         // samples per block
constexpr int SI_WAVES = BLOCK / 64;
constexpr int SI_SCAN_B = 8;                   // passes of the scan whose counts are in flight
constexpr unsigned SI_PERM_GRID_MAX = 1024;    // workgroups of k_sample_permute; outputs beyond them by grid stride
constexpr uint32_t SHUFFLE_KEY_TWEAK = 0x53485546u;  // "SHUF"

// the header's selection rule for sample s of S (a sample at or beyond S is not selected, and nothing is read for it)
template <bool SEAT, bool ACT>
__device__ __forceinline__ bool si_selected(const uint8_t* __restrict__ seat, const uint8_t* __restrict__ actions, uint32_t s, uint32_t S) {
    if (s >= S) return false;
    uint32_t st = 255u, ac = 0u;
    if (SEAT) st = seat[s >> 1];
    if (ACT) ac = actions[s];
    return st != (s & 1u) && ac <= 5u;
}

__device__ __forceinline__ uint32_t si_lanes_below(uint64_t m) {  // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <bool SEAT, bool ACT>
__global__ __launch_bounds__(BLOCK) void k_sample_count(const uint8_t* __restrict__ seat, const uint8_t* __restrict__ actions, uint32_t S,
                                                        uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_cnt[SI_WAVES];
    const uint32_t first = blockIdx.x * (uint32_t)SI_P + threadIdx.x;
    bool sel[SI_TILES];
#pragma unroll
    for (int k = 0; k < SI_TILES; ++k) sel[k] = si_selected<SEAT, ACT>(seat, actions, first + k * BLOCK, S);
    uint32_t n = 0;  // (wavefront-uniform)
#pragma unroll
    for (int k = 0; k < SI_TILES; ++k) n += (uint32_t)__popcll(__ballot(sel[k]));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < SI_WAVES; ++w) sum += s_cnt[w];
        counts[blockIdx.x] = sum;
    }
}

// counts[b] -> the sum of counts[0 .. b), in place; *d_count = the sum of all.  One workgroup.
__global__ __launch_bounds__(BLOCK) void k_sample_scan(uint32_t* counts, uint32_t n_blocks, int64_t* __restrict__ d_count) {
    __shared__ uint32_t s_tot[2][SI_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t passes = (n_blocks + BLOCK - 1) / BLOCK;
    uint32_t carry = 0, cur[SI_SCAN_B], nxt[SI_SCAN_B];
#pragma unroll
    for (int j = 0; j < SI_SCAN_B; ++j) {
        const uint32_t b = (uint32_t)j * BLOCK + threadIdx.x;
        cur[j] = b < n_blocks ? counts[b] : 0u;
    }
    for (uint32_t p0 = 0; p0 < passes; p0 += SI_SCAN_B) {
#pragma unroll
        for (int j = 0; j < SI_SCAN_B; ++j) {  // in flight while this run of passes is scanned
            const uint32_t b = (p0 + SI_SCAN_B + j) * BLOCK + threadIdx.x;
            nxt[j] = b < n_blocks ? counts[b] : 0u;
        }
#pragma unroll
        for (int j = 0; j < SI_SCAN_B; ++j) {
            if (p0 + j < passes) {  // (uniform)
                const uint32_t b = (p0 + j) * BLOCK + threadIdx.x;
                uint32_t x = cur[j];
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = __shfl_up(x, off, 64);
                    x += lane >= (uint32_t)off ? y : 0u;
                }
                if (lane == 63) s_tot[j & 1][wave] = x;
                __syncthreads();
                uint32_t before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < SI_WAVES; ++w) {
                    const uint32_t t = s_tot[j & 1][w];
                    before += (uint32_t)w < wave ? t : 0u;
                    total += t;
                }
                if (b < n_blocks) counts[b] = carry + before + (x - cur[j]);
                carry += total;
            }
        }
#pragma unroll
        for (int j = 0; j < SI_SCAN_B; ++j) cur[j] = nxt[j];
    }
    if (threadIdx.x == 0) *d_count = (int64_t)carry;
}

template <bool SEAT, bool ACT>
__global__ __launch_bounds__(BLOCK) void k_sample_write(const uint8_t* __restrict__ seat, const uint8_t* __restrict__ actions, uint32_t S,
                                                        const uint32_t* __restrict__ offsets, const int64_t* __restrict__ d_count,
                                                        int32_t* __restrict__ ids) {
    __shared__ uint32_t s_cnt[SI_TILES][SI_WAVES];
    const uint32_t first = blockIdx.x * (uint32_t)SI_P + threadIdx.x, wave = threadIdx.x >> 6;
    bool sel[SI_TILES];
    uint64_t m[SI_TILES];
#pragma unroll
    for (int k = 0; k < SI_TILES; ++k) sel[k] = si_selected<SEAT, ACT>(seat, actions, first + k * BLOCK, S);
#pragma unroll
    for (int k = 0; k < SI_TILES; ++k) m[k] = __ballot(sel[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < SI_TILES; ++k) s_cnt[k][wave] = (uint32_t)__popcll(m[k]);
    }
    __syncthreads();
    const uint32_t L = (uint32_t)*d_count;
    uint32_t at = offsets[blockIdx.x];  // the position of the first selected sample of (tile k, wavefront w), in that order
#pragma unroll
    for (int k = 0; k < SI_TILES; ++k) {
        const uint32_t s = first + k * BLOCK;
#pragma unroll
        for (int w = 0; w < SI_WAVES; ++w) {
            if ((uint32_t)w == wave && sel[k]) ids[at + si_lanes_below(m[k])] = (int32_t)s;
            at += s_cnt[k][w];
        }
        if (s < S && s >= L) ids[s] = -1;
    }
}

__device__ __forceinline__ uint32_t si_mix(uint32_t v) {
    v *= 0x9E3779B1u;
    v ^= v >> 16;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    return v;
}

// the top q bits of v, q in 0..31 (0 bits: 0)
__device__ __forceinline__ uint32_t si_top(uint32_t v, uint32_t q) { return (v >> 1) >> (31u - q); }

template <bool IDS>
__global__ __launch_bounds__(BLOCK) void k_sample_permute(const int32_t* __restrict__ ids, const int64_t* __restrict__ d_count, uint32_t n_out,
                                                          uint32_t seed_lo, uint32_t seed_hi, uint32_t epoch_lo, uint32_t epoch_hi,
                                                          uint32_t stride, int32_t* __restrict__ index) {
    const uint32_t L = (uint32_t)*d_count;
    uint32_t key[8];
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        uint32_t r[4];
        philox4x32_10(epoch_lo, epoch_hi, j, 0u, seed_lo, seed_hi ^ SHUFFLE_KEY_TWEAK, r);
#pragma unroll
        for (int q = 0; q < 4; ++q) key[4 * j + q] = r[q];
    }
    const uint32_t w = L >= 2u ? 32u - (uint32_t)__clz((int)(L - 1u)) : 1u;
    const uint32_t a = w >> 1, c = w - a, low = (1u << c) - 1u;
    for (uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x; i < n_out; i += stride) {
        int32_t v = -1;
        if (i < L) {
            uint32_t x = i;
            if (L >= 2u) {
                do {  // the cycle of the 2^w bijection through i comes back below L: i itself is
                    uint32_t l = x >> c, r = x & low;
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        l ^= si_top(si_mix(r + key[j]), a);
                        r ^= si_top(si_mix(l + key[j + 1]), c);
                    }
                    x = (l << c) | r;
                } while (x >= L);
            }
            v = IDS ? ids[x] : (int32_t)x;
        }
        index[i] = v;
    }
}

const char* const SELECT_WHO = "oc_sample_select";
const char* const PERMUTE_WHO = "oc_sample_permute";
constexpr int64_t SI_LIMIT = (int64_t)1 << 31;

int si_refuse(const char* who, const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail(OC_EINVAL, msg);
}

// the checks that need no array (oc_sample_index_plan makes these alone)
int select_check_shape(int64_t n_samples, bool with_seat) {
    if (n_samples < 0 || n_samples >= SI_LIMIT) return si_refuse(SELECT_WHO, "n_samples must be in 0 .. 2^31 - 1");
    if (with_seat && (n_samples & 1)) return si_refuse(SELECT_WHO, "d_seat needs an even n_samples");
    return OC_OK;
}

int permute_check_shape(int64_t n_out) {
    if (n_out < 0 || n_out >= SI_LIMIT) return si_refuse(PERMUTE_WHO, "n_out must be in 0 .. 2^31 - 1");
    return OC_OK;
}

inline unsigned select_blocks(int64_t n_samples) { return (unsigned)((n_samples + SI_P - 1) / SI_P); }
inline unsigned permute_grid(int64_t n_out) {
    const unsigned g = grid_for(n_out);
    return g < SI_PERM_GRID_MAX ? g : SI_PERM_GRID_MAX;
}

template <bool SEAT, bool ACT>
void select_go(const uint8_t* seat, const uint8_t* actions, uint32_t S, uint32_t* offsets, int64_t* count, int32_t* ids, hipStream_t stream) {
    const unsigned blocks = select_blocks(S);
    hipLaunchKernelGGL((k_sample_count<SEAT, ACT>), dim3(blocks), dim3(BLOCK), 0, stream, seat, actions, S, offsets);
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(BLOCK), 0, stream, offsets, (uint32_t)blocks, count);
    hipLaunchKernelGGL((k_sample_write<SEAT, ACT>), dim3(blocks), dim3(BLOCK), 0, stream, seat, actions, S, (const uint32_t*)offsets,
                       (const int64_t*)count, ids);
}

}  // namespace

extern "C" {

int oc_sample_select(int64_t n_samples, const uint8_t* d_seat, const uint8_t* d_actions, int32_t* d_ids, int64_t* d_count,
                     uint32_t* d_block_offsets, void* stream) {
    if (!d_ids || !d_count || !d_block_offsets) return si_refuse(SELECT_WHO, "NULL d_ids, d_count or d_block_offsets");
    if (((uintptr_t)d_ids | (uintptr_t)d_block_offsets) & 3u) return si_refuse(SELECT_WHO, "d_ids and d_block_offsets must be 4-byte aligned");
    if ((uintptr_t)d_count & 7u) return si_refuse(SELECT_WHO, "d_count must be 8-byte aligned");
    if (int rc = select_check_shape(n_samples, d_seat != nullptr)) return rc;
    const uint32_t S = (uint32_t)n_samples;
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(BLOCK), 0, st, d_block_offsets, 0u, d_count);  // (no pass: the count alone)
    else if (d_seat && d_actions) select_go<true, true>(d_seat, d_actions, S, d_block_offsets, d_count, d_ids, st);
    else if (d_seat) select_go<true, false>(d_seat, d_actions, S, d_block_offsets, d_count, d_ids, st);
    else if (d_actions) select_go<false, true>(d_seat, d_actions, S, d_block_offsets, d_count, d_ids, st);
    else select_go<false, false>(d_seat, d_actions, S, d_block_offsets, d_count, d_ids, st);
    return check_launch(SELECT_WHO);
}

int oc_sample_permute(const int32_t* d_ids, const int64_t* d_count, int64_t n_out, uint64_t seed, uint64_t epoch, int32_t* d_index,
                      void* stream) {
    if (!d_count || !d_index) return si_refuse(PERMUTE_WHO, "NULL d_count or d_index");
    if (((uintptr_t)d_ids | (uintptr_t)d_index) & 3u) return si_refuse(PERMUTE_WHO, "d_ids and d_index must be 4-byte aligned");
    if ((uintptr_t)d_count & 7u) return si_refuse(PERMUTE_WHO, "d_count must be 8-byte aligned");
    if (int rc = permute_check_shape(n_out)) return rc;
    if (n_out == 0) return OC_OK;
    const unsigned grid = permute_grid(n_out);
    const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32), ep_lo = (uint32_t)epoch, ep_hi = (uint32_t)(epoch >> 32);
    if (d_ids)
        hipLaunchKernelGGL(k_sample_permute<true>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, d_ids, d_count, (uint32_t)n_out, seed_lo,
                           seed_hi, ep_lo, ep_hi, (uint32_t)(grid * BLOCK), d_index);
    else
        hipLaunchKernelGGL(k_sample_permute<false>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, d_ids, d_count, (uint32_t)n_out, seed_lo,
                           seed_hi, ep_lo, ep_hi, (uint32_t)(grid * BLOCK), d_index);
    return check_launch(PERMUTE_WHO);
}

int oc_sample_index_plan(int64_t n_samples, int with_seat, int with_actions, int with_ids, int64_t n_out, int64_t n_learner, char* out,
                         size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_sample_index_plan: no output buffer");
    out[0] = 0;
    if (int rc = select_check_shape(n_samples, with_seat != 0)) return rc;
    if (int rc = permute_check_shape(n_out)) return rc;
    if (n_learner < 0 || n_learner >= SI_LIMIT) return fail(OC_EINVAL, "oc_sample_index_plan: n_learner must be in 0 .. 2^31 - 1");
    const unsigned blocks = select_blocks(n_samples);
    const char *seat = with_seat ? "true" : "false", *act = with_actions ? "true" : "false";
    char sel[400], perm[300];
    if (n_samples == 0)
        snprintf(sel, sizeof(sel), "select: k_sample_scan grid=1, %d lanes, 0 pass(es) (no samples: *d_count = 0); P = %d samples per block, scratch 4 B",
                 BLOCK, SI_P);
    else
        snprintf(sel, sizeof(sel),
                 "select: k_sample_count<SEAT=%s, ACT=%s> grid=%u, %d lanes + k_sample_scan grid=1, %d lanes, %u pass(es) of %d blocks, %d passes "
                 "in flight + k_sample_write<SEAT=%s, ACT=%s> grid=%u, %d lanes; P = %d samples per block, scratch %zu B",
                 seat, act, blocks, BLOCK, BLOCK, (blocks + BLOCK - 1) / BLOCK, BLOCK, SI_SCAN_B, seat, act, blocks, BLOCK, SI_P,
                 (size_t)blocks * sizeof(uint32_t));
    int w = 1;
    while (n_learner >= 2 && ((int64_t)1 << w) < n_learner) ++w;  // max(1, the bit length of L - 1)
    if (n_out == 0) snprintf(perm, sizeof(perm), "permute: nothing to launch (no output); L = %lld: w = %d, a = %d, c = %d", (long long)n_learner, w, w >> 1, w - (w >> 1));
    else
        snprintf(perm, sizeof(perm), "permute: k_sample_permute<IDS=%s> grid=%u, %d lanes (one per output, %u output(s) per lane at most); L = %lld: w = %d, a = %d, c = %d",
                 with_ids ? "true" : "false", permute_grid(n_out), BLOCK,
                 (unsigned)((n_out + (int64_t)permute_grid(n_out) * BLOCK - 1) / ((int64_t)permute_grid(n_out) * BLOCK)), (long long)n_learner, w, w >> 1,
                 w - (w >> 1));
    snprintf(out, out_size, "%s; %s", sel, perm);
    return OC_OK;
}

}  // extern "C"
