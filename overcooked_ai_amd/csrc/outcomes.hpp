// outcomes.hpp — episode outcomes of a collected batch by partner member and seat: k_outcomes, k_outcome_sum, oc_outcome_table,
// oc_outcome_plan (include/oc_amd.h: OcOutcomeBatch)
// Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, after common.hpp (BLOCK) and host_util.hpp
// (fail, check_launch, grid_for).  Nothing else of the library is used, and no other kernel or entry point knows of this file.
//
// k_outcomes: one lane per env walking t upwards in blocks of OUT_B steps, k_gae's shape: the one to three bytes per step (done,
// seat, member) of the block above are loaded before the current block is looked at, so that a wavefront has up to OUT_B * 3 byte
// loads in flight.  A block in which no lane of the wavefront is done — nearly every block — costs an OR of its done bytes and one
// ballot.  At a done step the done lanes alone load their 16-byte row of ep_returns (no other row is ever addressed: what the array
// holds elsewhere cannot reach the result) and work out their group; then the wavefront takes the done lanes one after the other,
// in ascending lane order: the lane's group and four floats are broadcast, and lanes 0..7 each update ONE column of the group's row
// in the wavefront's own LDS table [G + 1][8].  Column c of every row is only ever touched by lane c, in program order, so the
// order of the additions is the order of the turns and no lane reads what another lane wrote before the closing barrier.  After the
// barrier the workgroup adds its four wavefront tables in order into d_scratch[blockIdx.x] (every entry is written: what the
// scratch held does not matter), and k_outcome_sum, one wavefront behind it on the stream, adds the workgroups' partials in
// ascending order.  No atomics, no look-back, no spin flags: the same bits every time.
// The per-env table is four f64 registers of the lane, added to at its own done steps in ascending t.
// Cost of the turns: a wavefront whose 64 envs all finish on one step (equal horizons) takes 64 short turns on that step, once
// per horizon; a batch that is done on every step takes a turn per env and step — slow and correct.
#pragma once

namespace {

#ifndef OC_OUT_B
#define OC_OUT_B 16  // (a -D of the measurement builds: profiles/outcomes_prefetch_ab.txt has 8 and 20 beside profiles/outcomes.txt's 16)
#endif
constexpr int OUT_B = OC_OUT_B;                 // steps per prefetch block
constexpr int OUT_SUM_DEPTH = 32;               // partials k_outcome_sum has in flight per lane
constexpr int OUT_COLS = 8;                     // columns of the table
constexpr int OUT_MAX_MEMBERS = 16;             // K
constexpr int OUT_MAX_ROWS = 2 + 2 * OUT_MAX_MEMBERS;  // G + 1 at K = 16

struct OutcomeArgs {
    const uint8_t* done;     // [T][n]
    const float* ep;         // [T][n][4]
    const uint8_t* seat;     // [T][n] or NULL
    const uint8_t* member;   // [T][n] or NULL
    double* partials;        // [gridDim.x][rows][8]
    double* env_table;       // [n][4] or NULL
    int64_t n_steps;
    int n_members;           // K
    int rows;                // G + 1
};

// the bytes of OUT_B steps of one env
struct OutcomeBlock {
    uint32_t d[OUT_B], s[OUT_B], m[OUT_B];
};

// steps [t0, t0 + OUT_B) of env e; a step at or beyond T reads step T - 1 in its place (an address inside the arrays) and counts as
// not done, as does every step of a lane beyond the batch
template <bool SEAT, bool MEMBER>
__device__ __forceinline__ void outcome_load(OutcomeBlock& b, const OutcomeArgs& a, int64_t t0, int64_t e, int64_t n, bool live) {
#pragma unroll
    for (int j = 0; j < OUT_B; ++j) {
        const bool in = t0 + j < a.n_steps;
        const int64_t at = (in ? t0 + j : a.n_steps - 1) * n + e;
        const uint32_t d = a.done[at];
        b.d[j] = in && live ? d : 0u;
        b.s[j] = SEAT ? a.seat[at] : 255u;
        b.m[j] = MEMBER ? a.member[at] : 0u;
    }
}

__device__ __forceinline__ double outcome_start(int c) { return c == 3 ? (double)INFINITY : c == 4 ? -(double)INFINITY : 0.0; }

// acc (op) x of column c: min, max or sum
__device__ __forceinline__ double outcome_join(int c, double acc, double x) { return c == 3 ? fmin(acc, x) : c == 4 ? fmax(acc, x) : acc + x; }

template <bool SEAT, bool MEMBER, bool ENV>
__global__ __launch_bounds__(BLOCK) void k_outcomes(OutcomeArgs a, int64_t n) {
    __shared__ double tab[BLOCK / 64][OUT_MAX_ROWS][OUT_COLS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = a.rows;
    if (lane < OUT_COLS)
        for (int g = 0; g < rows; ++g) tab[w][g][lane] = outcome_start(lane);
    const int64_t e_lane = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = e_lane < n;
    const int64_t e = live ? e_lane : n - 1;  // (a lane beyond the batch reads the last env's bytes and is never done)
    const int64_t T = a.n_steps;
    double ec = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
    const int64_t blocks = (T + OUT_B - 1) / OUT_B;
    OutcomeBlock cur;
    outcome_load<SEAT, MEMBER>(cur, a, 0, e, n, live);
    for (int64_t k = 0; k < blocks; ++k) {
        const int64_t t0 = k * OUT_B;
        OutcomeBlock nxt = cur;
        if (k + 1 < blocks) outcome_load<SEAT, MEMBER>(nxt, a, t0 + OUT_B, e, n, live);  // in flight while this block is looked at
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < OUT_B; ++j) any |= cur.d[j];
        if (__ballot(any != 0) != 0) {
#pragma unroll
            for (int j = 0; j < OUT_B; ++j) {  // (unrolled: cur stays in registers)
                const bool dn = cur.d[j] != 0;
                uint64_t turns = __ballot(dn);
                if (turns == 0) continue;
                // (loading the rows of all done steps of the block before the first is used measured no faster at 65 536 envs and
                // slower at 16 384: docs/NOTEBOOK.md)
                float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                int g = 0;
                if (dn) {
                    r = reinterpret_cast<const float4*>(a.ep)[(t0 + j) * n + e];
                    if (SEAT) {
                        const uint32_t s = cur.s[j], m = cur.m[j];
                        g = s == 255u ? 0 : (s <= 1u && m < (uint32_t)a.n_members) ? 1 + 2 * (int)m + (int)s : rows - 1;
                    }
                    if (ENV) {
                        const double R = (double)r.x + (double)r.y;
                        ec += 1.0;
                        e1 += R;
                        e2 += R * R;
                        e3 += (double)r.z + (double)r.w;
                    }
                }
                while (turns) {  // (uniform: the done lanes in ascending order)
                    const int l = __builtin_ctzll(turns);
                    turns &= turns - 1;
                    const int gl = __shfl(g, l, 64);
                    const float s0 = __shfl(r.x, l, 64), s1 = __shfl(r.y, l, 64), h0 = __shfl(r.z, l, 64), h1 = __shfl(r.w, l, 64);
                    if (lane < OUT_COLS && (gl != rows - 1 || lane == 0)) {  // (the unattributed row: its count alone)
                        const double R = (double)s0 + (double)s1;
                        const double x = lane == 0 ? 1.0 : lane == 2 ? R * R : lane == 5 ? (double)h0 : lane == 6 ? (double)h1 : lane == 7 ? (double)s0 : R;
                        tab[w][gl][lane] = outcome_join(lane, tab[w][gl][lane], x);
                    }
                }
            }
        }
        cur = nxt;
    }
    if (ENV && live) {
        double* row = a.env_table + e * 4;
        row[0] = ec;
        row[1] = e1;
        row[2] = e2;
        row[3] = e3;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * OUT_COLS; i += BLOCK) {
        const int c = i & (OUT_COLS - 1);
        double v = outcome_start(c);
#pragma unroll
        for (int q = 0; q < BLOCK / 64; ++q) v = outcome_join(c, v, tab[q][i >> 3][c]);
        a.partials[(int64_t)blockIdx.x * rows * OUT_COLS + i] = v;
    }
}

// table[i] = start (op) partials[0][i] (op) partials[1][i] ... in ascending order: lane i, i + 64, ... of one wavefront,
// OUT_SUM_DEPTH loads at a time (one wavefront has nothing else to hide their latency with: at 256 partials eight at a time took
// 32 round trips, about 40 us); count == 0 writes the empty table
__global__ __launch_bounds__(64) void k_outcome_sum(const double* __restrict__ partials, int64_t count, int rows, double* __restrict__ table) {
    const int cells = rows * OUT_COLS;
    for (int i = threadIdx.x; i < cells; i += 64) {
        const int c = i & (OUT_COLS - 1);
        double v = outcome_start(c);
        for (int64_t k0 = 0; k0 < count; k0 += OUT_SUM_DEPTH) {
            double x[OUT_SUM_DEPTH];
#pragma unroll
            for (int j = 0; j < OUT_SUM_DEPTH; ++j) x[j] = k0 + j < count ? partials[(k0 + j) * cells + i] : 0.0;
#pragma unroll
            for (int j = 0; j < OUT_SUM_DEPTH; ++j)
                if (k0 + j < count) v = outcome_join(c, v, x[j]);
        }
        table[i] = v;
    }
}

const char* const OUTCOME_WHO = "oc_outcome_table";

int outcome_refuse(const char* why) {
    char msg[sizeof(g_err)];
    snprintf(msg, sizeof(msg), "%s: %s", OUTCOME_WHO, why);
    return fail(OC_EINVAL, msg);
}

// the checks that need no array (oc_outcome_plan makes these alone)
int outcome_check_shape(int64_t n_envs, int64_t n_steps, bool seat, bool member, int n_members) {
    if (n_steps < 1) return outcome_refuse("n_steps < 1");
    if (n_envs < 0) return outcome_refuse("n_envs < 0");
    if (n_envs > 0 && n_steps > ((int64_t)1 << 31) / n_envs) return outcome_refuse("n_steps * n_envs must be below 2^31");
    if (n_steps * n_envs >= ((int64_t)1 << 31)) return outcome_refuse("n_steps * n_envs must be below 2^31");
    if (member && !seat) return outcome_refuse("d_member needs d_seat");
    if (n_members < 1 || n_members > OUT_MAX_MEMBERS) return outcome_refuse("n_members must be in 1..16");
    if (!member && n_members != 1) return outcome_refuse("n_members must be 1 without d_member");
    return OC_OK;
}

int outcome_rows(bool seat, int n_members) { return (seat ? 1 + 2 * n_members : 1) + 1; }  // G + 1

int outcome_check(const OcOutcomeBatch* q) {
    if (!q) return outcome_refuse("batch is NULL");
    if (!q->d_table) return outcome_refuse("NULL d_table");
    if (q->n_envs > 0 && (!q->d_done || !q->d_ep_returns || !q->d_scratch)) return outcome_refuse("NULL d_done, d_ep_returns or d_scratch");
    if ((uintptr_t)q->d_ep_returns & 15u) return outcome_refuse("d_ep_returns must be 16-byte aligned");
    if (((uintptr_t)q->d_table | (uintptr_t)q->d_env_table | (uintptr_t)q->d_scratch) & 7u)
        return outcome_refuse("d_table, d_env_table and d_scratch must be 8-byte aligned");
    return outcome_check_shape(q->n_envs, q->n_steps, q->d_seat != nullptr, q->d_member != nullptr, q->n_members);
}

template <bool SEAT, bool MEMBER>
void outcome_go(const OutcomeArgs& a, int64_t n, hipStream_t stream) {
    if (a.env_table) hipLaunchKernelGGL((k_outcomes<SEAT, MEMBER, true>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, a, n);
    else hipLaunchKernelGGL((k_outcomes<SEAT, MEMBER, false>), dim3(grid_for(n)), dim3(BLOCK), 0, stream, a, n);
}

}  // namespace

extern "C" {

int oc_outcome_table(const OcOutcomeBatch* q, void* stream) {
    if (int rc = outcome_check(q)) return rc;
    const int64_t n = q->n_envs;
    const int rows = outcome_rows(q->d_seat != nullptr, q->n_members);
    if (n > 0) {
        OutcomeArgs a;
        a.done = q->d_done; a.ep = q->d_ep_returns; a.seat = q->d_seat; a.member = q->d_member;
        a.partials = q->d_scratch; a.env_table = q->d_env_table;
        a.n_steps = q->n_steps; a.n_members = q->n_members; a.rows = rows;
        if (a.member) outcome_go<true, true>(a, n, (hipStream_t)stream);
        else if (a.seat) outcome_go<true, false>(a, n, (hipStream_t)stream);
        else outcome_go<false, false>(a, n, (hipStream_t)stream);
    }
    hipLaunchKernelGGL(k_outcome_sum, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)q->d_scratch, (int64_t)(n > 0 ? grid_for(n) : 0), rows,
                       q->d_table);
    return check_launch(OUTCOME_WHO);
}

int oc_outcome_plan(int64_t n_envs, int64_t n_steps, int with_seat, int with_member, int n_members, int with_env_table, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_outcome_plan: no output buffer");
    out[0] = 0;
    if (int rc = outcome_check_shape(n_envs, n_steps, with_seat != 0, with_member != 0, n_members)) return rc;
    const int rows = outcome_rows(with_seat != 0, n_members);
    if (n_envs == 0)
        snprintf(out, out_size, "k_outcome_sum grid=1, 64 lanes (no envs: the empty table); G = %d group(s), table %d B, scratch 0 B", rows - 1,
                 rows * OUT_COLS * 8);
    else
        snprintf(out, out_size,
                 "k_outcomes<SEAT=%s, MEMBER=%s, ENV=%s> grid=%u, %d lanes (one per env; one partial per block of %d envs), %d steps per prefetch "
                 "block, %lld block(s) + k_outcome_sum grid=1, 64 lanes; G = %d group(s), table %d B, scratch %lld B",
                 with_seat ? "true" : "false", with_member ? "true" : "false", with_env_table ? "true" : "false", grid_for(n_envs), BLOCK, BLOCK,
                 OUT_B, (long long)((n_steps + OUT_B - 1) / OUT_B), rows - 1, rows * OUT_COLS * 8,
                 (long long)grid_for(n_envs) * rows * OUT_COLS * 8);
    return OC_OK;
}

}  // extern "C"
