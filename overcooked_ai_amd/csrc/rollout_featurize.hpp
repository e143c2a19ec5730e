// rollout_featurize.hpp — K transitions WITH the featurize_state observation of every step: k_rollout_featurize
// Part of liboc_amd.so: included by oc_amd.hip inside its anonymous namespace, after rollout_encode.hpp and featurize.hpp.
#pragma once

// ------------------------------------------------------------------------------------------
// k_rollout_featurize: the trajectory a behaviour-cloning data collection or evaluation rollout gathers — per step the
// reward, the flag and featurize_state (mdp.py:2579-2898) of both players — for a batch with ONE two-player layout of at
// most 64 cells and one or two pots, random policy or caller-supplied actions.
//
// Two launches per step (a one-step kernel, then k_featurize) pay two launch latencies and k_featurize's state round trip
// (4.6 of its 12.8 us on 65 536 envs, docs/NOTEBOOK.md round 6, 5b).  Here the env stays with its lane for all K steps
// exactly as in k_rollout_encode (Env3 in registers + [cell][lane] words in LDS), and after each step every WAVEFRONT
// featurizes its own 64 envs by itself:
//   * the wire-format header of each env (players, timestep, pot ticks) goes to a 16-byte LDS slot, the pots' soup codes
//     back into their cell words — then any lane can read any env of its wavefront;
//   * per sub-group of G envs: lane = (env, player) computes the rows of k_featurize (featurize_rows, featurize.hpp: the
//     arithmetic exists once) from the header, the layout's walk records and cost rows in the plan blob (through L2) and
//     the few object bytes it needs from the cell words, into the wavefront's private int16 LDS image (k_featurize's
//     odd-dword row stride); the image is streamed to its place in features[step] as contiguous 16-byte float4 stores —
//     a wavefront's 64 envs are one contiguous range of 64 * 2 * total * 4 bytes per step.
// No workgroup barrier in the step loop: LDS operations of one wavefront execute in order, so they need only wave_fence().
// An image holds RF_GROUP = 32 envs: the 64 lanes are the (env, player) tasks of one pass, a wavefront makes two passes per step.
// 65 536 envs, num_pots = 2: 9.4 us per step against 23.7 us for the two one-step launches (docs/NOTEBOOK.md 4.7b).
// ------------------------------------------------------------------------------------------

// the state of one env as the step loop keeps it: its wire header and its column of the [cell][lane] words
struct FeatCellState {
    uint4 h;             // pos0 | or0 << 8 | held0 << 16 | pos1 << 24 ; or1 | held1 << 8 | t << 16 ; pot ticks ; -
    const uint16_t* wc;  // cell c: wc[c * BLOCK], object in the low byte
    __device__ __forceinline__ uint32_t pos(uint32_t p) const { return p == 0u ? (h.x & 0xFFu) : (h.x >> 24); }
    __device__ __forceinline__ uint32_t ori(uint32_t p) const { return p == 0u ? ((h.x >> 8) & 0xFFu) : (h.y & 0xFFu); }
    __device__ __forceinline__ uint32_t held(uint32_t p) const { return p == 0u ? ((h.x >> 16) & 0xFFu) : ((h.y >> 8) & 0xFFu); }
    __device__ __forceinline__ uint32_t obj(uint32_t c) const { return wc[c * BLOCK] & 0xFFu; }
    __device__ __forceinline__ uint32_t obj_dword(uint32_t j) const {  // the object bytes of cells 4j .. 4j + 3
        const uint32_t c0 = wc[(4u * j + 0u) * BLOCK], c1 = wc[(4u * j + 1u) * BLOCK];
        const uint32_t c2 = wc[(4u * j + 2u) * BLOCK], c3 = wc[(4u * j + 3u) * BLOCK];
        return (c0 & 0xFFu) | ((c1 & 0xFFu) << 8) | ((c2 & 0xFFu) << 16) | (c3 << 24);
    }
    __device__ __forceinline__ uint32_t tick(uint32_t slot) const { return (h.z >> (8u * (slot & 3u))) & 0xFFu; }  // (at most two pots)
};

// floats of one (env, player) row, shorts of its row in the LDS image (featurize.hpp: an odd number of dwords)
__host__ __device__ constexpr int feat_total(int num_pots) { return 2 * (num_pots * 10 + 26) + 4; }
__host__ __device__ constexpr int feat_row_shorts(int num_pots) { return feat_total(num_pots) + 2; }
constexpr int RF_GROUP = 32;  // envs per image
// shorts of one wavefront's image: [RF_GROUP][2][row], whole 16-byte units
__host__ __device__ constexpr size_t feat_image_shorts(int num_pots) {
    return ((size_t)RF_GROUP * 2 * feat_row_shorts(num_pots) + 7) & ~(size_t)7;
}

template <int MAXP, int FAST>
__global__ __launch_bounds__(BLOCK) void k_rollout_featurize(const OcLayout* __restrict__ g_layouts, uint4* st,
                                                             const uint8_t* __restrict__ actions,
                                                             float4* __restrict__ rewards, uint8_t* __restrict__ flags,
                                                             float4* __restrict__ ep_returns,
                                                             const uint8_t* __restrict__ plan_blob,
                                                             const uint32_t* __restrict__ plan_off,
                                                             uint8_t* __restrict__ feat_bytes, int64_t feat_step_stride,
                                                             int64_t n, int W, int H, int n_obj, int num_pots, int horizon,
                                                             uint32_t options, uint32_t seed_lo, uint32_t seed_hi,
                                                             int64_t env_offset, int64_t t0, int n_steps,
                                                             StartArgs sa) {
    extern __shared__ __attribute__((aligned(16))) uint16_t s_cells3[];  // [n_obj * 16][BLOCK], then the headers and the images
    __shared__ uint4 s_lay[16];
    __shared__ uint2 s_lut[2 * LUT_ENTRIES];
    __shared__ uint8_t s_move[FAST == 3 ? 64 * 8 : 8];
    const int total = feat_total(num_pots), rs = feat_row_shorts(num_pots);
    uint4* s_hdr = reinterpret_cast<uint4*>(s_cells3 + (size_t)n_obj * 16 * BLOCK);  // [BLOCK] wire-format plane 0 of each env
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int16_t* img = reinterpret_cast<int16_t*>(s_hdr + BLOCK) + (size_t)wave * feat_image_shorts(num_pots);  // [RF_GROUP][2][rs]

    const uint32_t blk = xcd_block();  // (common.hpp: each XCD owns a contiguous eighth of the envs — and of every step's features)
    const int64_t e = (int64_t)blk * BLOCK + threadIdx.x;
    const bool active = e < n;
    // caller actions: the first step's are requested before the tables are staged, step k + 1's while step k is featurized
    uint32_t a01_next = (actions && active && n_steps > 0) ? reinterpret_cast<const uint16_t*>(actions)[e] : 0u;
    for (int i = threadIdx.x; i < 2 * LUT_ENTRIES; i += BLOCK) s_lut[i] = reinterpret_cast<const uint2*>(&g_lut)[i];
    const Lay L = stage_layouts<true>(g_layouts, 1, nullptr, e, active, s_lay);  // contains the barrier
    if (FAST == 3) {  // MOVE[cell * 8 + action] for the batch's single layout (at most 64 cells)
        const int nc = (int)L.u8(L_NCELLS);
        for (int i = threadIdx.x; i < nc * 8; i += BLOCK) {
            const int c = i >> 3, a = i & 7;
            int t = c;
            if (a < 4) {
                const int t2 = c + (a == 0 ? -W : a == 1 ? W : a == 2 ? 1 : -1);
                if (t2 >= 0 && t2 < nc && (L.terrain((uint32_t)t2) & 7u) == OC_T_FLOOR) t = t2;
            }
            s_move[i] = (uint8_t)t;
        }
    }
    __syncthreads();  // the last workgroup barrier: from here on every wavefront runs by itself
    const int64_t wave_e0 = (int64_t)blk * BLOCK + (int64_t)wave * 64;
    const int n_wave = (int)max((int64_t)0, min((int64_t)64, n - wave_e0));  // envs of this wavefront
    if (n_wave == 0) return;

    uint16_t* cells = s_cells3 + threadIdx.x;
    const LayC C = load_consts<true>(L);
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(s_lut) + (C.old_dyn ? LUT_ENTRIES * 8 : 0);
    const uint32_t delta4 = make_delta4(W);
    Env3<MAXP> s;
    float4 ep = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        load_env3<MAXP>(C, L, st, n, e, n_obj, s, cells);
        if (ep_returns) ep = ep_returns[e];
    }
    const uint64_t g = (uint64_t)(env_offset + e);
    const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
    uint32_t rnd[4] = {0, 0, 0, 0};
    const uint16_t* wcells = s_cells3 + wave * 64;  // cell c of this wavefront's env l: wcells[c * BLOCK + l]
    const uint4* whdr = s_hdr + wave * 64;
    const uint8_t* plan = plan_blob + plan_off[0];  // the layout's cost rows and walk section (one layout)
    const uint8_t* wsec = plan_blob + plan_off[1];
    const uint32_t q_per_row = (uint32_t)total / 4u;
    const uint32_t magic = 0xFFFFFFFFu / q_per_row + 1u;  // i / q_per_row == mulhi(i, magic) for i < 2^16

    for (int k = 0; k < n_steps; ++k) {
        // ---- the transition (get_state_transition + OvercookedEnv.step bookkeeping), as k_rollout_encode does it
        if (active) {
            uint32_t a0, a1;
            if (actions) {
                const uint32_t a01 = a01_next;
                if (k + 1 < n_steps) a01_next = reinterpret_cast<const uint16_t*>(actions)[(int64_t)(k + 1) * n + e];
                a0 = a01 & 0xFFu; a1 = a01 >> 8;
            } else {
                const uint64_t t = (uint64_t)(t0 + k);
                const uint32_t s8 = (uint32_t)t & 7u;
                if (k == 0 || s8 == 0u) {
                    const uint64_t blk = t >> 3;
                    philox4x32_10((uint32_t)blk, g_lo, g_hi, (uint32_t)(blk >> 32), seed_lo, seed_hi, rnd);
                }
                draw_actions(rnd, s8, a0, a1);
            }
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t fl;
            if (__builtin_expect(a0 > 5u || a1 > 5u, 0)) {
                fl = OC_F_BAD_ACTION;  // mdp.py:1394-1398 raises: the env stays untouched
            } else {
                env_step3<MAXP, FAST>(C, L, lut, cells, s, delta4, a0, a1, r, 0ull, s_move);
                fl = finish_step3<MAXP>(C, L, n_obj, cells, s, horizon, options, r, ep, sa, g, sa.epoch + (uint32_t)k);
            }
            if (rewards) rewards[(int64_t)k * n + e] = r;
            if (flags) flags[(int64_t)k * n + e] = (uint8_t)fl;
            // what the features need from this lane's registers: the wire header, the pots' soup codes in the grid
            uint4 h;
            h.x = s.pos0 | (s.or0 << 8) | (s.held0 << 16) | (s.pos1 << 24);
            h.y = s.or1 | (s.held1 << 8) | (min(s.t, 0xFFFFu) << 16);
            h.z = 0; h.w = 0;
#pragma unroll
            for (int p = 0; p < MAXP; ++p) {
                if ((uint32_t)p < C.n_pots) {
                    wr_obj3(cells, L.pot_cell(p), s.ps[p]);
                    h.z |= s.tk[p] << (8 * (p & 3));
                }
            }
            s_hdr[threadIdx.x] = h;
        }
        wave_fence();

        // ---- featurize_state of this wavefront's envs, RF_GROUP at a time through its private LDS image
        float* feat_k = reinterpret_cast<float*>(feat_bytes + (int64_t)k * feat_step_stride);
        for (int l0 = 0; l0 < n_wave; l0 += RF_GROUP) {
            const int ne = min(RF_GROUP, n_wave - l0);
            if (lane < 2 * ne) {  // lane = (env, player)
                const int le = lane >> 1;
                const uint32_t p = (uint32_t)lane & 1u;
                const FeatCellState fs = {whdr[l0 + le], wcells + l0 + le};
                featurize_rows(fs, L, plan, wsec, W, n_obj + 1, num_pots, p, img + ((size_t)le * 2 + p) * rs,
                               img + ((size_t)le * 2 + (1u - p)) * rs);
            }
            wave_fence();
            // rows are contiguous in the output: stream them out as 16-byte stores (total is a multiple of 4)
            const uint32_t n_q = (uint32_t)ne * 2u * q_per_row;
            float4* gdst = reinterpret_cast<float4*>(feat_k + (size_t)(wave_e0 + l0) * 2 * total);
            for (uint32_t i = (uint32_t)lane; i < n_q; i += 64u) {
                const uint32_t row = __umulhi(i, magic), col = i - row * q_per_row;
                const uint32_t* src = reinterpret_cast<const uint32_t*>(img + (size_t)row * rs + 4u * col);
                const uint32_t w0 = src[0], w1 = src[1];
                gdst[i] = make_float4((float)(int16_t)(w0 & 0xFFFFu), (float)((int32_t)w0 >> 16),
                                      (float)(int16_t)(w1 & 0xFFFFu), (float)((int32_t)w1 >> 16));
            }
            wave_fence();
        }
    }
    if (active) {
        store_env3<MAXP>(C, L, st, n, e, n_obj, s, cells);
        if (ep_returns) ep_returns[e] = ep;
    }
}
