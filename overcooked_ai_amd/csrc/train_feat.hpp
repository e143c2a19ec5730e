// train_feat.hpp — the batched step of the RLlib training environment WITH the featurize_state observation, one kernel: k_train_step_feat
// Part of liboc_amd.so: included by oc_amd.hip inside its anonymous namespace after train_obs.hpp (one_header, phi_record), which
// follows shaping.hpp (k_train_step1), featurize.hpp (featurize_rows), rollout_featurize.hpp (feat_total, feat_row_shorts),
// rollout_encode.hpp (wave_fence) and potential.hpp (potential2_core).
#pragma once

// ------------------------------------------------------------------------------------------
// k_train_step_feat: OvercookedMultiAgent.step (human_aware_rl/rllib/rllib.py:293-342) for a batch with ONE two-player layout whose
// agents observe featurize_state (mdp.py:2579-2898, the "bc" observation) — the transition (get_state_transition, mdp.py:1375),
// phi(s') and the shaped rewards, the restart of finished envs, and the features of the states the next step starts from — in one
// launch.  As two kernels (k_train_step1, then k_featurize) the step pays two launches and k_featurize's state round trip (4.6 of
// its 12.8 us on 65 536 envs, docs/NOTEBOOK.md round 6, 5b).  The shape is k_train_step_obs's head joined to k_rollout_featurize's
// tail.  A workgroup of EIGHT wavefronts owns 256 envs:
//   * wavefronts 0..3 (owners, lane = env) run k_train_step1's transition on the wire format, restart finished envs, store the
//     state, and leave in LDS the new object planes (their own rows), the new header, a record of s' before any restart and the
//     reward quad — the head of k_train_step_obs, restated here so that that kernel's instances keep their registers;
//   * after ONE workgroup barrier, wavefronts 4..7 (helpers, same lane = env) compute phi(s') and the shaped rewards from those
//     records while the owners already featurize;
//   * the features of a wavefront's 64 envs are produced in sub-groups of G envs: lane = (env, player) computes the rows of
//     k_featurize (featurize_rows, featurize.hpp: the arithmetic exists once) from the header and the object rows in LDS, the
//     layout's walk records and cost rows in the feature plan blob (through L2), into the wavefront's PRIVATE int16 image
//     (k_featurize's odd-dword row stride), and the image is streamed to its place as contiguous 16-byte float4 stores, with
//     wave-level fences only; owner w and helper w claim the sub-groups of owner w's envs from one LDS counter.
// Same outputs, bit for bit, as k_train_step1 + k_featurize (tests/test_gpu_train_featurize.py compares the two).
// SAMPLE (with one more argument, a SampleArgs): the owners draw both actions from the policy's logits (sample.hpp) and store them
// with their log-probabilities before they step.
// ------------------------------------------------------------------------------------------

// The state of one env as the head leaves it in LDS: its new wire header and its 16-byte row of every object plane
struct FeatRowState {
    uint4 h;            // pos0 | or0 << 8 | held0 << 16 | pos1 << 24 ; or1 | held1 << 8 | t << 16 ; pot ticks ; -
    const uint4* rows;  // object plane p of this env: rows[p * BLOCK]
    __device__ __forceinline__ uint32_t pos(uint32_t p) const { return p == 0u ? (h.x & 0xFFu) : (h.x >> 24); }
    __device__ __forceinline__ uint32_t ori(uint32_t p) const { return p == 0u ? ((h.x >> 8) & 0xFFu) : (h.y & 0xFFu); }
    __device__ __forceinline__ uint32_t held(uint32_t p) const { return p == 0u ? ((h.x >> 16) & 0xFFu) : ((h.y >> 8) & 0xFFu); }
    __device__ __forceinline__ uint32_t obj(uint32_t c) const { return reinterpret_cast<const uint8_t*>(rows + (c >> 4) * BLOCK)[c & 15u]; }
    __device__ __forceinline__ uint32_t obj_dword(uint32_t j) const { return reinterpret_cast<const uint32_t*>(rows + (j >> 2) * BLOCK)[j & 3u]; }
    __device__ __forceinline__ uint32_t tick(uint32_t slot) const { return (h.z >> (8u * (slot & 3u))) & 0xFFu; }  // (at most two pots)
};

constexpr int TF_WAVES = 8;  // wavefronts per workgroup: four owners, four helpers
// shorts of one wavefront's image of `group_envs` envs: [group_envs][2][row], whole 16-byte units
__host__ __device__ constexpr size_t train_feat_image_shorts(int group_envs, int num_pots) {
    return ((size_t)group_envs * 2 * feat_row_shorts(num_pots) + 7) & ~(size_t)7;
}
// dynamic LDS of a launch: rows | header | records before and after the restart | rewards | one image per wavefront
__host__ __device__ constexpr size_t train_feat_lds(int n_obj, int group_envs, int num_pots) {
    return ((size_t)n_obj + 4) * BLOCK * 16 + (size_t)TF_WAVES * train_feat_image_shorts(group_envs, num_pots) * sizeof(int16_t);
}

template <int MAXP, bool SAMPLE = false, typename... SMP>
__global__ __launch_bounds__(TF_WAVES * 64) void k_train_step_feat(
    const OcLayout* __restrict__ g_layouts, uint4* st, const uint8_t* __restrict__ actions, float4* __restrict__ rewards,
    uint8_t* __restrict__ flags, float4* ep_returns, float4* __restrict__ ep_out, const uint8_t* __restrict__ plan_blob,
    const uint32_t* __restrict__ plan_off, const uint8_t* __restrict__ phi_tables, double* __restrict__ phi_next,
    double* __restrict__ phi_cur, const double* __restrict__ phi_start, double factor, double* __restrict__ shaped,
    uint8_t* __restrict__ done, const uint8_t* __restrict__ feat_plan_blob, const uint32_t* __restrict__ feat_plan_off,
    float* __restrict__ features, int64_t n, int W, int H, int n_obj, int num_pots, int horizon, int group_envs, StartArgs sa,
    SMP... smp) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint4 s_dyn[];  // rows | header | records | rewards | images
    __shared__ uint4 s_lay[16];
    __shared__ uint2 s_lut[2 * LUT_ENTRIES];
    __shared__ uint32_t s_next[4];    // per owner wavefront: the next sub-group of its envs nobody has taken yet
    uint4* s_rows = s_dyn;                                     // [n_obj][BLOCK]: object planes, one 16-byte row per env
    uint4* s_hdr = s_rows + (size_t)n_obj * BLOCK;             // [BLOCK] header of the state the next step starts from
    uint4* s_pre = s_hdr + BLOCK;                              // [BLOCK] phi_record of s' before any restart
    uint4* s_post = s_pre + BLOCK;                             // [BLOCK] phi_record of a DRAWN start state
    float4* s_rw = reinterpret_cast<float4*>(s_post + BLOCK);  // [BLOCK] the step's reward quad
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int16_t* img = reinterpret_cast<int16_t*>(s_rw + BLOCK) + (size_t)wave * train_feat_image_shorts(group_envs, num_pots);  // [group_envs][2][rs]
    const bool owner = threadIdx.x < BLOCK;
    const int ow = wave & 3;
    const uint32_t tid = threadIdx.x & (BLOCK - 1);
    const uint32_t blk = xcd_block();  // (common.hpp: each XCD owns a contiguous eighth of the envs and of the features)
    const int64_t e = (int64_t)blk * BLOCK + tid;
    const bool active = e < n;
    const int64_t el = active ? e : n - 1;
    // ---- everything the step reads, requested before the first wait (owners); the helpers ask for phi(s)
    OneIn in;
    double phi_before = 0.0;
    if (owner) {
        in = one_load(st, actions, ep_returns, n, el, n_obj);
        if constexpr (SAMPLE) in.a01 = sample_env(first_of(smp...), el, active);  // (`actions` is then where the draws go)
    }
    else if (phi_tables) phi_before = phi_cur[el];
    for (int i = threadIdx.x; i < 2 * LUT_ENTRIES; i += TF_WAVES * 64) s_lut[i] = reinterpret_cast<const uint2*>(&g_lut)[i];
    if (threadIdx.x < 16) s_lay[threadIdx.x] = reinterpret_cast<const uint4*>(g_layouts)[threadIdx.x];
    if (threadIdx.x < 4) s_next[threadIdx.x] = 0u;
    __syncthreads();
    const Lay L{reinterpret_cast<const uint8_t*>(s_lay)};
    const LayC C = load_consts<true>(L);
    if (owner && active) {
        // ---- the transition on the wire format (k_train_step1), the restart, the state written once
#pragma unroll
        for (int p = 0; p < STEP1_MAX_PLANES; ++p)
            if (p < n_obj) s_rows[p * BLOCK + tid] = in.v[p];
        uint8_t* row = reinterpret_cast<uint8_t*>(s_rows + tid);
        const uint8_t* lut = reinterpret_cast<const uint8_t*>(s_lut) + (C.old_dyn ? LUT_ENTRIES * 8 : 0);
        One<MAXP> q;
        one_decode<MAXP>(C, L, in.h, row, q);
        Env3<MAXP>& s = q.s;
        const uint32_t a0 = in.a01 & 0xFFu, a1 = in.a01 >> 8;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f), ep = in.ep;
        uint32_t fl = 0;
        if (a0 > 5u || a1 > 5u) {
            fl = OC_F_BAD_ACTION;  // the env stays untouched (mdp.py:1394-1398 raises)
        } else {
            one_transition<MAXP>(C, L, lut, make_delta4(W), a0, a1, in.v, n_obj, row, q, r);
            ep.x += r.x; ep.y += r.y; ep.z += r.z; ep.w += r.w;
            if ((int)s.t >= horizon) fl |= OC_F_DONE;
        }
        const bool is_done = (fl & OC_F_DONE) != 0u;
        s_pre[tid] = phi_record<MAXP>(s, fl, (is_done && sa.enabled) ? 1u : 0u);
        s_rw[tid] = r;
        done[e] = is_done ? 1 : 0;
        if (ep_out) ep_out[e] = ep;
        if (!phi_tables) {  // the shaped rewards of the step itself (no potential: nothing for the helpers to compute)
            const double sparse = (double)r.x + (double)r.y;
            reinterpret_cast<double2*>(shaped)[e] = make_double2(sparse + factor * (double)r.z, sparse + factor * (double)r.w);
        }
        if (is_done) {  // the next episode: the standard start state, or one drawn from the batch's start_state_fn
            one_restart<MAXP>(C, L, sa, (uint64_t)(sa.env_offset + e), s);
            if (sa.enabled) s_post[tid] = phi_record<MAXP>(s, 0u, 0u);
            ep = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        one_store<MAXP>(C, L, st, n, e, n_obj, q, is_done, row);  // header + every plane, the planes left in this lane's rows
        s_hdr[tid] = one_header<MAXP>(C, s);
        rewards[e] = r;
        flags[e] = (uint8_t)fl;
        if (ep_returns) ep_returns[e] = ep;
    }
    __syncthreads();  // the only barrier behind the staging one: rows, headers and records are in LDS
    if (!owner && active && phi_tables) {
        // ---- phi(s'), the shaped rewards, phi(s) of the next step (k_train_step1's arithmetic, from the records)
        const Phi Tb{phi_tables};
        const uint8_t* plan = plan_blob + plan_off[0];
        auto phi_of = [&](const uint4 rec) {
            return potential2_core(L, Tb, plan, (uint32_t)(W * H), 2u, rec.x & 0xFFu, (rec.x >> 8) & 0xFFu, (rec.x >> 16) & 0xFFu,
                                   rec.x >> 24, rec.y & 0xFFu, (rec.y >> 8) & 0xFFu, (rec.y >> 16) & 0xFFu, rec.y >> 24,
                                   rec.z & 0xFFu, (rec.z >> 8) & 0xFFu);
        };
        const uint4 pre = s_pre[tid];
        const float4 r = s_rw[tid];
        const bool is_done = ((pre.z >> 16) & OC_F_DONE) != 0u;
        const double pn = phi_of(pre);
        const double sparse = (double)r.x + (double)r.y;
        const double d = pn - phi_before;
        phi_next[e] = pn;
        double pc = is_done ? phi_start[0] : pn;
        if ((pre.z >> 24) != 0u) pc = phi_of(s_post[tid]);  // a drawn start state: phi(s) of the next step is ITS potential
        phi_cur[e] = pc;
        reinterpret_cast<double2*>(shaped)[e] = make_double2(sparse + factor * d, sparse + factor * d);
    }
    // ---- featurize_state of the owner wavefront's 64 envs, sub-group by sub-group, owner and helper taking turns
    const int64_t wave_e0 = (int64_t)blk * BLOCK + (int64_t)ow * 64;
    const int n_wave = (int)max((int64_t)0, min((int64_t)64, n - wave_e0));
    const int n_groups = (n_wave + group_envs - 1) / group_envs;
    const int total = feat_total(num_pots), rs = feat_row_shorts(num_pots);
    const uint8_t* fplan = feat_plan_blob + feat_plan_off[0];  // the layout's cost rows and walk section (one layout)
    const uint8_t* wsec = feat_plan_blob + feat_plan_off[1];
    const uint32_t q_per_row = (uint32_t)total / 4u;
    const uint32_t magic = 0xFFFFFFFFu / q_per_row + 1u;  // i / q_per_row == mulhi(i, magic) for i < 2^16
    for (;;) {
        uint32_t g = 0;
        if (lane == 0) g = atomicAdd(&s_next[ow], 1u);
        g = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        if ((int)g >= n_groups) break;
        const int l0 = (int)g * group_envs;
        const int ne = min(group_envs, n_wave - l0);
        if (lane < 2 * ne) {  // lane = (env, player)
            const int le = lane >> 1;
            const uint32_t p = (uint32_t)lane & 1u;
            const int l = ow * 64 + l0 + le;
            const FeatRowState fs = {s_hdr[l], s_rows + l};
            featurize_rows(fs, L, fplan, wsec, W, n_obj + 1, num_pots, p, img + ((size_t)le * 2 + p) * rs,
                           img + ((size_t)le * 2 + (1u - p)) * rs);
        }
        wave_fence();
        // rows are contiguous in the output: stream them out as 16-byte stores (total is a multiple of 4)
        const uint32_t n_q = (uint32_t)ne * 2u * q_per_row;
        float4* gdst = reinterpret_cast<float4*>(features + (size_t)(wave_e0 + l0) * 2 * total);
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
