// stores_only.hpp — the store-rate yardstick of the rollout kernels (oc_output_stores_only, include/oc_amd.h); included by
// oc_amd.hip inside its anonymous namespace, after every other kernel header.
#pragma once

// oc_output_stores_only: the output stores of a rollout and nothing else (include/oc_amd.h) — one store of each kind per step,
// in step order, through (row pointer of the step, lane offset) exactly as k_rollout4 addresses its rows
__global__ __launch_bounds__(BLOCK) void k_output_stores_only(float4* __restrict__ rewards, uint8_t* __restrict__ flags, int64_t n,
                                                              int n_steps) {
    const uint32_t blk = xcd_block();  // (as k_rollout4: each XCD owns a contiguous eighth of the envs)
    const int64_t e = (int64_t)blk * BLOCK + threadIdx.x;
    if (e >= n) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* rew_k = rewards + (int64_t)blk * BLOCK;                      // wave-uniform row pointers
    uint8_t* flg_k = flags ? flags + (int64_t)blk * BLOCK : nullptr;
#pragma unroll 1
    for (int k = 0; k < n_steps; ++k) {
        stream_store16(reinterpret_cast<uint4*>(rew_k + threadIdx.x), make_uint4(0u, 0u, 0u, 0u));  // (as k_rollout4 stores them beside [step][env] flags)
        if (flg_k) { flg_k[threadIdx.x] = 0; flg_k += n; }
        rew_k += n;
    }
}
// ... with the flags array tiled by 8 steps (OC_OPT_FLAGS_TILED8): per block of 8 steps eight reward rows and ONE 8-byte store
// per lane into the block's tile row, as the kernels that serve that layout write it
__global__ __launch_bounds__(BLOCK) void k_output_stores_only_tiled8(float4* __restrict__ rewards, uint2* __restrict__ flag_tiles,
                                                                     int64_t n, int n_blocks) {
    const uint32_t blk = xcd_block();
    const int64_t e = (int64_t)blk * BLOCK + threadIdx.x;
    if (e >= n) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* rew_k = rewards + (int64_t)blk * BLOCK;
    uint2* flg_k = flag_tiles + (int64_t)blk * BLOCK;
#pragma unroll 1
    for (int b = 0; b < n_blocks; ++b) {
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) rew_k[(int64_t)k8 * n + threadIdx.x] = zero4;
        flg_k[threadIdx.x] = make_uint2(0u, 0u);
        rew_k += 8 * n;
        flg_k += n;
    }
}
