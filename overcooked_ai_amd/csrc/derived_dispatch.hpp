// derived_dispatch.hpp — host only: what is derived from a batch of states — featurize_state (oc_featurize), the potential
// function (oc_potential, oc_phi_table_size) and the shaped reward (oc_shape_rewards).  oc_featurize and oc_potential plan a call
// (the argument checks, the kernel instance, the grid, the dynamic LDS bytes; no launch, no device address), then launch from the
// plan — or, by oc_featurize_plan / oc_potential_plan, describe it.
// Part of liboc_amd.so: included by oc_amd.hip at file scope, before train_dispatch.hpp and observation_dispatch.hpp, which use
// plan_featurize and the entry points.  The kernels are featurize.hpp, potential.hpp and shaping.hpp (k_shape_rewards).
#pragma once

namespace {
struct FeaturizePlan {
    int rc = OC_OK;
    bool nothing = false;  // no envs
    bool lay_lds = false;  // the layout table fits LDS: k_featurize<true>
    int n_planes = 0;
    unsigned grid = 0;
    size_t smem = 0;
};

// have: every required pointer is there; aligned: d_features is 16-byte aligned
FeaturizePlan plan_featurize(const OcBatch* b, bool have, bool aligned, int num_pots) {
    FeaturizePlan p;
    int n_obj = 0;
    if ((p.rc = check_batch(b, &n_obj)) != OC_OK) return p;
    if (!have) { p.rc = fail(OC_EINVAL, "oc_featurize: NULL pointer"); return p; }
    if (num_pots < 0 || num_pots > 4) { p.rc = fail(OC_EINVAL, "oc_featurize: num_pots must be in 0..4"); return p; }
    if (!(b->batch_flags & OC_BATCH_TWO_PLAYERS)) { p.rc = fail(OC_EINVAL, "oc_featurize: needs 2-player layouts"); return p; }
    if (!aligned) { p.rc = fail(OC_EINVAL, "oc_featurize: d_features must be 16-byte aligned"); return p; }
    if (b->n_envs == 0) { p.nothing = true; return p; }
    p.n_planes = 1 + n_obj;
    const int total = 2 * (num_pots * 10 + 26) + 4;
    p.smem = (size_t)FEAT_ENVS * p.n_planes * 16 + (size_t)FEAT_ENVS * 2 * (total + 2) * sizeof(int16_t);
    p.grid = (unsigned)((b->n_envs + FEAT_ENVS - 1) / FEAT_ENVS);
    p.lay_lds = b->n_layouts <= LDS_LAYOUT_MAX;
    return p;
}

template <bool LAY_LDS>
void launch_featurize(const FeaturizePlan& p, const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off,
                      const void* d_state, float* d_features, int num_pots, hipStream_t s) {
    if (!want_lds(k_featurize<LAY_LDS>, p.smem)) return;
    hipLaunchKernelGGL((k_featurize<LAY_LDS>), dim3(p.grid), dim3(BLOCK), p.smem, s, b->d_layouts, b->n_layouts, b->d_layout_id,
                       d_plan_blob, d_plan_off, (const uint4*)d_state, d_features, b->n_envs, b->width, b->height, p.n_planes, num_pots);
}

struct PotentialPlan {
    int rc = OC_OK;
    bool nothing = false;   // no envs
    bool two_pots = false;  // the table's hint promises one or two pots everywhere: k_potential2
    unsigned grid = 0;
};

// have: every required pointer is there; aligned: d_phi_tables and d_phi are 8-byte aligned
PotentialPlan plan_potential(const OcBatch* b, bool have, bool aligned) {
    PotentialPlan p;
    int n_obj = 0;
    if ((p.rc = check_batch(b, &n_obj)) != OC_OK) return p;
    if (!have) { p.rc = fail(OC_EINVAL, "oc_potential: NULL pointer"); return p; }
    if (!aligned) { p.rc = fail(OC_EINVAL, "oc_potential: d_phi_tables / d_phi must be 8-byte aligned"); return p; }
    if (b->n_envs == 0) { p.nothing = true; return p; }
    p.two_pots = b->max_pots >= 1 && b->max_pots <= 2;  // (0 = unknown: the general kernel)
    p.grid = (unsigned)grid_for(b->n_envs);
    return p;
}
}  // namespace

extern "C" {

int oc_featurize(const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const void* d_state,
                 float* d_features, int num_pots, void* stream) {
    const FeaturizePlan p = plan_featurize(b, d_plan_blob && d_plan_off && d_state && d_features, ((uintptr_t)d_features & 15u) == 0, num_pots);
    if (p.rc != OC_OK || p.nothing) return p.rc;
    if (p.lay_lds) launch_featurize<true>(p, b, d_plan_blob, d_plan_off, d_state, d_features, num_pots, (hipStream_t)stream);
    else launch_featurize<false>(p, b, d_plan_blob, d_plan_off, d_state, d_features, num_pots, (hipStream_t)stream);
    return check_launch("oc_featurize");
}

int oc_featurize_plan(const OcBatch* b, int num_pots, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_featurize_plan: no output buffer");
    out[0] = 0;
    const FeaturizePlan p = plan_featurize(b, true, true, num_pots);
    if (p.rc != OC_OK) return p.rc;
    if (p.nothing) snprintf(out, out_size, "nothing to launch (no envs)");
    else snprintf(out, out_size, "k_featurize<LAY_LDS=%s> grid=%u, %zu B LDS", p.lay_lds ? "true" : "false", p.grid, p.smem);
    return OC_OK;
}

int oc_phi_table_size(void) { return PHI_BYTES; }

int oc_shape_rewards(const OcBatch* b, const float* d_rewards, const uint8_t* d_flags, const double* d_phi_next,
                     double* d_phi_cur, const double* d_phi_start, double reward_shaping_factor, double* d_out,
                     uint8_t* d_done, void* stream) {
    if (!b) return fail(OC_EINVAL, "batch is NULL");
    if (!d_rewards || !d_flags || !d_out) return fail(OC_EINVAL, "oc_shape_rewards: NULL rewards/flags/out pointer");
    if (d_phi_next && (!d_phi_cur || !d_phi_start)) return fail(OC_EINVAL, "oc_shape_rewards: phi_next needs phi_cur and phi_start");
    if (((uintptr_t)d_out & 15u) != 0) return fail(OC_EINVAL, "oc_shape_rewards: d_out must be 16-byte aligned");
    if (b->n_envs == 0) return OC_OK;
    hipLaunchKernelGGL(k_shape_rewards, dim3(grid_for(b->n_envs)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const float4*)d_rewards, d_flags, b->n_layouts > 1 ? b->d_layout_id : nullptr, d_phi_next, d_phi_cur,
                       d_phi_start, reward_shaping_factor, d_out, d_done, b->n_envs);
    return check_launch("oc_shape_rewards");
}

int oc_potential(const OcBatch* b, const uint8_t* d_plan_blob, const uint32_t* d_plan_off, const uint8_t* d_phi_tables,
                 const void* d_state, double* d_phi, void* stream) {
    const PotentialPlan p = plan_potential(b, d_plan_blob && d_plan_off && d_phi_tables && d_state && d_phi,
                                           ((uintptr_t)d_phi_tables & 7u) == 0 && ((uintptr_t)d_phi & 7u) == 0);
    if (p.rc != OC_OK || p.nothing) return p.rc;
    if (p.two_pots)
        hipLaunchKernelGGL(k_potential2, dim3(p.grid), dim3(BLOCK), 0, (hipStream_t)stream, b->d_layouts, b->d_layout_id, d_plan_blob,
                           d_plan_off, d_phi_tables, (const uint4*)d_state, d_phi, b->n_envs, b->width, b->height);
    else
        hipLaunchKernelGGL(k_potential, dim3(p.grid), dim3(BLOCK), 0, (hipStream_t)stream, b->d_layouts, b->d_layout_id, d_plan_blob,
                           d_plan_off, d_phi_tables, (const uint4*)d_state, d_phi, b->n_envs, b->width, b->height);
    return check_launch("oc_potential");
}

int oc_potential_plan(const OcBatch* b, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_potential_plan: no output buffer");
    out[0] = 0;
    const PotentialPlan p = plan_potential(b, true, true);
    if (p.rc != OC_OK) return p.rc;
    if (p.nothing) snprintf(out, out_size, "nothing to launch (no envs)");
    else snprintf(out, out_size, "%s grid=%u", p.two_pots ? "k_potential2" : "k_potential", p.grid);
    return OC_OK;
}

}  // extern "C"
