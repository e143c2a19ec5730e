// observation_plan.hpp — host side of the observation paths: the geometry of a lossless observation and the plans of
// oc_encode_lossless, oc_rollout_encode and oc_rollout_featurize.  A plan makes every check and every choice of a call; nothing here launches, touches
// device memory or takes a device address (the one thing read from the runtime is simd_count()).  oc_amd.hip launches from
// the plans; oc_observation_plan puts them into words.  Included by oc_amd.hip inside its anonymous namespace, after the checks
// and the tuning knobs it uses.
#pragma once

// ---- the geometry: bytes of one env's observation, envs per template, envs per private LDS image
struct ObsGeometry {
    size_t env_bytes;  // both players' [W][H][26] encodings of one env
    int unit;          // envs per observation template: the fewest whose bytes are a multiple of 16 (1, 2 or 4)
    ObsGeometry(int width, int height, int obs_dtype)
        : env_bytes((size_t)2 * width * height * OC_NUM_LAYERS * (obs_dtype == OC_OBS_U8 ? 1 : 4)), unit(1) {
        while (((env_bytes * unit) & 15u) != 0) unit *= 2;
    }
    // envs each of w wavefronts' images can hold when a workgroup's LDS is `fixed` bytes plus the images and stays within
    // `budget`; at most 64 (a wavefront's envs)
    int envs_per_image(size_t fixed, size_t budget, int w) const {
        const int g = fixed < budget ? (int)((budget - fixed) / ((size_t)w * env_bytes)) : 0;
        return g > 64 ? 64 : g;
    }
    int whole_units(int g) const { return g - g % unit; }
};

// tuning builds: wavefronts per workgroup / envs per image of k_rollout_encode, forced
inline int rollout_encode_forced_waves() {
    static const int v = tuning_int("OC_ROLLOUT_ENCODE_WAVES", 0);
    return v;
}
inline int rollout_encode_forced_g() {
    static const int v = tuning_int("OC_ROLLOUT_ENCODE_G", 0);
    return v;
}

// ---- oc_encode_lossless.  The instances: k_encode_uniform<u8> (one layout, u8: persistent workgroups around an LDS template)
//      and k_encode<T, LAY_LDS> (T = u8 / f32; LAY_LDS: the layout table staged in LDS)
struct EncodePlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    enum Kernel { NOTHING, UNIFORM, GENERIC } kernel = NOTHING;  // no envs / k_encode_uniform / k_encode
    bool f32 = false;      // the instance's T
    bool lay_lds = false;  // GENERIC: the instance's LAY_LDS
    int n_planes = 0;
    unsigned grid = 0;
    size_t smem = 0;         // dynamic LDS
    int epb = 0;             // GENERIC: envs per workgroup
    int unit = 0, upg = 0;   // UNIFORM: envs per template, templates' worth of envs per group
};

EncodePlan plan_encode(const OcBatch* b, int obs_dtype, bool have_state, bool have_obs, bool obs_aligned16) {
    EncodePlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    int n_obj = 0;
    if (int rc = check_batch(b, &n_obj)) return refused(rc);
    if (!have_state || !have_obs) return refused(fail(OC_EINVAL, "oc_encode_lossless: NULL pointer"));
    if (int rc = check_obs("oc_encode_lossless", obs_dtype, obs_aligned16)) return refused(rc);
    if (b->n_envs == 0) return p;
    p.f32 = obs_dtype != OC_OBS_U8;
    p.n_planes = 1 + n_obj;
    const ObsGeometry geo(b->width, b->height, obs_dtype);
    const size_t env_bytes = geo.env_bytes;
    // envs per workgroup: fill ~40 KiB of LDS; a multiple of 4 keeps every block's byte range 16-byte aligned
    int epb = (int)((size_t)enc_lds_budget() / (env_bytes + (size_t)p.n_planes * 16));
    if (epb >= 4) epb &= ~3;
    if (epb < 1) epb = 1;
    if (epb > 32) epb = 32;
    if (!p.f32 && (epb & 3) != 0 && (env_bytes & 15u) != 0) {
        epb = 4;  // u8 rows of odd cell counts are only 4-byte multiples: keep blocks 16-byte aligned
    }
    const size_t smem = (size_t)epb * p.n_planes * 16 + (((size_t)epb * env_bytes + 15) & ~(size_t)15);
    if (smem > 160 * 1024) return refused(fail(OC_EINVAL, "oc_encode_lossless: grid too large for LDS staging"));
    // single layout + u8: the persistent template kernel (27.4 vs 32.4 us for the generic kernel on 65 536
    // asymmetric_advantages envs).  f32 is HBM-write bound either way: through the template kernel 5x4 grids gain when
    // encodes run back to back (43.5 vs 54.4 us) but not inside a training loop (43.5 vs 41.9 us), 9x5 is 112 us both ways
    if (b->n_layouts == 1 && !p.f32) {
        const int unit = geo.unit;
        const size_t unit_bytes = env_bytes * unit;
        int upg = (int)(enc_uniform_budget(env_bytes) / unit_bytes);     // units per group
        if (upg < 1) upg = 1;
        if (upg * unit > 32) upg = 32 / unit > 0 ? 32 / unit : 1;
        const size_t smem_u = unit_bytes + unit_bytes * upg + (size_t)unit * upg * p.n_planes * 16;
        if (smem_u <= 150 * 1024) {
            const int64_t n_groups = (b->n_envs + (int64_t)unit * upg - 1) / ((int64_t)unit * upg);
            int per_cu = (int)((150 * 1024) / (smem_u + 512));
            if (per_cu > 8) per_cu = 8;
            if (per_cu < 1) per_cu = 1;
            int64_t grid_u = (simd_count() / 4) * per_cu;
            if (grid_u > n_groups) grid_u = n_groups;
            p.kernel = EncodePlan::UNIFORM;
            p.unit = unit; p.upg = upg;
            p.grid = (unsigned)grid_u;
            p.smem = smem_u;
            return p;
        }
    }
    p.kernel = EncodePlan::GENERIC;
    p.lay_lds = b->n_layouts <= LDS_LAYOUT_MAX;
    p.epb = epb;
    p.grid = (unsigned)((b->n_envs + epb - 1) / epb);
    p.smem = smem;
    return p;
}

// A plan in words: up to and including '>' the kernel instance, as tests match it
void describe_encode_plan(const EncodePlan& p, char* out, size_t out_size) {
    const char* const t = p.f32 ? "f32" : "u8";
    if (p.kernel == EncodePlan::NOTHING)
        snprintf(out, out_size, "nothing to launch (no envs)");
    else if (p.kernel == EncodePlan::UNIFORM)
        snprintf(out, out_size, "k_encode_uniform<T=%s> unit=%d, upg=%d, grid=%u, %zu B LDS", t, p.unit, p.upg, p.grid, p.smem);
    else
        snprintf(out, out_size, "k_encode<T=%s, LAY_LDS=%s> epb=%d, grid=%u, %zu B LDS", t, p.lay_lds ? "true" : "false", p.epb, p.grid, p.smem);
}

// ---- oc_rollout_encode.  The instances: k_rollout_encode<MAXP=2, FAST, T, NW> (FAST = 3: two players everywhere and at most
//      64 cells, else 0; T = u8 / f32; NW = 4 or 8 wavefronts per workgroup), or the one-step entry points, step by step

// The dynamic LDS a k_rollout_encode workgroup may ask for: what the runtime says of the instance family (rollout_encode_lds),
// or the 144 KiB assumed where it cannot be asked
struct LdsBudget {
    size_t bytes;
    bool queried;
};
inline LdsBudget lds_budget_fallback() { return {(size_t)144 * 1024, false}; }
// FAST of the instance that would serve the batch
inline bool rollout_encode_fast(const OcBatch* b) { return (b->batch_flags & OC_BATCH_TWO_PLAYERS) != 0 && b->width * b->height <= 64; }

// What a plan needs to know of a call's arrays: which ones are there, never where
struct RolloutEncodeArrays {
    bool state, actions, rewards, flags, obs;
    bool obs_aligned16;  // d_obs and obs_step_stride are multiples of 16 bytes
    bool rewards_aligned16 = true, ep_returns_aligned16 = true;
};
struct RolloutEncodePlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    enum Path { NOTHING, ONE_KERNEL, STEP_BY_STEP } path = NOTHING;  // no envs or no steps / k_rollout_encode / the one-step entry points
    int n_obj = 0;
    StartArgs sa = {};
    bool fast = false, f32 = false;  // ONE_KERNEL: the instance's FAST (3 or 0), T and NW
    int nw = 0;
    int unit = 0, g = 0;             // ONE_KERNEL: envs per template, envs per image
    size_t smem = 0;                 // ONE_KERNEL: dynamic LDS
    LdsBudget budget = lds_budget_fallback();  // ONE_KERNEL: what the choice of NW and g was made within
};

RolloutEncodePlan plan_rollout_encode(const OcBatch* b, const RolloutEncodeArrays& have, int obs_dtype, int horizon, uint32_t options,
                                      int64_t env_offset, int n_steps, const OcStartSpec* start, const LdsBudget& budget) {
    const char* const who = "oc_rollout_encode";
    RolloutEncodePlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
    if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
    if (!have.state || !have.obs) return refused(refuse(who, "NULL state / observation pointer"));
    if (!obs_dtype_ok(obs_dtype)) return refused(refuse(who, "bad obs_dtype"));
    if (!have.obs_aligned16) return refused(refuse(who, "d_obs and obs_step_stride must be multiples of 16 bytes"));
    if (int rc = check_quads(who, have.rewards_aligned16, have.ep_returns_aligned16)) return refused(rc);
    if (int rc = check_horizon(who, horizon)) return refused(rc);
    if (n_steps < 0 || n_steps > (1 << 30)) return refused(refuse(who, "n_steps must be in 0..2^30"));
    if (options & ~(uint32_t)(OC_OPT_AUTO_RESET | OC_OPT_ONE_KERNEL))
        return refused(refuse(who, "options other than OC_OPT_AUTO_RESET / OC_OPT_ONE_KERNEL"));
    if (have.actions && (!have.rewards || !have.flags)) return refused(refuse(who, "caller actions need the rewards and flags arrays"));
    if (start && start->env_offset != env_offset)  // (both paths: the one-step fallback would refuse it, the single kernel must too)
        return refused(refuse(who, "start.env_offset differs from env_offset"));
    if (b->n_envs == 0 || n_steps == 0) return p;
    p.path = RolloutEncodePlan::STEP_BY_STEP;  // every table the single kernel does not take: the same result from the one-step kernels
    // one layout, at most two pots, at most 48 cells (three object planes), u8 or f32 observations: the whole trajectory in one
    // launch (k_rollout_encode).  The LDS of a workgroup holds the cell words of its 256 envs, the template, the headers and one
    // image per wavefront.
    // It keeps 256 envs per CU on chip and is bound by what one CU's four wavefronts can encode per step (~27 us for
    // 9x5), so it pays once every CU has a workgroup: 30 us vs 37 us per step at 65 536 envs, but 27 us vs 18 us at 16 384
    // (a single step is a wash against the two one-step kernels — 36.4 vs 37.2 us on 9x5, 25.1 vs 24.4 us on 5x4 — and
    // stays with them unless OC_OPT_ONE_KERNEL asks)
    const bool fills_gpu = b->n_envs >= (simd_count() / 4) * 192 && n_steps >= 2;
    if (!((fills_gpu || (options & OC_OPT_ONE_KERNEL)) && b->n_layouts == 1 && b->max_pots >= 1 && b->max_pots <= 2 && p.n_obj <= 3)) return p;
    const ObsGeometry geo(b->width, b->height, obs_dtype);
    const int unit = geo.unit;
    const size_t cell_bytes = (size_t)p.n_obj * 16 * BLOCK * sizeof(uint16_t);
    const size_t fixed = cell_bytes + geo.env_bytes * unit + (size_t)BLOCK * 16 + RE_LIST_BYTES;
    // eight wavefronts (four of them helpers that only encode) when eight images of at least 8 envs fit: small grids,
    // where four wavefronts cannot encode 256 envs in the time HBM takes them (5x4 u8: 14.4 vs 17.4 us per step); 9x5
    // is at the write ceiling either way (30.1 vs 30.4 us), f32 loses with one-env images (128 vs 117 us)
    const int forced_nw = rollout_encode_forced_waves();
    // round 6: u8 observations take eight wavefronts down to 4-env images — a wavefront that is issuing its image's stores into a
    // busy store path is not building the next one, and eight of them leave the path idle less often (65 536 envs, us per step,
    // four vs eight: 9x5 29.2 -> 27.6-28.3, 8x5 26.1 -> 24.2, 5x5 16.1 -> 15.4; profiles/r06_rollout_encode_ablation.txt)
    const int min_g8 = obs_dtype == OC_OBS_U8 ? 4 : 8;
    int nw = 8;
    int gmax = geo.envs_per_image(fixed, budget.bytes, nw);
    if (((gmax < min_g8 || gmax < unit) && forced_nw != 8) || forced_nw == 4) {
        nw = 4;
        gmax = geo.envs_per_image(fixed, budget.bytes, nw);
    }
    if (gmax < unit) return p;  // not one template's envs per image
    const int span = nw == 8 ? 32 : 64;                  // envs one wavefront encodes per step
    const int parts = (span + gmax - 1) / gmax;          // its sub-groups, as even as the budget allows
    int g = (span + parts - 1) / parts;
    g = (g + unit - 1) / unit * unit;
    if (g > gmax) g = geo.whole_units(gmax);
    const int forced_g = rollout_encode_forced_g();
    if (forced_g > 0 && forced_g <= g && forced_g % unit == 0) g = forced_g;
    p.path = RolloutEncodePlan::ONE_KERNEL;
    p.fast = rollout_encode_fast(b);
    p.f32 = obs_dtype != OC_OBS_U8;
    p.nw = nw;
    p.unit = unit; p.g = g;
    p.smem = fixed + (size_t)nw * g * geo.env_bytes;
    p.budget = budget;
    return p;
}

// A plan in words.  Step by step, one step is the one-step entry point named here and then oc_encode_lossless, whose own plan
// (`one_step`) follows
void describe_rollout_encode_plan(const RolloutEncodePlan& p, bool caller_actions, const EncodePlan& one_step,
                                  char* out, size_t out_size) {
    if (p.path == RolloutEncodePlan::NOTHING) {  // (no steps: oc_observation_plan answers for oc_encode_lossless instead)
        snprintf(out, out_size, "nothing to launch (no envs)");
    } else if (p.path == RolloutEncodePlan::ONE_KERNEL) {
        snprintf(out, out_size, "k_rollout_encode<MAXP=2, FAST=%d, T=%s, NW=%d> unit=%d, G=%d, %zu B LDS, budget %zu B (%s)", p.fast ? 3 : 0,
                 p.f32 ? "f32" : "u8", p.nw, p.unit, p.g, p.smem, p.budget.bytes, p.budget.queried ? "queried" : "fallback");
    } else {
        const int used = snprintf(out, out_size, "step by step: %s + ", caller_actions ? "oc_step" : "oc_rollout_random");
        if (used > 0 && (size_t)used < out_size) describe_encode_plan(one_step, out + used, out_size - used);
    }
}

// ---- oc_rollout_featurize.  The instance: k_rollout_featurize<MAXP=2, FAST=3> (one two-player layout of at most 64 cells with
//      one or two pots), or the one-step entry points and oc_featurize, step by step

// tuning builds: the batch size from which the single kernel is taken without OC_OPT_ONE_KERNEL, forced (read at every call:
// tools/time_rollout_featurize.py alternates the two paths in one process)
inline int64_t rollout_featurize_fill(int64_t dflt) {
    const int v = tuning_int("OC_ROLLOUT_FEATURIZE_FILL", -1);
    return v >= 0 ? (int64_t)v : dflt;
}

struct RolloutFeaturizeArrays {
    bool plan, state, actions, rewards, flags, features;  // plan: the blob and its offsets
    bool features_aligned16;  // d_features and feat_step_stride are multiples of 16 bytes
    bool rewards_aligned16 = true, ep_returns_aligned16 = true;
};
struct RolloutFeaturizePlan {
    int rc = OC_OK;  // the call is refused with this code (the message: oc_last_error)
    enum Path { NOTHING, ONE_KERNEL, STEP_BY_STEP } path = NOTHING;  // no envs or no steps / k_rollout_featurize / the one-step entry points
    int n_obj = 0;
    StartArgs sa = {};
    unsigned grid = 0; // ONE_KERNEL
    size_t smem = 0;   // ONE_KERNEL: dynamic LDS
};

RolloutFeaturizePlan plan_rollout_featurize(const OcBatch* b, const RolloutFeaturizeArrays& have, int num_pots, int horizon, uint32_t options,
                                            int64_t env_offset, int n_steps, const OcStartSpec* start) {
    const char* const who = "oc_rollout_featurize";
    RolloutFeaturizePlan p;
    const auto refused = [&p](int rc) { p.rc = rc; return p; };
    if (int rc = check_batch(b, &p.n_obj)) return refused(rc);
    if (int rc = check_start(who, start, &p.sa, b)) return refused(rc);
    if (!have.plan || !have.state || !have.features) return refused(refuse(who, "NULL plan / state / features pointer"));
    if (num_pots < 0 || num_pots > 4) return refused(refuse(who, "num_pots must be in 0..4"));
    if (!(b->batch_flags & OC_BATCH_TWO_PLAYERS)) return refused(refuse(who, "needs 2-player layouts"));
    if (!have.features_aligned16) return refused(refuse(who, "d_features and feat_step_stride must be multiples of 16 bytes"));
    if (int rc = check_quads(who, have.rewards_aligned16, have.ep_returns_aligned16)) return refused(rc);
    if (int rc = check_horizon(who, horizon)) return refused(rc);
    if (n_steps < 0 || n_steps > (1 << 30)) return refused(refuse(who, "n_steps must be in 0..2^30"));
    if (options & ~(uint32_t)(OC_OPT_AUTO_RESET | OC_OPT_ONE_KERNEL))
        return refused(refuse(who, "options other than OC_OPT_AUTO_RESET / OC_OPT_ONE_KERNEL"));
    if (have.actions && (!have.rewards || !have.flags)) return refused(refuse(who, "caller actions need the rewards and flags arrays"));
    if (start && start->env_offset != env_offset)  // (both paths: the one-step fallback would refuse it, the single kernel must too)
        return refused(refuse(who, "start.env_offset differs from env_offset"));
    if (b->n_envs == 0 || n_steps == 0) return p;
    p.path = RolloutFeaturizePlan::STEP_BY_STEP;  // every table the single kernel does not take: the same result from the one-step kernels
    // one layout of at most 64 cells with one or two pots: the whole trajectory in one launch (k_rollout_featurize), from 64
    // envs per CU (16 384 on MI355X) and two steps on — or where OC_OPT_ONE_KERNEL asks.  oc_rollout_encode's rule, 192 envs per
    // CU, was the starting point; measured (us per step, one kernel vs step by step, cramped_room / asymmetric_advantages):
    // 16 384 envs 7.0 vs 15.8 / 7.3 vs 18.3, 32 768 envs 7.1 vs 18.2 / 7.4 vs 21.1, 65 536 envs 9.4 vs 23.7 / 8.9 vs 26.2
    // (profiles/rollout_featurize.txt): a step of the kernel costs less than the second launch it saves long before every CU has
    // a workgroup.  16 384 is the smallest batch measured; below it the one-step kernels stay
    const bool fills_gpu = b->n_envs >= rollout_featurize_fill((simd_count() / 4) * 64) && n_steps >= 2;
    if (!((fills_gpu || (options & OC_OPT_ONE_KERNEL)) && b->n_layouts == 1 && b->max_pots >= 1 && b->max_pots <= 2 &&
          b->width * b->height <= 64))
        return p;
    // the LDS of a workgroup: the cell words of its 256 envs, their headers and one int16 image of RF_GROUP envs per wavefront
    // (at most 32768 + 4096 + 4 * 17664 = 107 520 bytes: 64 cells, num_pots = 4)
    p.grid = grid_for(b->n_envs);
    p.smem = (size_t)p.n_obj * 16 * BLOCK * sizeof(uint16_t) + (size_t)BLOCK * 16 + 4 * feat_image_shorts(num_pots) * sizeof(int16_t);
    p.path = RolloutFeaturizePlan::ONE_KERNEL;
    return p;
}
