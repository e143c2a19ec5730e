// bc_update.hpp — a run of behaviour-cloning minibatches in one C call: oc_bc_update, oc_bc_update_plan (include/oc_amd.h: OcBcUpdate)
// Host code only.  Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind bc_loss.hpp.  It
// is ppo_update.hpp with the cross-entropy head in the loss's place: for minibatch k of the index it enqueues, on the caller's stream
// and without synchronising, what the four entry points enqueue —
//   oc_policy_forward -> oc_bc_loss (with stats) -> oc_policy_backward (on the RAW gradients) -> oc_adam_step (d_grad_scale = &stats[k][7])
// — through their own launch code (pol_run_forward, bc_run, pol_run_backward, adam_run): no kernel is duplicated or changed.  Every
// refusal of every stage of every minibatch is made, under this entry point's name, before the first launch (pol_check_forward,
// bc_check, pol_check_backward, adam_check).  The scratch is one minibatch's and is reused: the stream orders the minibatches.
#pragma once

namespace {

const char* const BCU_WHO = "oc_bc_update";

struct BcuStage {  // the four calls of one minibatch
    OcPolicyRows rows;
    OcBcLoss q;
    OcAdam ad;
};

BcuStage bcu_stage(const OcBcLoss* loss, const OcAdam* adam, const OcBcUpdate* u, int64_t k) {
    BcuStage s;
    const int64_t lo = k * u->minibatch, rest = u->n_index - lo;
    const int64_t m = rest < u->minibatch ? (rest > 0 ? rest : 0) : u->minibatch;
    s.rows.d_features = u->d_features;
    s.rows.n_feature_rows = u->n_feature_rows;
    s.rows.d_index = u->d_index ? u->d_index + lo : nullptr;
    s.rows.first_row = 0;
    s.rows.n_rows = m;
    s.q = *loss;  // the actions, their number and the class weights
    s.q.d_logits = u->d_logits;
    s.q.d_index = s.rows.d_index;
    s.q.first_sample = 0;
    s.q.n_minibatch = m;
    s.q.d_grad_logits = u->d_grad_logits;
    s.q.d_grad_values = u->d_grad_values;
    s.q.d_loss_out = nullptr;
    s.q.d_partials = u->d_loss_partials;
    s.q.d_stats = u->d_stats ? u->d_stats + 8 * k : nullptr;
    s.ad = *adam;
    s.ad.d_grad_scale = s.q.d_stats ? s.q.d_stats + 7 : nullptr;
    s.ad.d_info = u->d_info ? u->d_info + 4 * k : nullptr;
    return s;
}

// the checks that need no array (oc_bc_update_plan makes these alone)
int bcu_check_shape(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2) {
    if (n_index < 0) return pol_refuse(BCU_WHO, "n_index < 0");
    if (n_index >= ((int64_t)1 << 31)) return pol_refuse(BCU_WHO, "n_index must be below 2^31");
    if (minibatch < 1) return pol_refuse(BCU_WHO, "minibatch < 1");
    return pol_check_shape(BCU_WHO, n_index < minibatch ? n_index : minibatch, in_dim, h1, h2);
}

}  // namespace

extern "C" {

int oc_bc_update(const OcActorCritic* pol, const OcBcLoss* loss, const OcAdam* adam, const OcBcUpdate* u, void* stream) {
    const char* const who = BCU_WHO;
    if (!pol) return pol_refuse(who, "policy is NULL");
    if (!loss) return pol_refuse(who, "loss is NULL");
    if (!adam) return pol_refuse(who, "adam is NULL");
    if (!u) return pol_refuse(who, "update is NULL");
    if (int rc = bcu_check_shape(u->n_index, u->minibatch, pol->in_dim, pol->h1, pol->h2)) return rc;
    if (!u->d_index) return pol_refuse(who, "update.d_index is NULL");
    if (!u->d_stats || !u->d_info) return pol_refuse(who, "NULL update.d_stats or update.d_info");
    if (!u->d_loss_partials) return pol_refuse(who, "update.d_loss_partials is NULL");
    if ((uintptr_t)u->d_info & 7u) return pol_refuse(who, "update.d_info must be 8-byte aligned");
    const int64_t K = upd_count(u->n_index, u->minibatch);
    // ---- every refusal of every stage: minibatch 0 is the longest; the others differ in their addresses and the last in its length
    for (int64_t k = 0; k < (K > 0 ? K : 1); ++k) {
        const BcuStage s = bcu_stage(loss, adam, u, k);
        if (int rc = pol_check_forward(who, pol, &s.rows, u->d_logits, u->d_values)) return rc;
        // (the backward pass's ahead of the head's: an update needs the gradient arrays that an evaluation may leave out)
        if (int rc = pol_check_backward(who, pol, &s.rows, u->d_grad_logits, u->d_grad_values, &u->grads, u->d_policy_partials)) return rc;
        if (int rc = bc_check(&s.q, who)) return rc;
        if (int rc = adam_check(who, pol, &u->grads, &s.ad)) return rc;
    }
    // ---- the launches
    for (int64_t k = 0; k < K; ++k) {
        const BcuStage s = bcu_stage(loss, adam, u, k);
        if (int rc = pol_run_forward(who, pol, &s.rows, u->d_logits, u->d_values, (hipStream_t)stream)) return rc;
        if (int rc = bc_run(&s.q, (hipStream_t)stream, who)) return rc;
        if (int rc = pol_run_backward(who, pol, &s.rows, u->d_grad_logits, u->d_grad_values, &u->grads, u->d_policy_partials, (hipStream_t)stream)) return rc;
        if (int rc = adam_run(who, pol, &u->grads, &s.ad, (hipStream_t)stream)) return rc;
    }
    return OC_OK;
}

int oc_bc_update_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_class_weights, char* out, size_t out_size) {
    if (!out || out_size == 0) return fail(OC_EINVAL, "oc_bc_update_plan: no output buffer");
    out[0] = 0;
    if (int rc = bcu_check_shape(n_index, minibatch, in_dim, h1, h2)) return rc;
    const int64_t K = upd_count(n_index, minibatch), m = n_index < minibatch ? n_index : minibatch, last = n_index - (K - 1) * minibatch;
    const int size = pol_layout(in_dim, h1, h2).size;
    const long long loss_rows = (long long)((m + PPO_P - 1) / PPO_P), pol_rows = pol_grid(m, pol_backward_waves(in_dim));
    char scratch[320];
    snprintf(scratch, sizeof(scratch), "scratch: logits %lld x 6 f32, values %lld f32, grad_logits %lld x 6 f32, grad_values %lld f32, loss partials %lld x 4 f64, "
             "policy partials %lld x %d f32, gradients %d f32; out: stats %lld x 8 f64, info %lld x 4 f64", (long long)m, (long long)m, (long long)m,
             (long long)m, loss_rows > 0 ? loss_rows : 1, pol_rows > 0 ? pol_rows : 1, size, size, (long long)K, (long long)K);
    if (K == 0) {
        snprintf(out, out_size, "nothing to launch (no index); %s", scratch);
        return OC_OK;
    }
    char fwd[512], los[384], bwd[640], adm[256];
    if (int rc = oc_policy_plan(m, 1, in_dim, h1, h2, 0, fwd, sizeof(fwd))) return rc;
    if (int rc = oc_bc_loss_plan(m, 1, with_class_weights, 1, 0, los, sizeof(los))) return rc;
    if (int rc = oc_policy_plan(m, 1, in_dim, h1, h2, 1, bwd, sizeof(bwd))) return rc;
    adam_describe(in_dim, h1, h2, adm, sizeof(adm));
    snprintf(out, out_size, "%lld minibatch(es) of %lld rows (the last %lld), no host synchronisation, each: [%s] + [%s] + [%s] + [%s]; %s",
             (long long)K, (long long)m, (long long)last, fwd, los, bwd, adm, scratch);
    return OC_OK;
}

}  // extern "C"
