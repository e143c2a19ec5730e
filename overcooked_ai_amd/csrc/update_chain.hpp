// update_chain.hpp — a run of minibatches in one C call, for every loss head: oc_ppo_update, oc_ppo_update_plan (include/oc_amd.h:
// OcPpoUpdate), oc_bc_update, oc_bc_update_plan (OcBcUpdate), and the split of an index into minibatches that bc_fused.hpp shares
// Host code only.  Part of liboc_amd.so: included at file scope by rollout4.hip in its OC_R4_PART == 2 unit, behind bc_loss.hpp.  For
// minibatch k of the index the chain enqueues, on the caller's stream and without synchronising, what the four entry points enqueue —
//   oc_policy_forward -> the head's loss (with stats) -> oc_policy_backward (on the RAW gradients) -> oc_adam_step (d_grad_scale = &stats[k][7])
// — through their own launch code (pol_run_forward, the head's run, pol_run_backward, adam_run): no kernel is duplicated or changed.
// Every refusal of every stage of every minibatch is made, under the entry point's name, before the first launch (pol_check_forward,
// the head's check, pol_check_backward, adam_check).  The scratch is one minibatch's and is reused: the stream orders the minibatches.
//
// A head is a struct of static members (PpoHead, BcHead: no table of function pointers, so that the calls of ppo_run and bc_run stay
// direct) that names
//   Loss, Update   its two structs of include/oc_amd.h; the update structs have the same members, and a Loss has d_logits, d_index,
//                  first_sample, n_minibatch, d_grad_logits, d_grad_values, d_partials and d_stats, which upd_stage binds
//   WHO            the entry point's name, under which every refusal is made (the plan call's: WHO with "_plan" behind it)
//   bind           the per-minibatch members of its Loss that the others do not have
//   check, run     the two halves of its loss entry point
//   PARTIAL        the f64 of a row of its loss partials, for the plan's words
//   plan           its loss entry point's plan call for a minibatch of m rows with an index, gradients and stats, and the plan's flags
//   CHECK_FIRST    whether its check is made ahead of pol_check_backward's.  The order shows in the words of a refusal: oc_ppo_update
//                  refuses a NULL update.d_grad_logits in ppo_check's words; oc_bc_update in pol_check_backward's, since an update needs
//                  the gradient arrays that bc_check, which serves evaluations too, lets a caller leave out
// A further head is such a struct and two one-line entry points.
#pragma once

namespace {

// ---- the split of an index of n_index entries into minibatches
int64_t upd_count(int64_t n_index, int64_t minibatch) { return (n_index + minibatch - 1) / minibatch; }

struct UpdSplit {
    int64_t K, m, last;  // the minibatches, the rows of the first (the longest) and of the last
};

UpdSplit upd_split(int64_t n_index, int64_t minibatch) {
    const int64_t K = upd_count(n_index, minibatch);
    return {K, n_index < minibatch ? n_index : minibatch, n_index - (K - 1) * minibatch};
}

int upd_check_index(const char* who, int64_t n_index) {
    if (n_index < 0) return pol_refuse(who, "n_index < 0");
    if (n_index >= ((int64_t)1 << 31)) return pol_refuse(who, "n_index must be below 2^31");
    return OC_OK;
}

// the checks that need no array (the plan calls make these alone)
int upd_check_shape(const char* who, int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2) {
    if (int rc = upd_check_index(who, n_index)) return rc;
    if (minibatch < 1) return pol_refuse(who, "minibatch < 1");
    return pol_check_shape(who, n_index < minibatch ? n_index : minibatch, in_dim, h1, h2);
}

// ---- the heads
struct PpoHead {
    using Loss = OcPpoLoss;
    using Update = OcPpoUpdate;
    static constexpr const char* WHO = "oc_ppo_update";
    static constexpr int PARTIAL = 6;
    static constexpr bool CHECK_FIRST = true;
    static void bind(Loss& q, const Update* u) {
        q.d_values = u->d_values;
        q.d_terms_out = nullptr;
    }
    static int check(const Loss* q) { return ppo_check(q, WHO); }
    static int run(const Loss* q, hipStream_t stream) { return ppo_run(q, stream, WHO); }
    static int plan(int64_t m, char* out, size_t out_size, int with_seat, int with_moments, int with_old_logits) {
        return oc_ppo_loss_plan(m, 1, with_seat, with_moments, with_old_logits, 0, out, out_size);
    }
};

struct BcHead {
    using Loss = OcBcLoss;
    using Update = OcBcUpdate;
    static constexpr const char* WHO = "oc_bc_update";
    static constexpr int PARTIAL = 4;
    static constexpr bool CHECK_FIRST = false;
    static void bind(Loss& q, const Update*) { q.d_loss_out = nullptr; }
    static int check(const Loss* q) { return bc_check(q, WHO); }
    static int run(const Loss* q, hipStream_t stream) { return bc_run(q, stream, WHO); }
    static int plan(int64_t m, char* out, size_t out_size, int with_class_weights) { return oc_bc_loss_plan(m, 1, with_class_weights, 1, 0, out, out_size); }
};

// ---- the chain
template <class Head>
struct UpdStage {  // the four calls of one minibatch
    OcPolicyRows rows;
    typename Head::Loss q;
    OcAdam ad;
};

template <class Head>
UpdStage<Head> upd_stage(const typename Head::Loss* loss, const OcAdam* adam, const typename Head::Update* u, int64_t k) {
    UpdStage<Head> s;
    const int64_t lo = k * u->minibatch, rest = u->n_index - lo;
    const int64_t m = rest < u->minibatch ? (rest > 0 ? rest : 0) : u->minibatch;
    s.rows.d_features = u->d_features;
    s.rows.n_feature_rows = u->n_feature_rows;
    s.rows.d_index = u->d_index ? u->d_index + lo : nullptr;
    s.rows.first_row = 0;
    s.rows.n_rows = m;
    s.q = *loss;  // the batch side and the head's coefficients
    s.q.d_logits = u->d_logits;
    s.q.d_index = s.rows.d_index;
    s.q.first_sample = 0;
    s.q.n_minibatch = m;
    s.q.d_grad_logits = u->d_grad_logits;
    s.q.d_grad_values = u->d_grad_values;
    s.q.d_partials = u->d_loss_partials;
    s.q.d_stats = u->d_stats ? u->d_stats + 8 * k : nullptr;
    Head::bind(s.q, u);
    s.ad = *adam;
    s.ad.d_grad_scale = s.q.d_stats ? s.q.d_stats + 7 : nullptr;
    s.ad.d_info = u->d_info ? u->d_info + 4 * k : nullptr;
    return s;
}

template <class Head>
int upd_run(const OcActorCritic* pol, const typename Head::Loss* loss, const OcAdam* adam, const typename Head::Update* u, hipStream_t stream) {
    const char* const who = Head::WHO;
    if (!pol) return pol_refuse(who, "policy is NULL");
    if (!loss) return pol_refuse(who, "loss is NULL");
    if (!adam) return pol_refuse(who, "adam is NULL");
    if (!u) return pol_refuse(who, "update is NULL");
    if (int rc = upd_check_shape(who, u->n_index, u->minibatch, pol->in_dim, pol->h1, pol->h2)) return rc;
    if (!u->d_index) return pol_refuse(who, "update.d_index is NULL");
    if (!u->d_stats || !u->d_info) return pol_refuse(who, "NULL update.d_stats or update.d_info");
    if (!u->d_loss_partials) return pol_refuse(who, "update.d_loss_partials is NULL");
    if ((uintptr_t)u->d_info & 7u) return pol_refuse(who, "update.d_info must be 8-byte aligned");
    const int64_t K = upd_count(u->n_index, u->minibatch);
    // ---- every refusal of every stage: minibatch 0 is the longest; the others differ in their addresses and the last in its length
    for (int64_t k = 0; k < (K > 0 ? K : 1); ++k) {
        const UpdStage<Head> s = upd_stage<Head>(loss, adam, u, k);
        if (int rc = pol_check_forward(who, pol, &s.rows, u->d_logits, u->d_values)) return rc;
        if (int rc = Head::CHECK_FIRST ? Head::check(&s.q) : OC_OK) return rc;
        if (int rc = pol_check_backward(who, pol, &s.rows, u->d_grad_logits, u->d_grad_values, &u->grads, u->d_policy_partials)) return rc;
        if (int rc = Head::CHECK_FIRST ? OC_OK : Head::check(&s.q)) return rc;
        if (int rc = adam_check(who, pol, &u->grads, &s.ad)) return rc;
    }
    // ---- the launches
    for (int64_t k = 0; k < K; ++k) {
        const UpdStage<Head> s = upd_stage<Head>(loss, adam, u, k);
        if (int rc = pol_run_forward(who, pol, &s.rows, u->d_logits, u->d_values, stream)) return rc;
        if (int rc = Head::run(&s.q, stream)) return rc;
        if (int rc = pol_run_backward(who, pol, &s.rows, u->d_grad_logits, u->d_grad_values, &u->grads, u->d_policy_partials, stream)) return rc;
        if (int rc = adam_run(who, pol, &u->grads, &s.ad, stream)) return rc;
    }
    return OC_OK;
}

template <class Head, class... Flags>
int upd_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, char* out, size_t out_size, Flags... flags) {
    if (!out || out_size == 0) {
        char who[64];
        snprintf(who, sizeof(who), "%s_plan", Head::WHO);
        return pol_refuse(who, "no output buffer");
    }
    out[0] = 0;
    if (int rc = upd_check_shape(Head::WHO, n_index, minibatch, in_dim, h1, h2)) return rc;
    const auto [K, m, last] = upd_split(n_index, minibatch);
    const int size = pol_layout(in_dim, h1, h2).size;
    const long long loss_rows = (long long)((m + PPO_P - 1) / PPO_P), pol_rows = pol_grid(m, pol_backward_waves(in_dim));
    char scratch[320];
    snprintf(scratch, sizeof(scratch), "scratch: logits %lld x 6 f32, values %lld f32, grad_logits %lld x 6 f32, grad_values %lld f32, loss partials %lld x %d f64, "
             "policy partials %lld x %d f32, gradients %d f32; out: stats %lld x 8 f64, info %lld x 4 f64", (long long)m, (long long)m, (long long)m,
             (long long)m, loss_rows > 0 ? loss_rows : 1, Head::PARTIAL, pol_rows > 0 ? pol_rows : 1, size, size, (long long)K, (long long)K);
    if (K == 0) {
        snprintf(out, out_size, "nothing to launch (no index); %s", scratch);
        return OC_OK;
    }
    char fwd[512], los[384], bwd[640], adm[256];
    if (int rc = oc_policy_plan(m, 1, in_dim, h1, h2, 0, fwd, sizeof(fwd))) return rc;
    if (int rc = Head::plan(m, los, sizeof(los), flags...)) return rc;
    if (int rc = oc_policy_plan(m, 1, in_dim, h1, h2, 1, bwd, sizeof(bwd))) return rc;
    adam_describe(in_dim, h1, h2, adm, sizeof(adm));
    snprintf(out, out_size, "%lld minibatch(es) of %lld rows (the last %lld), no host synchronisation, each: [%s] + [%s] + [%s] + [%s]; %s",
             (long long)K, (long long)m, (long long)last, fwd, los, bwd, adm, scratch);
    return OC_OK;
}

}  // namespace

extern "C" {

int oc_ppo_update(const OcActorCritic* pol, const OcPpoLoss* loss, const OcAdam* adam, const OcPpoUpdate* u, void* stream) {
    return upd_run<PpoHead>(pol, loss, adam, u, (hipStream_t)stream);
}

int oc_ppo_update_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_seat, int with_moments, int with_old_logits,
                       char* out, size_t out_size) {
    return upd_plan<PpoHead>(n_index, minibatch, in_dim, h1, h2, out, out_size, with_seat, with_moments, with_old_logits);
}

int oc_bc_update(const OcActorCritic* pol, const OcBcLoss* loss, const OcAdam* adam, const OcBcUpdate* u, void* stream) {
    return upd_run<BcHead>(pol, loss, adam, u, (hipStream_t)stream);
}

int oc_bc_update_plan(int64_t n_index, int64_t minibatch, int in_dim, int h1, int h2, int with_class_weights, char* out, size_t out_size) {
    return upd_plan<BcHead>(n_index, minibatch, in_dim, h1, h2, out, out_size, with_class_weights);
}

}  // extern "C"
