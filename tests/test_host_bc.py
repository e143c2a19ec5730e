"""oc_bc_loss / oc_bc_update without a GPU: the restatement of tests/bc_cases.py against its float64 reference, whose gradients are
held to torch autograd's F.cross_entropy in float64 (H1), the exports and structs against the header (H2), the plans (H3), every
refusal — made before any device call: this host has no device — (H4), the float64 end-to-end run (H5) and the Python surface's own
refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import bc_cases as BC
import learner_cases as LC
from case_support import P, ROOT
from test_host_learner import _adam_refusals, _adam_structs, _defaults

EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ H1: the arithmetic
def test_h1_the_recorded_error_is_the_measured_one():
    """F32_ERROR is the largest error of bc_f32's losses and gradients against bc_f64's over the case list: no smaller than what is
    measured here, and no more than twice it.  Counts, correct rows and left-out rows are the same in both (the argmax is exact)."""
    worst, where = 0.0, None
    for c in BC.CASES:
        got, ref = BC.bc_f32(c), BC.reference_of(c)
        err = max(BC.rel_error(got.loss, ref.loss), BC.rel_error(got.grad_logits, ref.grad_logits))
        if err > worst:
            worst, where = err, c.id
        assert np.array_equal(got.correct, ref.correct) and np.array_equal(got.left_out, ref.left_out), c.id
        assert got.sums[0] == ref.sums[0] and got.sums[2] == ref.sums[2], c.id
        assert not got.loss[ref.left_out].view(np.uint32).any() and not got.grad_logits[ref.left_out].view(np.uint32).any(), c.id
    print("largest error of bc_f32 over %d cases: %.4g (%s)" % (len(BC.CASES), worst, where))
    assert BC.F32_ERROR / 2 <= worst <= BC.F32_ERROR, (worst, BC.F32_ERROR)
    assert BC.DEVICE_FACTOR == 4 and BC.DEVICE_TOL == 4 * BC.F32_ERROR


@pytest.mark.parametrize("c", [c for c in BC.CASES if c.M <= 1100], ids=lambda c: c.id)
def test_h1_the_reference_s_gradients_are_torch_autograd_s(c):
    """bc_f64's per-row loss and analytic gradients against F.cross_entropy(..., weight, reduction="sum") and its backward in
    float64 on the kept rows, at 1e-12.  (A -inf logit at the taken action: the loss is +inf on both sides and torch's gradient of it
    is not defined; those rows are compared by their loss alone.)"""
    import torch
    import torch.nn.functional as F

    a, ref = BC.arrays_of(c), BC.reference_of(c)
    keep = ~ref.left_out
    if not keep.any():
        assert not ref.sums.any() and not ref.stats.any()
        return
    at = a.sample[keep]
    finite = np.isfinite(ref.loss[keep])
    logits = torch.from_numpy(a.logits[keep].astype(np.float64)).requires_grad_(True)
    target = torch.from_numpy(a.actions[at].astype(np.int64))
    weight = torch.from_numpy(a.class_weights.astype(np.float64)) if a.class_weights is not None else None
    per_row = F.cross_entropy(logits, target, weight=weight, reduction="none")
    F.cross_entropy(logits[torch.from_numpy(finite)], target[torch.from_numpy(finite)], weight=weight, reduction="sum").backward()
    assert BC.rel_error(ref.loss[keep], per_row.detach().numpy()) <= 1e-12, c.id
    assert BC.rel_error(ref.grad_logits[keep][finite], logits.grad.numpy()[finite]) <= 1e-12, c.id
    assert np.isfinite(ref.grad_logits).all()
    if finite.all():
        total = F.cross_entropy(logits.detach(), target, weight=weight, reduction="sum")
        assert abs(ref.sums[1] - float(total)) <= 1e-12 * max(1.0, abs(float(total)))
        assert abs(ref.stats[1] - float(total) / keep.sum()) <= 1e-12 * max(1.0, abs(ref.stats[1]))  # Keras's convention: / count


def test_h1_the_cases_cover_what_they_must():
    Pn = BC.partial_samples()
    tile = Pn // 4
    sizes = {c.M for c in BC.CASES}
    assert set(BC.SIZES) | {3 * tile + 1, 4 * tile + 1, 65 * Pn + 3} <= sizes
    for M in BC.SIZES + (3 * tile + 1, 4 * tile + 1):
        both = [c for c in BC.CASES if c.M == M and c.special in ("", "tiles")]
        assert {c.mode for c in both} == {"contiguous", "indexed"} and {c.weights for c in both} == {True, False}, M
    assert {c.weights for c in BC.CASES if c.special == "big"} == {True, False}
    assert {c.special for c in BC.CASES} >= {"invalid", "count0", "zero_weight", "ties", "neginf_away", "neginf_at", "nan_left_out", "skewed"}
    for c in BC.CASES:
        a, ref = BC.arrays_of(c), BC.reference_of(c)
        assert a.logits.shape == (c.M, 6) and (c.mode == "contiguous") == (a.index is None)
        if c.mode == "contiguous":
            assert a.first > 0
        elif c.M >= 8:
            inside = (a.sample >= 0) & (a.sample < a.S)
            assert (~inside).sum() >= 2 and (c.special == "count0" or len(np.unique(a.sample[inside])) < inside.sum()), c.id
        for x in (ref.loss, ref.grad_logits, ref.stats, ref.sums):  # FILL equals no result
            assert not (x == BC.FILL).any(), c.id
        if c.special == "count0":
            assert ref.sums[0] == 0 and not ref.stats.any() and ref.left_out.all()
        else:
            assert ref.sums[0] > 0 and ref.stats[7] == 1.0 / ref.sums[0]
        if c.special == "invalid":
            assert (a.actions == 255).sum() > 50 and ref.left_out.sum() > 100
        if c.special == "zero_weight":
            zero = a.class_weights == 0
            assert zero.sum() == 1 and (a.actions[a.sample[~ref.left_out]] == np.nonzero(zero)[0][0]).any()
        if c.special == "ties":
            top = (a.logits == a.logits.max(1, keepdims=True)).sum(1)
            first = a.logits.argmax(1)
            act = a.actions[np.clip(a.sample, 0, a.S - 1)]
            tied_hit = (top > 1) & ~ref.left_out & (a.logits[np.arange(c.M), np.minimum(act, 5)] == a.logits.max(1))
            assert (top > 1).mean() > 0.5 and (tied_hit & (act != first)).any() and (tied_hit & (act == first)).any()
            assert not ref.correct[tied_hit & (act != first)].any() and ref.correct[tied_hit & (act == first)].all()
        if c.special == "neginf_away":
            assert np.isneginf(a.logits).any() and np.isfinite(ref.loss).all() and (ref.grad_logits[np.isneginf(a.logits)] == 0).all()
        if c.special == "neginf_at":
            assert np.isposinf(ref.loss).sum() >= 5 and np.isposinf(ref.sums[1]) and np.isposinf(ref.stats[1]) and np.isfinite(ref.grad_logits).all()
        if c.special == "nan_left_out":
            assert np.isnan(a.logits[ref.left_out]).all() and ref.left_out.sum() > 10 and np.isfinite(ref.stats).all()
        if c.special == "skewed":
            hist = np.bincount(a.actions[a.actions <= 5], minlength=6) / (a.actions <= 5).sum()
            assert hist[4] > 0.5 and a.class_weights[4] < a.class_weights.min() * 1.0001


# ------------------------------------------------------------------------------------------ H2: the ABI
def test_h2_exports_and_structs_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_bc_loss", "oc_bc_loss_plan", "oc_bc_update", "oc_bc_update_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    Q, U = _lib.OcBcLoss, _lib.OcBcUpdate
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct OcBcLoss \{(.*?)\} OcBcLoss;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(d_\w+|n_samples|first_sample|n_minibatch)\b", body) == [f[0] for f in Q._fields_]
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == list(range(0, 96, 8)) and ctypes.sizeof(Q) == 96
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct OcBcUpdate \{(.*?)\} OcBcUpdate;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(d_\w+|n_feature_rows|n_index|minibatch|grads)\b", body) == [f[0] for f in U._fields_]
    assert [getattr(U, f).offset for f, _ in U._fields_] == list(range(0, 96, 8)) + [152, 160] and ctypes.sizeof(U) == 168
    assert "int oc_bc_loss(const OcBcLoss* q, void* stream);" in hdr
    assert "int oc_bc_update(const OcActorCritic* policy, const OcBcLoss* loss, const OcAdam* adam, const OcBcUpdate* update, void* stream);" in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr
    for words in ("c = d_class_weights[a], or 1.0f without d_class_weights", "ce = -lp_a", "d/dl_i = c * (p_i - [i == a])", "d/dv   = +0.0f",
                  "the lowest i with l_i == m", "ce = +inf", "stays finite", "{count, sum c * ce, number correct, sum c}",
                  "Keras's class_weight convention", "the host checks the\n * pointer's alignment and nothing else", "before the FIRST launch",
                  "on those RAW gradients"):
        assert words in hdr, words


# ------------------------------------------------------------------------------------------ H3: the plans
def test_h3_the_plans_words_carry_their_numbers():
    from overcooked_ai_amd import _lib, bc, learner, policy, ppo_loss

    hdr = _header()
    Pn = bc.partial_samples()
    assert Pn == ppo_loss.partial_samples() == 1024 and "P = %d\n * (oc_bc_loss_plan states it)" % Pn in hdr
    assert bc.plan_bc_loss(4096 * Pn, index=True, class_weights=True) in hdr
    for M in (1, Pn, Pn + 1, 65 * Pn + 3):
        text = bc.plan_bc_loss(M, index=bool(M & 1), class_weights=True, gradients=M != Pn, loss_out=M == Pn)
        grid = (M + Pn - 1) // Pn
        assert text.startswith("k_bc_loss<GRAD=%s> grid=%d, 256 lanes (one per sample, 4 tiles of 256), %d samples per partial, index=%s class_weights=yes loss_out=%s"
                               % ("false" if M == Pn else "true", grid, Pn, "yes" if M & 1 else "no", "yes" if M == Pn else "no")), text
        assert text.endswith("+ k_bc_loss_stats grid=1, 64 lanes, %d partial(s) (with d_stats)" % grid)
    assert bc.plan_bc_loss(0) == "nothing to launch (no samples)"
    whole = bc.plan_bc_update(16 * 4096, 4096)
    assert whole.startswith("16 minibatch(es) of 4096 rows (the last 4096), no host synchronisation")
    for quoted in (policy.plan(4096, index=True), bc.plan_bc_loss(4096, index=True), policy.plan(4096, index=True, backward=True), learner.plan_adam()):
        assert "[" + quoted + "]" in whole, quoted
    assert whole.endswith("scratch: logits 4096 x 6 f32, values 4096 f32, grad_logits 4096 x 6 f32, grad_values 4096 f32, loss partials 4 x 4 f64, "
                          "policy partials 32 x 10823 f32, gradients 10823 f32; out: stats 16 x 8 f64, info 16 x 4 f64")
    for n, M, in_dim in ((1, 1, 96), (33, 33, 56), (1000, 64, 96), (70000, 32801, 96), (5, 4096, 136), (12000, 2000, 136)):
        text = bc.plan_bc_update(n, M, in_dim, 64, 64, class_weights=True)
        K, rows = (n + M - 1) // M, min(n, M)
        assert text.startswith("%d minibatch(es) of %d rows (the last %d)" % (K, rows, n - (K - 1) * M)), text
        assert "k_bc_loss<GRAD=true>" in text and "class_weights=yes" in text
        assert bc.scratch_rows(n, M, in_dim, 64, 64) == (rows, (rows + Pn - 1) // Pn, *policy.partials_shape(rows, in_dim, 64, 64)), text
        assert "out: stats %d x 8 f64, info %d x 4 f64" % (K, K) in text
    assert bc.plan_bc_update(0, 64).startswith("nothing to launch (no index); scratch: ")
    L = _lib.load()
    out = ctypes.create_string_buffer(2048)
    assert L.oc_bc_loss_plan(10, 0, 0, 1, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_bc_loss_plan: no output buffer"
    assert L.oc_bc_update_plan(10, 5, 96, 64, 64, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_bc_update_plan: no output buffer"
    for M, why in ((-1, "n_minibatch < 0"), (2 ** 38 + 1, "n_minibatch above 2^38")):
        assert L.oc_bc_loss_plan(M, 0, 0, 1, 0, out, len(out)) == EINVAL and L.oc_last_error().decode() == "oc_bc_loss: " + why
    for args, why in (((97, 64, 64), "policy.in_dim must be a feature length"), ((96, 0, 64), "policy.h1 and policy.h2 must be in 1..64")):
        assert L.oc_bc_update_plan(10, 5, *args, 0, out, len(out)) == EINVAL and L.oc_last_error().decode().startswith("oc_bc_update: " + why)
    for n, M, why in ((-1, 5, "n_index < 0"), (2 ** 31, 5, "n_index must be below 2^31"), (10, 0, "minibatch < 1"), (10, -3, "minibatch < 1")):
        assert L.oc_bc_update_plan(n, M, 96, 64, 64, 0, out, len(out)) == EINVAL and L.oc_last_error().decode() == "oc_bc_update: " + why


# ------------------------------------------------------------------------------------------ H4: the refusals
_LOSS = dict(d_actions=P + 1, d_class_weights=P, n_samples=3000, d_logits=P + 8, d_index=P + 4, first_sample=0, n_minibatch=1000, d_grad_logits=P + 8,
             d_grad_values=P + 4, d_loss_out=P + 4, d_partials=P + 8, d_stats=P + 8)


def _loss_refusals():
    """(the fields that differ from an accepted call, the refusal's words) of oc_bc_loss's own checks on the arrays a caller of
    several stages hands over as well: those of the batch side"""
    return [(dict(d_actions=None), "NULL d_actions or d_logits"),
            (dict(d_class_weights=P + 2), "d_class_weights, d_index, d_grad_values and d_loss_out must be 4-byte aligned"),
            (dict(n_samples=-1), "n_samples < 0"), (dict(n_samples=2 ** 31), "n_samples must be below 2^31 with d_index")]


def test_h4_oc_bc_loss_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    fields = [f for f, _ in _lib.OcBcLoss._fields_]

    def call(**kw):
        v = dict(_LOSS, **kw)
        q = _lib.OcBcLoss(*[v[f] for f in fields])
        return L.oc_bc_loss(ctypes.byref(q), None), L.oc_last_error().decode()

    assert (L.oc_bc_loss(None, None), L.oc_last_error().decode()) == (EINVAL, "oc_bc_loss: loss is NULL")
    four = "d_class_weights, d_index, d_grad_values and d_loss_out must be 4-byte aligned"
    eight = "d_logits, d_grad_logits, d_partials and d_stats must be 8-byte aligned"
    together = "d_grad_logits and d_grad_values must be given together"
    inside = "first_sample .. first_sample + n_minibatch must lie inside 0 .. n_samples without d_index"
    cases = _loss_refusals() + [
        (dict(d_logits=None), "NULL d_actions or d_logits"), (dict(d_grad_logits=None), together), (dict(d_grad_values=None), together),
        (dict(d_index=P + 2), four), (dict(d_grad_values=P + 2), four), (dict(d_loss_out=P + 1), four),
        (dict(d_logits=P + 4), eight), (dict(d_grad_logits=P + 4), eight), (dict(d_partials=P + 4), eight), (dict(d_stats=P + 4), eight),
        (dict(n_minibatch=-1), "n_minibatch < 0"), (dict(n_minibatch=2 ** 38 + 1), "n_minibatch above 2^38"),
        (dict(d_index=None, first_sample=-1), inside), (dict(d_index=None, first_sample=2001), inside), (dict(d_index=None, first_sample=3001, n_minibatch=0), inside),
        (dict(d_index=None, n_minibatch=3001), inside), (dict(d_partials=None), "d_stats needs d_partials")]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith("oc_bc_loss: " + why), (kw, rc, msg)
    # accepted, and nothing to launch: no rows, no stats (in the gradient mode and in evaluation mode)
    assert call(n_minibatch=0, d_stats=None)[0] == 0
    assert call(n_minibatch=0, d_stats=None, d_partials=None, d_grad_logits=None, d_grad_values=None, d_index=None, first_sample=3000)[0] == 0


def test_h4_oc_bc_update_makes_every_refusal_of_every_stage_before_its_first_launch():
    """With stand-in pointers, a NULL stream and more than one minibatch: a refusal behind the first launch would come behind a fault,
    and this host has no device.  The stages' refusals come in their own words under oc_bc_update's name."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    loss_fields = [f for f, _ in _lib.OcBcLoss._fields_]
    upd_fields = [f for f, _ in _lib.OcBcUpdate._fields_ if f != "grads"]

    def call(pol=(), loss=(), ad=(), upd=(), **kw):
        v = _defaults()
        v.update(d_grad_scale=None, d_info=None)
        q = dict(d_actions=P + 1, d_class_weights=P, n_samples=3000, d_logits=None, d_index=None, first_sample=0, n_minibatch=0, d_grad_logits=None,
                 d_grad_values=None, d_loss_out=None, d_partials=None, d_stats=None)
        u = dict(d_features=P, n_feature_rows=3000, d_index=P, n_index=2500, minibatch=1000, d_logits=P + 8, d_values=P + 4, d_grad_logits=P + 8,
                 d_grad_values=P + 4, d_loss_partials=P, d_policy_partials=P, d_stats=P, d_info=P)
        for k, x in kw.items():
            if k.startswith("q_"):
                q[k[2:]] = x
            elif k.startswith("u_"):
                u[k[2:]] = x
            else:
                v[k] = x
        s = _adam_structs(v)
        pol, ad = (s[0] if pol == () else pol), (s[2] if ad == () else ad)
        loss = _lib.OcBcLoss(*[q[f] for f in loss_fields]) if loss == () else loss
        if upd == ():
            upd = _lib.OcBcUpdate(**{f: u[f] for f in upd_fields}, grads=s[1])
        ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        return L.oc_bc_update(ref(pol), ref(loss), ref(ad), ref(upd), None), L.oc_last_error().decode()

    eight = "d_logits, d_grad_logits, d_partials and d_stats must be 8-byte aligned"
    cases = [(dict(pol=None), "policy is NULL"), (dict(loss=None), "loss is NULL"), (dict(ad=None), "adam is NULL"), (dict(upd=None), "update is NULL"),
             (dict(u_n_index=-1), "n_index < 0"), (dict(u_n_index=2 ** 31), "n_index must be below 2^31"), (dict(u_minibatch=0), "minibatch < 1"),
             (dict(u_d_index=None), "update.d_index is NULL"), (dict(u_d_stats=None), "NULL update.d_stats or update.d_info"),
             (dict(u_d_info=None), "NULL update.d_stats or update.d_info"), (dict(u_d_loss_partials=None), "update.d_loss_partials is NULL"),
             (dict(u_d_info=P + 4), "update.d_info must be 8-byte aligned"),
             # oc_policy_forward's
             (dict(u_d_features=None), "rows.d_features is NULL"), (dict(u_d_features=P + 8), "rows.d_features must be 16-byte aligned"),
             (dict(u_d_index=P + 2), "rows.d_index must be 4-byte aligned"), (dict(u_n_feature_rows=-1), "rows.n_feature_rows < 0"),
             (dict(u_n_feature_rows=2 ** 31), "rows.n_feature_rows must be below 2^31 with d_index"),
             (dict(u_d_logits=None), "NULL d_logits or d_values"), (dict(u_d_values=None), "NULL d_logits or d_values"),
             (dict(u_d_logits=P + 4), "d_logits must be 8-byte aligned"), (dict(u_d_values=P + 2), "d_values must be 4-byte aligned"),
             # oc_policy_backward's
             (dict(u_d_grad_logits=None), "NULL d_grad_logits or d_grad_values"), (dict(u_d_grad_values=None), "NULL d_grad_logits or d_grad_values"),
             (dict(u_d_grad_logits=P + 4), "d_grad_logits must be 8-byte aligned"), (dict(u_d_grad_values=P + 2), "d_grad_values must be 4-byte aligned"),
             (dict(u_d_policy_partials=None), "d_partials is NULL"), (dict(u_d_policy_partials=P + 2), "d_partials must be 4-byte aligned"),
             # oc_bc_loss's (what the stages before it have not refused already)
             (dict(u_d_loss_partials=P + 4), eight), (dict(u_d_stats=P + 4), eight)]
    cases += [({"q_" + k: x for k, x in kw.items()}, why) for kw, why in _loss_refusals()]
    # oc_adam_step's (d_grad_scale and d_info are the call's own)
    cases += [(kw, why) for kw, why in _adam_refusals() if not set(kw) & {"d_grad_scale", "d_info"}]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith("oc_bc_update: " + why), (kw, rc, msg)
    # accepted, and nothing to launch: no index entries (every check is made all the same: see the refusal below)
    assert call(u_n_index=0)[0] == 0 and call(u_n_index=0, u_minibatch=1)[0] == 0 and call(u_n_index=0, q_d_class_weights=None)[0] == 0
    rc, msg = call(u_n_index=0, lr=-1.0)
    assert rc == EINVAL and msg == "oc_bc_update: adam.lr must be finite and >= 0"


# ------------------------------------------------------------------------------------------ H5: the end-to-end run in float64
def test_h5_the_reference_run_improves():
    """The float64 restatement of the run tests/test_gpu_bc.py makes on the device: 2 048 rows, minibatches of 256, three epochs.  Its
    loss falls and its accuracy rises by margins that leave the device's midpoints meaningful; the four numbers are the recorded ones."""
    e = BC.E2E
    feats, actions, student, perms = BC.e2e_inputs()
    assert feats.shape == (2048, 96) and actions.shape == (2048,) and perms.shape == (3, 2048) and e.minibatch == 256
    assert len(np.unique(actions)) == 6 and all(sorted(p.tolist()) == list(range(2048)) for p in perms)
    losses, acc0, acc1 = BC.e2e_reference()
    print("float64 run: loss %.4f -> %.4f over %d minibatches, accuracy %.4f -> %.4f" % (losses[0], losses[-1], len(losses), acc0, acc1))
    assert len(losses) == 24 and losses[-1] < 0.6 * losses[0] and acc1 > acc0 + 0.3
    assert np.allclose((losses[0], losses[-1], acc0, acc1), BC.E2E_RECORDED, atol=5e-4, rtol=0)


# ------------------------------------------------------------------------------------------ the Python surface
def test_the_python_surface_validates_its_arguments():
    import torch

    from overcooked_ai_amd.bc import BCLearner, BcStats, bc_loss
    from overcooked_ai_amd.policy import ActorCritic

    pol = ActorCritic(96, 40, 24, seed=3)
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=0.0), dict(max_grad_norm=0.0), dict(class_weights=(1.0,) * 5),
               dict(class_weights=(1, 1, 1, 1, 1, -0.5)), dict(class_weights=(1, 1, 1, 1, 1, float("nan"))), dict(class_weights=(1, 1, 1, 1, 1, float("inf"))),
               dict(class_weights="balanced")):
        with pytest.raises(ValueError):
            BCLearner(pol, **kw)
    with pytest.raises(ValueError, match="must be an ActorCritic"):
        BCLearner(torch.nn.Linear(2, 2))
    learner = BCLearner(pol, class_weights=(1, 2, 3, 4, 0, 6), max_grad_norm=0.1)
    assert learner.adam.lr == 1e-3 and learner.adam.max_grad_norm == 0.1 and learner.class_weights.tolist() == [1.0, 2.0, 3.0, 4.0, 0.0, 6.0]
    assert BcStats._fields == ("tensor", "count", "loss", "accuracy", "mean_weight", "inv_count")
    feats, acts, index = torch.zeros((24, 96)), torch.zeros(24, dtype=torch.uint8), torch.zeros(5, dtype=torch.int32)
    for call in (lambda: learner.update(feats, acts, index), lambda: learner.epoch(feats, acts, index, 2), lambda: learner.evaluate(feats, acts),
                 lambda: bc_loss(torch.zeros((5, 6)), acts, index)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    for logits, actions, kw in ((torch.zeros((5, 5)), acts, {}), (torch.zeros((5, 6), dtype=torch.float64), acts, {}), (torch.zeros((5, 6)), acts.long(), {}),
                                (torch.zeros((5, 6)), acts, dict(index=index.long())), (torch.zeros((5, 6)), acts, dict(index=index[:4])),
                                (torch.zeros((5, 6)), acts, dict(first=20)), (torch.zeros((5, 6)), acts, dict(first=-1)),
                                (torch.zeros((5, 6)), acts, dict(class_weights=(1, 2, 3)))):
        with pytest.raises(ValueError):
            bc_loss(logits, actions, **kw)
