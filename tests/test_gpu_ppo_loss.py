"""oc_ppo_loss on the device: every case of tests/ppo_loss_cases.py against the float64 reference within the tolerances recorded
there, the partial sums and the stats, repeatability, the isolation of left-out samples, split calls, `ppo_loss` under autograd and
the whole chain from a collecting env to the loss of its minibatches."""
import ctypes
import types

import numpy as np
import pytest
import torch

import partner_cases as PTC
import ppo_loss_cases as PC
from gpu_support import GUARD, gpu, guarded, guards_untouched  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = PC.FILL
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8,
          np.dtype(np.int32): torch.int32}


def placed(a, align, dev):
    """A device copy of numpy array `a` (None stays None) whose first byte lies `align` bytes behind a multiple of 2 * align: the
    minimum alignment include/oc_amd.h allows, which a fresh allocation never has (align 1: an odd address)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    raw = torch.zeros((a.nbytes + 2 * align + 64,), dtype=torch.uint8, device=dev)
    off = align + (-raw.data_ptr()) % (2 * align)
    part = raw[off:off + a.nbytes]
    part.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))  # (a byte copy: NaN payloads arrive as they are)
    t = part.view(_TORCH[a.dtype]).view(a.shape)
    assert t.data_ptr() % (2 * align) == align
    return t


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


Out = types.SimpleNamespace


def run(c, a, dev, terms=None, stats=True, rows=None):
    """One oc_ppo_loss call through the C-ABI on placed inputs and sentinel-filled outputs between guard rows; rows = (lo, hi): the
    call of minibatch rows lo .. hi - 1 alone.  Numpy arrays: grad_logits, grad_values, partials, stats, terms (None where not asked)."""
    from overcooked_ai_amd import _lib

    lo, hi = rows if rows is not None else (0, a.M)
    M = hi - lo
    terms = c.terms if terms is None else terms
    d_batch = [placed(a.actions, 1, dev), placed(a.logp_old, 4, dev), placed(a.advantages, 4, dev), placed(a.targets, 4, dev),
               placed(a.seat, 1, dev), placed(a.logits_old, 8, dev), placed(a.moments, 8, dev)]
    d_mini = [placed(a.logits[lo:hi], 16, dev), placed(a.values[lo:hi], 4, dev), placed(a.index[lo:hi] if a.index is not None else None, 4, dev)]
    K = (M + PC.partial_samples() - 1) // PC.partial_samples()
    gl, g_gl = guarded(M, (6,), torch.float32, FILL, dev, before=2)
    gv, g_gv = guarded(M, (), torch.float32, FILL, dev, before=GUARD)
    assert gl.data_ptr() % 32 == 16 and gv.data_ptr() % 8 == 4
    outs = [("grad_logits", gl, g_gl), ("grad_values", gv, g_gv)]
    part = st = tm = None
    if stats:
        part, g_part = guarded(K, (6,), torch.float64, FILL, dev, before=1)
        st, g_st = guarded(1, (8,), torch.float64, FILL, dev, before=1)
        outs += [("partials", part, g_part), ("stats", st, g_st)]
    if terms:
        tm, g_tm = guarded(M, (4,), torch.float32, FILL, dev, before=GUARD)
        assert tm.data_ptr() % 32 == 16
        outs.append(("terms", tm, g_tm))
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    q = _lib.OcPpoLoss(*[ptr(t) for t in d_batch], a.S, *[ptr(t) for t in d_mini], a.first + lo if a.index is None else 0, M,
                       ptr(gl), ptr(gv), ptr(part), ptr(st), ptr(tm), c.clip, c.vf_clip, c.vf_coeff, c.ent, c.kl)
    L = _lib.load()
    rc = L.oc_ppo_loss(ctypes.byref(q), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for what, _, guards in outs:
        guards_untouched(c.id, what, guards, FILL)
    return Out(grad_logits=gl.cpu().numpy(), grad_values=gv.cpu().numpy(), partials=part.cpu().numpy() if stats else None,
               stats=st.view(8).cpu().numpy() if stats else None, terms=tm.cpu().numpy() if terms else None)


def same_bits(x, y):
    return all((p is None and q is None) or np.array_equal(bits(p), bits(q)) for p, q in
               ((getattr(x, k), getattr(y, k)) for k in ("grad_logits", "grad_values", "partials", "stats", "terms")))


def check_against_reference(c, a, got, ref):
    """Terms everywhere, gradients outside the bands, within DEVICE_TOL of the float64 reference; left-out rows +0.0f by bit pattern."""
    near_ratio, near_vf = PC.bands(c, ref)
    figures = dict(grad_logits=PC.rel_error(got.grad_logits, ref.grad_logits, ~near_ratio),
                   grad_values=PC.rel_error(got.grad_values, ref.grad_values, ~near_vf))
    if got.terms is not None:
        figures["terms"] = PC.rel_error(got.terms, ref.terms)
    print("%s: largest error / max(1, |reference|): %s; tolerance %.3g; rows in a band %d + %d"
          % (c.id, ", ".join("%s %.3g" % kv for kv in figures.items()), PC.DEVICE_TOL, near_ratio.sum(), near_vf.sum()))
    for what, err in figures.items():
        assert err <= PC.DEVICE_TOL, (c.id, what, err)
    out = ref.left_out
    assert not bits(got.grad_logits[out]).any() and not bits(got.grad_values[out]).any()
    assert got.terms is None or not bits(got.terms[out]).any()
    assert not (got.grad_logits == FILL).any() and not (got.grad_values == FILL).any()  # (every row written)


def check_sums(c, got, ref, terms):
    """count exact; each sum within count * 2^-53 * sum |x| of numpy's float64 sum of the device's own `terms`; the stats the ascending
    sum of the partials and the means derived from it, bit for bit; the clipped count off the reference's by banded rows at most."""
    Pn = PC.partial_samples()
    K = (c.M + Pn - 1) // Pn
    assert got.partials.shape == (K, 6)
    total = np.zeros(6)
    for k in range(K):
        keep = ~ref.left_out[Pn * k:Pn * k + Pn]
        assert got.partials[k, 0] == keep.sum(), (c.id, k)
        t = terms[Pn * k:Pn * k + Pn].astype(np.float64)[keep]
        for col, x in ((1, -t[:, 0]), (2, t[:, 1]), (3, t[:, 2]), (4, t[:, 3])):
            assert abs(got.partials[k, col] - x.sum()) <= keep.sum() * 2.0 ** -53 * np.abs(x).sum(), (c.id, k, col)
        total = total + got.partials[k]
    assert np.array_equal(bits(got.stats), bits(PC.stats_of(total, c))), (c.id, got.stats, PC.stats_of(total, c))
    near_ratio, _ = PC.bands(c, ref)
    assert abs(total[5] - ref.sums[5]) <= near_ratio.sum() and total[0] == ref.sums[0]
    tol = mean_tolerances(c, ref)
    for i in (1, 2, 3, 4, 5):  # total and the four means, against the reference's
        assert abs(got.stats[i] - ref.stats[i]) <= tol[i], (c.id, PC.STATS[i], got.stats[i], ref.stats[i], tol[i])
    assert abs(got.stats[6] - ref.stats[6]) <= near_ratio.sum() / max(total[0], 1) and got.stats[7] == ref.stats[7]


def mean_tolerances(c, ref):
    """What the per-sample tolerance leaves of d_stats[1..5]: a mean of terms that are each within DEVICE_TOL * max(1, |term|) is within
    DEVICE_TOL * mean max(1, |term|); the total is the four means weighted by the coefficients.  [8], indices 1..5 filled."""
    keep = ~ref.left_out
    tol = np.zeros(8)
    if keep.any():
        tol[2:6] = PC.DEVICE_TOL * np.maximum(1.0, np.abs(ref.terms[keep])).mean(0)
        tol[1] = tol[2] + float(np.float32(c.vf_coeff)) * tol[3] + float(np.float32(c.ent)) * tol[4] + float(np.float32(c.kl)) * tol[5]
    return tol


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_every_case_is_within_the_tolerance_of_the_f64_reference(c, gpu):
    a, ref = PC.arrays_of(c), PC.reference_of(c)
    got = run(c, a, gpu)
    check_against_reference(c, a, got, ref)
    terms = got.terms
    if terms is None:  # a case without d_terms_out: the terms of a second call that asks for them, which changes nothing else
        again = run(c, a, gpu, terms=True)
        terms, again.terms = again.terms, None
        assert same_bits(got, again), c.id
        assert PC.rel_error(terms, ref.terms) <= PC.DEVICE_TOL and not bits(terms[ref.left_out]).any()
    check_sums(c, got, ref, terms)


def test_a_second_call_gives_identical_bytes(gpu):
    for c in (next(c for c in PC.CASES if c.id.endswith("-big")), next(c for c in PC.CASES if c.M == 257 and c.mode == "contiguous")):
        a = PC.arrays_of(c)
        assert same_bits(run(c, a, gpu), run(c, a, gpu)), c.id


ISOLATION = [c for c in PC.CASES if c.seat != "none" and c.M >= 255 and PC.reference_of(c).sums[0] > 0][:4]


@pytest.mark.parametrize("c", ISOLATION, ids=lambda c: c.id)
def test_nan_in_every_input_of_a_left_out_sample_changes_no_output_bit(c, gpu):
    dirty = PC.poisoned(c)
    assert np.isnan(dirty.logits).any() and np.isnan(dirty.advantages).any() and PC.reference_of(c).left_out.any()
    assert same_bits(run(c, PC.arrays_of(c), gpu, terms=True), run(c, dirty, gpu, terms=True))


def test_the_terms_output_changes_no_gradient_and_no_stat(gpu):
    for c in [c for c in PC.CASES if c.terms and c.M in (65, 488)][:3]:
        a = PC.arrays_of(c)
        with_terms, without = run(c, a, gpu, terms=True), run(c, a, gpu, terms=False)
        assert without.terms is None
        with_terms.terms = None
        assert same_bits(with_terms, without), c.id
        no_stats = run(c, a, gpu, stats=False)  # (neither do the sums)
        assert np.array_equal(bits(no_stats.grad_logits), bits(without.grad_logits))
        assert np.array_equal(bits(no_stats.grad_values), bits(without.grad_values))


def test_one_call_of_488_rows_equals_calls_of_200_and_288(gpu):
    for c in (next(c for c in PC.CASES if c.id.endswith("-split")), next(c for c in PC.CASES if c.M == 488 and c.mode == "indexed")):
        a = PC.arrays_of(c)
        whole, head, tail = run(c, a, gpu), run(c, a, gpu, rows=(0, 200)), run(c, a, gpu, rows=(200, 488))
        assert np.array_equal(bits(whole.grad_logits), bits(np.concatenate([head.grad_logits, tail.grad_logits]))), c.id
        assert np.array_equal(bits(whole.grad_values), bits(np.concatenate([head.grad_values, tail.grad_values]))), c.id
        assert head.stats[0] + tail.stats[0] == whole.stats[0]


def test_no_rows_launch_nothing_and_zero_the_stats(gpu):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    st, g_st = guarded(1, (8,), torch.float64, FILL, gpu, before=1)
    buf = torch.full((64,), FILL, dtype=torch.float64, device=gpu)
    p = buf.data_ptr()
    q = _lib.OcPpoLoss(p, p, p, p, None, None, None, 40, p, p, None, 40, 0, p, p, p, st.data_ptr(), None, 0.05, 10.0, 0.5, 0.1, 0.0)
    assert L.oc_ppo_loss(ctypes.byref(q), torch.cuda.current_stream(gpu).cuda_stream) == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(gpu)
    assert not bits(st.cpu().numpy()).any() and bool((buf == FILL).all())
    guards_untouched("M=0", "stats", g_st, FILL)


# ------------------------------------------------------------------------------------------ ppo_loss under autograd
def _learner_batch(a, dev):
    from overcooked_ai_amd.ppo_loss import LearnerBatch

    t = lambda x: torch.from_numpy(np.array(x)).to(dev) if x is not None else None  # noqa: E731
    return LearnerBatch(t(a.actions), t(a.logp_old), t(a.advantages), t(a.targets), t(a.seat), t(a.logits_old), t(a.moments))


def _torch_loss64(out64, sample, batch, c):
    """The textbook loss in torch float64 on the device from the head's output [M, 7] (its logits and values as the f32 numbers
    ppo_loss is given): the mean over the learner samples, their mask, and what the per-sample tolerance leaves of that mean."""
    f32 = np.float32
    s = sample.long()
    inside = (s >= 0) & (s < batch.actions.shape[0])
    s = torch.where(inside, s, torch.zeros_like(s))  # (an index outside the batch names no sample, and must not be followed here either)
    keep = inside & (batch.actions[s] <= 5)
    if batch.seat is not None:
        keep &= batch.seat[s >> 1].long() != (s & 1)
    # the learner rows alone: a left-out row's NaN would reach the gradients through a product with 0
    out64, s, everyone = out64[keep], s[keep], keep
    keep = torch.ones_like(s, dtype=torch.bool)
    logits = out64[:, :6].float().double()
    values = out64[:, 6].float().double()
    act = batch.actions[s].long()
    A = batch.advantages[s].double()
    if batch.moments is not None:
        n, m1, m2 = batch.moments
        mean = m1 / n
        A = (A - mean) / torch.clamp(torch.sqrt(torch.clamp(m2 / n - mean * mean, min=0.0)), min=1e-4)
    lp = torch.log_softmax(logits, -1)
    logp = lp.gather(1, act[:, None])[:, 0]
    ratio = torch.exp(logp - batch.logp_old[s].double())
    lo, hi = float(f32(1) - f32(c.clip)), float(f32(1) + f32(c.clip))
    surr = torch.min(ratio * A, torch.clamp(ratio, lo, hi) * A)
    H = -(lp.exp() * lp).sum(-1)
    vf = (values - batch.targets[s].double()) ** 2
    vfc = torch.clamp(vf, max=float(f32(c.vf_clip)))
    lq = torch.log_softmax(batch.logits_old[s].double(), -1)
    kl = (lq.exp() * (lq - lp)).sum(-1)
    coeff = [1.0, float(f32(c.vf_coeff)), float(f32(c.ent)), float(f32(c.kl))]
    per = -surr + coeff[1] * vfc - coeff[2] * H + coeff[3] * kl
    tol = sum(k * torch.clamp(t.detach().abs(), min=1.0)[keep].mean() for k, t in zip(coeff, (surr, vfc, H, kl))) * PC.DEVICE_TOL
    banded = ((ratio - lo).abs() <= PC.RATIO_BAND) | ((ratio - hi).abs() <= PC.RATIO_BAND) | ((vf - c.vf_clip).abs() <= PC.VF_BAND * c.vf_clip)
    return per.sum() / keep.sum(), everyone, float(tol), int(banded.sum())


def test_ppo_loss_backward_gives_a_policy_head_the_gradients_of_the_f64_restatement(gpu):
    """A 96 -> 6 + 1 linear head in float64 on random features, its output rounded to the f32 logits and values ppo_loss takes (the
    casts carry gradients unchanged), so that both sides start from the same f32 numbers and the matrix products of backward add no
    f32 rounding of their own.  M = 488 indexed rows, seats, moments, old logits, every coefficient non-zero.  Bound of a parameter's
    gradient sum_m g[m, j] x[m, k] / count: the per-sample tolerance of g, DEVICE_TOL * max(1, |g|), summed with |x| — at most that
    tolerance times the row norm of the features —, plus 2^-22 of the terms' magnitudes for the two f32 roundings of backward (the
    scale grad_out / count, and its product with g)."""
    from overcooked_ai_amd.ppo_loss import ppo_loss

    c = PC.Case("head", 488, "indexed", 0, "mixed", True, True, False, 0.05, 10.0, 0.5, 0.2, 0.2, False, 77)
    a = PC.arrays_of(c)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((c.M, 96))).to(gpu)
    head = torch.nn.Linear(96, 7).double().to(gpu)
    index = torch.from_numpy(a.index.copy()).to(gpu)
    # the collecting policy's logits are a perturbation of the head's own and the targets lie around its values, so that the ratios and
    # the squared errors lie on both sides of their clips (on the host: where the index repeats a sample, its last row decides)
    out0 = head(x).detach().cpu().numpy()
    inside = (a.sample >= 0) & (a.sample < a.S)
    old, targets = a.logits_old.copy(), a.targets.copy()
    old[a.sample[inside]] = (out0[inside, :6] + 0.05 * rng.standard_normal((c.M, 6))[inside]).astype(np.float32)
    targets[a.sample[inside]] = (out0[inside, 6] + 2 * rng.standard_normal(c.M)[inside]).astype(np.float32)
    logp_old = np.take_along_axis(PC._log_softmax64(old), np.minimum(a.actions, 5)[:, None].astype(np.int64), 1)[:, 0].astype(np.float32)
    logp_old[a.actions > 5] = np.nan
    batch = _learner_batch(types.SimpleNamespace(actions=a.actions, logp_old=logp_old, advantages=a.advantages, targets=targets, seat=a.seat,
                                                 logits_old=old, moments=a.moments), gpu)
    hyper = dict(clip_param=c.clip, vf_clip_param=c.vf_clip, vf_loss_coeff=c.vf_coeff, entropy_coeff=c.ent, kl_coeff=c.kl)
    # ---- the library
    out = head(x)
    logits, values = out[:, :6].float().contiguous(), out[:, 6].float().contiguous()
    logits.retain_grad()
    values.retain_grad()
    loss, stats = ppo_loss(logits, values, batch, index, **hyper)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and stats.tensor.dtype == torch.float64 and stats.tensor.shape == (8,)
    assert stats.terms is None and stats.total.data_ptr() == stats.tensor[1:].data_ptr()
    loss.backward()
    got_w, got_b = head.weight.grad.clone(), head.bias.grad.clone()
    g_all = torch.cat([logits.grad.double(), values.grad.double()[:, None]], 1)  # [M, 7]: d loss / d (logits, value) of every row
    head.zero_grad()
    # ---- the float64 restatement
    ref_loss, keep, tol_loss, banded = _torch_loss64(head(x), index, batch, c)
    ref_loss.backward()
    ref_w, ref_b = head.weight.grad, head.bias.grad
    count = float(keep.sum())
    assert banded == 0  # (a row in a band has no defined gradient; this seed has none)
    assert float(stats.count) == count and 100 < count < c.M and loss.item() == float(np.float32(float(stats.total)))
    assert 0 < float(stats.clip_frac) < 1
    assert abs(float(stats.total) - float(ref_loss.detach())) <= tol_loss, (float(stats.total), float(ref_loss.detach()), tol_loss)
    per_sample = PC.DEVICE_TOL * torch.clamp(g_all.abs() * count, min=1.0) / count  # the tolerance of a row's gradients, / count
    xa = x.abs()
    bound_w = per_sample.t() @ xa + 2.0 ** -22 * (g_all.abs().t() @ xa)
    bound_b = per_sample.sum(0) + 2.0 ** -22 * g_all.abs().sum(0)
    err_w, err_b = (got_w - ref_w).abs(), (got_b - ref_b).abs()
    print("head: largest error / bound: weights %.3g, bias %.3g; largest gradient %.3g" % (float((err_w / bound_w).max()),
                                                                                         float((err_b / bound_b).max()), float(ref_w.abs().max())))
    assert bool((err_w <= bound_w).all()) and bool((err_b <= bound_b).all())
    assert float(ref_w.abs().max()) > 1e-3  # (there is a gradient to compare)
    with pytest.raises(ValueError):
        ppo_loss(logits.detach().cpu(), values.detach().cpu(), batch, index, **hyper)


# ------------------------------------------------------------------------------------------ from the env to the loss
def test_the_minibatches_of_a_collected_buffer_give_the_reference_s_losses(gpu):
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy
    from overcooked_ai_amd.ppo_loss import ppo_loss
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    n, T = 33, 5
    policy = DensePolicy(*PTC.glorot(5, PTC.total_of(2), 64, 64), device=gpu)
    env = VecOvercookedMultiAgent("cramped_room", n, horizon=4, obs="features", device=gpu, seed=31, reward_shaping_factor=1.0, use_phi=True,
                                  bc_policy=policy)
    env.set_bc_factor(0.5)
    env.reset()
    buf = TrajectoryBuffer(env, T, keep_obs=True, keep_logits=True)
    rng = np.random.default_rng(3)
    for t in range(T):
        logits = torch.from_numpy((rng.standard_normal((n, 2, 6)) * 2).astype(np.float32)).to(gpu)
        values = torch.from_numpy(rng.uniform(-3, 3, (n, 2)).astype(np.float32)).to(gpu)
        env.step_sampled(logits, into=buf.row(t, values, logits))
    buf.last_values.copy_(torch.from_numpy(rng.uniform(-3, 3, (n, 2)).astype(np.float32)).to(gpu))
    adv, tgt, mom = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, tgt, mom)
    S = T * n * 2
    assert buf.features.shape[:3] == (T, n, 2) and batch.seat.shape == (S // 2,) and batch.logits_old.shape == (S, 6)
    seats = buf.seat.cpu().numpy()
    assert (seats != 255).any() and (seats == 255).any()
    parts = list(buf.minibatches(S // 2 + 1, generator=torch.Generator(device=gpu).manual_seed(9)))
    assert len(parts) == 2 and sorted(torch.cat(parts).tolist()) == list(range(S))
    c = PC.Case("buffer", 0, "indexed", 0, "mixed", True, True, True, 0.05, 10.0, 0.5, 0.2, 0.2, False, 0)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    for k, index in enumerate(parts):
        M = len(index)
        new_logits = (batch.logits_old[index.long()] + 0.05 * torch.from_numpy(rng.standard_normal((M, 6)).astype(np.float32)).to(gpu)).contiguous()
        new_values = (batch.targets[index.long()] + torch.from_numpy((2 * rng.standard_normal(M)).astype(np.float32)).to(gpu)).contiguous()
        new_logits.requires_grad_(True)
        loss, stats = ppo_loss(new_logits, new_values, batch, index, clip_param=c.clip, vf_clip_param=c.vf_clip, vf_loss_coeff=c.vf_coeff,
                               entropy_coeff=c.ent, kl_coeff=c.kl, terms=True)
        loss.backward()
        a = types.SimpleNamespace(S=S, M=M, actions=host(batch.actions), logp_old=host(batch.logp_old), advantages=host(batch.advantages),
                                  targets=host(batch.targets), seat=host(batch.seat), logits_old=host(batch.logits_old), moments=host(mom),
                                  logits=host(new_logits.detach()), values=host(new_values), index=host(index), first=0,
                                  sample=host(index).astype(np.int64))
        ref = PC.loss_f64(c._replace(M=M), a)
        assert 0 < ref.sums[0] < M and float(stats.count) == ref.sums[0], k
        err = PC.rel_error(host(stats.terms), ref.terms)
        print("minibatch %d: %d learner samples of %d, loss %.6f, reference %.6f, largest term error %.3g" % (k, ref.sums[0], M, float(stats.total), ref.stats[1], err))
        assert err <= PC.DEVICE_TOL and abs(float(stats.total) - ref.stats[1]) <= mean_tolerances(c, ref)[1]
        assert loss.item() == float(np.float32(float(stats.total)))
        near_ratio, _ = PC.bands(c, ref)
        grad = host(new_logits.grad).astype(np.float64) * ref.sums[0]  # (backward divided by the count)
        assert PC.rel_error(grad, ref.grad_logits, ~near_ratio) <= PC.DEVICE_TOL + 2.0 ** -22
