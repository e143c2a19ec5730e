"""oc_bc_loss and oc_bc_update on the device, through the C-ABI on inputs at the header's minimum alignments and sentinel-filled
outputs between guards, and through `bc.bc_loss` / `bc.BCLearner`.

G1  every case of tests/bc_cases.py within DEVICE_TOL = 4 x F32_ERROR of the float64 reference; left-out rows +0.0f by bit pattern
    in gradients and d_loss_out; d_grad_values +0.0f everywhere; the count and the number of correct rows exact; the loss sum within
    n * 2^-53 * sum |x| of numpy's float64 sum of the device's own d_loss_out; d_stats the ascending sum of the partials, bit for bit.
G2  a call repeats bit for bit; 488 rows = 200 + 288; NaN logits in left-out rows change no output bit; evaluation mode gives the
    partials and stats of the gradient mode bit for bit and stores no gradient.
G3  oc_bc_update with K = 1 = the four entry points one by one, bit for bit: parameters, moments, clock, stats, info, gradients.
G4  K = 3 with a shorter last minibatch = three K = 1 calls; a minibatch whose rows are all left out is skipped.
G5  bc_loss + loss.backward() through a linear head against the float64 restatement; one BCLearner.update within
    learner_cases.update_bound of the float64 chain; a small end-to-end run against its float64 restatement (tests/bc_cases.py:
    e2e_reference); dense_policy() of the trained policy seated through oc_partner_logits.
Observed on an MI355X: G1 largest error 5.97e-7 (the big indexed case; 2.4e-6 allowed); G5 head: largest error / bound 0.003; update:
largest |device step - float64 step| / bound 0.0213; the run: loss 1.9345 -> 0.9401 and accuracy 0.1475 -> 0.6372, the float64 run's
figures to four places."""
import ctypes
import types

import numpy as np
import pytest
import torch

import bc_cases as BC
import learner_cases as LC
import policy_cases as PC
from gpu_support import _TORCH, GUARD, Fenced, bits, gpu, guarded, guards_untouched, same  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = BC.FILL


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


def run(c, a, dev, grads=True, stats=True, rows=None):
    """One oc_bc_loss call through the C-ABI on placed inputs and sentinel-filled outputs between guards; rows = (lo, hi): the call of
    minibatch rows lo .. hi - 1 alone; grads=False: evaluation mode (the gradient arrays are allocated all the same and not handed
    over).  Numpy arrays: grad_logits, grad_values, loss_out, partials, stats (None where not asked)."""
    from overcooked_ai_amd import _lib

    lo, hi = rows if rows is not None else (0, a.M)
    M = hi - lo
    d_in = [placed(a.actions, 1, dev), placed(a.class_weights, 4, dev), placed(a.logits[lo:hi], 8, dev),
            placed(a.index[lo:hi] if a.index is not None else None, 4, dev)]
    K = (M + BC.partial_samples() - 1) // BC.partial_samples()
    gl, g_gl = guarded(M, (6,), torch.float32, FILL, dev, before=1)
    gv, g_gv = guarded(M, (), torch.float32, FILL, dev, before=GUARD)
    lo_, g_lo = guarded(M, (), torch.float32, FILL, dev, before=1)
    assert gl.data_ptr() % 16 == 8 and gv.data_ptr() % 8 == 4 and lo_.data_ptr() % 8 == 4
    outs = [("grad_logits", gl, g_gl), ("grad_values", gv, g_gv), ("loss_out", lo_, g_lo)]
    part = st = None
    if stats:
        part, g_part = guarded(K * 4, (), torch.float64, FILL, dev, before=1)
        st, g_st = guarded(8, (), torch.float64, FILL, dev, before=1)
        assert part.data_ptr() % 16 == 8 and st.data_ptr() % 16 == 8
        outs += [("partials", part, g_part), ("stats", st, g_st)]
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    q = _lib.OcBcLoss(ptr(d_in[0]), ptr(d_in[1]), a.S, ptr(d_in[2]), ptr(d_in[3]), a.first + lo if a.index is None else 0, M,
                      ptr(gl) if grads else None, ptr(gv) if grads else None, ptr(lo_), ptr(part), ptr(st))
    L = _lib.load()
    rc = L.oc_bc_loss(ctypes.byref(q), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for what, _, guards in outs:
        guards_untouched(c.id, what, guards, FILL)
    return types.SimpleNamespace(grad_logits=gl.cpu().numpy(), grad_values=gv.cpu().numpy(), loss_out=lo_.cpu().numpy(),
                                 partials=part.view(K, 4).cpu().numpy() if stats else None, stats=st.cpu().numpy() if stats else None)


def same_outputs(x, y, keys=("grad_logits", "grad_values", "loss_out", "partials", "stats")):
    return all((p is None and q is None) or same(p, q) for p, q in ((getattr(x, k), getattr(y, k)) for k in keys))


def close_sum(got, x):
    """got is the float64 sum of x in some order: within n * 2^-53 * sum |x| of numpy's (an infinite or NaN sum: the same one)"""
    with np.errstate(invalid="ignore"):
        want = x.sum()
    if not np.isfinite(want):
        return same(np.float64(got), np.float64(want)) or (np.isnan(got) and np.isnan(want))
    return abs(got - want) <= len(x) * 2.0 ** -53 * np.abs(x).sum()


def check_case(c, a, got, ref):
    errs = dict(grad_logits=BC.rel_error(got.grad_logits, ref.grad_logits), loss_out=BC.rel_error(got.loss_out, ref.loss))
    print("%s: largest error / max(1, |reference|): %s; tolerance %.3g" % (c.id, ", ".join("%s %.3g" % kv for kv in errs.items()), BC.DEVICE_TOL))
    for what, err in errs.items():
        assert err <= BC.DEVICE_TOL, (c.id, what, err)
    out = ref.left_out
    assert not bits(got.grad_logits[out]).any() and not bits(got.loss_out[out]).any() and not bits(got.grad_values).any(), c.id
    assert not (got.grad_logits == FILL).any() and not (got.loss_out == FILL).any()  # (every row written)
    # ---- the partials and the stats
    Pn = BC.partial_samples()
    K = (c.M + Pn - 1) // Pn
    assert got.partials.shape == (K, 4)
    weight = a.class_weights.astype(np.float64)[np.minimum(a.actions[np.clip(a.sample, 0, a.S - 1)], 5)] if a.class_weights is not None else np.ones(c.M)
    total = np.zeros(4)
    for k in range(K):
        window = slice(Pn * k, Pn * k + Pn)
        keep = ~out[window]
        assert got.partials[k, 0] == keep.sum() and got.partials[k, 2] == ref.correct[window].sum(), (c.id, k)
        assert close_sum(got.partials[k, 1], got.loss_out[window].astype(np.float64)[keep]), (c.id, k)
        assert close_sum(got.partials[k, 3], weight[window][keep]), (c.id, k)
        with np.errstate(invalid="ignore"):
            total = total + got.partials[k]
    assert same(got.stats, BC.stats_of(total)), (c.id, got.stats, BC.stats_of(total))
    assert total[0] == ref.sums[0] and total[2] == ref.sums[2] and got.stats[2] == ref.stats[2] and got.stats[7] == ref.stats[7]
    keep = ~out
    if keep.any() and np.isfinite(ref.stats[1]):  # a mean of terms that are each within DEVICE_TOL * max(1, |term|)
        assert abs(got.stats[1] - ref.stats[1]) <= BC.DEVICE_TOL * np.maximum(1.0, np.abs(ref.loss[keep])).mean(), (c.id, got.stats[1], ref.stats[1])
        assert abs(got.stats[3] - ref.stats[3]) <= 1e-12 * ref.stats[3]
    else:
        assert same(got.stats[1], ref.stats[1]) or (np.isnan(got.stats[1]) and np.isnan(ref.stats[1]))


# ------------------------------------------------------------------------------------------ G1, G2: oc_bc_loss
@pytest.mark.parametrize("c", BC.CASES, ids=lambda c: c.id)
def test_g1_every_case_is_within_the_tolerance_of_the_f64_reference(c, gpu):
    a, ref = BC.arrays_of(c), BC.reference_of(c)
    check_case(c, a, run(c, a, gpu), ref)


def _named(special, M=None):
    return next(c for c in BC.CASES if c.special == special and (M is None or c.M == M))


def test_g2_a_second_call_gives_identical_bytes(gpu):
    for c in (next(c for c in BC.CASES if c.special == "big" and c.weights), next(c for c in BC.CASES if c.M == 257 and c.mode == "contiguous")):
        a = BC.arrays_of(c)
        assert same_outputs(run(c, a, gpu), run(c, a, gpu)), c.id


def test_g2_one_call_of_488_rows_equals_calls_of_200_and_288(gpu):
    for c in (_named("split"), next(c for c in BC.CASES if c.M == 488 and c.mode == "indexed" and not c.special)):
        a = BC.arrays_of(c)
        whole, head, tail = run(c, a, gpu), run(c, a, gpu, rows=(0, 200)), run(c, a, gpu, rows=(200, 488))
        assert same(whole.grad_logits, np.concatenate([head.grad_logits, tail.grad_logits])), c.id
        assert same(whole.loss_out, np.concatenate([head.loss_out, tail.loss_out])), c.id
        assert head.stats[0] + tail.stats[0] == whole.stats[0] and head.partials[0, 2] + tail.partials[0, 2] == whole.partials[0, 2]


@pytest.mark.parametrize("c", [c for c in BC.CASES if c.special in ("invalid", "nan_left_out") or (c.special == "tiles" and c.mode == "indexed")],
                         ids=lambda c: c.id)
def test_g2_nan_logits_in_left_out_rows_change_no_output_bit(c, gpu):
    dirty = BC.poisoned(c)
    assert np.isnan(dirty.logits).any() and BC.reference_of(c).left_out.any()
    clean = BC.arrays_of(c) if c.special != "nan_left_out" else types.SimpleNamespace(**dict(vars(dirty), logits=np.nan_to_num(dirty.logits, nan=1.5)))
    assert same_outputs(run(c, clean, gpu), run(c, dirty, gpu)), c.id


def test_g2_evaluation_mode_gives_the_same_sums_and_stores_no_gradient(gpu):
    for c in (_named("skewed"), _named("tiles", 4 * (BC.partial_samples() // 4) + 1), _named("count0", 65), _named("neginf_at")):
        a = BC.arrays_of(c)
        train, evaluate = run(c, a, gpu), run(c, a, gpu, grads=False)
        assert same_outputs(train, evaluate, ("loss_out", "partials", "stats")), c.id
        assert (evaluate.grad_logits == FILL).all() and (evaluate.grad_values == FILL).all(), c.id
        no_stats = run(c, a, gpu, stats=False)  # (the sums change no gradient)
        assert same_outputs(train, no_stats, ("grad_logits", "grad_values", "loss_out")), c.id


def test_g2_no_rows_launch_nothing_and_zero_the_stats(gpu):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    st, g_st = guarded(8, (), torch.float64, FILL, gpu, before=1)
    buf = torch.full((64,), FILL, dtype=torch.float64, device=gpu)
    p = buf.data_ptr()
    q = _lib.OcBcLoss(p, None, 40, p, None, 40, 0, p, p, p, p, st.data_ptr())
    assert L.oc_bc_loss(ctypes.byref(q), torch.cuda.current_stream(gpu).cuda_stream) == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(gpu)
    assert not bits(st.cpu().numpy()).any() and bool((buf == FILL).all())
    guards_untouched("M=0", "stats", g_st, FILL)


# ------------------------------------------------------------------------------------------ G3, G4: oc_bc_update
HYPER = LC.Hyper(1e-3, 0.9, 0.999, 1e-8, 0.1)


class Update:
    """The device arrays of oc_bc_update calls on one policy case: features, actions, class weights, index, scratch, parameters,
    moments and clock, each Fenced"""

    def __init__(self, c, dev, weights=True, index=None, all_out=False, K=1):
        from overcooked_ai_amd.bc import scratch_rows

        a = PC.arrays_of(c)
        self.c, self.dev, self.dims = c, dev, (c.in_dim, c.h1, c.h2)
        rng = np.random.default_rng(c.seed + 77)
        R = len(a.features)
        actions = rng.choice(6, size=R, p=BC.STAY_SKEW).astype(np.uint8)
        actions[rng.random(R) < 0.03] = 255
        if all_out:
            actions[:] = 255
        index = (a.index if index is None else index).copy()
        self.index_host, self.actions_host, self.R = index, actions, R
        self.cw_host = rng.uniform(0.25, 4.0, 6).astype(np.float32) if weights else None
        self.feats, self.index, self.actions = Fenced(a.features, 16, dev), Fenced(index, 4, dev), Fenced(actions, 1, dev)
        self.cw = Fenced(self.cw_host, 4, dev) if weights else None
        self.M = M = -(-len(index) // K)
        rows, loss_rows, pol_rows, size = scratch_rows(len(index), M, *self.dims)
        f32 = np.float32
        self.logits, self.values = Fenced(np.full((rows, 6), FILL, f32), 8, dev), Fenced(np.full(rows, FILL, f32), 4, dev)
        self.gl, self.gv = Fenced(np.full((rows, 6), FILL, f32), 8, dev), Fenced(np.full(rows, FILL, f32), 4, dev)
        self.lp, self.pp = Fenced(np.full((loss_rows, 4), FILL), 8, dev), Fenced(np.full((pol_rows, size), FILL, f32), 4, dev)
        zeros = [np.zeros(s, f32) for s in LC.shapes(*self.dims)]
        self.p, self.m, self.v, self.g = ([Fenced(x, 4, dev) for x in xs] for xs in (a.weights, zeros, zeros, zeros))
        self.clock = Fenced(LC.CLOCK0, 8, dev)
        self.n_stats = -(-len(index) // M)
        self.stats, self.info = Fenced(np.full((self.n_stats, 8), FILL), 8, dev), Fenced(np.full((self.n_stats, 4), FILL), 8, dev)

    def structs(self):
        from overcooked_ai_amd import _lib

        ptrs = ctypes.c_void_p * 8
        pol = _lib.OcActorCritic(*[f.ptr for f in self.p], *self.dims)
        grads = _lib.OcPolicyGrads(*[f.ptr for f in self.g])
        ad = _lib.OcAdam(ptrs(*[f.ptr for f in self.m]), ptrs(*[f.ptr for f in self.v]), self.clock.ptr, None, None, HYPER.lr, HYPER.beta1, HYPER.beta2,
                         HYPER.eps, HYPER.max_grad_norm)
        return pol, grads, ad

    def loss_struct(self, **kw):
        from overcooked_ai_amd import _lib

        v = dict(d_logits=None, d_index=None, n_minibatch=0, d_grad_logits=None, d_grad_values=None, d_partials=None, d_stats=None)
        v.update(kw)
        return _lib.OcBcLoss(self.actions.ptr, self.cw.ptr if self.cw else None, self.R, v["d_logits"], v["d_index"], 0, v["n_minibatch"],
                             v["d_grad_logits"], v["d_grad_values"], None, v["d_partials"], v["d_stats"])

    def update(self, lo=0, n=None, M=None, k0=0):
        """oc_bc_update on index entries lo .. lo + n - 1 in minibatches of M, stats and info from row k0 on"""
        from overcooked_ai_amd import _lib

        n = len(self.index_host) - lo if n is None else n
        pol, grads, ad = self.structs()
        u = _lib.OcBcUpdate(self.feats.ptr, self.R, self.index.ptr + 4 * lo, n, self.M if M is None else M, self.logits.ptr, self.values.ptr,
                            self.gl.ptr, self.gv.ptr, self.lp.ptr, self.pp.ptr, grads, self.stats.ptr + 64 * k0, self.info.ptr + 32 * k0)
        q = self.loss_struct()
        L = _lib.load()
        rc = L.oc_bc_update(ctypes.byref(pol), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(u), torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)

    def four_calls(self):
        """The same minibatch (the whole index) by the four entry points one by one, with the same scratch"""
        from overcooked_ai_amd import _lib

        n = len(self.index_host)
        pol, grads, ad = self.structs()
        ad.d_grad_scale, ad.d_info = self.stats.ptr + 56, self.info.ptr
        rows = _lib.OcPolicyRows(self.feats.ptr, self.R, self.index.ptr, 0, n)
        q = self.loss_struct(d_logits=self.logits.ptr, d_index=self.index.ptr, n_minibatch=n, d_grad_logits=self.gl.ptr, d_grad_values=self.gv.ptr,
                             d_partials=self.lp.ptr, d_stats=self.stats.ptr)
        L, stream = _lib.load(), torch.cuda.current_stream(self.dev).cuda_stream
        for rc in (lambda: L.oc_policy_forward(ctypes.byref(pol), ctypes.byref(rows), self.logits.ptr, self.values.ptr, stream),
                   lambda: L.oc_bc_loss(ctypes.byref(q), stream),
                   lambda: L.oc_policy_backward(ctypes.byref(pol), ctypes.byref(rows), self.gl.ptr, self.gv.ptr, ctypes.byref(grads), self.pp.ptr, stream),
                   lambda: L.oc_adam_step(ctypes.byref(pol), ctypes.byref(grads), ctypes.byref(ad), stream)):
            assert rc() == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)

    def results(self):
        flat = lambda fs: LC.flat([f.host() for f in fs])  # noqa: E731
        return flat(self.p), flat(self.m), flat(self.v), self.clock.host(), self.stats.host(), self.info.host(), flat(self.g)

    def intact(self):
        fenced = [self.feats, self.index, self.actions, self.logits, self.values, self.gl, self.gv, self.lp, self.pp, self.stats, self.info, self.clock]
        return all(f.intact() for f in fenced + self.p + self.m + self.v + self.g + ([self.cw] if self.cw else []))


def assert_results(x, y, what):
    for name, p, q in zip(("parameters", "first moments", "second moments", "clock", "stats", "info", "gradients"), x, y):
        assert same(p, q), "%s: the %s differ" % (what, name)


def _policy_case(tail):
    return next(c for c in PC.CASES if c.id.endswith(tail))


@pytest.mark.parametrize("tail,weights,all_out", (("96_64_64-1rows-indexed-dense", False, False), ("96_64_64-33rows-indexed-dense", True, False),
                                                  ("96_64_64-488rows-indexed-dense", False, False), ("96_64_64-488rows-indexed-dense", True, False),
                                                  ("96_64_64-488rows-indexed-dense", True, True), ("136_64_64-257rows-indexed-dense", True, False)))
def test_g3_one_minibatch_equals_the_four_calls_bit_for_bit(tail, weights, all_out, gpu):
    c = _policy_case(tail)
    one, four = Update(c, gpu, weights, all_out=all_out), Update(c, gpu, weights, all_out=all_out)
    one.update()
    four.four_calls()
    what = "%s weights %s" % (c.id, weights)
    assert_results(one.results(), four.results(), what)
    assert one.intact() and four.intact(), what + ": guard bytes written"
    stats, info = one.stats.host()[0], one.info.host()[0]
    idx = one.index_host.astype(np.int64)
    inside = (idx >= 0) & (idx < one.R)
    kept = inside & (one.actions_host[np.where(inside, idx, 0)] <= 5)
    assert stats[0] == kept.sum() and not (one.logits.host() == FILL).any() and not (stats == FILL).any() and not (info == FILL).any()
    assert not bits(one.gv.host()).any()  # the value head's upstream gradients: +0.0f
    start = LC.flat(PC.arrays_of(c).weights)
    if all_out:  # count 0: the step is skipped, weights and moments stay
        assert not stats.any() and info[3] == 1.0 and info[2] == 0.0 and one.clock.host().tolist() == [0.0, 1.0, 1.0, 1.0]
        params, m, v = one.results()[:3]
        assert same(params, start) and not bits(m).any() and not bits(v).any()
    else:
        assert stats[0] > 0 and stats[7] == 1.0 / stats[0] and info[3] == 0.0 and info[2] == float(np.float32(stats[7])) and info[0] > 0
        assert one.clock.host()[0] == 1.0 and not same(one.results()[0], start)
        wv, bv = one.g[6].host(), one.g[7].host()
        assert not wv.any() and not bv.any()  # zero gradients for the value head


def test_g4_an_epoch_equals_its_minibatches_one_by_one_and_skips_an_empty_one(gpu):
    c = _policy_case("96_64_64-488rows-indexed-dense")
    base = PC.arrays_of(c).index
    M = -(-len(base) // 3)
    emptied = base.copy()
    emptied[M:2 * M] = -1  # the second minibatch names no sample
    for index, weights in ((base, True), (emptied, False)):
        whole, again, single = (Update(c, gpu, weights, index=index, K=3) for _ in range(3))
        n = len(whole.index_host)
        assert whole.M == M and whole.n_stats == 3 and 0 < n - 2 * M < M  # a shorter last minibatch
        whole.update()
        again.update()
        states = []
        for k in range(3):
            single.update(lo=k * M, n=min(M, n - k * M), M=M, k0=k)  # (K = 1 each, from the weights the one before left)
            states.append(single.results()[:3])
        assert_results(whole.results(), again.results(), "epoch twice")
        assert_results(whole.results(), single.results(), "epoch against its minibatches")
        assert whole.intact() and single.intact()
        stats, info = whole.stats.host(), whole.info.host()
        if index is base:
            assert (stats[:, 0] > 0).all() and not info[:, 3].any() and whole.clock.host()[0] == 3.0 and len({float(x) for x in info[:, 0]}) == 3
        else:
            assert stats[0, 0] > 0 and not stats[1].any() and stats[2, 0] > 0 and info[:, 3].tolist() == [0.0, 1.0, 0.0]
            assert whole.clock.host().tolist()[0] == 2.0 and whole.clock.host()[3] == 1.0
            assert all(same(x, y) for x, y in zip(states[0], states[1]))  # weights and moments untouched by the skipped minibatch
            assert not same(states[1][0], states[2][0])


# ------------------------------------------------------------------------------------------ G5: the Python surface
def test_g5_bc_loss_backward_gives_a_linear_head_the_gradients_of_the_f64_restatement(gpu):
    """A 96 -> 6 linear head in float64 on random features, its output rounded to the f32 logits bc_loss takes (the casts carry
    gradients unchanged), so that both sides start from the same f32 numbers and the matrix products of backward add no f32 rounding
    of their own.  Bound of a parameter's gradient sum_m g[m, j] x[m, k] / count: the per-sample tolerance of g, DEVICE_TOL *
    max(1, |g|), summed with |x|, plus 2^-22 of the terms' magnitudes for the two f32 roundings of backward (the scale grad_out /
    count, and its product with g)."""
    import torch.nn.functional as F

    from overcooked_ai_amd.bc import bc_loss

    c = BC.Case("head", 488, "indexed", 0, True, "skewed", 77)
    a = BC.arrays_of(c)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((c.M, 96))).to(gpu)
    head = torch.nn.Linear(96, 6).double().to(gpu)
    index, actions = torch.from_numpy(a.index.copy()).to(gpu), torch.from_numpy(a.actions.copy()).to(gpu)
    logits = head(x).float().contiguous()
    logits.retain_grad()
    loss, stats = bc_loss(logits, actions, index, class_weights=a.class_weights.copy())
    assert loss.dtype == torch.float32 and loss.dim() == 0 and stats.tensor.dtype == torch.float64 and stats.tensor.shape == (8,)
    assert stats.loss.data_ptr() == stats.tensor[1:].data_ptr() and stats.accuracy.data_ptr() == stats.tensor[2:].data_ptr()
    loss.backward()
    got_w, got_b, g_all = head.weight.grad.clone(), head.bias.grad.clone(), logits.grad.double()
    head.zero_grad()
    # ---- the float64 restatement, on the kept rows
    s = index.long()
    inside = (s >= 0) & (s < a.S)
    s = torch.where(inside, s, torch.zeros_like(s))
    keep = inside & (actions[s] <= 5)
    count = float(keep.sum())
    weight = torch.from_numpy(a.class_weights.astype(np.float64)).to(gpu)
    ref_loss = F.cross_entropy(head(x).float().double()[keep], actions[s][keep].long(), weight=weight, reduction="sum") / count
    ref_loss.backward()
    assert float(stats.count) == count and 100 < count < c.M and loss.item() == float(np.float32(float(stats.loss)))
    ref = BC.bc_f64(c)
    tol_loss = BC.DEVICE_TOL * float(np.maximum(1.0, np.abs(ref.loss[~ref.left_out])).mean())
    assert abs(float(stats.loss) - float(ref_loss.detach())) <= tol_loss
    per_sample = BC.DEVICE_TOL * torch.clamp(g_all.abs() * count, min=1.0) / count
    xa = x.abs()
    bound_w = per_sample.t() @ xa + 2.0 ** -22 * (g_all.abs().t() @ xa)
    bound_b = per_sample.sum(0) + 2.0 ** -22 * g_all.abs().sum(0)
    err_w, err_b = (got_w - head.weight.grad).abs(), (got_b - head.bias.grad).abs()
    print("head: largest error / bound: weights %.3g, bias %.3g; largest gradient %.3g" % (float((err_w / bound_w).max()), float((err_b / bound_b).max()),
                                                                                         float(head.weight.grad.abs().max())))
    assert bool((err_w <= bound_w).all()) and bool((err_b <= bound_b).all()) and float(head.weight.grad.abs().max()) > 1e-3
    with pytest.raises(ValueError):
        bc_loss(logits.detach().cpu(), actions.cpu(), index.cpu())


def test_g5_one_update_lies_within_the_bound_of_the_float64_chain(gpu):
    from overcooked_ai_amd.bc import BCLearner
    from overcooked_ai_amd.policy import ActorCritic

    c = _policy_case("96_64_64-488rows-indexed-dense")
    a = PC.arrays_of(c)
    R = len(a.features)
    index = np.where(a.unstable, -1, a.index).astype(np.int32)  # the rows on the ReLU edge are silenced: they name no row
    assert a.unstable.sum() <= PC.UNSTABLE_CAP * c.M
    rng = np.random.default_rng(78)
    actions = rng.choice(6, size=R, p=BC.STAY_SKEW).astype(np.uint8)
    actions[rng.random(R) < 0.03] = 255
    cw = rng.uniform(0.25, 4.0, 6).astype(np.float32)
    lr, eps = 1e-2, 1e-2
    policy = ActorCritic.from_weights(*a.weights, device=gpu)
    learner = BCLearner(policy, lr, class_weights=cw, eps=eps)
    dev = lambda x: torch.from_numpy(x.copy()).to(gpu)  # noqa: E731
    stats, info = learner.update(dev(a.features), dev(actions), dev(index))
    assert stats.shape == (1, 8) and info.shape == (1, 4) and stats.device.type == "cuda" and all(p.grad is None for p in policy._params())
    stats, info = stats.cpu().numpy()[0], info.cpu().numpy()[0]
    s = learner.scratch(c.M)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    # ---- link 1: the logits within policy_cases' bound of the float64 forward pass
    idx = index.astype(np.int64)
    valid = (idx >= 0) & (idx < R)
    xs = np.where(valid[:, None], a.features[np.where(valid, idx, 0)], np.float32(0)).astype(np.float32)
    _, _, out64 = PC.forward_f64(xs, a.weights)
    got = np.concatenate([host(s["logits"]), host(s["values"])[:, None]], 1)
    assert (np.abs(got - out64) <= PC.forward_bound(xs, a.weights))[valid].all() and not bits(got[~valid]).any()
    # ---- link 2: the head's raw gradients and stats against bc_f64 on those logits
    case = types.SimpleNamespace(S=R, M=c.M, actions=actions, class_weights=cw, logits=host(s["logits"]), index=index, first=0, sample=idx)
    ref = BC.bc_f64(None, case)
    assert BC.rel_error(host(s["grad_logits"]), ref.grad_logits) <= BC.DEVICE_TOL and not bits(host(s["grad_values"])).any()
    count = ref.sums[0]
    assert count == stats[0] > 100 and stats[7] == 1.0 / count and stats[2] == ref.stats[2]
    assert abs(stats[1] - ref.stats[1]) <= BC.DEVICE_TOL * np.maximum(1.0, np.abs(ref.loss[~ref.left_out])).mean()
    # ---- link 3: the raw parameter gradients against the float64 backward pass on those upstream gradients
    up = np.concatenate([host(s["grad_logits"]), host(s["grad_values"])[:, None]], 1)
    up = np.where(valid[:, None], up, np.float32(0)).astype(np.float32)
    back = PC._backward(xs, a.weights, up, np.float64)
    errs = PC.scaled_errors([host(g) for g in s["grads"]], back)
    assert max(errs) <= PC.DEVICE_FACTOR * PC.F32_ERROR, dict(zip(PC.NAMES, errs))
    # ---- link 4: the parameter change against the float64 Adam on those float64 gradients, within update_bound
    g64 = LC.flat(back.grads) / count
    p_old = LC.flat(a.weights).astype(np.float64)
    st, info64 = LC.adam_f64(LC.state0(a.weights, np.float64), LC.split(LC.flat(back.grads), c.in_dim, c.h1, c.h2), LC.Hyper(lr, 0.9, 0.999, eps, None), 1.0 / count)
    p_new = LC.flat([host(p) for p in policy._params()]).astype(np.float64)
    bound = LC.update_bound(g64, LC.flat(back.scales) / count + 2.0 ** -24 * np.abs(g64), float(np.float32(lr)), float(np.float32(eps)), p_old)
    err = np.abs((p_new - p_old) - (st.params - p_old))
    print("largest |device step - float64 step| / bound %.3g; largest step %.3g, smallest bound %.3g" % ((err / bound).max(), np.abs(st.params - p_old).max(), bound.min()))
    assert (err <= bound).all() and np.abs(st.params - p_old).max() > 100 * bound.min()
    assert info[3] == 0.0 and info[1] == 1.0 and abs(info[0] - info64[0]) <= 1e-3 * info64[0]


def test_g5_a_small_run_learns_what_its_float64_restatement_learns(gpu):
    """2 048 rows, labels from a random teacher, minibatches of 256, three epoch() calls with the reference's permutations and initial
    weights.  The device's last-minibatch loss lies below the midpoint of the reference's first and last losses, evaluate()'s accuracy
    above the midpoint of the reference's initial and final accuracies; then the trained policy's dense_policy(), seated through
    oc_partner_logits, gives policy.forward's logits bit for bit."""
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.bc import BCLearner
    from overcooked_ai_amd.policy import ActorCritic

    e = BC.E2E
    feats_h, actions_h, student, perms = BC.e2e_inputs()
    losses64, acc0, acc1 = BC.e2e_reference()
    feats, actions = torch.from_numpy(feats_h.copy()).to(gpu), torch.from_numpy(actions_h.copy()).to(gpu)
    policy = ActorCritic.from_weights(*student, device=gpu)
    learner = BCLearner(policy, lr=e.lr)
    before = learner.evaluate(feats, actions)
    assert float(before.count) == e.rows and abs(float(before.accuracy) - acc0) <= 2.0 / e.rows
    assert all(torch.equal(p.detach().cpu(), torch.from_numpy(w.copy())) for p, w in zip(policy._params(), student)) and all(p.grad is None for p in policy._params())
    got = []
    for perm in perms:
        stats, info = learner.epoch(feats, actions, torch.from_numpy(perm.copy()).to(gpu), e.minibatch)
        assert stats.shape == (e.rows // e.minibatch, 8) and info.shape == (e.rows // e.minibatch, 4) and not bool(info[:, 3].any())
        got += stats[:, 1].tolist()
    after = learner.evaluate(feats, actions)
    held_out = learner.evaluate(feats, actions, torch.arange(e.rows - 512, e.rows, dtype=torch.int32, device=gpu))
    print("loss %.4f -> %.4f on the device, %.4f -> %.4f in float64; accuracy %.4f -> %.4f on the device, %.4f -> %.4f in float64"
          % (got[0], got[-1], losses64[0], losses64[-1], float(before.accuracy), float(after.accuracy), acc0, acc1))
    assert float(learner.adam.clock[0]) == len(losses64) == len(got)
    assert abs(got[0] - losses64[0]) <= 1e-5 * losses64[0]  # (the first minibatch: the same weights on both sides)
    assert got[-1] < 0.5 * (losses64[0] + losses64[-1])
    assert float(after.accuracy) > 0.5 * (acc0 + acc1) and float(held_out.count) == 512 and 0 < float(held_out.accuracy) <= 1
    # ---- the trained policy as a partner
    n = 300
    dense = policy.dense_policy()
    seat = torch.full((n,), 7, dtype=torch.uint8, device=gpu)
    theirs = torch.full((n, 2, 6), FILL, dtype=torch.float32, device=gpu)
    seats = _lib.OcPartnerSeats(seat.data_ptr(), None, 1.0, 12345, 3, 8)
    b = _lib.OcBatch(n_envs=n)
    L = _lib.load()
    rc = L.oc_partner_logits(ctypes.byref(b), dense._ref, ctypes.byref(seats), feats.data_ptr(), (e.in_dim - 56) // 20, theirs.data_ptr(),
                             torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    with torch.no_grad():
        mine, _ = policy(feats[:2 * n].contiguous())
    seat, theirs, mine = seat.cpu().numpy(), theirs.cpu().numpy(), mine.cpu().numpy().reshape(n, 2, 6)
    env = np.arange(n)
    assert (seat <= 1).all() and same(theirs[env, seat], mine[env, seat])
    assert not same(mine, PC.forward_f64(feats_h[:2 * n], student)[2][:, :6].astype(np.float32).reshape(n, 2, 6))  # (the weights moved)
