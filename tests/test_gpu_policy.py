"""oc_policy_forward and oc_policy_backward on the device, through the C-ABI on inputs at the header's minimum alignments and
sentinel-filled outputs between guard rows, and through `ActorCritic`.

F1  every logit and value of every case within its a-priori bound of the float64 reference.
F2  the six logits bit for bit what oc_partner_logits writes for an env seated at that row (dense_policy(), bc_factor 1).
F3  488 rows = 200 + 288 via first_row; an indexed call = the contiguous call on the gathered rows; out-of-range rows +0.0f by bit
    pattern; act = forward on the [2 N, F] view.
B1  every gradient tensor of every case: scaled error (tests/policy_cases.py) at most DEVICE_FACTOR * F32_ERROR = 4e-4.  Largest
    observed on an MI355X: 0.481 of that (1.9e-4, w2 of 96_64_64-32rows-indexed-dense; every other case below 0.13 of it); F1's
    largest error / bound: 0.0063 (profiles/policy.txt).  The eight cases at 76 and 116 inputs: F1 at most 0.00059 of the bound
    (76_40_24-65rows-indexed-dense), B1 at most 0.128 of the tolerance (5.1e-5, w2 of 116_64_64-32rows-indexed-dense).  Every exact
    case (E1, E2, E3) matched.
B2  a call repeats bit for bit; sentinel-filled gradient arrays are overwritten; NaN in a feature row that only out-of-range
    entries could name changes nothing; no rows give zero gradients.
B3  a tiny collected buffer -> policy(buf.features, index) -> ppo_loss -> loss.backward(), held link by link to the float64
    restatement of the chain: the logits and values within F1's bound, ppo_loss's gradients of them within ppo_loss_cases' tolerance
    of loss_f64 on those logits and values, and the parameter gradients within B1's bound of backward_f64 on those gradients.
B4  after an in-place SGD step the next forward equals the reference on the NEW weights.
E1  the exact cases (tests/policy_cases.py: integer weights, features and upstream gradients, every sum far below 2^24, so every
    float32 evaluation IS the float64 reference): all seven outputs of every row equal the reference; out-of-range rows +0.0f.
E2  their eight gradient arrays equal the reference; the float64 sum of the partials equals the gradients; the partial of workgroup
    p equals the reference gradient of the rows policy.hpp's dealing gives p (the first workgroup and tensor that differ are named).
E3  a three-pass exact call at 96 and at 116 inputs repeats bit for bit, ignores NaN in feature rows it does not name, and is the
    sum of the calls on its rows [0, a) and [a, M)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import partner_cases as PTC
import policy_cases as PC
import ppo_loss_cases as LC
from gpu_support import GUARD, gpu, guarded, guards_untouched  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = PC.FILL
TOL = PC.DEVICE_FACTOR * PC.F32_ERROR
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


def placed(a, align, dev):
    """A device copy of numpy array `a` (None stays None) whose first byte lies `align` bytes behind a multiple of 2 * align: the
    minimum alignment include/oc_amd.h allows, which a fresh allocation never has."""
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
    return np.ascontiguousarray(a).view(np.uint32)


def _structs(c, a, dev, features=None, index=(), first=None, n_rows=None):
    from overcooked_ai_amd import _lib

    keep = [placed(w, 4, dev) for w in a.weights]
    feats = placed(a.features if features is None else features, 16, dev)
    index = a.index if isinstance(index, tuple) else index  # (() = the case's own)
    ix = placed(index, 4, dev)
    keep += [feats, ix]
    pol = _lib.OcActorCritic(*[t.data_ptr() for t in keep[:8]], c.in_dim, c.h1, c.h2)
    rows = _lib.OcPolicyRows(feats.data_ptr(), feats.shape[0], ix.data_ptr() if ix is not None else None,
                             a.first if first is None else first, c.M if n_rows is None else n_rows)
    return pol, rows, keep


def forward(c, a, dev, fill=FILL, **kw):
    """One oc_policy_forward call: float32 [M, 7] (logits and value) as numpy"""
    from overcooked_ai_amd import _lib

    pol, rows, keep = _structs(c, a, dev, **kw)
    M = rows.n_rows
    lg, g_lg = guarded(M, (6,), torch.float32, fill, dev, before=1)
    vl, g_vl = guarded(M, (), torch.float32, fill, dev, before=GUARD)
    assert lg.data_ptr() % 16 == 8 and vl.data_ptr() % 8 == 4
    L = _lib.load()
    rc = L.oc_policy_forward(ctypes.byref(pol), ctypes.byref(rows), lg.data_ptr(), vl.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    guards_untouched(c.id, "logits", g_lg, fill)
    guards_untouched(c.id, "values", g_vl, fill)
    return np.concatenate([lg.cpu().numpy(), vl.cpu().numpy()[:, None]], 1)


def backward(c, a, dev, fill=FILL, features=None, n_rows=None, lo=0, part_fill=FILL):
    """One oc_policy_backward call: (the eight gradient arrays, the partials) as numpy.  lo, n_rows: the call is rows
    [lo, lo + n_rows) of the case's: from first_row on (contiguous), a slice of the index (indexed); part_fill: the partials' sentinel"""
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.policy import partials_shape, shapes

    M = c.M - lo if n_rows is None else n_rows
    index = () if a.index is None or not lo else a.index[lo:lo + max(M, 1)]
    pol, rows, keep = _structs(c, a, dev, features=features, index=index, first=a.first + lo, n_rows=M)
    assert rows.n_rows == M
    gl, gv = placed(a.grad_logits[lo:lo + max(M, 1)], 8, dev), placed(a.grad_values[lo:lo + max(M, 1)], 4, dev)
    count, size = partials_shape(M, c.in_dim, c.h1, c.h2)
    grads, guards = [], []
    for shape in shapes(c.in_dim, c.h1, c.h2):
        t, g = guarded(shape[0], shape[1:], torch.float32, fill, dev, before=GUARD)
        grads.append(t)
        guards.append(g)
    part, g_part = guarded(max(count, 1), (size,), torch.float32, part_fill, dev, before=1)
    g = _lib.OcPolicyGrads(*[t.data_ptr() for t in grads])
    L = _lib.load()
    rc = L.oc_policy_backward(ctypes.byref(pol), ctypes.byref(rows), gl.data_ptr(), gv.data_ptr(), ctypes.byref(g), part.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for name, gd in zip(PC.NAMES, guards):
        guards_untouched(c.id, "gradient of " + name, gd, fill)
    guards_untouched(c.id, "partials", g_part, part_fill)
    return [t.cpu().numpy() for t in grads], part[:count].cpu().numpy()


def case_named(tail):
    return next(c for c in PC.CASES if c.id.endswith(tail))


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_f1_every_output_is_within_its_bound_of_the_f64_reference(c, gpu):
    a = PC.arrays_of(c)
    ref, bound, _ = PC.reference_of(c)
    got = forward(c, a, gpu)
    assert not (got == FILL).any()  # (every row written)
    assert not bits(got[~a.valid]).any()  # out-of-range rows: +0.0f
    ratio = np.abs(got.astype(np.float64) - ref)[a.valid] / bound[a.valid]
    print("%s: largest error / bound %.3g" % (c.id, ratio.max() if ratio.size else 0.0))
    assert (ratio <= 1.0).all(), (c.id, float(ratio.max()))


@pytest.mark.parametrize("tail", ("96_64_64-488rows-contiguous-dense", "96_33_17-257rows-contiguous-dense", "56_64_64-65rows-contiguous-dense",
                                  "136_33_17-%drows-contiguous-zero_tiles" % PC.BIG_136, "76_64_64-257rows-contiguous-dense",
                                  "116_64_64-65rows-contiguous-dense"))
def test_f2_the_logits_are_oc_partner_logits_bit_for_bit(tail, gpu):
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.policy import ActorCritic

    c = case_named(tail)
    a = PC.arrays_of(c)
    n = min(len(a.features) // 2, 300)  # envs: feature rows 2 e and 2 e + 1 are env e's two players'
    feats = torch.from_numpy(a.features[:2 * n].copy()).to(gpu)
    policy = ActorCritic.from_weights(*a.weights, device=gpu)
    dense = policy.dense_policy()
    seat = torch.full((n,), 7, dtype=torch.uint8, device=gpu)
    theirs = torch.full((n, 2, 6), FILL, dtype=torch.float32, device=gpu)
    seats = _lib.OcPartnerSeats(seat.data_ptr(), None, 1.0, 12345 + c.seed, 3, 8)
    b = _lib.OcBatch(n_envs=n)
    L = _lib.load()
    rc = L.oc_partner_logits(ctypes.byref(b), dense._ref, ctypes.byref(seats), feats.data_ptr(), (c.in_dim - 56) // 20, theirs.data_ptr(),
                             torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    with torch.no_grad():
        mine, _ = policy(feats)
    seat, theirs, mine = seat.cpu().numpy(), theirs.cpu().numpy(), mine.cpu().numpy().reshape(n, 2, 6)
    assert set(seat.tolist()) == ({0, 1} if n > 8 else set(seat.tolist())) and (seat <= 1).all()  # bc_factor 1: everybody, both seats
    e = np.arange(n)
    assert np.array_equal(bits(theirs[e, seat]), bits(mine[e, seat]))
    assert (theirs[e, 1 - seat] == FILL).all()


def test_f3_split_gathered_out_of_range_and_act(gpu):
    from overcooked_ai_amd.policy import ActorCritic

    # 488 rows = 200 + 288 via first_row
    c = case_named("96_64_64-488rows-contiguous-dense")
    a = PC.arrays_of(c)
    whole = forward(c, a, gpu)
    parts = [forward(c, a, gpu, first=a.first + lo, n_rows=hi - lo) for lo, hi in ((0, 200), (200, 488))]
    assert np.array_equal(bits(whole), bits(np.concatenate(parts)))
    # an indexed call = the contiguous call on the gathered rows; out-of-range rows are +0.0f by bit pattern
    for tail in ("96_64_64-488rows-indexed-dense", "136_64_64-257rows-indexed-dense", "96_1_1-65rows-indexed-dense", "76_40_24-65rows-indexed-dense",
                 "116_33_17-257rows-indexed-dense"):
        c = case_named(tail)
        a = PC.arrays_of(c)
        got = forward(c, a, gpu)
        gathered = forward(c, a, gpu, features=PC.rows_of(a), index=None, first=0)
        assert (~a.valid).sum() >= 2 and np.array_equal(bits(got[a.valid]), bits(gathered[a.valid])) and not bits(got[~a.valid]).any()
    # act = forward on the [2 N, F] view, also into the caller's tensors
    c = case_named("96_64_64-488rows-contiguous-dense")
    a = PC.arrays_of(c)
    policy = ActorCritic.from_weights(*a.weights, device=gpu)
    n = 20
    feats = torch.from_numpy(a.features[:2 * n].reshape(n, 2, c.in_dim).copy()).to(gpu)
    logits, values = policy.act(feats)
    with torch.no_grad():
        l2, v2 = policy(feats.view(2 * n, c.in_dim))
    assert logits.shape == (n, 2, 6) and values.shape == (n, 2) and not logits.requires_grad
    assert torch.equal(logits.view(-1, 6), l2) and torch.equal(values.view(-1), v2)
    out = (torch.full((n, 2, 6), FILL, device=gpu), torch.full((n, 2), FILL, device=gpu))
    assert policy.act(feats, out=out)[0] is out[0] and torch.equal(out[0], logits) and torch.equal(out[1], values)
    l3, v3 = policy(feats, first=7)
    assert torch.equal(l3, l2[7:]) and torch.equal(v3, v2[7:]) and l3.requires_grad


# ------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_b1_every_gradient_is_within_four_times_the_f32_restatement_s_error(c, gpu):
    a = PC.arrays_of(c)
    _, _, ref = PC.reference_of(c)
    grads, partials = backward(c, a, gpu)
    for name, g in zip(PC.NAMES, grads):
        assert not (g == FILL).any() and np.isfinite(g).all(), (c.id, name)
    assert not (partials == FILL).any()
    errs = PC.scaled_errors(grads, ref)
    print("%s: largest scaled error / (4 * F32_ERROR) %.3g (%s)" % (c.id, max(errs) / TOL, ", ".join("%s %.2g" % (n, e) for n, e in zip(PC.NAMES, errs))))
    assert max(errs) <= TOL, (c.id, dict(zip(PC.NAMES, errs)))


def same(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x[0] + [x[1]], y[0] + [y[1]]))


def test_b2_repeatable_overwriting_isolated_and_zero_without_rows(gpu):
    for tail in ("96_64_64-%drows-indexed-zero_tiles" % PC.BIG, "136_64_64-257rows-indexed-dense", "96_64_64-33rows-contiguous-at_zero"):
        c = case_named(tail)
        a = PC.arrays_of(c)
        first = backward(c, a, gpu)
        assert same(first, backward(c, a, gpu)), tail                    # a call repeats bit for bit
        assert same(first, backward(c, a, gpu, fill=0.0)), tail          # and overwrites what the arrays held
        assert same(first, backward(c, a, gpu, fill=1e30)), tail
        if a.nan_row is not None:                                        # a feature row that only out-of-range entries could name
            dirty = a.features.copy()
            dirty[a.nan_row] = np.nan
            assert same(first, backward(c, a, gpu, features=dirty)), tail
            assert np.array_equal(bits(forward(c, a, gpu)), bits(forward(c, a, gpu, features=dirty))), tail
    grads, partials = backward(c, a, gpu, n_rows=0)
    assert all(not bits(g).any() for g in grads) and partials.shape[0] == 0


# ------------------------------------------------------------------------------------------ the exact cases
EXACT = pytest.mark.parametrize("c", PC.EXACT_CASES, ids=lambda c: c.id)
EXACT_FILL = PC.EXACT_FILL


@EXACT
def test_e1_every_output_of_an_exact_case_is_the_reference_s(c, gpu):
    a = PC.exact_arrays_of(c)
    ref, _ = PC.exact_reference_of(c)
    got = forward(c, a, gpu, fill=EXACT_FILL)
    assert not (got == EXACT_FILL).any()  # (every row written)
    assert not bits(got[~a.valid]).any()  # out-of-range rows: +0.0f
    wrong = np.flatnonzero((got.astype(np.float64) != ref).any(1) & a.valid)
    assert wrong.size == 0, "%s: %d rows differ, the first %d (tile %d): %s, not %s" % (c.id, wrong.size, wrong[0], wrong[0] // 32, got[wrong[0]], ref[wrong[0]])


def first_difference(c, got, ref):
    """Words for the first element (in the layout's order) at which float32 [size] got differs from float64 [size] ref, or None"""
    if np.array_equal(got.astype(np.float64), ref):
        return None
    for name, where in PC.layout_of(c).items():
        at = np.flatnonzero(got[where].astype(np.float64) != ref[where])
        if at.size:
            return "%s: %d of %d elements differ, the first [%d]: %r, not %r" % (name, at.size, ref[where].size, at[0], float(got[where][at[0]]), float(ref[where][at[0]]))


@EXACT
def test_e2_every_gradient_and_partial_of_an_exact_case_is_the_reference_s(c, gpu):
    a = PC.exact_arrays_of(c)
    _, ref = PC.exact_reference_of(c)
    grads, partials = backward(c, a, gpu, fill=EXACT_FILL, part_fill=EXACT_FILL)
    grid, waves = PC.backward_plan_of(c)
    assert partials.shape == (grid, len(PC.flat(ref.grads)))
    # ---- the partial of workgroup p is the reference gradient of the rows dealt to p: tile = (pass * grid + p) * wavefronts + wavefront
    want = PC.exact_partials_of(c)
    for p in range(grid):
        said = first_difference(c, partials[p], want[p])
        if said:
            owner = PC.owner_of_rows(c.M, grid, waves)
            tiles = np.unique(np.flatnonzero(owner == p) // 32)
            pytest.fail("%s: the partial of workgroup %d of %d (%d wavefronts; tiles %s) is not its rows' gradient: %s" % (c.id, p, grid, waves, tiles.tolist(), said))
    # ---- the gradients are the partials' sum (in float64: exact whatever the order) and the reference
    assert not (partials == EXACT_FILL).any()  # (no result is the sentinel: the comparison above has named an element left unwritten)
    got = np.concatenate([g.reshape(-1) for g in grads])
    total = partials.astype(np.float64).sum(0)
    said = first_difference(c, got, total)
    if said:
        lost = [p for p in range(grid) if partials[p].any() and np.array_equal(got + partials[p].astype(np.float64), total)]
        pytest.fail("%s: the gradients are not the sum of the %d partials (%s): %s" % (c.id, grid, "they are the sum without partial %s" % lost if lost else "no one partial is missing", said))
    assert not (got == EXACT_FILL).any()
    for name, g, r in zip(PC.NAMES, grads, ref.grads):
        assert np.array_equal(g.astype(np.float64).reshape(r.shape), r), (c.id, name)


@pytest.mark.parametrize("tail", ("96_64_64-%drows-contiguous-three_pass" % PC.three_passes(96), "116_64_64-%drows-indexed-three_pass" % PC.three_passes(116)))
def test_e3_exact_three_pass_calls_repeat_ignore_unnamed_rows_and_split(tail, gpu):
    c = PC.exact_named(tail)
    a = PC.exact_arrays_of(c)
    _, ref = PC.exact_reference_of(c)
    run = lambda **kw: backward(c, a, gpu, fill=EXACT_FILL, part_fill=EXACT_FILL, **kw)  # noqa: E731
    whole = run()
    assert same(whole, run()), tail  # a call repeats bit for bit
    # NaN in the feature rows no row of the call names: the one no in-range entry has (indexed), those around first .. first + M (contiguous)
    dirty = a.features.copy()
    unnamed = np.setdiff1d(np.arange(len(dirty)), a.rows[a.valid])
    assert (a.nan_row in unnamed if a.index is not None else len(unnamed) == a.first + 5)
    dirty[unnamed] = np.nan
    assert same(whole, run(features=dirty)), tail
    # rows [0, cut) + rows [cut, M), the cut inside a tile of the second pass: other tiles, other workgroups, the same sums
    cut = PC.one_pass(c.in_dim) + 45
    lower, upper = run(n_rows=cut), run(lo=cut)
    for name, w, p, q, r in zip(PC.NAMES, whole[0], lower[0], upper[0], ref.grads):
        assert np.array_equal(p.astype(np.float64) + q, w) and np.array_equal(w.astype(np.float64).reshape(r.shape), r), (tail, name)
        assert p.any() and q.any(), (tail, name)


def _policy_and_reference_weights(policy):
    return tuple(p.detach().cpu().numpy() for p in policy._params())


def test_b3_a_collected_buffer_through_policy_and_ppo_loss(gpu):
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.policy import ActorCritic
    from overcooked_ai_amd.ppo_loss import ppo_loss
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    n, T, F = 33, 5, 96
    env = VecOvercookedMultiAgent("cramped_room", n, horizon=4, obs="features", device=gpu, seed=31, reward_shaping_factor=1.0, use_phi=True)
    obs = env.reset()
    policy = ActorCritic(F, seed=11).to(gpu)
    with torch.no_grad():
        for b in (policy.b1, policy.b2, policy.bp, policy.bv):
            b.uniform_(-0.5, 0.5, generator=torch.Generator(device=gpu).manual_seed(2))
    buf = TrajectoryBuffer(env, T, keep_obs=True)
    for t in range(T):
        logits, values = policy.act(env.observations("features"))
        env.step_sampled(logits, into=buf.row(t, values))
    buf.last_values.copy_(policy.act(env.observations("features"))[1])
    adv, tgt, mom = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, tgt, mom)
    S = T * n * 2
    assert buf.features.shape == (T, n, 2, F)
    weights = _policy_and_reference_weights(policy)
    feats = buf.features.view(S, F).cpu().numpy()
    c = LC.Case("buffer", 0, "indexed", 0, "none", True, False, False, 0.05, 10.0, 0.5, 0.2, 0.0, False, 0)
    hyper = dict(clip_param=c.clip, vf_clip_param=c.vf_clip, vf_loss_coeff=c.vf_coeff, entropy_coeff=c.ent, kl_coeff=c.kl)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    for k, index in enumerate(buf.minibatches(S // 2 + 1, generator=torch.Generator(device=gpu).manual_seed(9))):
        M = len(index)
        policy.zero_grad()
        logits, values = policy(buf.features, index)
        logits.retain_grad()
        values.retain_grad()
        loss, stats = ppo_loss(logits, values, batch, index, **hyper)
        loss.backward()
        rows = host(index).astype(np.int64)
        xs = feats[rows]
        # ---- link 1: the logits and values within F1's bound
        _, _, out64 = PC.forward_f64(xs, weights)
        got = np.concatenate([host(logits), host(values)[:, None]], 1)
        assert (np.abs(got - out64) <= PC.forward_bound(xs, weights)).all(), k
        # ---- link 2: ppo_loss's gradients of those logits and values against loss_f64 on them
        a = types.SimpleNamespace(S=S, M=M, actions=host(batch.actions), logp_old=host(batch.logp_old), advantages=host(batch.advantages),
                                  targets=host(batch.targets), seat=None, logits_old=None, moments=host(mom), logits=host(logits), values=host(values),
                                  index=host(index), first=0, sample=rows)
        ref = LC.loss_f64(c._replace(M=M), a)
        count = ref.sums[0]
        assert count == M == float(stats.count)
        near_ratio, near_vf = LC.bands(c, ref)
        up = np.concatenate([host(logits.grad), host(values.grad)[:, None]], 1)  # what backward handed the policy: divided by the count
        assert LC.rel_error(up[:, :6].astype(np.float64) * count, ref.grad_logits, ~near_ratio) <= LC.DEVICE_TOL + 2.0 ** -22
        assert LC.rel_error(up[:, 6].astype(np.float64) * count, ref.grad_values, ~near_vf) <= LC.DEVICE_TOL + 2.0 ** -22
        # ---- link 3: the parameter gradients against backward_f64 on those upstream gradients (B1's situation, B1's bound).  No
        # row of this buffer is unstable: every mask is the float64 reference's in any float32 evaluation
        pre1, pre2, _ = PC.forward_f64(xs, weights)
        e1, e2 = PC.hidden_bounds(xs, weights)
        flips = lambda pre, e: ((pre > 0) & (pre - e <= 0)) | ((pre <= 0) & (pre + e > 0))  # noqa: E731
        unstable = flips(pre1, e1).any(1) | flips(pre2, e2).any(1)
        up = np.where(unstable[:, None], 0, up).astype(np.float32)
        assert unstable.sum() <= PC.UNSTABLE_CAP * M, (k, int(unstable.sum()))
        if unstable.any():  # (the chain cannot silence a row: the call is repeated with those rows' upstream gradients zeroed)
            policy.zero_grad()
            l2, v2 = policy(buf.features, index)
            torch.autograd.backward([l2, v2], [torch.from_numpy(up[:, :6].copy()).to(gpu), torch.from_numpy(up[:, 6].copy()).to(gpu)])
        ref_back = PC._backward(xs, weights, up, np.float64)
        errs = PC.scaled_errors([host(p.grad) for p in policy._params()], ref_back)
        print("minibatch %d: %d rows (%d unstable), loss %.6f, largest scaled error / (4 * F32_ERROR) %.3g" % (k, M, unstable.sum(), float(loss.detach()), max(errs) / TOL))
        assert max(errs) <= TOL, (k, dict(zip(PC.NAMES, errs)))
        assert all(np.abs(g).max() > 0 for g in ref_back.grads)


def test_b4_an_in_place_optimiser_step_is_seen_by_the_next_forward(gpu):
    from overcooked_ai_amd.policy import ActorCritic

    c = case_named("96_64_64-257rows-indexed-dense")
    a = PC.arrays_of(c)
    policy = ActorCritic.from_weights(*a.weights, device=gpu)
    feats, index = torch.from_numpy(a.features.copy()).to(gpu), torch.from_numpy(a.index.copy()).to(gpu)
    opt = torch.optim.SGD(policy.parameters(), lr=0.05)
    before = [p.data_ptr() for p in policy.parameters()]
    logits, values = policy(feats, index)
    ref, bound, _ = PC.reference_of(c)
    got = np.concatenate([logits.detach().cpu().numpy(), values.detach().cpu().numpy()[:, None]], 1)
    assert (np.abs(got - ref) <= bound)[a.valid].all()
    torch.autograd.backward([logits, values], [torch.from_numpy(a.grad_logits.copy()).to(gpu), torch.from_numpy(a.grad_values.copy()).to(gpu)])
    _, _, back = PC.reference_of(c)
    assert max(PC.scaled_errors([p.grad.cpu().numpy() for p in policy._params()], back)) <= TOL
    opt.step()
    assert before == [p.data_ptr() for p in policy.parameters()]  # (in place)
    new = tuple(p.detach().cpu().numpy() for p in policy._params())
    assert all(not np.array_equal(x, y) for x, y in zip(new, a.weights))
    with torch.no_grad():
        l2, v2 = policy(feats, index)
    xs = PC.rows_of(a)
    _, _, out64 = PC.forward_f64(xs, new)
    got2 = np.concatenate([l2.cpu().numpy(), v2.cpu().numpy()[:, None]], 1)
    assert (np.abs(got2 - out64) <= PC.forward_bound(xs, new))[a.valid].all() and not bits(got2[~a.valid]).any()
    assert np.abs(got2 - got)[a.valid].max() > 1e-3  # (the step moved the outputs)
    with pytest.raises(ValueError, match="no CPU fallback"):
        policy.cpu()(feats.cpu())
