"""oc_bc_loss's case list and two numpy restatements of the arithmetic include/oc_amd.h states (OcBcLoss): bc_f32, the header's f32
operations one by one, and bc_f64, the reference — the same losses, sums, stats and analytic gradients in float64 on the same f32
inputs (the class weights widened).  numpy only; imported like helpers.py.  Also the inputs and the float64 restatement of the small
end-to-end training run that tests/test_host_bc.py checks on the CPU and tests/test_gpu_bc.py holds the device to.

Tolerances, measured here on the CPU over the whole case list (test_host_bc.py measures them again and holds them to these):
  F32_ERROR      the largest |bc_f32 - bc_f64| / max(1, |bc_f64|) of any row's loss or gradient.
  DEVICE_FACTOR  4: the device is held to DEVICE_FACTOR x F32_ERROR, the project's convention.  Its expf / logf differ from numpy's by
                 a few ulp.
There are no branch bands: the only branch is the argmax on the inputs, which is exact in either precision."""
import collections
import functools
import types

import numpy as np

F32_ERROR = 6.0e-7  # measured 5.97e-7 (grad_logits of the big indexed case): see test_h1_the_recorded_error_is_the_measured_one
DEVICE_FACTOR = 4
DEVICE_TOL = DEVICE_FACTOR * F32_ERROR
FILL = -7.0  # what the output arrays of a GPU test start as: no result of a case equals it (test_host_bc.py checks)
SIZES = (1, 63, 64, 65, 255, 256, 257, 488)
STATS = ("count", "loss", "accuracy", "mean_weight", "zero4", "zero5", "zero6", "inv_count")
STAY_SKEW = (0.05, 0.05, 0.08, 0.08, 0.64, 0.10)  # a six-way histogram skewed towards STAY (index 4), as the human data's is

Case = collections.namedtuple("Case", "id M mode first weights special seed")


@functools.lru_cache(maxsize=None)
def partial_samples():
    """P, the minibatch rows per partial, read from oc_bc_loss_plan's words (no device needed)."""
    from overcooked_ai_amd.bc import partial_samples as P

    return P()


def _case(M, mode, i, special="", weights=None, first=None):
    weights = bool(i & 1) if weights is None else weights
    first = (0 if mode != "contiguous" else 3 + 2 * i + (i & 1)) if first is None else first
    name = "M%d-%s%s%s" % (M, mode, "-weights" if weights else "", "-" + special if special else "")
    return Case(name, M, mode, first, weights, special, 700 + i)


def _cases():
    out, i = [], 0
    for M in SIZES:  # every size contiguous (first_sample > 0) and indexed, class weights taking turns (shifted by one between the modes)
        for mode in ("contiguous", "indexed"):
            out.append(_case(M, mode, i, weights=bool((i + (i >> 1)) & 1)))
            i += 1
    tile = partial_samples() // 4  # a workgroup walks four tiles of rows: one row into the fourth, and one row into a second workgroup
    for M in (3 * tile + 1, 4 * tile + 1):
        for mode in ("contiguous", "indexed"):
            out.append(_case(M, mode, i, "tiles", weights=bool((i + (i >> 1)) & 1)))
            i += 1
    big = 65 * partial_samples() + 3  # more partials than the finishing wavefront has lanes
    out.append(_case(big, "contiguous", 30, "big", weights=False))
    out.append(_case(big, "indexed", 31, "big", weights=True))
    out.append(_case(488, "contiguous", 32, "invalid", weights=True))
    out.append(_case(257, "contiguous", 33, "count0", weights=False))   # every action invalid
    out.append(_case(65, "indexed", 34, "count0", weights=True))        # every index out of range
    out.append(_case(488, "indexed", 35, "zero_weight", weights=True))
    out.append(_case(488, "contiguous", 36, "ties", weights=False))
    out.append(_case(257, "indexed", 37, "ties", weights=True))
    out.append(_case(488, "indexed", 38, "neginf_away", weights=True))
    out.append(_case(257, "contiguous", 39, "neginf_at", weights=True))
    out.append(_case(488, "indexed", 40, "nan_left_out", weights=False))
    out.append(_case(488, "contiguous", 41, "skewed", weights=True))
    out.append(_case(488, "contiguous", 42, "split", weights=True))     # (one call, and 200 + 288)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """The arrays of a case, read-only, as a namespace: actions u8 [S], class_weights f32 [6] or None, logits f32 [M, 6] ~ N(0, 2),
    index i32 [M] or None, first, and sample i64 [M], the sample of every row (an out-of-range one as the index has it)."""
    rng = np.random.default_rng(c.seed)
    M = c.M
    S = c.first + M + 38 if c.mode == "contiguous" else M + 10
    actions = rng.integers(0, 6, S).astype(np.uint8)
    if c.special == "skewed":
        actions = rng.choice(6, size=S, p=STAY_SKEW).astype(np.uint8)
    bad = rng.random(S) < 0.03  # a few invalid rows in every case
    if S >= 60:
        bad[rng.integers(0, S, 2)] = True
    if c.special == "invalid":
        bad = rng.random(S) < 0.35
    if c.special == "count0" and c.mode == "contiguous":
        bad[:] = True
    actions[bad] = np.where(rng.random(bad.sum()) < 0.7, 255, rng.choice(np.array([6, 7, 100, 200], np.uint8), size=bad.sum())).astype(np.uint8)
    weights = None
    if c.weights:
        weights = rng.uniform(0.25, 4.0, 6).astype(np.float32)
        if c.special == "zero_weight":
            weights[int(actions[actions <= 5][0])] = 0.0
        if c.special == "skewed":  # the balancing weights: inverse frequency, normalised to a mean of 1 over the samples
            freq = np.bincount(actions[actions <= 5], minlength=6) / max((actions <= 5).sum(), 1)
            weights = (1.0 / (6.0 * np.maximum(freq, 1e-3))).astype(np.float32)
    index = None
    if c.mode == "contiguous":
        sample = c.first + np.arange(M, dtype=np.int64)
    else:  # a permutation with repeats and a few entries outside 0 .. S - 1
        sample = rng.permutation(S)[:M].astype(np.int64)
        if M >= 8:
            rep = rng.integers(0, M, max(M // 20, 2))
            sample[rep] = sample[(rep + 3) % M]
            out_of_range = np.array([-1, S, S + 5, -2 ** 31, 2 ** 31 - 1][:max(2, min(5, M // 12))], np.int64)
            sample[rng.choice(M, len(out_of_range), replace=False)] = out_of_range
        if c.special == "count0":
            sample = np.resize(np.array([-1, S, S + 5, -2 ** 31, 2 ** 31 - 1], np.int64), M)
        index = sample.astype(np.int32)
    inside = (sample >= 0) & (sample < S)
    act = np.where(inside, actions[np.where(inside, sample, 0)], 255)
    left_out = ~inside | (act > 5)
    logits = (rng.standard_normal((M, 6)) * 2).astype(np.float32)
    if c.special == "ties":  # small integers: every row's maximum is shared with probability above a half
        logits = rng.integers(-1, 2, (M, 6)).astype(np.float32)
    kept = np.nonzero(~left_out)[0]
    if c.special == "neginf_away":  # a -inf logit on an action not taken, in a fifth of the rows
        rows = kept[rng.random(len(kept)) < 0.2]
        logits[rows, (act[rows] + 1 + rng.integers(0, 5, len(rows))) % 6] = -np.inf
    if c.special == "neginf_at":  # a -inf logit at the taken action, in a tenth of the rows
        rows = kept[rng.random(len(kept)) < 0.1]
        logits[rows, act[rows]] = -np.inf
    if c.special == "nan_left_out":
        logits[left_out] = np.nan
    a = types.SimpleNamespace(S=S, M=M, actions=actions, class_weights=weights, logits=logits, index=index, first=c.first, sample=sample)
    for x in vars(a).values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a


Result = collections.namedtuple("Result", "loss grad_logits correct left_out sums stats")


def _softmax(l):
    m = l.max(-1, keepdims=True)
    d = l - m
    w = np.exp(d)
    S = w[:, 0]
    for i in range(1, 6):
        S = S + w[:, i]
    lp = d - np.log(S)[:, None]
    p = w / S[:, None]
    return lp, p


def stats_of(sums):
    """d_stats of the four sums, as k_bc_loss_stats derives them."""
    n = sums[0]
    if not n > 0:
        return np.zeros(8)
    with np.errstate(invalid="ignore"):
        return np.array([n, sums[1] / n, sums[2] / n, sums[3] / n, 0.0, 0.0, 0.0, 1.0 / n], np.float64)


def _bc(a, f):
    """The header's arithmetic in dtype f, one numpy operation per rounding; the sums and stats in float64."""
    s = a.sample
    inside = (s >= 0) & (s < a.S)
    at = np.where(inside, s, 0)
    act = a.actions[at]
    left_out = ~inside | (act > 5)
    a5 = np.minimum(act, 5).astype(np.int64)
    with np.errstate(all="ignore"):
        l = a.logits.astype(f)
        lp, p = _softmax(l)
        c = a.class_weights.astype(f)[a5] if a.class_weights is not None else np.ones(len(s), f)
        ce = -np.take_along_axis(lp, a5[:, None], 1)[:, 0]
        loss = c * ce
        onehot = (np.arange(6)[None, :] == act[:, None]).astype(f)
        gl = c[:, None] * (p - onehot)
        m = l.max(-1)
        hit = l == m[:, None]  # the lowest i with l_i == m (none in a row with a NaN)
        best = np.where(hit.any(1), hit.argmax(1), 6)
    correct = (best == act) & ~left_out
    loss = np.where(left_out, f(0), loss)
    gl = np.where(left_out[:, None], f(0), gl)
    assert loss.dtype == f and gl.dtype == f
    keep = ~left_out
    with np.errstate(invalid="ignore"):
        sums = np.array([keep.sum(), loss.astype(np.float64)[keep].sum(), correct.sum(), c.astype(np.float64)[keep].sum()], np.float64)
    return Result(loss, gl, correct, left_out, sums, stats_of(sums))


def bc_f32(c, a=None):
    return _bc(arrays_of(c) if a is None else a, np.float32)


def bc_f64(c, a=None):
    return _bc(arrays_of(c) if a is None else a, np.float64)


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """bc_f64 of a case, computed once and shared, read-only."""
    r = bc_f64(c)
    for x in r:
        x.setflags(write=False)
    return r


def rel_error(got, ref, rows=None):
    """The largest |got - ref| / max(1, |ref|) over rows (all of them by default); 0 where there is none.  Equal infinities agree."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.where(got == ref, 0.0, np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))
    return float(err.max())  # (a NaN where the reference has a number is an error of NaN, and fails every comparison)


def poisoned(c):
    """The arrays of a case with NaN in the logits of every left-out row, as a namespace of writable copies."""
    a = arrays_of(c)
    b = types.SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(a).items()})
    b.logits[reference_of(c).left_out] = np.nan
    return b


CASES = _cases()


# ------------------------------------------------------------------------------------------ the small end-to-end run
E2E = types.SimpleNamespace(rows=2048, in_dim=96, h1=64, h2=64, minibatch=256, epochs=3, lr=3e-3, seed=4242)
# what test_host_bc.py measures of the float64 run: (first minibatch's loss, last minibatch's loss, accuracy before, accuracy after)
E2E_RECORDED = (1.9345, 0.9401, 0.1475, 0.6372)  # to four places; see test_h5_the_reference_run_improves


@functools.lru_cache(maxsize=None)
def e2e_inputs():
    """(features f32 [rows, in_dim] ~ N(0, 1), actions u8 [rows]: the argmax of a seeded random teacher of the partner's shape, the
    student's eight initial float32 arrays, the epochs' permutations i32 [epochs, rows]), read-only."""
    import partner_cases as PTC
    import policy_cases as PC

    e = E2E
    rng = np.random.default_rng(e.seed)
    feats = rng.standard_normal((e.rows, e.in_dim)).astype(np.float32)
    w1, b1, w2, b2, w3, b3 = (np.asarray(x, np.float64) for x in PTC.glorot(e.seed + 1, e.in_dim, e.h1, e.h2))
    teacher = np.maximum(np.maximum(feats.astype(np.float64) @ w1 + b1, 0) @ w2 + b2, 0) @ w3 + b3
    actions = teacher.argmax(1).astype(np.uint8)
    student = PC.weights_of(PC.Case("e2e", e.rows, e.in_dim, e.h1, e.h2, "indexed", "dense", e.seed + 2))
    perms = np.stack([rng.permutation(e.rows) for _ in range(e.epochs)]).astype(np.int32)
    for x in (feats, actions, perms) + tuple(student):
        x.setflags(write=False)
    return feats, actions, tuple(student), perms


def _f64_eval(weights, feats, actions):
    import policy_cases as PC

    _, _, out = PC.forward_f64(feats, weights)
    a = types.SimpleNamespace(S=len(actions), M=len(actions), actions=actions, class_weights=None, logits=out[:, :6], index=None, first=0,
                              sample=np.arange(len(actions), dtype=np.int64))
    return _bc(a, np.float64)


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """The run in float64 on the CPU (the weights rounded to float32 between the steps, as they are stored): (the loss of every
    minibatch [epochs * K], accuracy over all rows before, accuracy after)."""
    import learner_cases as LC
    import policy_cases as PC

    e = E2E
    feats, actions, student, perms = e2e_inputs()
    dims = (e.in_dim, e.h1, e.h2)
    hyper = LC.Hyper(e.lr, 0.9, 0.999, 1e-8, None)
    st, losses = LC.state0(student, np.float64), []
    acc0 = _f64_eval(student, feats, actions).stats[2]
    for perm in perms:
        for lo in range(0, e.rows, e.minibatch):
            idx = perm[lo:lo + e.minibatch].astype(np.int64)
            w = [x.astype(np.float32) for x in LC.split(st.params, *dims)]
            ref = _f64_eval(w, feats[idx], actions[idx])
            up = np.concatenate([ref.grad_logits, np.zeros((len(idx), 1))], 1)
            back = PC._backward(feats[idx], w, up, np.float64)
            losses.append(ref.stats[1])
            st, _ = LC.adam_f64(st, LC.split(LC.flat(back.grads), *dims), hyper, ref.stats[7])
    w = [x.astype(np.float32) for x in LC.split(st.params, *dims)]
    return np.array(losses), float(acc0), float(_f64_eval(w, feats, actions).stats[2])
