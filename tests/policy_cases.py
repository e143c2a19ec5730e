"""The cases of oc_policy_forward and oc_policy_backward (include/oc_amd.h: OcActorCritic; csrc/policy.hpp) and their references.

Forward: `forward_f64` is partner_cases.mlp_f64 with the value head as a seventh output column (float64 numpy on the float32 inputs
and weights), and its a-priori bound is partner_cases.mlp_bound's argument with that column (it holds for ANY float32 evaluation).
`hidden_bounds` restates the argument to keep what mlp_bound does not return: the bounds e1, e2 of the hidden PRE-activations.

Backward: `backward_f64` — analytic gradients in float64, ReLU masks from the float64 forward pass (derivative 0 at 0) — and
`backward_f32`, the same in plain float32 numpy (np.matmul's order of summation, masks from its own float32 forward pass).
A row in which a hidden pre-activation could get another sign in float32 than in float64 (pre > 0 but pre - bound <= 0, or pre <= 0
but pre + bound > 0) is `unstable`: the case gives it ZERO upstream gradients, so it contributes exact zeros under either mask.  At
most UNSTABLE_CAP of a case's rows may be.

The scaled error of a gradient tensor g against the reference g64: max over its elements of |g - g64| / (sum over rows of
|input_i| * |delta_j| + TINY), inputs and deltas the reference's.  F32_ERROR is the largest scaled error of backward_f32 over the
case list, measured on the CPU (tests/test_host_policy.py re-measures it); the device is held to DEVICE_FACTOR times that: another
float32 order of summation (MFMA chains and a fixed tree of partials against numpy's) under the same kind of bound, the margin the
oc_ppo_loss tests give for the same situation."""
import ctypes
import re
from collections import namedtuple
from functools import lru_cache

import numpy as np

import partner_cases as PC

NAMES = ("w1", "b1", "w2", "b2", "wp", "bp", "wv", "bv")
TINY = 1e-30
UNSTABLE_CAP = 0.02
F32_ERROR = 1.0e-4        # measured: see test_the_recorded_error_is_the_measured_one
DEVICE_FACTOR = 4
FILL = -7.0               # the sentinel of output arrays: no result holds it
FIRST = 7                 # the first feature row of the contiguous cases


def plan(n_rows, index, in_dim, h1, h2, backward):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(512)
    rc = L.oc_policy_plan(int(n_rows), int(index), in_dim, h1, h2, int(backward), out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def plan_numbers(text):
    """The numbers a plan's words carry"""
    out = {}
    for key, pat in (("grid", r"k_policy_(?:forward|backward)(?:<[^>]*>)? grid=(\d+)"), ("lanes", r"grid=\d+, (\d+) lanes"), ("per_pass", r"(\d+) rows per workgroup per pass"),
                     ("lds", r"(\d+) B LDS"), ("partials", r"(\d+) partial\(s\)"), ("size", r"partial\(s\) of (\d+) floats"),
                     ("sum_grid", r"k_policy_grad_sum grid=(\d+)")):
        m = re.search(pat, text)
        if m:
            out[key] = int(m.group(1))
    return out


def one_pass(in_dim, h1=64, h2=64):
    """The rows one pass of the backward kernel's persistent grid takes, from the plan's words"""
    rc, text = plan(2 ** 24, 0, in_dim, h1, h2, 1)
    assert rc == 0, text
    n = plan_numbers(text)
    return n["grid"] * n["per_pass"]


# ------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "id M in_dim h1 h2 mode pattern seed")
CASES = []


def case(M, in_dim, h1, h2, mode, pattern="dense"):
    k = len(CASES)
    CASES.append(Case("%d_%d_%d-%drows-%s-%s" % (in_dim, h1, h2, M, mode, pattern), M, in_dim, h1, h2, mode, pattern, 211 + k))


SIZES = (1, 31, 32, 33, 64, 65, 257, 256 + 232)
BIG = one_pass(96) + 33
BIG_136 = one_pass(136) + 33
for _M in SIZES:
    case(_M, 96, 64, 64, "contiguous")
    case(_M, 96, 64, 64, "indexed")
case(BIG, 96, 64, 64, "indexed", "zero_tiles")      # one pass of the persistent grid and 33 rows
case(488, 96, 64, 64, "indexed", "zero_tiles")      # whole 32-row tiles of zero upstream gradients: the partner's samples
case(257, 96, 64, 64, "contiguous", "zero_tiles")
case(65, 96, 1, 1, "indexed")
case(257, 96, 33, 17, "contiguous")
case(65, 56, 64, 64, "contiguous")
case(488, 56, 33, 17, "indexed")
case(257, 136, 64, 64, "indexed")
case(BIG_136, 136, 33, 17, "contiguous", "zero_tiles")
case(33, 96, 64, 64, "contiguous", "at_zero")       # zero biases, all-zero feature rows under non-zero upstream gradients
case(65, 96, 33, 17, "indexed", "at_zero")
# the other two feature lengths: a partial third feature tile at 76, the instance <3, 1, false> at 116 (appended: a case's seed is its place)
case(65, 76, 40, 24, "indexed")
case(257, 76, 64, 64, "contiguous")
case(33, 76, 64, 64, "contiguous", "at_zero")
case(65, 116, 64, 64, "contiguous")
case(257, 116, 33, 17, "indexed")
case(488, 116, 64, 64, "indexed", "zero_tiles")
case(32, 116, 64, 64, "indexed")
case(32, 76, 64, 64, "indexed")
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)

Arrays = namedtuple("Arrays", "weights features index first rows valid grad_logits grad_values unstable nan_row")


def weights_of(c):
    """The eight float32 arrays in NAMES' order: partner_cases.glorot's six and a drawn value head"""
    w1, b1, w2, b2, w3, b3 = PC.glorot(c.seed, c.in_dim, c.h1, c.h2)
    rng = np.random.default_rng([c.seed, 0x7A1])
    lim = np.sqrt(6.0 / (c.h2 + 1))
    wv, bv = rng.uniform(-lim, lim, (c.h2,)).astype(np.float32), rng.uniform(-0.5, 0.5, (1,)).astype(np.float32)
    if c.pattern == "at_zero":
        b1, b2 = np.zeros_like(b1), np.zeros_like(b2)
    return (w1, b1, w2, b2, w3, b3, wv, bv)


def head(weights):
    """partner_cases' six-array form with the value head as the seventh output column"""
    w1, b1, w2, b2, wp, bp, wv, bv = weights
    return (w1, b1, w2, b2, np.concatenate([wp, wv[:, None]], 1), np.concatenate([bp, bv]))


@lru_cache(maxsize=None)
def arrays_of(c):
    """Everything a call of the case takes.  rows: int64 [M], the feature row of every row of the call (-1: out of range); index: the
    int32 [M] the call is given or None; unstable: the rows whose upstream gradients were zeroed; nan_row: a feature row that no
    in-range entry names (indexed cases), for the NaN test.  The draw is repeated with the next salt until at most UNSTABLE_CAP of
    the rows are unstable (a property of the reference alone; one row of 32 is already more)."""
    for salt in range(64):
        a = _draw(c, salt)
        if a.unstable.sum() <= UNSTABLE_CAP * c.M:
            return a
    raise AssertionError("%s: no draw with at most %g of its rows unstable" % (c.id, UNSTABLE_CAP))


def _draw(c, salt):
    rng = np.random.default_rng([c.seed, 0xA11, salt])
    M = c.M
    weights = weights_of(c)
    if c.mode == "contiguous":
        R, first, index, nan_row = FIRST + M + 5, FIRST, None, None
        rows = first + np.arange(M, dtype=np.int64)
    else:
        R, first = max(M // 2, 3) + 2, 0
        nan_row = R - 1
        index = rng.integers(0, R - 1, size=M).astype(np.int32)  # repeats once M > R; never the last row
        if M >= 8:
            bad = rng.choice(M, size=max(2, M // 16), replace=False)
            index[bad] = np.resize(np.array([-1, R, 2 ** 31 - 1, -2 ** 31, R + 1], np.int64), len(bad)).astype(np.int32)
        rows = np.where((index >= 0) & (index < R), index, -1).astype(np.int64)
    x = rng.integers(-6, 7, size=(R, c.in_dim)).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0
    if c.pattern == "at_zero":
        zero_rows = np.unique(rows[rows >= 0][::3])
        x[zero_rows] = 0
    valid = rows >= 0
    gl = rng.standard_normal((M, 6)).astype(np.float32)
    gv = rng.standard_normal((M,)).astype(np.float32)
    if c.pattern == "zero_tiles":
        tile = np.arange(M) // 32
        off = (tile % 3 == 1) | (tile % 7 == 5)
        gl[off], gv[off] = 0, 0
        lone = (np.arange(M) % 32 == 9) & (tile % 3 == 1) & (tile % 2 == 0)  # one live row in some of those tiles
        gl[lone, 2] = 0.5
    # the rows whose masks float32 could decide otherwise: zero upstream gradients
    xs = x[np.where(valid, rows, 0)]
    pre1, pre2, _ = forward_f64(xs, weights)
    e1, e2 = hidden_bounds(xs, weights)
    flips = lambda pre, e: ((pre > 0) & (pre - e <= 0)) | ((pre <= 0) & (pre + e > 0))  # noqa: E731
    unstable = valid & (flips(pre1, e1).any(1) | flips(pre2, e2).any(1))
    gl[unstable], gv[unstable] = 0, 0
    for a in (x, gl, gv, rows, valid, unstable) + weights + ((index,) if index is not None else ()):
        a.setflags(write=False)
    return Arrays(weights, x, index, first, rows, valid, gl, gv, unstable, nan_row)


# ------------------------------------------------------------------------------------------ the references
def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def forward_f64(x, weights):
    """(pre1, pre2, out [..., 7]) in float64: the hidden pre-activations, six logits and the value"""
    w1, b1, w2, b2, w3, b3 = (f64(a) for a in head(weights))
    pre1 = f64(x) @ w1 + b1
    pre2 = np.maximum(pre1, 0.0) @ w2 + b2
    return pre1, pre2, np.maximum(pre2, 0.0) @ w3 + b3


def hidden_bounds(x, weights):
    """(e1, e2): partner_cases.mlp_bound's bounds of the hidden pre-activations, which it does not return"""
    w1, b1, w2, b2, _, _ = (np.abs(f64(a)) for a in head(weights))
    pre1, _, _ = forward_f64(x, weights)
    e1 = PC.gamma(w1.shape[0] + 1) * (np.abs(f64(x)) @ w1 + b1)
    e2 = PC.gamma(w2.shape[0] + 1) * ((np.maximum(pre1, 0.0) + e1) @ w2 + b2) + e1 @ w2
    return e1, e2


def forward_bound(x, weights):
    """float64 [..., 7]: mlp_bound's argument with the value head as the seventh output"""
    return PC.mlp_bound(x, head(weights))


Backward = namedtuple("Backward", "grads scales")


def _backward(x, weights, d3, dtype):
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float32).astype(dtype) for a in head(weights))
    x = np.asarray(x, np.float32).astype(dtype)
    zero = dtype(0)
    pre1 = np.matmul(x, w1) + b1
    a1 = np.maximum(pre1, zero)
    pre2 = np.matmul(a1, w2) + b2
    a2 = np.maximum(pre2, zero)
    d3 = d3.astype(dtype)
    d2 = np.where(pre2 > 0, np.matmul(d3, w3.T), zero)
    d1 = np.where(pre1 > 0, np.matmul(d2, w2.T), zero)
    g3 = np.matmul(a2.T, d3)
    grads = (np.matmul(x.T, d1), d1.sum(0), np.matmul(a1.T, d2), d2.sum(0), g3[:, :6], d3[:, :6].sum(0), g3[:, 6], d3[:, 6:].sum(0))
    absd = [np.abs(d).astype(np.float64) for d in (d1, d2, d3)]
    s3 = np.abs(a2).astype(np.float64).T @ absd[2]
    scales = (np.abs(x).astype(np.float64).T @ absd[0], absd[0].sum(0), np.abs(a1).astype(np.float64).T @ absd[1], absd[1].sum(0),
              s3[:, :6], absd[2][:, :6].sum(0), s3[:, 6], absd[2][:, 6:].sum(0))
    return Backward(tuple(np.ascontiguousarray(g) for g in grads), scales)


def upstream(a):
    """float32 [M, 7] delta3 of the case's arrays: zeros for out-of-range rows"""
    d3 = np.concatenate([a.grad_logits, a.grad_values[:, None]], 1)
    return np.where(a.valid[:, None], d3, np.float32(0)).astype(np.float32)


def rows_of(a):
    """float32 [M, in_dim]: the feature row of every row of the call (zeros for an out-of-range row)"""
    return np.where(a.valid[:, None], a.features[np.where(a.valid, a.rows, 0)], np.float32(0)).astype(np.float32)


@lru_cache(maxsize=None)
def reference_of(c):
    """(out float64 [M, 7] with zeros for out-of-range rows, bound [M, 7], Backward in float64)"""
    a = arrays_of(c)
    xs = rows_of(a)
    _, _, out = forward_f64(xs, a.weights)
    out = np.where(a.valid[:, None], out, 0.0)
    return out, forward_bound(xs, a.weights), _backward(xs, a.weights, upstream(a), np.float64)


def backward_f32(c):
    a = arrays_of(c)
    return _backward(rows_of(a), a.weights, upstream(a), np.float32)


def scaled_errors(grads, ref):
    """The scaled error of each of the eight tensors against the float64 Backward `ref`"""
    return [float((np.abs(np.asarray(g, np.float64).reshape(r.shape) - r) / (s + TINY)).max()) if r.size else 0.0
            for g, r, s in zip(grads, ref.grads, ref.scales)]


# ------------------------------------------------------------------------------------------ the exact cases
# Small-integer weights, biases, features and upstream gradients: every product and every partial sum the network forms, forward
# and backward, is an integer far below 2^24 (exact_sums; tests/test_host_policy.py asserts it), so EVERY float32 evaluation, in
# any order of summation — MFMA chains, the wavefronts' ((w0 + w1) + w2) + w3, the tree of partials — equals the float64 reference
# exactly.  The device is held to equality: one lost, doubled or misplaced row among 65 000 fails.  No row is silenced: the
# pre-activations are exact, so every ReLU mask is the reference's, and a few percent of them are exactly 0 (derivative 0 at 0).
EXACT_SALT = 0xE4
EXACT_FILL = -7.5       # the sentinel of the exact cases' output arrays: every result is an integer
EXACT_ROWS = 300          # feature rows of the indexed exact cases
EXACT_WIDTHS = ((64, 64), (40, 24), (33, 17), (1, 1))
ExactCase = namedtuple("ExactCase", "id M in_dim h1 h2 mode kind seed")
EXACT_CASES = []


def exact_case(M, in_dim, h1, h2, mode, kind):
    k = len(EXACT_CASES)
    EXACT_CASES.append(ExactCase("exact-%d_%d_%d-%drows-%s-%s" % (in_dim, h1, h2, M, mode, kind), M, in_dim, h1, h2, mode, kind, 911 + k))


def per_pass(in_dim):
    """The rows one workgroup of the backward kernel takes per pass, from the plan's words"""
    rc, text = plan(2 ** 24, 0, in_dim, 64, 64, 1)
    assert rc == 0, text
    return plan_numbers(text)["per_pass"]


def three_passes(in_dim):
    """Two passes of the persistent grid, then two full workgroups, one full tile more and a tile of ONE row: the smallest call
    that reaches a wavefront's third tile (the grid is pol_grid's)"""
    return 2 * one_pass(in_dim) + 2 * per_pass(in_dim) + 33


for _i, _in_dim in enumerate((56, 76, 96, 116, 136)):
    for _j, _M in enumerate((1, 33, 257)):
        # the widths in rotation, two places on per feature length: each length sees a padded width, both modes and (64, 64) or
        # (33, 17) at one row (ONE row through ONE unit cannot have both a pre-activation at 0 and eight non-zero gradients)
        _k = 3 * _i + _j
        exact_case(_M, _in_dim, *EXACT_WIDTHS[(2 * _i + _j) % 4], ("contiguous", "indexed")[(_k + _k // 4) % 2], "small")
exact_case(three_passes(96), 96, 64, 64, "indexed", "three_pass")
exact_case(three_passes(96), 96, 64, 64, "contiguous", "three_pass")
exact_case(three_passes(116), 116, 64, 64, "indexed", "three_pass")
exact_case(three_passes(136), 136, 33, 17, "contiguous", "three_pass")
exact_case(three_passes(76), 76, 40, 24, "indexed", "three_pass")
EXACT_CASES = tuple(EXACT_CASES)
assert len({c.id for c in EXACT_CASES}) == len(EXACT_CASES)


def exact_named(tail):
    return next(c for c in EXACT_CASES if c.id.endswith(tail))


@lru_cache(maxsize=None)
def exact_arrays_of(c):
    """Arrays of an exact case: no row is unstable; nan_row (indexed cases) is a feature row that no in-range entry names.  The
    upstream gradients of out-of-range rows are drawn like the others: the device must not add them.  The draw is repeated with
    the next salt until the case bites (exact_misses: conditions on the reference alone)."""
    for salt in range(64):
        a = _exact_draw(c, salt)
        if not exact_misses(c, a):
            return a
    raise AssertionError("%s: no draw that bites: %s" % (c.id, exact_misses(c, a)))


def _exact_draw(c, salt):
    rng = np.random.default_rng([c.seed, EXACT_SALT] + ([salt] if salt else []))

    def tern(shape, d):
        return (rng.integers(-1, 2, shape) * (rng.random(shape) < d)).astype(np.float32)

    M = c.M
    weights = (tern((c.in_dim, c.h1), 0.25), tern((c.h1,), 1.0), tern((c.h1, c.h2), 0.25), tern((c.h2,), 1.0),
               tern((c.h2, 6), 0.5), tern((6,), 1.0), tern((c.h2,), 0.5), tern((1,), 1.0))
    if c.mode == "contiguous":
        R, first, index, nan_row = FIRST + M + 5, FIRST, None, None
        rows = first + np.arange(M, dtype=np.int64)
    else:
        R, first = EXACT_ROWS, 0
        nan_row = R - 1
        index = rng.integers(0, R - 1, size=M).astype(np.int32)
        if M // 16:
            bad = rng.choice(M - 1, size=M // 16, replace=False)  # (the last row of the call stays in range: the one-row tile's)
            index[bad] = np.resize(np.array([-1, R, 2 ** 31 - 1, -2 ** 31, R + 1], np.int64), len(bad)).astype(np.int32)
        rows = np.where((index >= 0) & (index < R), index, -1).astype(np.int64)
    x = rng.integers(-6, 7, size=(R, c.in_dim)).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0
    valid = rows >= 0
    up = tern((M, 7), 0.5)
    gl, gv = np.ascontiguousarray(up[:, :6]), np.ascontiguousarray(up[:, 6])
    unstable = np.zeros(M, bool)
    for a in (x, gl, gv, rows, valid, unstable) + weights + ((index,) if index is not None else ()):
        a.setflags(write=False)
    return Arrays(weights, x, index, first, rows, valid, gl, gv, unstable, nan_row)


RowTerms = namedtuple("RowTerms", "x pre1 pre2 a1 a2 d1 d2 d3")


def row_terms(x, weights, d3):
    """Per row, in float64: what _backward's eight sums over the rows are made of"""
    w1, b1, w2, b2, w3, b3 = (f64(a) for a in head(weights))
    x, d3 = f64(x), f64(d3)
    pre1 = x @ w1 + b1
    a1 = np.maximum(pre1, 0.0)
    pre2 = a1 @ w2 + b2
    a2 = np.maximum(pre2, 0.0)
    d2 = np.where(pre2 > 0, d3 @ w3.T, 0.0)
    d1 = np.where(pre1 > 0, d2 @ w2.T, 0.0)
    return RowTerms(x, pre1, pre2, a1, a2, d1, d2, d3)


def flat_grads(t, rows=slice(None)):
    """float64 [size]: the gradients of the rows `rows` of RowTerms t in a partial's layout, w1 b1 w2 b2 wp bp wv bv"""
    x, a1, a2, d1, d2, d3 = (q[rows] for q in (t.x, t.a1, t.a2, t.d1, t.d2, t.d3))
    g3 = a2.T @ d3
    parts = (x.T @ d1, d1.sum(0), a1.T @ d2, d2.sum(0), g3[:, :6], d3[:, :6].sum(0), g3[:, 6], d3[:, 6:].sum(0))
    return np.concatenate([np.asarray(p).reshape(-1) for p in parts])


def flat(grads):
    return np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in grads])


def layout_of(c):
    """name -> slice of a partial's floats"""
    sizes = (c.in_dim * c.h1, c.h1, c.h1 * c.h2, c.h2, c.h2 * 6, 6, c.h2, 1)
    ends = np.cumsum(sizes)
    return {n: slice(int(e - s), int(e)) for n, s, e in zip(NAMES, sizes, ends)}


@lru_cache(maxsize=1)  # (a quarter of a gigabyte at 65 825 rows: the tests go case by case)
def exact_terms_of(c):
    a = exact_arrays_of(c)
    return row_terms(rows_of(a), a.weights, upstream(a))


def exact_misses(c, a):
    """What keeps the drawn arrays `a` from biting, as words (none: []).  The share of positive hidden pre-activations lies in
    0.3..0.7; a live row has a pre-activation exactly 0 under a non-zero upstream gradient; each of the eight reference gradients
    has non-zero elements — of the whole call and, in a three-pass case, of the third pass alone (rows >= 2 * one_pass) and of
    the last tile's ONE row alone."""
    t = row_terms(rows_of(a), a.weights, upstream(a))
    lay = layout_of(c)
    out = []
    pre = np.concatenate([t.pre1[a.valid].reshape(-1), t.pre2[a.valid].reshape(-1)])
    if not 0.3 <= (pre > 0).mean() <= 0.7:
        out.append("%.2f of the hidden pre-activations are positive" % (pre > 0).mean())
    if not (((t.pre1 == 0).any(1) | (t.pre2 == 0).any(1)) & t.d3.any(1)).any():
        out.append("no live row with a pre-activation at 0")
    some = [("the call", slice(None))]
    if c.kind == "three_pass":
        some += [("the third pass", slice(2 * one_pass(c.in_dim), None)), ("the last row", slice(c.M - 1, None))]
    for what, rows in some:
        g = flat_grads(t, rows)
        out += ["%s: the gradient of %s is zero" % (what, n) for n in NAMES if not g[lay[n]].any()]
    return out


@lru_cache(maxsize=None)
def exact_reference_of(c):
    """(out float64 [M, 7] with zeros for out-of-range rows, Backward in float64): forward_f64 and _backward as they are"""
    a = exact_arrays_of(c)
    xs = rows_of(a)
    _, _, out = forward_f64(xs, a.weights)
    return np.where(a.valid[:, None], out, 0.0), _backward(xs, a.weights, upstream(a), np.float64)


def exact_sums(c):
    """name -> the largest sum of ABSOLUTE values of the terms of any sum the network forms for the quantity: every partial sum, in any
    order, is at most this in magnitude.  Below 2^24 with integer terms, every float32 evaluation is exact."""
    a = exact_arrays_of(c)
    t = exact_terms_of(c)
    w1, b1, w2, b2, w3, b3 = (np.abs(f64(q)) for q in head(a.weights))
    _, ref = exact_reference_of(c)
    out = {"pre1": np.abs(t.x) @ w1 + b1, "pre2": t.a1 @ w2 + b2, "out": t.a2 @ w3 + b3,
           "delta2": np.abs(t.d3) @ w3.T, "delta1": np.abs(t.d2) @ w2.T}  # (the deltas before their masks: the device forms them all)
    out.update(("g" + n, s) for n, s in zip(NAMES, ref.scales))
    return {k: float(np.max(v)) for k, v in out.items()}


def backward_plan_of(c):
    """(grid, wavefronts per workgroup) of the case's backward call, from the plan's words"""
    rc, text = plan(c.M, c.mode == "indexed", c.in_dim, c.h1, c.h2, 1)
    assert rc == 0, text
    n = plan_numbers(text)
    return n["grid"], n["lanes"] // 64


def owner_of_rows(M, grid, waves):
    """int64 [M]: the workgroup that owns each row under policy.hpp's dealing, tile = (pass * grid + workgroup) * waves + wavefront"""
    tile = np.arange(M, dtype=np.int64) // 32
    return (tile // waves) % grid


def exact_partials_of(c):
    """float64 [grid, size]: the reference gradient of the rows each workgroup owns"""
    grid, waves = backward_plan_of(c)
    owner = owner_of_rows(c.M, grid, waves)
    t = exact_terms_of(c)
    return np.stack([flat_grads(t, np.flatnonzero(owner == p)) for p in range(grid)])
