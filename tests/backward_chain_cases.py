"""The calls on which oc_policy_backward is held bit for bit to tests/backward_chain.py (tests/test_gpu_backward_chain.py), and their
cached restatements.

REAL    every real-valued case of policy_cases.CASES of at most 488 rows, arrays_of's arrays as they are: all five feature lengths,
        widths (64, 64), (40, 24), (33, 17) and (1, 1), contiguous and indexed calls with out-of-range entries and repeated rows,
        zero_tiles and at_zero, one wavefront up to four workgroups.  (The two cases of one pass and 33 rows stay with B1 of
        tests/test_gpu_policy.py: restating 32 801 dense rows takes most of a minute.)  ONE of them is drawn anew, REDRAWN:
        policy_cases zeroes the feature row of every third in-range entry of 96_33_17-65rows-indexed-at_zero, half of the rows the
        call reads, and over its zero biases those add nothing to six of the eight arrays, so that only 0.37 of its gradient
        elements differ in their bits from plain float32 numpy, on every salt (the cases of its size must reach 0.5:
        tests/test_host_backward_chain.py).  Here every fifth of the feature rows the call names is zeros (`_at_zero_draw`:
        weights, index, features and gradients otherwise as policy_cases._draw makes them, no row silenced), redrawn with the next
        salt until `bite_share` is above 0.5 and a live row still has its pre-activations at exactly 0.
SPARSE  calls of policy_cases.three_passes(in_dim) rows — the smallest in which a wavefront reaches a third tile; the grid cannot be
        smaller than 256 — whose upstream gradients are zero except in `listed_tiles`: every tile, in passes 0, 1 and 2, of
        workgroups 0, 1, 2 and G - 1, but not wavefront 1 of workgroup 0 in pass 1 (a skipped tile between two live ones of the same
        accumulator), and the last tile, whose ONE row is live.  The kernel skips the other two thousand tiles and the restatement
        touches about 40.  Weights as policy_cases.weights_of draws them, features and index as policy_cases._draw does, real
        standard_normal gradients in the listed tiles — also at the out-of-range entries of the indexed calls, which must not be
        added.  The draw is repeated with the next salt until `sparse_misses` (conditions on the float64 reference alone) is empty.
        A LIMIT: the four non-zero partials 0, 1, 2 and G - 1 among zeros give the same bits under any order of adding the partials
        that keeps these four in their relative order — a pairwise tree (mutant f) and eight strided accumulators among them — so
        "d_partials[0] + d_partials[1] + ... in ascending order" is held by non-zero partials only up to G = 4 (the 488-row cases).
        A fifth live workgroup such as 8, or a pair such as (4, 5), would tell those orders apart at G = 256.
NAN     the two contiguous sparse calls with the feature rows of every all-zero tile NaN: "its features are not read".

No row is silenced here: the masks come from the float32 chain itself.  Where a reused case zeroed the upstream gradients of its
`unstable` rows, that stays as it is."""
from functools import lru_cache

import numpy as np

import backward_chain as BC
import mlp_chain as MC
import policy_cases as PC

REAL = tuple(c for c in PC.CASES if c.M <= 488)
assert len(REAL) == len(PC.CASES) - 2 == 33

REDRAWN = "96_33_17-65rows-indexed-at_zero"
assert sum(c.id == REDRAWN for c in REAL) == 1
BITE = 0.5                # the share of gradient elements that must differ in their bits from plain float32 numpy
AT_ZERO_SALT = 0xA70
SPARSE_SALT = 0x5BA


def _sparse(k, in_dim, h1, h2, mode):
    M = PC.three_passes(in_dim)
    return PC.Case("%d_%d_%d-%drows-%s-sparse" % (in_dim, h1, h2, M, mode), M, in_dim, h1, h2, mode, "sparse", 611 + k)


SPARSE = (_sparse(0, 96, 64, 64, "contiguous"), _sparse(1, 96, 64, 64, "indexed"), _sparse(2, 116, 64, 64, "indexed"),
          _sparse(3, 136, 33, 17, "contiguous"), _sparse(4, 76, 40, 24, "indexed"))
NAN = tuple(c._replace(id=c.id + "_nan", pattern="sparse_nan") for c in SPARSE if c.mode == "contiguous")
CASES = REAL + SPARSE + NAN
assert len({c.id for c in CASES}) == len(CASES) and len(NAN) == 2


def named(tail):
    return next(c for c in CASES if c.id.endswith(tail))


def base_of(c):
    """The sparse case whose arrays a NaN-filled case shares"""
    return next(s for s in SPARSE if s.seed == c.seed)


def dealing(c):
    """(workgroup, wavefront, pass) of every tile of the case's call under the header's dealing"""
    grid, waves = PC.backward_plan_of(c)
    k = np.arange(-(-c.M // 32), dtype=np.int64)
    return (k // waves) % grid, k % waves, k // (waves * grid)


def listed_tiles(c):
    """The tiles of a sparse case that hold upstream gradients, ascending"""
    grid, _ = PC.backward_plan_of(c)
    group, wave, turn = dealing(c)
    on = np.isin(group, (0, 1, 2, grid - 1)) & ~((group == 0) & (wave == 1) & (turn == 1))
    on[-1] = True
    return np.flatnonzero(on)


def _sparse_draw(c, salt):
    rng = np.random.default_rng([c.seed, SPARSE_SALT, salt])
    M = c.M
    weights = PC.weights_of(c)
    if c.mode == "contiguous":
        R, first, index, nan_row = PC.FIRST + M + 5, PC.FIRST, None, None
        rows = first + np.arange(M, dtype=np.int64)
    else:
        R, first = M // 2 + 2, 0
        nan_row = R - 1
        index = rng.integers(0, R - 1, size=M).astype(np.int32)
        bad = rng.choice(M - 1, size=M // 16, replace=False)  # (the last row of the call stays in range: the one-row tile's)
        index[bad] = np.resize(np.array([-1, R, 2 ** 31 - 1, -2 ** 31, R + 1], np.int64), len(bad)).astype(np.int32)
        rows = np.where((index >= 0) & (index < R), index, -1).astype(np.int64)
    x = rng.integers(-6, 7, size=(R, c.in_dim)).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0
    valid = rows >= 0
    hot = np.isin(np.arange(M) // 32, listed_tiles(c))
    gl, gv = np.zeros((M, 6), np.float32), np.zeros((M,), np.float32)
    gl[hot] = rng.standard_normal((int(hot.sum()), 6)).astype(np.float32)
    gv[hot] = rng.standard_normal((int(hot.sum()),)).astype(np.float32)
    unstable = np.zeros(M, bool)
    for a in (x, gl, gv, rows, valid, unstable) + weights + ((index,) if index is not None else ()):
        a.setflags(write=False)
    return PC.Arrays(weights, x, index, first, rows, valid, gl, gv, unstable, nan_row)


def _at_zero_draw(c, salt):
    rng = np.random.default_rng([c.seed, AT_ZERO_SALT, salt])
    M = c.M
    weights = PC.weights_of(c)  # (at_zero: zero biases)
    R = max(M // 2, 3) + 2
    index = rng.integers(0, R - 1, size=M).astype(np.int32)
    bad = rng.choice(M, size=max(2, M // 16), replace=False)
    index[bad] = np.resize(np.array([-1, R, 2 ** 31 - 1, -2 ** 31, R + 1], np.int64), len(bad)).astype(np.int32)
    rows = np.where((index >= 0) & (index < R), index, -1).astype(np.int64)
    x = rng.integers(-6, 7, size=(R, c.in_dim)).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0
    x[np.unique(rows[rows >= 0])[::5]] = 0
    valid = rows >= 0
    gl, gv = rng.standard_normal((M, 6)).astype(np.float32), rng.standard_normal((M,)).astype(np.float32)
    unstable = np.zeros(M, bool)
    for a in (x, gl, gv, rows, valid, unstable, index) + weights:
        a.setflags(write=False)
    return PC.Arrays(weights, x, index, 0, rows, valid, gl, gv, unstable, R - 1)


def bite_share(c, a):
    """The share of the call's gradient elements whose bit pattern in the restatement is not plain float32 numpy's
    (policy_cases.backward_f32's order, np.matmul and np.sum, on these arrays)"""
    grid, waves = PC.backward_plan_of(c)
    xs, d3 = PC.rows_of(a), PC.upstream(a)
    mine = BC.flat(BC.restate(xs, d3, a.weights, grid, waves).grads)
    plain = BC.flat(PC._backward(xs, a.weights, d3, np.float32).grads)
    return float((MC.canon(mine) != MC.canon(plain)).mean())


def at_zero_misses(c, a):
    """What keeps a redrawn at_zero case from biting, as words (none: [])"""
    xs = PC.rows_of(a)
    out = []
    if not ((xs == 0).all(1) & a.valid & (PC.upstream(a) != 0).any(1)).sum() >= 8:
        out.append("fewer than 8 live rows of zeros (pre-activations at exactly 0)")
    share = bite_share(c, a)
    if not share > BITE:
        out.append("%.3f of the gradient elements differ from plain float32 numpy" % share)
    return out


def rows_alone(c, a, rows):
    """float64 [size]: the reference gradient (policy_cases.row_terms) of the rows `rows` of the call alone, in a partial's layout"""
    rows = np.asarray(rows)
    ok = a.valid[rows]
    x = np.where(ok[:, None], a.features[np.where(ok, a.rows[rows], 0)], np.float32(0))
    d3 = np.where(ok[:, None], np.concatenate([a.grad_logits[rows], a.grad_values[rows, None]], 1), np.float32(0))
    return PC.flat_grads(PC.row_terms(x, a.weights, d3))


def sparse_misses(c, a):
    """What keeps the drawn arrays from biting, as words (none: []): the third pass alone (rows >= 2 * one_pass) and the last row
    alone give each of the eight reference gradients non-zero elements; an indexed call has out-of-range entries with non-zero
    upstream gradients inside live tiles"""
    lay = PC.layout_of(c)
    out = []
    for what, rows in (("the third pass", np.arange(2 * PC.one_pass(c.in_dim), c.M)), ("the last row", np.array([c.M - 1]))):
        g = rows_alone(c, a, rows)
        out += ["%s: the gradient of %s is zero" % (what, n) for n in PC.NAMES if not g[lay[n]].any()]
    if a.index is not None and not (~a.valid & (a.grad_logits != 0).any(1)).sum() >= 8:
        out.append("fewer than 8 out-of-range rows under upstream gradients")
    return out


@lru_cache(maxsize=None)
def arrays_of(c):
    if c.pattern == "sparse":
        for salt in range(64):
            a = _sparse_draw(c, salt)
            if not sparse_misses(c, a):
                return a
        raise AssertionError("%s: no draw that bites: %s" % (c.id, sparse_misses(c, a)))
    if c.pattern == "sparse_nan":
        a = arrays_of(base_of(c))
        dead = ~np.isin(np.arange(c.M) // 32, listed_tiles(c))
        x = a.features.copy()
        x[a.rows[dead]] = np.nan  # (contiguous: a feature row is named by one row of the call)
        x.setflags(write=False)
        return a._replace(features=x)
    if c.id == REDRAWN:
        for salt in range(64):
            a = _at_zero_draw(c, salt)
            if not at_zero_misses(c, a):
                return a
        raise AssertionError("%s: no draw that bites: %s" % (c.id, at_zero_misses(c, a)))
    return PC.arrays_of(c)


def raw_upstream(a):
    """float32 [M, 7]: the upstream gradients as the caller's arrays hold them, out-of-range rows included"""
    return np.concatenate([a.grad_logits, a.grad_values[:, None]], 1).astype(np.float32)


@lru_cache(maxsize=None)
def restated_of(c, mutants=frozenset(), only=None, watch=False):
    """backward_chain.restate of the case's call, W and G from oc_policy_plan's words"""
    a = arrays_of(c)
    grid, waves = PC.backward_plan_of(c)
    return BC.restate(PC.rows_of(a), PC.upstream(a), a.weights, grid, waves, frozenset(mutants), raw_d3=raw_upstream(a), only=only, watch=watch)
