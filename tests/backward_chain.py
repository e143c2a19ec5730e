"""The backward arithmetic of the learner's actor-critic (include/oc_amd.h: OcActorCritic "Backward arithmetic"), restated in numpy so
that oc_policy_backward's partials and gradients can be held to it bit for bit.  The header's sentences, in its order:

  "delta2_u = pre2_u > 0 ? fmaf(wv[u], gv, fmaf(wp[u][5], gl_5, ... fmaf(wp[u][0], gl_0, +0) ...)) : 0"
  "delta1_i = pre1_i > 0 ? the fmaf chain over u = 0 .. h2-1 of w2[i][u] * delta2_u, from +0 : 0"
  "The ReLU derivative is 1 where the f32 pre-activation is > 0 and 0 elsewhere (0 at exactly 0 and at a NaN)"
  "rows are taken in tiles of 32 consecutive rows of the call; tile k belongs to wavefront k % W of workgroup (k / W) % G"
  "a wavefront adds its tiles in ascending order and the rows of a tile in ascending order into ONE f32 accumulator per element, by
   fmaf for the weights (one rounding per row) and by addition for the biases, from +0"
  "a workgroup adds its wavefronts' accumulators in ascending order, ((w0 + w1) + w2) + w3, into d_partials[workgroup]"
  "the gradient is d_partials[0] + d_partials[1] + ... in ascending order"
  "A tile whose 32 rows have only zero upstream gradients is not computed ...; its features are not read."

Every step is float32: the pre-activations are mlp_chain.evaluate's (the header's forward chain), every fused multiply-add is
mlp_chain.fma32 (ONE rounding, exact), every plain addition numpy's float32 `+` (correctly rounded).  The upstream gradients of a row
that is out of range are zeros whatever the caller's arrays hold, and so are the rows behind the call's last in its last tile; a tile
is all zero when none of its 32 masked delta3 rows holds a value != 0 (-0 is zero).

`restate(x, d3, weights, grid, waves)` takes the call's gathered feature rows (policy_cases.rows_of), its masked upstream gradients
(policy_cases.upstream) and the G and W that oc_policy_plan states (policy_cases.backward_plan_of), and returns the [G, size] partials
in the flat layout w1 b1 w2 b2 wp bp wv bv, the eight gradients, the live tiles, the wavefronts' own sums (owners, [n, size]) and —
watch=True — the smallest non-zero magnitude among the backward products and partial sums, which `no_subnormals` holds to 2^-126
with the forward chain's: the header is silent on subnormal numbers, so no case may come near one.  Row terms and accumulators
exist only for wavefronts that own a live tile, all of them side by side in the arrays; `only` restricts the work to some
workgroups' partials (the gradients are then not formed).  Compare with mlp_chain.canon: no accumulator here is ever -0 (x + -x is
+0, and +0 + -0 is +0), so it costs nothing.

MUTANTS: one switch per sentence, each restating it differently, for tests/test_host_backward_chain.py (which shows that the cases
tell every one of them from the header) and for naming the sentence a device result breaks.  numpy only; imported like helpers.py."""
from collections import namedtuple

import numpy as np

import mlp_chain as MC

F32 = np.float32
MUTANTS = {
    "a": "a weight product is rounded to float32 before it is added (no fmaf)",
    "b": "tile k goes to wavefront (k / G) % W of workgroup k % G",
    "c": "one weight accumulator per tile; the tiles are added afterwards",
    "d": "the rows of a tile run in descending order",
    "e": "the wavefronts are added as (w0 + w1) + (w2 + w3)",
    "f": "the partials are added by a pairwise tree",
    "g": "a bias gradient is a per-tile column sum that is then added in",
    "h": "the delta2 chain takes the value head first",
    "i": "the delta1 chain runs in descending u",
    "j": "the ReLU derivative is 1 at a pre-activation of exactly 0",
    "k": "the upstream gradients of out-of-range rows are added",
    "l": "all-zero tiles are computed, not skipped (the same bits on finite features)",
}


def unfused(a, b, c):
    """float32 round(round(a * b) + c): what mutant (a) puts where the header has an fmaf.  (mlp_chain.fma32_plain is NOT this: it
    rounds the exact product's SUM twice and differs from the fmaf on rare ties only, which no case list could be held to.)"""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * b).astype(F32) + c).astype(F32)


def _smallest(v, so_far):
    v = np.abs(np.asarray(v, np.float64))
    v = v[(v != 0) & np.isfinite(v)]
    return min(so_far, float(v.min())) if v.size else so_far


Terms = namedtuple("Terms", "x a1 a2 d1 d2 d3 smallest")


def row_terms(x, d3, weights, mutants=frozenset(), watch=False):
    """Terms of float32 rows x [n, in_dim] under the masked upstream gradients d3 [n, 7]: the inputs (x, a1, a2) and the deltas
    (d1, d2, d3) whose products the eight sums over the rows are made of"""
    w1, b1, w2, b2, w3, b3 = MC.head(weights)
    x, d3 = np.asarray(x, F32).reshape(-1, w1.shape[0]), np.asarray(d3, F32).reshape(-1, 7)
    ch = MC.evaluate(x, weights, watch=watch)
    small = ch.smallest if watch else np.inf
    on = (lambda pre: pre >= 0) if "j" in mutants else (lambda pre: pre > 0)  # (False at a NaN either way)

    def chain(w, d, order):
        nonlocal small
        acc = np.zeros((len(d), w.shape[0]), F32)
        for k in order:
            acc = MC.fma32(w[:, k][None, :], d[:, k:k + 1], acc)
            if watch:
                small = _smallest(w[:, k][None, :].astype(np.float64) * d[:, k:k + 1].astype(np.float64), _smallest(acc, small))
        return acc

    d2 = np.where(on(ch.pre2), chain(w3, d3, [6, 0, 1, 2, 3, 4, 5] if "h" in mutants else range(7)), F32(0)).astype(F32)
    d1 = np.where(on(ch.pre1), chain(w2, d2, range(w2.shape[1])[::-1] if "i" in mutants else range(w2.shape[1])), F32(0)).astype(F32)
    return Terms(x, MC.relu(ch.pre1), MC.relu(ch.pre2), d1, d2, d3, small)


def owner_of_tiles(tiles, grid, waves, mutants=frozenset()):
    """(workgroup, wavefront) of every tile number in `tiles`"""
    tiles = np.asarray(tiles, np.int64)
    if "b" in mutants:
        return tiles % grid, (tiles // grid) % waves
    return (tiles // waves) % grid, tiles % waves


def live_tiles(d3):
    """The numbers of the 32-row tiles of masked upstream gradients d3 [M, 7] that hold a value != 0, ascending"""
    d3 = np.asarray(d3, F32).reshape(-1, 7)
    hot = (d3 != 0).any(1)
    hot = np.concatenate([hot, np.zeros(-len(hot) % 32, bool)])
    return np.flatnonzero(hot.reshape(-1, 32).any(1))


def sizes_of(weights):
    return tuple(int(np.asarray(w).size) for w in weights)


Restated = namedtuple("Restated", "partials grads live smallest sums")


def restate(x, d3, weights, grid, waves, mutants=frozenset(), raw_d3=None, only=None, watch=False):
    """Restated(partials float32 [grid, size], the eight gradients, the live tiles, the smallest non-zero magnitude formed, the
    wavefronts' sums (owners = workgroup * waves + wavefront, float32 [n, size])) of ONE call: x float32 [M, in_dim], row r's feature
    row (zeros for an out-of-range row, as in a tile's image); d3 float32 [M, 7], its upstream gradients with zeros for out-of-range
    rows; raw_d3: what the caller's arrays hold (mutant k adds those).  only: the workgroups whose partials are formed (the others
    stay +0 and grads is None)."""
    mutants = frozenset(mutants)
    assert mutants <= set(MUTANTS)
    weights = tuple(np.asarray(w, F32) for w in weights)
    x = np.asarray(x, F32).reshape(-1, weights[0].shape[0])
    masked = np.asarray(d3, F32).reshape(-1, 7)
    d3 = np.asarray(raw_d3, F32).reshape(-1, 7) if "k" in mutants else masked
    M = len(x)
    n_tiles = -(-M // 32)
    tiles = np.arange(n_tiles) if "l" in mutants else live_tiles(d3)
    live = tiles
    group, wave = owner_of_tiles(tiles, grid, waves, mutants)
    if only is not None:
        keep = np.isin(group, list(only))
        tiles, group, wave = tiles[keep], group[keep], wave[keep]
    size = sum(sizes_of(weights))
    partials, sums = np.zeros((grid, size), F32), (np.zeros(0, np.int64), np.zeros((0, size), F32))
    small = np.inf
    if len(tiles):
        # ---- the row terms of the tiles that are computed, [tile, row of the tile, ...]; rows behind the call's last are zeros
        at = tiles[:, None] * 32 + np.arange(32)[None, :]
        inside = at < M
        at = np.where(inside, at, 0).reshape(-1)
        t = row_terms(np.where(inside.reshape(-1, 1), x[at], F32(0)), np.where(inside.reshape(-1, 1), d3[at], F32(0)), weights, mutants, watch)
        small = t.smallest
        shaped = lambda v: v.reshape(len(tiles), 32, -1)  # noqa: E731
        products = [(shaped(t.x), shaped(t.d1)), (shaped(t.a1), shaped(t.d2)), (shaped(t.a2), shaped(t.d3))]
        # ---- one accumulator per element and wavefront; a wavefront's s-th computed tile is its `slot` s
        key = group * waves + wave
        owners, which = np.unique(key, return_inverse=True)
        slot = np.zeros(len(tiles), np.int64)
        for o in range(len(owners)):
            mine = np.flatnonzero(which == o)
            slot[mine] = np.arange(len(mine))  # (tiles is ascending)
        fma = unfused if "a" in mutants else MC.fma32
        acc_w = [np.zeros((len(owners), inp.shape[2], dl.shape[2]), F32) for inp, dl in products]
        acc_b = [np.zeros((len(owners), dl.shape[2]), F32) for _, dl in products]
        with np.errstate(invalid="ignore", over="ignore"):
            for s in range(int(slot.max()) + 1):
                sel = np.flatnonzero(slot == s)
                wf = which[sel]
                for (inp, dl), aw, ab in zip(products, acc_w, acc_b):
                    w_now = np.zeros_like(aw[wf]) if "c" in mutants else aw[wf]
                    b_now = np.zeros_like(ab[wf]) if "g" in mutants else ab[wf]
                    for r in (range(31, -1, -1) if "d" in mutants else range(32)):
                        a_r, d_r = inp[sel, r][:, :, None], dl[sel, r][:, None, :]
                        w_now = fma(a_r, d_r, w_now)
                        b_now = (b_now + dl[sel, r]).astype(F32)
                        if watch:
                            small = _smallest(a_r.astype(np.float64) * d_r.astype(np.float64), _smallest(w_now, _smallest(b_now, small)))
                    aw[wf] = (aw[wf] + w_now).astype(F32) if "c" in mutants else w_now
                    ab[wf] = (ab[wf] + b_now).astype(F32) if "g" in mutants else b_now
        # ---- the flat layout: w1 b1 w2 b2 wp bp wv bv; the value head is the seventh column of the last product
        n = len(owners)
        flat = np.concatenate([acc_w[0].reshape(n, -1), acc_b[0], acc_w[1].reshape(n, -1), acc_b[1], np.ascontiguousarray(acc_w[2][:, :, :6]).reshape(n, -1),
                               acc_b[2][:, :6], acc_w[2][:, :, 6], acc_b[2][:, 6:]], 1)
        assert flat.shape == (n, size) and flat.dtype == F32
        partials = add_wavefronts(owners, flat, grid, waves, "e" in mutants)
        if watch:
            small = _smallest(partials, small)
        sums = (owners, flat)
    grads = None
    if only is None:
        total = add_partials(partials, "f" in mutants)
        if watch:
            small = _smallest(total, small)
        grads = split(total, weights)
    return Restated(partials, grads, live, small, sums)


def add_wavefronts(owners, sums, grid, waves, pairs=False):
    """float32 [grid, size] partials of the wavefronts' accumulators sums [n, size], owners [n] = workgroup * waves + wavefront (a
    wavefront that is not listed holds +0): ((w0 + w1) + w2) + w3, each + rounded once; pairs: mutant e's (w0 + w1) + (w2 + w3)"""
    partials = np.zeros((grid, sums.shape[1]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in np.unique(owners // waves):
            w = np.zeros((waves, sums.shape[1]), F32)
            mine = np.flatnonzero(owners // waves == g)
            w[owners[mine] % waves] = sums[mine]
            if pairs and waves == 4:
                partials[g] = (w[0] + w[1]) + (w[2] + w[3])
            else:
                total = w[0]
                for k in range(1, waves):
                    total = total + w[k]
                partials[g] = total
    return partials


def split(total, weights):
    """The eight gradient arrays of a flat float32 [size]"""
    ends = np.cumsum(sizes_of(weights))
    return tuple(total[e - np.asarray(w).size:e].reshape(np.shape(w)) for w, e in zip(weights, ends))


def add_partials(partials, tree=False):
    """float32 [size]: partials[0] + partials[1] + ... in ascending order (no partial: +0); tree: mutant f's pairwise tree"""
    partials = np.asarray(partials, F32)
    if len(partials) == 0:
        return np.zeros(partials.shape[1], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if not tree:
            total = partials[0].copy()
            for p in partials[1:]:
                total = total + p
            return total
        level = list(partials)
        while len(level) > 1:
            level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        return level[0].copy()


def flat(grads):
    return np.concatenate([np.asarray(g, F32).reshape(-1) for g in grads])


def no_subnormals(restated):
    """No product and no partial sum of the call, forward or backward, other than an exact 0, is below 2^-126 in magnitude (a
    Restated of watch=True)"""
    assert restated.smallest >= MC.MIN_NORMAL, "a product or partial sum of magnitude %.3g < 2^-126" % restated.smallest
