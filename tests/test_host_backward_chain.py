"""tests/backward_chain.py, the numpy restatement of the header's backward arithmetic that oc_policy_backward is held to bit for bit
(tests/test_gpu_backward_chain.py), and its case list (tests/backward_chain_cases.py), on the CPU (the library only for the words of
oc_policy_plan):

- against a scalar loop of exact rational fused multiply-adds and additions (test_host_mlp_chain's fma_exact) that follows the
  header's sentences one element at a time, on 70 rows of 56/3/2 with an all-zero middle tile and out-of-range entries;
- against the integer-exact references of tests/policy_cases.py, which the suite already trusts, on every exact case of at most 257
  rows: partials and gradients;
- the cases bite: in every case of at least 64 rows and widths of at least (33, 17) more than half of the gradient elements differ in
  their bits from plain float32 numpy (policy_cases.backward_f32's order: np.matmul and np.sum), the shares printed
  (96_33_17-65rows-indexed-at_zero in backward_chain_cases' own draw, which says why); every mutant (a)-(k) of the restatement, one per sentence of the header, changes
  bits in at least three cases, and only where it can (the table is printed); mutant (l) changes none on finite features and turns
  the NaN-filled cases into NaN;
- the sparse multi-pass cases are what backward_chain_cases says of them;
- the time every restatement took, printed; none above 10 s."""
import time
from fractions import Fraction

import numpy as np
import pytest

import backward_chain as BC
import backward_chain_cases as CC
import mlp_chain as MC
import policy_cases as PC
from test_host_mlp_chain import fma_exact, round_f32

F32 = np.float32
FINITE = CC.REAL + CC.SPARSE
DURATIONS = {}


def restated(c):
    """backward_chain_cases.restated_of(c) with watch=True (what the device tests compare with), timed at its first evaluation"""
    t0 = time.perf_counter()
    r = CC.restated_of(c, watch=True)
    DURATIONS.setdefault(c.id, time.perf_counter() - t0)
    return r


def differs(x, y):
    """The partials or the gradients of Restated x and y differ in a bit (after -0 -> +0; a NaN differs from a number)"""
    return bool((MC.canon(x.partials) != MC.canon(y.partials)).any() or (MC.canon(BC.flat(x.grads)) != MC.canon(BC.flat(y.grads))).any())


# ------------------------------------------------------------------------------------------ against rational arithmetic
def add_exact(a, b):
    return round_f32(Fraction(float(a)) + Fraction(float(b)))


def scalar_backward(x, d3, weights, grid, waves):
    """The header's sentences one element at a time on exact arithmetic: (partials [grid][size], gradients [size]) as float32 lists"""
    w1, b1, w2, b2, w3, b3 = MC.head(weights)
    M, zero = len(x), F32(0)

    def chain(v, w, j, start):  # the fmaf chain of unit j over the inputs v in ascending index
        acc = start
        for k in range(len(v)):
            acc = fma_exact(v[k], w[k, j], acc)
        return acc

    rows = []
    for r in range(M):
        pre1 = [chain(x[r], w1, j, b1[j]) for j in range(w1.shape[1])]
        a1 = [max(p, zero) for p in pre1]
        pre2 = [chain(a1, w2, j, b2[j]) for j in range(w2.shape[1])]
        a2 = [max(p, zero) for p in pre2]
        delta2 = [chain(d3[r], w3.T, u, zero) if pre2[u] > 0 else zero for u in range(w2.shape[1])]   # wp[u][0] gl_0 first, wv[u] gv last
        delta1 = [chain(delta2, w2.T, i, zero) if pre1[i] > 0 else zero for i in range(w1.shape[1])]  # u = 0 .. h2 - 1
        rows.append((list(x[r]), a1, a2, delta1, delta2, list(d3[r])))
    size = sum(BC.sizes_of(weights))
    acc = {}  # (workgroup, wavefront) -> its ONE accumulator per element
    for k in range(-(-M // 32)):
        mine = range(32 * k, min(32 * k + 32, M))
        if not any(v != 0 for r in mine for v in d3[r]):
            continue  # "is not computed"
        mine_acc = acc.setdefault(((k // waves) % grid, k % waves), [zero] * size)
        for r in mine:
            xs, a1, a2, delta1, delta2, delta3 = rows[r]
            at = 0
            for inp, dl in ((xs, delta1), (a1, delta2)):
                for i in range(len(inp)):
                    for j in range(len(dl)):
                        mine_acc[at] = fma_exact(inp[i], dl[j], mine_acc[at])
                        at += 1
                for j in range(len(dl)):
                    mine_acc[at] = add_exact(mine_acc[at], dl[j])
                    at += 1
            for cols in (range(6), range(6, 7)):  # wp bp, then wv bv
                for i in range(len(a2)):
                    for j in cols:
                        mine_acc[at] = fma_exact(a2[i], delta3[j], mine_acc[at])
                        at += 1
                for j in cols:
                    mine_acc[at] = add_exact(mine_acc[at], delta3[j])
                    at += 1
            assert at == size
    partials = []
    for g in range(grid):
        total = acc.get((g, 0), [zero] * size)
        for w in range(1, waves):
            total = [add_exact(p, q) for p, q in zip(total, acc.get((g, w), [zero] * size))]
        partials.append(total)
    grads = partials[0]
    for p in partials[1:]:
        grads = [add_exact(s, q) for s, q in zip(grads, p)]
    return np.array(partials, F32), np.array(grads, F32)


SCALAR = PC.Case("56_3_2-70rows-indexed-scalar", 70, 56, 3, 2, "indexed", "dense", 9102)


@pytest.mark.parametrize("dealt", ("as planned", "two workgroups of one wavefront"))
def test_the_restatement_is_the_scalar_loop_of_exact_fused_multiply_adds(dealt):
    c = SCALAR
    a = PC._draw(c, 0)
    d3 = PC.upstream(a).copy()
    d3[32:64] = 0  # tile 1 is skipped
    assert (~a.valid).sum() >= 2 and (~a.valid[:32]).any()
    grid, waves = PC.backward_plan_of(c) if dealt == "as planned" else (2, 1)  # (2, 1): tiles 0 and 2 in ONE accumulator of workgroup 0
    assert (grid, waves) in ((1, 4), (2, 1))
    got = BC.restate(PC.rows_of(a), d3, a.weights, grid, waves, watch=True)
    assert got.live.tolist() == [0, 2]
    BC.no_subnormals(got)
    partials, grads = scalar_backward(PC.rows_of(a), d3, a.weights, grid, waves)
    assert np.array_equal(got.partials.view(np.uint32), partials.view(np.uint32))
    assert np.array_equal(BC.flat(got.grads).view(np.uint32), grads.view(np.uint32))
    lay = PC.layout_of(c)
    assert all(grads[lay[n]].any() for n in PC.NAMES) and [g.shape for g in got.grads] == [w.shape for w in a.weights]
    # (the scalar loop is not numpy's float32 order either)
    assert (grads != BC.flat(PC._backward(PC.rows_of(a), a.weights, d3, np.float32).grads)).any()


# ------------------------------------------------------------------------------------------ against the integer-exact references
@pytest.mark.parametrize("c", [c for c in PC.EXACT_CASES if c.M <= 257], ids=lambda c: c.id)
def test_the_restatement_is_the_integer_exact_reference(c):
    a = PC.exact_arrays_of(c)
    grid, waves = PC.backward_plan_of(c)
    got = BC.restate(PC.rows_of(a), PC.upstream(a), a.weights, grid, waves)
    assert np.array_equal(got.partials.astype(np.float64), PC.exact_partials_of(c))
    _, ref = PC.exact_reference_of(c)
    for name, g, r in zip(PC.NAMES, got.grads, ref.grads):
        assert np.array_equal(g.astype(np.float64).reshape(r.shape), r), (c.id, name)


# ------------------------------------------------------------------------------------------ the cases bite
def test_more_than_half_of_the_gradient_bits_are_not_plain_float32_numpy_s():
    said = []
    for c in FINITE:
        if c.M < 64 or c.h1 < 33 or c.h2 < 17:
            continue
        a = CC.arrays_of(c)
        share = CC.bite_share(c, a)
        print("%-48s %.3f of %d gradient elements differ in their bits from plain float32 numpy" % (c.id, share, sum(BC.sizes_of(a.weights))))
        if share <= CC.BITE:
            said.append("%s: %.3f" % (c.id, share))
    assert not said, said


def sums_mutant(c, letter):
    """Mutants (e) and (f) change what is done with the wavefronts' sums: from the restatement's own, at no cost"""
    base = restated(c)
    grid, waves = PC.backward_plan_of(c)
    a = CC.arrays_of(c)
    partials = BC.add_wavefronts(*base.sums, grid, waves, pairs=letter == "e")
    return BC.Restated(partials, BC.split(BC.add_partials(partials, tree=letter == "f"), a.weights), base.live, None, base.sums)


def multi_pass(c):
    """A wavefront of the case's call owns two live tiles or more"""
    r = restated(c)
    grid, waves = PC.backward_plan_of(c)
    group, wave = BC.owner_of_tiles(r.live, grid, waves)
    return len(np.unique(group * waves + wave)) < len(r.live)


def test_every_mutant_changes_bits_where_it_can_and_nowhere_else():
    small = tuple(CC.named(t) for t in ("96_64_64-65rows-contiguous-dense", "96_64_64-65rows-indexed-dense", "76_40_24-65rows-indexed-dense"))
    at_zero = tuple(c for c in CC.REAL if c.pattern == "at_zero")
    some_sparse = tuple(c for c in CC.SPARSE if c.in_dim in (136, 76))
    where = {m: CC.REAL + some_sparse for m in "abdhi"}
    where.update({m: small + CC.SPARSE for m in "cg"})
    where.update({m: FINITE for m in "ef"})
    where["j"] = at_zero + small
    where["k"] = tuple(c for c in CC.REAL if c.mode == "indexed") + tuple(c for c in some_sparse if c.mode == "indexed")
    assert len(at_zero) == 3 and sorted(where) == sorted(set(BC.MUTANTS) - {"l"})
    bites = {}
    for m, cases in where.items():
        for c in cases:
            mutant = sums_mutant(c, m) if m in "ef" else CC.restated_of(c, frozenset(m))
            bites[m, c.id] = differs(mutant, restated(c))
    # (e) and (f) through restate itself, once: the shortcut above is the same thing
    c = CC.named("56_33_17-488rows-indexed-dense")
    for m in "ef":
        assert not differs(CC.restated_of(c, frozenset(m)), sums_mutant(c, m)) and bites[m, c.id]
    print("\n%-48s %s" % ("bits change under mutant", " ".join(sorted(where))))
    for c in FINITE:
        print("%-48s %s" % (c.id, " ".join({True: "X", False: "=", None: "."}[bites.get((m, c.id))] for m in sorted(where))))
    for m, words in sorted(BC.MUTANTS.items()):
        print("(%s) %s" % (m, words))
    for m in where:
        seen = [c for c in where[m] if bites[m, c.id]]
        assert len(seen) >= 3, (m, [c.id for c in seen])
    for c in FINITE:
        grid, waves = PC.backward_plan_of(c)
        group, wave = BC.owner_of_tiles(restated(c).live, grid, waves)
        on = lambda m: bites.get((m, c.id), False)  # noqa: E731
        if c.M == 1:  # one row: the first fmaf from +0 is the rounded product, and there is no order of rows
            assert not on("a") and not on("d"), c.id
        # the other dealing: from two workgroups up
        assert on("b") == (grid > 1) or ("b", c.id) not in bites, c.id
        # an accumulator or a bias sum per tile: only where a wavefront has a second tile, and in every sparse case
        assert all(on(m) == multi_pass(c) for m in "cg" if (m, c.id) in bites), c.id
        # (w0 + w1) + (w2 + w3): where a workgroup of four has live wavefronts 2 and 3 (97 rows and up), and nowhere else
        both = any({2, 3} <= set(wave[group == g].tolist()) for g in np.unique(group))
        assert on("e") == (waves == 4 and both), c.id
        # a tree of partials: only from four workgroups up (488 rows; in the sparse calls the tree of workgroups 0, 1, 2 and
        # G - 1 among zeros IS ((p0 + p1) + p2) + p255, as is every order that keeps these four in their relative order: the
        # order of adding the partials is held at G <= 4 only — backward_chain_cases, SPARSE, says what would hold it at 256)
        assert not on("f") or grid >= 4, c.id
        assert on("f") or grid < 4 or c.pattern == "sparse", c.id
        # the derivative at 0: the cases made for it, and no other
        assert on("j") == (c.pattern == "at_zero") or ("j", c.id) not in bites, c.id
        # out-of-range rows' gradients: indexed calls only
        assert not on("k") or c.mode == "indexed", c.id
    assert all(multi_pass(c) for c in CC.SPARSE) and not any(multi_pass(c) for c in CC.REAL)


def test_computing_the_all_zero_tiles_changes_nothing_but_a_nan():
    dead = [c for c in CC.REAL if len(restated(c).live) < -(-c.M // 32)]
    # (the zero_tiles cases, and a call whose last tile of ONE row is an out-of-range entry)
    assert {c for c in CC.REAL if c.pattern == "zero_tiles"} < set(dead) and len(dead) == 4
    for c in dead:
        assert not differs(CC.restated_of(c, frozenset("l")), restated(c)), c.id
    # the sparse calls: workgroup 0 alone, which owns the skipped tile between two live ones (two thousand tiles are not restated)
    for c in CC.SPARSE + CC.NAN:
        base = restated(c)
        all_tiles = CC.restated_of(c, frozenset("l"), only=(0,))
        assert len(all_tiles.live) == -(-c.M // 32) > len(base.live)
        same = np.array_equal(MC.canon(all_tiles.partials[0]), MC.canon(base.partials[0]))
        if c in CC.NAN:
            assert np.isnan(all_tiles.partials[0]).any() and not same, c.id
            assert np.isfinite(base.partials).all() and not differs(base, restated(CC.base_of(c))), c.id
        else:
            assert same, c.id


# ------------------------------------------------------------------------------------------ the sparse cases
@pytest.mark.parametrize("c", CC.SPARSE, ids=lambda c: c.id)
def test_a_sparse_case_is_what_its_list_says(c):
    a = CC.arrays_of(c)
    grid, waves = PC.backward_plan_of(c)
    assert grid == 256 and c.M == PC.three_passes(c.in_dim) and waves == (3 if c.in_dim == 136 else 4)
    r = restated(c)
    # the live tiles are exactly the listed ones
    assert np.array_equal(r.live, CC.listed_tiles(c)) and np.array_equal(BC.live_tiles(PC.upstream(a)), r.live)
    assert len(r.live) == 10 * waves + 1 and r.live[-1] == -(-c.M // 32) - 1 and c.M % 32 == 1
    # every live wavefront has three live tiles, except the one with the skipped middle tile and those the third pass does not reach
    group, wave, turn = (v[r.live] for v in CC.dealing(c))
    n_tiles = -(-c.M // 32)
    for g in (0, 1, 2, grid - 1):
        for w in range(waves):
            mine = turn[(group == g) & (wave == w)].tolist()
            reached = (2 * grid + g) * waves + w < n_tiles
            assert mine == ([0, 2] if (g, w) == (0, 1) else [0, 1, 2] if reached else [0, 1]), (c.id, g, w, mine)
    assert set(group.tolist()) == {0, 1, 2, grid - 1}
    assert sum(((2 * grid + g) * waves + w < n_tiles) for g in (0, 1, 2) for w in range(waves)) == 2 * waves + 2
    # the third pass alone and the last row alone reach each of the eight arrays (float64 reference); out-of-range rows under gradients
    assert CC.sparse_misses(c, a) == []
    assert a.valid[-1] and (c.mode == "contiguous" or (~a.valid[np.isin(np.arange(c.M) // 32, r.live)]).sum() >= 8)
    # the partials of all other workgroups are +0
    others = np.setdiff1d(np.arange(grid), (0, 1, 2, grid - 1))
    assert not r.partials[others].view(np.uint32).any() and all(r.partials[g].any() for g in (0, 1, 2, grid - 1))
    BC.no_subnormals(r)


def test_no_case_comes_near_a_subnormal_number():
    for c in CC.CASES:
        BC.no_subnormals(restated(c))
    # (the watch sees a product below 2^-126)
    w = [np.full((56, 1), 2.0 ** -70, F32), np.zeros(1, F32), np.ones((1, 1), F32), np.zeros(1, F32), np.ones((1, 6), F32), np.zeros(6, F32), np.ones(1, F32), np.zeros(1, F32)]
    x, d3 = np.full((1, 56), 1.0, F32), np.full((1, 7), 2.0 ** -70, F32)
    with pytest.raises(AssertionError, match="2\\^-126"):
        BC.no_subnormals(BC.restate(x, d3, w, 1, 4, watch=True))  # a1 = 56 * 2^-70 times delta2 = 7 * 2^-70
    BC.no_subnormals(BC.restate(x, np.full((1, 7), 1.0, F32), w, 1, 4, watch=True))


def test_zz_every_restatement_takes_a_few_seconds_at_most():
    for c in CC.CASES:
        restated(c)
    for c in CC.CASES:
        print("%-48s %5.2f s (%d live tiles)" % (c.id, DURATIONS[c.id], len(restated(c).live)))
    print("all %d restatements: %.1f s" % (len(DURATIONS), sum(DURATIONS.values())))
    worst = max(DURATIONS, key=DURATIONS.get)
    assert DURATIONS[worst] <= 10.0, (worst, DURATIONS[worst])
