"""The dense cases of tests/partner_dense_cases.py and their restatement (tests/mlp_chain.py) without a GPU: the chain against the
float64 reference and its a-priori bound, exactly on the integer kind, and AWAY from numpy's own float32 order in most of its bits —
the evidence that the device comparison of tests/test_gpu_mlp_chain.py tells the header's arithmetic from another; no case near a
subnormal number; every case bites; every seat pattern and pool case has the property it is named for; four mutants of the
reference are seen."""
import numpy as np
import pytest

import mlp_chain as MC
import partner_cases as PC
import partner_dense_cases as D

REAL = [c for c in D.CASES if c.kind == "real"]
INT = [c for c in D.CASES if c.kind == "int"]
ID = dict(ids=lambda c: c.id)


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def rows_of(c):
    a = D.arrays_of(c)
    return a.rows[a.seated, a.p]


# ------------------------------------------------------------------------------------------ the chain on the cases
@pytest.mark.parametrize("c", REAL, **ID)
def test_the_chain_is_within_the_bound_of_f64_and_is_not_numpy_s_order(c):
    a, x, r = D.arrays_of(c), rows_of(c), D.reference_of(c)
    ref, _ = PC.mlp_f64(x, a.weights)
    err = np.abs(r.out.astype(np.float64) - ref)
    assert np.isfinite(r.out).all() and (err <= PC.mlp_bound(x, a.weights)).all(), c.id
    other = PC.mlp_f32(x, a.weights)
    share = float((MC.canon(other) != MC.canon(r.out)).mean())
    print("%s: %d logits, largest error %.3g (numpy's order: %.3g), %.1f %% differ in their bits from numpy's order"
          % (c.id, r.out.size, err.max(), np.abs(other.astype(np.float64) - ref).max(), 100 * share))
    if min(c.h1, c.h2) >= 17:
        assert share > 0.5, (c.id, share)


def abs_sums(x, weights):
    """The largest sum of absolute terms of any unit of the three layers: every partial sum, in any order, is at most this"""
    w1, b1, w2, b2, w3, b3 = (np.abs(f64(w)) for w in weights)
    _, (a1, a2) = PC.mlp_f64(x, weights)
    return max(float(np.max(np.abs(f64(x)) @ w1 + b1)), float(np.max(a1 @ w2 + b2)), float(np.max(a2 @ w3 + b3)))


@pytest.mark.parametrize("c", INT, **ID)
def test_the_chain_of_an_integer_case_is_the_f64_reference_exactly(c):
    a, x, r = D.arrays_of(c), rows_of(c), D.reference_of(c)
    for v in (x,) + a.weights:
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 6
    assert abs_sums(x, a.weights) < 2 ** 24
    ref, (a1, a2) = PC.mlp_f64(x, a.weights)
    assert np.array_equal(r.out.astype(np.float64), ref), c.id
    assert np.array_equal(np.maximum(r.pre1, 0).astype(np.float64), a1) and np.array_equal(np.maximum(r.pre2, 0).astype(np.float64), a2)
    assert np.array_equal(PC.mlp_f32(x, a.weights).astype(np.float64), ref)  # (any order is)


@pytest.mark.parametrize("c", D.CASES, **ID)
def test_no_case_comes_near_a_subnormal_number(c):
    assert D.reference_of(c).smallest >= MC.MIN_NORMAL


# ------------------------------------------------------------------------------------------ the cases bite
@pytest.mark.parametrize("c", D.CASES, **ID)
def test_every_case_bites(c):
    a = D.arrays_of(c)
    n_rows = len(a.seated)
    assert n_rows >= 1 and np.array_equal(a.seat, D.seats_of(c))
    r = D.report(c, a)
    assert r.cols == [], "zeroing feature column(s) %s changes no seated logit" % r.cols
    assert (rows_of(c)[:D.BITE_ROWS] != 0).any(0).all()
    if n_rows >= 16 or (c.h1, c.h2) == (1, 1):
        assert r.units1 == [] and r.units2 == [], (r.units1, r.units2)
    if min(c.h1, c.h2) >= 17:
        assert 0.3 <= r.live <= 0.7 and r.other_row >= 0.5 and (r.next_row is None or r.next_row >= 0.5), r
        assert (r.next_row is None) == (c.n_envs == 1)
    if c.kind == "int" and r.n_pre >= 64:
        assert r.zeros > 0
    assert D.misses(c, a) == []
    # the device's features: the dense rows where a seat names them, NaN everywhere else; both players' rows of an env differ
    named = np.zeros((c.n_envs, 2), bool)
    named[a.seated, a.p] = True
    assert np.array_equal(np.isnan(a.features).all(-1), ~named) and np.array_equal(np.isnan(a.features).any(-1), ~named)
    assert np.array_equal(a.features[named], a.rows[named]) and (a.rows[:, 0] != a.rows[:, 1]).any(-1).all()
    assert np.isfinite(a.rows).all() and a.features.dtype == np.float32 and a.features.shape == (c.n_envs, 2, c.in_dim)


def test_the_case_list_covers_what_it_says():
    for kind in D.KINDS:
        mine = [c for c in D.CASES if c.kind == kind]
        shapes = {(c.in_dim, c.h1, c.h2) for c in mine}
        assert {(d, h1, h2) for d in D.LENGTHS for h1, h2 in D.WIDTHS} <= shapes
        assert {c.n_envs for c in mine if (c.in_dim, c.h1, c.h2) == (96, 64, 64) and c.pattern == "seeded"} == set(D.SIZES)
        assert {c.n_envs for c in mine if c.pattern == "seeded"} == set(D.SIZES)
        assert {c.in_dim for c in mine if c.pattern == "drawn"} == set(D.LENGTHS)
        for name in D.SEAT_PATTERNS:
            sizes = {c.n_envs for c in mine if c.pattern == name}
            assert sizes == ({600} if name == "empty_workgroup_between" else {488, 600}), name  # (a middle workgroup takes three)
    assert len(REAL) == len(INT) and [c.id.split("-", 1)[1] for c in REAL] == [c.id.split("-", 1)[1] for c in INT]
    fill = D.logits_fill(600)
    assert len(np.unique(fill)) == fill.size and not (fill == np.round(fill)).any() and np.isfinite(fill).all()


@pytest.mark.parametrize("n", (488, 600))
def test_every_seat_pattern_has_the_property_it_is_named_for(n):
    two = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    e = np.arange(n)
    tile, wave, group = e // 32, (e % 256) // 64, e // 256
    on = lambda s: s <= 1  # noqa: E731
    seat = {name: fn(n, two) for name, fn in D.SEAT_PATTERNS.items() if n >= 513 or name != "empty_workgroup_between"}
    for name, s in seat.items():
        assert s.dtype == np.uint8 and s.shape == (n,) and on(s).any(), name
        assert np.array_equal(s[on(s)], two[on(s)]) or name in ("all0", "all1", "alternate"), name
    assert (seat["all0"] == 0).all() and (seat["all1"] == 1).all()
    assert np.array_equal(seat["alternate"], e % 2)
    s = seat["one_per_tile"]
    per_tile = np.bincount(tile[on(s)], minlength=tile.max() + 1)
    assert (per_tile == 1).all() and len(set((e[on(s)] % 32).tolist())) >= 8 and (s[~on(s)] == 255).all()
    for name, first in (("empty_first_tile", True), ("empty_second_tile", False)):
        s = seat[name]
        assert np.array_equal(on(s), (tile % 2 == 1) == first), name  # the wavefront's envs 0..31 are tile 2 w, 32..63 tile 2 w + 1
        assert {int(w) for w in np.unique(e // 64)} == {int(w) for w in np.unique((e // 64)[on(s)])} or n % 64 <= 32, name
    s = seat["empty_waves_between"]
    assert np.array_equal(on(s), (wave == 0) | (wave == 3))
    for g in np.unique(group):  # every workgroup with four wavefronts has seated ones on both sides of its empty pair
        if (group == g).sum() == 256:
            assert on(s[(group == g) & (wave == 0)]).all() and on(s[(group == g) & (wave == 3)]).all() and not on(s[(group == g) & ((wave == 1) | (wave == 2))]).any()
    if "empty_workgroup_between" in seat:
        s = seat["empty_workgroup_between"]
        assert group.max() == 2 and on(s[group == 0]).all() and not on(s[group == 1]).any() and on(s[group == 2]).all()
    s = seat["last_env_only"]
    assert on(s).sum() == 1 and on(s[-1]) and (s[:-1] == 255).all()
    s = seat["other_bytes"]
    rest = s[~on(s)]
    assert on(s).sum() > n // 3 and len(rest) > n // 3 and rest.min() == 2 and rest.max() == 254 and len(np.unique(rest)) > 100
    # every 32-env tile holds seated and unseated envs: such a byte sits beside a live column of its tile
    assert all(on(s[tile == t]).any() and (~on(s[tile == t])).any() for t in np.unique(tile))


# ------------------------------------------------------------------------------------------ the pool cases
@pytest.mark.parametrize("c", D.POOL_CASES, **ID)
def test_every_pool_case_holds_what_it_claims(c):
    a = D.pool_arrays_of(c)
    K = c.n_members
    counts = D.bucket_counts(c)
    seat, member = a.seat, a.member
    served = (seat <= 1) & (member < K)
    assert np.array_equal(np.flatnonzero(served), a.served) and counts.sum() == len(a.served) > 0
    if c.drawn:
        assert (counts > 32).all() and ((member == 255) == (seat == 255)).all() and (seat == 255).sum() > c.n_envs // 3
    else:
        assert counts.tolist() == list(c.counts)
        q = D.NULL_EACH
        assert ((seat <= 1) & (member == 255)).sum() == q                      # a seat, and member 255
        beyond = (seat <= 1) & (member >= K) & (member < 255)
        assert beyond.sum() == q and member[beyond].min() == K and member[beyond].max() == 254  # a seat, and a member beyond the pool
        assert ((seat == 255) & (member < K)).sum() == q                       # a member, and seat 255
        other = (seat > 1) & (seat < 255) & (member < K)
        assert other.sum() == q and len(np.unique(seat[other])) == q           # a member, and another seat byte
        assert ((seat == 255) & (member == 255)).sum() == q
        assert c.n_envs == sum(c.counts) + 5 * q
        # interleaved: the bucket order is no identity, and every member's envs are spread over the batch
        assert not np.array_equal(a.served, np.arange(len(a.served)))
        if K > 1:
            assert (np.diff(member[a.served].astype(int)) < 0).sum() > len(a.served) // (2 * K + 2)
    assert D.pool_shapes_of(c) == tuple(D.WIDTHS[m % 5] for m in range(K)) and len(a.weights) == K
    for m, w in enumerate(a.weights):
        assert [v.shape for v in w] == [(c.in_dim, D.pool_shapes_of(c)[m][0]), (D.pool_shapes_of(c)[m][0],), D.pool_shapes_of(c)[m],
                                        (D.pool_shapes_of(c)[m][1],), (D.pool_shapes_of(c)[m][1], 6), (6,)]
    assert D.pool_misses(c, a) == []
    named = np.zeros((c.n_envs, 2), bool)
    named[a.served, a.p] = True
    assert np.array_equal(np.isnan(a.features).all(-1), ~named) and np.array_equal(a.features[named], a.rows[named])
    ref, smallest = D.pool_reference_of(c)
    assert smallest >= MC.MIN_NORMAL and np.isfinite(ref).all()
    for m in range(K):
        mine = member[a.served] == m
        if not mine.any():
            continue
        x = a.rows[a.served[mine], a.p[mine]]
        want, _ = PC.mlp_f64(x, a.weights[m])
        if c.kind == "int":
            assert np.array_equal(ref[mine].astype(np.float64), want) and abs_sums(x, a.weights[m]) < 2 ** 24
        else:
            assert (np.abs(ref[mine].astype(np.float64) - want) <= PC.mlp_bound(x, a.weights[m])).all()


def test_the_pool_cases_cover_the_edges_of_tile_pass_and_chunk():
    for kind in D.KINDS:
        mine = [c for c in D.POOL_CASES if c.kind == kind]
        seen = set()
        for c in mine:
            seen |= set(D.bucket_counts(c).tolist())
        assert set(D.POOL_SIZES) <= seen, sorted(set(D.POOL_SIZES) - seen)
        assert {c.n_members for c in mine} == {1, 3, 16} and {c.in_dim for c in mine if not c.drawn} == set(D.LENGTHS)
        assert sum(c.drawn for c in mine) == 1 and max(c.n_envs for c in mine) < 2000
        # every width is weighed (16 rows or more) at some member
        weighed = {D.pool_shapes_of(c)[m] for c in mine for m in range(c.n_members) if D.bucket_counts(c)[m] >= 16}
        assert weighed == set(D.WIDTHS)


# ------------------------------------------------------------------------------------------ mutants of the reference
def mutants(c):
    """name -> float32 logits of the first BITE_ROWS seated rows under a mutant of the chain (None: the mutant does not apply)"""
    a = D.arrays_of(c)
    e, p = a.seated[:D.BITE_ROWS], a.p[:D.BITE_ROWS]
    x, d = a.rows[e, p], c.in_dim
    w1, b1, w2, b2, w3, b3 = a.weights
    return {"last_step_dropped": MC.chain_f32(x, a.weights, order=range(d - 1)),
            "last_two_steps_swapped": MC.chain_f32(x, a.weights, order=list(range(d - 2)) + [d - 1, d - 2]),
            "last_unit_dropped": MC.chain_f32(x, (w1[:, :-1], b1[:-1], w2[:-1], b2, w3, b3)),
            "other_player_s_row": MC.chain_f32(a.rows[e, 1 - p], a.weights)}


@pytest.mark.parametrize("c", D.CASES, **ID)
def test_the_mutants_of_the_reference_are_seen(c):
    """The last K step of layer 1 dropped; its two K indices taken in the other order; unit h1 - 1 dropped; the other player's row
    read.  Where a mutant applies — the dropped step always (every column bites); the dropped unit where the unit condition is asked
    (16 seated rows, or widths (1, 1)); the other row at widths >= 17 (asked there) and at 16 rows; the swap, which changes one
    rounding of a chain in about one chain of three, at 16 rows of widths >= 17 — it changes the result; all but the swap, to which
    exact sums are blind, change the integer kind's too."""
    a = D.arrays_of(c)
    n_rows = min(len(a.seated), D.BITE_ROWS)
    want = MC.canon(D.reference_of(c).out[:n_rows])
    wide, many = min(c.h1, c.h2) >= 17, n_rows >= 16
    applies = {"last_step_dropped": True, "last_two_steps_swapped": c.kind == "real" and wide and many,
               "last_unit_dropped": many or (c.h1, c.h2) == (1, 1), "other_player_s_row": wide or many}
    for name, got in mutants(c).items():
        changed = bool((MC.canon(got) != want).any())
        if applies[name]:
            assert changed, (c.id, name)
        if c.kind == "int" and name == "last_two_steps_swapped":
            assert not changed, c.id
