"""oc_partner_pool_logits without a GPU: the exports and the struct against the header, the plan's words, every refusal (made before
any device call: this host has no device), the member draw restated twice — near counters and far ones —, the seats equal to the
single-policy stream's, the uniform thresholds against the multiply-high form, PartnerPool's weighted thresholds, the statistics of
the draw, the truncations a kernel could commit, and the case list's own claims."""
import ctypes
import os
import re

import numpy as np
import pytest

import partner_cases as PC
import pool_cases as PP
from case_support import P, ROOT, synthetic_batch

EINVAL = -1
WHO = "oc_partner_pool_logits: "


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_the_struct_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_partner_pool_logits", "oc_partner_pool_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert "#define OC_MAX_POOL 16" in hdr and _lib.MAX_POOL == PP.MAX_POOL == 16
    body = re.search(r"typedef struct OcPartnerPool \{(.*?)\} OcPartnerPool;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(members|n_members|thresholds|d_member)\b", body) == [f[0] for f in _lib.OcPartnerPool._fields_]
    S = _lib.OcPartnerPool
    assert ctypes.sizeof(S) == 32 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24]
    assert ("int oc_partner_pool_logits(const OcBatch* batch, const OcPartnerPool* pool, const OcPartnerSeats* seats, const float* d_features,\n"
            "                           int num_pots, float* d_logits, void* d_scratch, void* stream);") in hdr
    assert "int oc_partner_pool_plan(const OcBatch* batch, const OcPartnerPool* pool, int num_pots, char* out, size_t out_size);" in hdr
    assert len(L.oc_partner_pool_logits.argtypes) == 8 and len(L.oc_partner_pool_plan.argtypes) == 5
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_draw_the_restatements_restate():
    hdr = _header()
    for words in ("member = #{ m < n_members - 1 : r[2] >= thresholds[m] }", "thresholds[m] = ceil((m + 1) * 2^32 / n_members)",
                  "member = (r[2] * n_members) >> 32", "255 where the reseated env has no partner", "keeps both its seat and its member",
                  "Word 3\n * stays reserved", "byte-equal", "bit-equal", "repeats byte for byte", "contents after a call are unspecified"):
        assert words in hdr, words


def _policy(in_dim=96, h1=64, h2=64, ptrs=(P,) * 6):
    from overcooked_ai_amd import _lib

    return _lib.OcDensePolicy(*ptrs, in_dim, h1, h2)


def _pool(members=None, n=None, thresholds=None, d_member=P):
    """(OcPartnerPool, what it points to)"""
    from overcooked_ai_amd import _lib

    members = [_policy(), _policy(h1=40, h2=24), _policy(h1=1, h2=1)] if members is None else members
    arr = (_lib.OcDensePolicy * max(1, len(members)))(*members)
    thr = (ctypes.c_uint32 * len(thresholds))(*thresholds) if thresholds is not None else None
    return _lib.OcPartnerPool(arr, len(members) if n is None else n, thr, d_member), (arr, thr)


def _plan(b, pool, num_pots=2):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(512)
    rc = L.oc_partner_pool_plan(ctypes.byref(b) if b is not None else None, ctypes.byref(pool) if pool is not None else None, num_pots, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def scratch_bytes(n, k):
    """Restated: the count (8 bytes, padded to 64), sixteen 64-byte rows of the member table, k counts per 256-env block and one
    more, an order entry per env"""
    return 64 + 16 * 64 + 4 * (k * ((n + 255) // 256) + 1) + 4 * n


def test_the_plan_in_words():
    pool, keep = _pool([_policy()] * 4)
    rc, text = _plan(synthetic_batch(5, 4, 65536), pool)
    assert rc == 0 and text == ("k_pool_seat grid=256, 256 lanes + k_sample_scan grid=1, 256 lanes, 5 pass(es) of 256 counts + k_pool_write grid=256, 256 lanes + "
                                "k_pool_logits grid=260 (256 blocks of envs + 4 members), 256 lanes (128 j rows of one member), 32 x 32 x 2 f32 MFMA, "
                                "K 96 -> 64 -> 64 -> 32, 101248 B LDS; scratch 267332 B"), text
    assert text in _header() and scratch_bytes(65536, 4) == 267332
    for num_pots, k, n in ((1, 1, 1), (4, 3, 488), (0, 16, 257), (2, 16, 1500)):
        d = PC.total_of(num_pots)
        lds = 4 * (d * 64 + 64 * 64 + 64 * 32 + 160 + 64 + 256 + 4 * 32 * (d + 2))  # partner.hpp's, and an env per row
        pool, keep = _pool([_policy(d, *PP.SHAPES[m % 3]) for m in range(k)])
        rc, text = _plan(synthetic_batch(5, 4, n), pool, num_pots)
        blocks = (n + 255) // 256
        assert rc == 0 and text.startswith("k_pool_seat grid=%d, " % blocks) and text.endswith(", %d B LDS; scratch %d B" % (lds, scratch_bytes(n, k))), text
        assert "k_pool_write grid=%d, " % blocks in text and "k_pool_logits grid=%d (%d blocks of envs + %d members)" % (blocks + k, blocks, k) in text
        assert "%d pass(es) of 256 counts" % ((k * blocks + 1 + 255) // 256) in text and "K %d -> 64 -> 64 -> 32" % d in text and lds <= 160 * 1024
    pool, keep = _pool()
    assert _plan(synthetic_batch(5, 4, 0), pool) == (0, "nothing to launch (no envs)")
    b = synthetic_batch(5, 4, 10)
    for bb, pp, num_pots, why in ((None, _pool(), 2, "batch is NULL"), (b, (None, None), 2, "pool is NULL"), (b, _pool(), 5, "num_pots must be in 0..4"),
                                  (b, _pool(n=0), 2, "pool.n_members must be in 1..16"), (b, _pool(n=17), 2, "pool.n_members must be in 1..16"),
                                  (b, _pool(), 1, "policy.in_dim must equal the feature length"),
                                  (b, _pool([_policy(), _policy(in_dim=76)]), 2, "policy.in_dim must equal the feature length"),
                                  (b, _pool([_policy(), _policy(), _policy(h2=65)]), 2, "policy.h1 and policy.h2 must be in 1..64"),
                                  (b, _pool(thresholds=[5, 4]), 2, "pool.thresholds must not decrease"),
                                  (synthetic_batch(5, 4, 2**31), _pool(), 2, "batch.n_envs must be below 2^31"),
                                  (synthetic_batch(5, 4, -1), _pool(), 2, "batch.n_envs < 0")):
        rc, msg = _plan(bb, pp[0], num_pots)
        assert rc == EINVAL and msg.startswith(WHO + why), (why, msg)
    rc, msg = _plan(b, _pool([_policy(), _policy(), _policy(h2=65)])[0])
    assert msg.endswith("(members[2])"), msg
    from overcooked_ai_amd import _lib

    nomem = _lib.OcPartnerPool(None, 3, None, P)
    assert _plan(b, nomem)[1].startswith(WHO + "pool.members is NULL")
    assert _plan(b, _pool(thresholds=[4, 4])[0])[0] == 0  # (equal thresholds: a member of probability 0)


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()

    def call(b=(), pool=(), seats=(), features=P, num_pots=2, logits=P, seat=P, done=P, factor=0.5, scratch=P):
        b = synthetic_batch(5, 4, 1000) if b == () else b
        pool, keep = _pool() if pool == () else pool
        seats = _lib.OcPartnerSeats(seat, done, factor, 7, 0, 0) if seats == () else seats
        rc = L.oc_partner_pool_logits(ctypes.byref(b) if b is not None else None, ctypes.byref(pool) if pool is not None else None,
                                      ctypes.byref(seats) if seats is not None else None, features, num_pots, logits, scratch, None)
        return rc, L.oc_last_error().decode()

    null = lambda i: tuple(None if k == i else P for k in range(6))  # noqa: E731
    off = lambda i: tuple(P + 2 if k == i else P for k in range(6))  # noqa: E731
    refusals = [(dict(pool=(None, None)), "pool is NULL"), (dict(pool=(_lib.OcPartnerPool(None, 3, None, P), None)), "pool.members is NULL"),
                (dict(pool=_pool(d_member=None)), "pool.d_member is NULL"), (dict(scratch=None), "d_scratch is NULL"),
                (dict(scratch=P + 8), "d_scratch must be 16-byte aligned"),
                (dict(pool=_pool(n=0)), "pool.n_members must be in 1..16"), (dict(pool=_pool([_policy()] * 17)), "pool.n_members must be in 1..16"),
                (dict(pool=_pool([_policy(), _policy(in_dim=76)])), "policy.in_dim must equal the feature length"),
                (dict(pool=_pool([_policy(h1=0)])), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(pool=_pool([_policy(), _policy(h1=65)])), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(pool=_pool([_policy(), _policy(h2=0)])), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(pool=_pool([_policy()] * 15 + [_policy(h2=65)])), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(pool=_pool(thresholds=[9, 8])), "pool.thresholds must not decrease"),
                (dict(pool=_pool([_policy()] * 4, thresholds=[1, 2**32 - 1, 2**32 - 2])), "pool.thresholds must not decrease"),
                # ---- whatever oc_partner_logits refuses
                (dict(b=None), "batch is NULL"), (dict(seats=None), "seats is NULL"), (dict(seat=None), "seats.d_seat is NULL"),
                (dict(features=None), "NULL d_features or d_logits"), (dict(logits=None), "NULL d_features or d_logits"),
                (dict(features=P + 8), "d_features must be 16-byte aligned"), (dict(logits=P + 4), "d_logits must be 8-byte aligned"),
                (dict(num_pots=1), "policy.in_dim must equal the feature length"),
                (dict(factor=-0.001), "seats.bc_factor must be in [0, 1]"), (dict(factor=1.001), "seats.bc_factor must be in [0, 1]"),
                (dict(factor=float("nan")), "seats.bc_factor must be in [0, 1]"),
                (dict(num_pots=-1), "num_pots must be in 0..4"), (dict(num_pots=5), "num_pots must be in 0..4"),
                (dict(b=synthetic_batch(5, 4, -1)), "batch.n_envs < 0"), (dict(b=synthetic_batch(5, 4, 2**31)), "batch.n_envs must be below 2^31")]
    for m in (0, 2):
        mk = lambda bad: [bad if k == m else _policy() for k in range(3)]  # noqa: E731
        refusals += [(dict(pool=_pool(mk(_policy(ptrs=null(i))))), "NULL weight or bias array") for i in range(6)]
        refusals += [(dict(pool=_pool(mk(_policy(ptrs=off(i))))), "weight and bias arrays must be 4-byte aligned") for i in range(6)]
    for kw, why in refusals:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith(WHO + why), (kw, rc, msg)
    assert call(pool=_pool([_policy(), _policy(ptrs=null(3))]))[1].endswith("(members[1])")
    # accepted on no envs (nothing to launch): no scratch, no done mask, both ends of bc_factor, equal thresholds, one member
    for kw in (dict(scratch=None), dict(done=None), dict(factor=0.0), dict(factor=1.0), dict(pool=_pool(thresholds=[7, 7])),
               dict(pool=_pool([_policy()])), dict(pool=_pool([_policy()] * 16)), dict(logits=P + 8)):
        assert call(b=synthetic_batch(5, 4, 0), **kw)[0] == 0, kw


# ------------------------------------------------------------------------------------------ the draw
NEAR = dict(seed=61, env_offset=3 * 488 + 37, step=5, n=488)


def _far():
    c = PC.far_case()
    return dict(seed=c.seed, env_offset=c.env_offset, step=c.step, n=c.n_envs)


@pytest.mark.parametrize("at", (NEAR, _far()), ids=("near", "far"))
def test_the_two_restatements_of_the_draw_agree_and_the_seats_are_the_single_policy_streams(at):
    for k in (1, 2, 3, 5, 16):
        for factor in (0.0, 0.5, 1.0):
            seat, member = PP.draws(bc_factor=factor, thresholds=PP.uniform_thresholds(k), **at)
            s2, m2 = PP.draws_by_the_header(bc_factor=factor, n_members=k, **at)
            assert seat.dtype == member.dtype == np.uint8 and np.array_equal(seat, s2) and np.array_equal(member, m2), (k, factor)
            assert np.array_equal(seat, PC.seats(bc_factor=factor, **at)), (k, factor)
            assert ((member == PP.NO_MEMBER) == (seat == PC.NO_SEAT)).all() and (member[seat != PC.NO_SEAT] < k).all()
    thr = [2**30, 2**30, 3 * 2**30]  # weighted, with a member of probability 0
    seat, member = PP.draws(bc_factor=0.5, thresholds=thr, **at)
    s2, m2 = PP.draws_by_the_header(bc_factor=0.5, n_members=4, thresholds=thr, **at)
    assert np.array_equal(seat, s2) and np.array_equal(member, m2) and set(np.unique(member)) == {0, 2, 3, PP.NO_MEMBER}


@pytest.mark.parametrize("k", (1, 2, 3, 5, 7, 16))
def test_uniform_thresholds_are_the_multiply_high_form(k):
    thr = PP.uniform_thresholds(k)
    assert len(thr) == k - 1 and all(0 < t < 2**32 for t in thr) and thr == sorted(thr)
    assert thr == [((m + 1) * 2**32 + k - 1) // k for m in range(k - 1)]
    r2 = PP.words(77, 0, 3, 200000)[2]
    edges = np.array([t + d for t in thr for d in (-1, 0, 1)] + [0, 2**32 - 1], dtype=np.uint64)  # and either side of every threshold
    for w in (r2.astype(np.uint64), edges):
        assert np.array_equal(PP.members_of_words(w, thr), ((w * np.uint64(k)) >> np.uint64(32)).astype(np.uint8))


def test_the_weighted_thresholds_of_partner_pool():
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool, thresholds_of

    assert thresholds_of([1, 1, 1, 1]) == PP.uniform_thresholds(4) and thresholds_of([2.0] * 7) == PP.uniform_thresholds(7)
    assert thresholds_of([1, 0, 2, 1]) == [2**30, 2**30, 3 * 2**30]
    assert thresholds_of([1, 3]) == [2**30] and thresholds_of([5]) == [] and thresholds_of([0, 1]) == [0]
    assert thresholds_of([1, 0]) == [2**32 - 1]  # (the cap: a last member of weight 0 keeps 2^-32)
    assert thresholds_of([1, 2]) == [-(-2**32 // 3)]  # rounded up
    for bad in ([], [0, 0], [1, -1]):
        with pytest.raises(ValueError):
            thresholds_of(bad)
    c = next(c for c in PP.CASES if c.weights)
    assert thresholds_of(c.weights) == PP.thresholds_of(c)
    member = PP.draws(9, 0, 0, 65536, 1.0, PP.thresholds_of(c))[1]
    counts = np.bincount(member, minlength=4)
    assert counts[1] == 0 and abs(PP.chi_square_z(np.delete(counts, 1), 65536 * np.array([0.25, 0.5, 0.25]))) <= 6
    # ---- the Python surface (no device)
    pols = [DensePolicy(*PC.glorot(m, 96, *PP.SHAPES[m % 3]), device="cpu") for m in range(4)]
    pool = PartnerPool(pols, weights=c.weights)
    assert (pool.n_members, pool.in_dim, pool.thresholds) == (4, 96, PP.thresholds_of(c)) and PartnerPool(pols).thresholds is None
    import torch

    member = torch.full((8,), 255, dtype=torch.uint8)
    s = pool.struct_for(member)
    assert s.n_members == 4 and s.d_member == member.data_ptr() and[s.thresholds[m] for m in range(3)] == pool.thresholds
    assert [s.members[m].h1 for m in range(4)] == [64, 40, 1, 64] and s.members[1].d_w1 == pols[1].struct.d_w1
    other = DensePolicy(*PC.glorot(9, 96, 7, 9), device="cpu")
    pool.set_member(1, other)
    assert (s.members[1].h1, s.members[1].h2, s.members[1].d_w1) == (7, 9, other.struct.d_w1) and pool.policies[1] is other
    for bad in (lambda: PartnerPool([]), lambda: PartnerPool(pols * 5), lambda: PartnerPool(pols, weights=[1, 2]),
                lambda: PartnerPool(pols + [DensePolicy(*PC.glorot(1, 76, 8, 8), device="cpu")]), lambda: pool.set_member(4, other),
                lambda: pool.set_member(0, "x")):
        with pytest.raises(ValueError):
            bad()


STAT_SEED = 2024  # (partner_cases' too)


@pytest.mark.parametrize("k", (2, 3, 5, 16))
def test_member_counts_are_uniform_and_independent_of_the_seat(k):
    n = 65536
    seat, member = PP.draws(STAT_SEED, 0, 0, n, 1.0, PP.uniform_thresholds(k))
    assert abs(PP.chi_square_z(np.bincount(member, minlength=k), np.full(k, n / k))) <= 6
    table = np.array([[((seat == p) & (member == m)).sum() for m in range(k)] for p in (0, 1)], np.float64)
    expected = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / n
    z = (((table - expected) ** 2 / expected).sum() - (k - 1)) / np.sqrt(2.0 * (k - 1))  # (2 - 1)(k - 1) degrees of freedom
    assert abs(z) <= 6, z


@pytest.mark.parametrize("drop", ("t_hi", "g_hi", "seed_hi", "tweak"))
def test_dropping_the_key_tweak_or_a_counter_half_changes_the_members(drop):
    at = _far()
    thr = PP.uniform_thresholds(3)
    a, b = PP.draws(bc_factor=1.0, thresholds=thr, **at)[1], PP.draws(bc_factor=1.0, thresholds=thr, drop=drop, **at)[1]
    changed = a != b
    assert changed.any(), drop
    if drop == "g_hi":  # only the envs above the wrap of g_lo can change
        assert not changed[: at["n"] // 2 + 37].any() and changed[at["n"] // 2 + 37:].any()


def test_redraw_keeps_seat_and_member_of_an_env_that_is_not_done():
    at = dict(NEAR)
    n = at.pop("n")
    thr = PP.uniform_thresholds(5)
    s1, m1 = PP.redraw(np.full(n, 255, np.uint8), np.full(n, 255, np.uint8), None, bc_factor=0.5, thresholds=thr, **at)
    done = (np.arange(n) % 3 == 0).astype(np.uint8) * 7
    at["step"] += 1
    s2, m2 = PP.redraw(s1, m1, done, bc_factor=0.5, thresholds=thr, **at)
    d2 = PP.draws(n=n, bc_factor=0.5, thresholds=thr, **at)
    assert np.array_equal(s2[done == 0], s1[done == 0]) and np.array_equal(m2[done == 0], m1[done == 0])
    assert np.array_equal(s2[done != 0], d2[0][done != 0]) and np.array_equal(m2[done != 0], d2[1][done != 0]) and (m2 != m1).any()
    assert ((m2 == PP.NO_MEMBER) == (s2 == PC.NO_SEAT)).all()


# ------------------------------------------------------------------------------------------ the case list
def test_the_case_list_covers_what_it_must():
    shape = {(c.n_envs, c.n_members, c.bc_factor) for c in PP.CASES}
    assert shape >= {(1, 3, 1.0), (33, 3, 1.0), (33, 16, 1.0), (65, 2, 0.5), (488, 3, 0.5), (488, 3, 1.0), (488, 16, 1.0), (1500, 2, 1.0)}
    assert any(c.n_members == 1 for c in PP.CASES) and any(c.weights for c in PP.CASES)
    assert sorted(PC.total_of(c.num_pots) for c in PP.CASES if c.num_pots != 2) == [76, 136]
    for c in PP.CASES + (PP.far_case(),):
        PP.check_claims(c)
        w = PP.weights_of(c)
        assert [(x[0].shape[1], x[2].shape[1]) for x in w] == list(PP.shapes_of(c)) and all(x[0].shape[0] == PC.total_of(c.num_pots) for x in w)
    assert set(PP.shapes_of(next(c for c in PP.CASES if c.n_members == 3))) == {(64, 64), (40, 24), (1, 1)}
    f, p = PP.far_case(), PC.far_case()
    assert (f.seed, f.env_offset, f.step, f.n_envs) == (p.seed, p.env_offset, p.step, p.n_envs)


def test_the_vector_env_refuses_a_pool_it_cannot_feed():
    """(both refusals are made before the env allocates anything: no device is needed)"""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool

    pool = PartnerPool([DensePolicy(*PC.glorot(1, 96, 64, 64), device="cpu")] * 2)
    with pytest.raises(ValueError, match="needs obs="):
        VecOvercookedMultiAgent("cramped_room", 4, obs="ppo", bc_policy=pool, device="cpu")
    with pytest.raises(ValueError, match="feature length"):
        VecOvercookedMultiAgent("cramped_room", 4, obs="features", num_pots=1, bc_policy=pool, device="cpu")
