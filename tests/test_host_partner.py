"""oc_partner_logits without a GPU: the exports and the two structs against the header, the plan's words, every refusal (made before
any device call: this host has no device), the seating stream restated twice — near counters and far ones, every part of the far
counters reaching a seat, the two ends of bc_factor, the binomial statistics —, the error bound of tests/partner_cases.py shown to
hold for another float32 evaluation and to catch a wrong network, and the Python surface's own refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import far_cases as F
import partner_cases as PC
from case_support import P, ROOT, synthetic_batch

EINVAL = -1
WHO = "oc_partner_logits: "


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_structs_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_partner_logits", "oc_partner_logits_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    body = re.search(r"typedef struct OcDensePolicy \{(.*?)\} OcDensePolicy;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(d_\w+|in_dim|h1|h2)\b", body) == [f[0] for f in _lib.OcDensePolicy._fields_]
    D = _lib.OcDensePolicy  # six pointers, three ints, padded to the pointers' alignment
    assert ctypes.sizeof(D) == 64 and [getattr(D, f).offset for f, _ in D._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56]
    body = re.search(r"typedef struct OcPartnerSeats \{(.*?)\} OcPartnerSeats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(d_seat|d_done|bc_factor|seed|env_offset|step)\b", body) == [f[0] for f in _lib.OcPartnerSeats._fields_]
    S = _lib.OcPartnerSeats  # (the float is followed by four bytes of padding)
    assert ctypes.sizeof(S) == 48 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 40]
    assert "uint8_t* d_seat" in hdr and "const uint8_t* d_done" in hdr and "float bc_factor" in hdr and "uint64_t seed; int64_t env_offset; int64_t step;" in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_stream_and_the_arithmetic_the_references_restate():
    hdr = _header()
    for words in ("{t_lo, g_lo, g_hi, t_hi}", "seed_hi ^ 0x53454154", "(float)(r[0] >> 8) * 2^-24 < bc_factor", "r[1] & 1", "d_seat[e] = 255",
                  "d_done == NULL or d_done[e] != 0", "in ascending index", "starts from\n * the bias", "max(., 0)", "v_mfma_f32_32x32x2_f32"):
        assert words in hdr, words
    assert PC.SEAT_TWEAK == 0x53454154 == int.from_bytes(b"SEAT", "big")


def _policy(in_dim=96, h1=64, h2=64, ptrs=(P,) * 6):
    from overcooked_ai_amd import _lib

    return _lib.OcDensePolicy(*ptrs, in_dim, h1, h2)


def _plan(b, pol, num_pots=2):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    rc = L.oc_partner_logits_plan(ctypes.byref(b) if b is not None else None, ctypes.byref(pol) if pol is not None else None, num_pots,
                                  out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def test_the_plan_in_words():
    rc, text = _plan(synthetic_batch(5, 4, 65536), _policy())
    assert rc == 0 and text == ("k_partner_logits grid=256, 256 lanes (4 wavefronts x 64 envs), 32 x 32 x 2 f32 MFMA, K 96 -> 64 -> 64 -> 32 "
                                "(h1 = 64, h2 = 64, 6 logits, zero-padded), 100224 B LDS"), text
    assert text in _header()
    # the LDS bytes, restated: three weight matrices in operand order, the padded biases, 256 seat bytes, four 32-row feature images
    for num_pots, h1, h2, n in ((1, 40, 24, 1), (4, 40, 24, 488), (0, 1, 1, 257)):
        d = PC.total_of(num_pots)
        lds = 4 * (d * 64 + 64 * 64 + 64 * 32 + 160 + 64 + 4 * 32 * (d + 2))
        rc, text = _plan(synthetic_batch(5, 4, n), _policy(d, h1, h2), num_pots)
        assert rc == 0 and text.startswith("k_partner_logits grid=%d, " % ((n + 255) // 256)) and text.endswith(", %d B LDS" % lds), text
        assert "K %d -> 64 -> 64 -> 32 (h1 = %d, h2 = %d," % (d, h1, h2) in text and lds <= 160 * 1024
    assert _plan(synthetic_batch(5, 4, 0), _policy()) == (0, "nothing to launch (no envs)")
    for b, pol, num_pots, why in ((None, _policy(), 2, "batch is NULL"), (synthetic_batch(5, 4, 10), None, 2, "policy is NULL"),
                                  (synthetic_batch(5, 4, 10), _policy(), 5, "num_pots must be in 0..4"),
                                  (synthetic_batch(5, 4, 10), _policy(), 1, "policy.in_dim must equal the feature length"),
                                  (synthetic_batch(5, 4, 10), _policy(h1=65), 2, "policy.h1 and policy.h2 must be in 1..64"),
                                  (synthetic_batch(5, 4, -1), _policy(), 2, "batch.n_envs < 0")):
        rc, msg = _plan(b, pol, num_pots)
        assert rc == EINVAL and msg.startswith(WHO + why), (why, msg)


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()

    def call(b=(), pol=(), seats=(), features=P, num_pots=2, logits=P, seat=P, done=P, factor=0.5):
        b = synthetic_batch(5, 4, 1000) if b == () else b
        pol = _policy() if pol == () else pol
        seats = _lib.OcPartnerSeats(seat, done, factor, 7, 0, 0) if seats == () else seats
        rc = L.oc_partner_logits(ctypes.byref(b) if b is not None else None, ctypes.byref(pol) if pol is not None else None,
                                 ctypes.byref(seats) if seats is not None else None, features, num_pots, logits, None)
        return rc, L.oc_last_error().decode()

    null = lambda i: tuple(None if k == i else P for k in range(6))  # noqa: E731
    off = lambda i: tuple(P + 2 if k == i else P for k in range(6))  # noqa: E731
    refusals = [(dict(b=None), "batch is NULL"), (dict(pol=None), "policy is NULL"), (dict(seats=None), "seats is NULL"),
                (dict(seat=None), "seats.d_seat is NULL"), (dict(features=None), "NULL d_features or d_logits"),
                (dict(logits=None), "NULL d_features or d_logits"),
                (dict(features=P + 8), "d_features must be 16-byte aligned"), (dict(logits=P + 4), "d_logits must be 8-byte aligned"),
                (dict(pol=_policy(in_dim=76)), "policy.in_dim must equal the feature length"),
                (dict(num_pots=1), "policy.in_dim must equal the feature length"),
                (dict(pol=_policy(h1=0)), "policy.h1 and policy.h2 must be in 1..64"), (dict(pol=_policy(h1=65)), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(pol=_policy(h2=0)), "policy.h1 and policy.h2 must be in 1..64"), (dict(pol=_policy(h2=65)), "policy.h1 and policy.h2 must be in 1..64"),
                (dict(factor=-0.001), "seats.bc_factor must be in [0, 1]"), (dict(factor=1.001), "seats.bc_factor must be in [0, 1]"),
                (dict(factor=float("nan")), "seats.bc_factor must be in [0, 1]"),
                (dict(num_pots=-1), "num_pots must be in 0..4"), (dict(num_pots=5), "num_pots must be in 0..4"),
                (dict(b=synthetic_batch(5, 4, -1)), "batch.n_envs < 0")]
    refusals += [(dict(pol=_policy(ptrs=null(i))), "NULL weight or bias array") for i in range(6)]
    refusals += [(dict(pol=_policy(ptrs=off(i))), "weight and bias arrays must be 4-byte aligned") for i in range(6)]
    for kw, why in refusals:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith(WHO + why), (kw, rc, msg)
    # accepted: a logits array that is 8-byte but not 16-byte aligned, no done mask, both ends of bc_factor — on no envs: nothing to launch
    for kw in (dict(logits=P + 8), dict(done=None), dict(factor=0.0), dict(factor=1.0), dict(seat=P + 1, done=P + 3)):
        assert call(b=synthetic_batch(5, 4, 0), **kw)[0] == 0, kw


# ------------------------------------------------------------------------------------------ the seating stream
NEAR = dict(seed=61, env_offset=3 * 488 + 37, step=5, n=488)


def _far():
    c = PC.far_case()
    return dict(seed=c.seed, env_offset=c.env_offset, step=c.step, n=c.n_envs)


@pytest.mark.parametrize("at", (NEAR, _far()), ids=("near", "far"))
def test_the_two_restatements_of_the_seating_stream_agree(at):
    for factor in (0.0, 0.25, 0.5, 0.9, 1.0):
        a, b = PC.seats(bc_factor=factor, **at), PC.seats_by_the_header(bc_factor=factor, **at)
        assert a.dtype == np.uint8 and np.array_equal(a, b), factor
        assert set(np.unique(a)) <= {0, 1, PC.NO_SEAT}
    assert {0, 1, PC.NO_SEAT} == set(np.unique(PC.seats(bc_factor=0.5, **at)))


def test_the_far_case_is_far():
    c = PC.far_case()
    assert c.seed == F.FAR_SEED and c.seed >> 32 and c.seed & 0xFFFFFFFF
    assert c.env_offset == F.far_env_offset(c.n_envs) and c.env_offset < 2**32 < c.env_offset + c.n_envs
    assert c.step > 2**32 and c.step & 0xFFFFFFFF
    assert (c.env_offset + c.n_envs // 2 + 36) >> 32 == 0 and (c.env_offset + c.n_envs // 2 + 37) >> 32 == 1


@pytest.mark.parametrize("drop", ("t_hi", "g_hi", "carry", "seed_hi", "tweak"))
def test_at_the_far_counters_every_part_of_them_reaches_a_seat(drop):
    at = _far()
    a, b = PC.seats(bc_factor=0.5, **at), PC.seats(bc_factor=0.5, drop=drop, **at)
    changed = a != b
    assert changed.any(), drop
    if drop in ("g_hi", "carry"):  # only the envs above the wrap of g_lo can change
        assert not changed[: at["n"] // 2 + 37].any() and changed[at["n"] // 2 + 37:].any()


def test_both_ends_of_bc_factor():
    for at in (NEAR, _far()):
        assert (PC.seats(bc_factor=0.0, **at) == PC.NO_SEAT).all()  # u >= 0 is never below 0
        assert (PC.seats(bc_factor=1.0, **at) != PC.NO_SEAT).all()  # u < 1 always: (r >> 8) * 2^-24 <= 1 - 2^-24
    r0 = np.array([0xFFFFFFFF], np.uint32)
    assert float((r0 >> np.uint32(8)).astype(np.float32)[0] * np.float32(2.0 ** -24)) == 1 - 2.0 ** -24


STAT_SEED = 2024  # chosen here: the restatement itself satisfies both bands below, which this test shows


def test_the_partner_count_and_the_slot_share_are_binomial():
    n, f = 4096, 0.25
    s = PC.seats(STAT_SEED, 0, 0, n, f)
    partners = int((s != PC.NO_SEAT).sum())
    assert abs(partners - 1024) <= 139, partners  # 5 sigma: sqrt(4096 * 0.25 * 0.75) = 27.7
    slot1 = int((s == 1).sum())
    assert abs(slot1 - partners / 2) <= 5 * np.sqrt(partners) / 2, (slot1, partners)


def test_reseat_keeps_the_seat_of_an_env_that_is_not_done():
    at = dict(NEAR)
    n = at.pop("n")
    first = PC.reseat(np.full(n, PC.NO_SEAT, np.uint8), None, bc_factor=0.5, **at)
    assert np.array_equal(first, PC.seats(n=n, bc_factor=0.5, **at))
    done = (np.arange(n) % 3 == 0).astype(np.uint8) * 7  # (any non-zero byte)
    at["step"] += 1
    second = PC.reseat(first, done, bc_factor=0.5, **at)
    assert np.array_equal(second[done == 0], first[done == 0]) and np.array_equal(second[done != 0], PC.seats(n=n, bc_factor=0.5, **at)[done != 0])
    assert (second != first).any()


# ------------------------------------------------------------------------------------------ the bound
SHAPES = sorted({(c.num_pots, c.h1, c.h2, c.seed) for c in PC.CASES if c.n_envs == PC.SIZES[-1]})


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.n_envs == PC.SIZES[-1]], ids=lambda c: c.id)
def test_the_bound_holds_for_another_f32_evaluation_and_catches_a_wrong_network(c):
    w = PC.weights_of(c)
    x = PC.synthetic_features(c)
    assert x.shape[1] == w[0].shape[0] == PC.total_of(c.num_pots) and w[0].shape[1] == c.h1 and w[2].shape == (c.h1, c.h2) and w[4].shape == (c.h2, 6)
    ref, _ = PC.mlp_f64(x, w)
    bound = PC.mlp_bound(x, w)
    assert bound.shape == ref.shape == (len(x), 6) and (bound > 0).all()
    err = np.abs(PC.mlp_f32(x, w).astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / bound).max())
    # two rows of W1 swapped (inputs 0 and 1, which differ in the rows used): outside the bound on some logit
    swapped = (w[0].copy(),) + w[1:]
    k = next(k for k in range(1, x.shape[1]) if (x[:, 0] != x[:, k]).any())
    swapped[0][[0, k]] = swapped[0][[k, 0]]
    assert (np.abs(PC.mlp_f32(x, swapped).astype(np.float64) - ref) > bound).any()
    # the last input dropped (a K loop one step short)
    short = (w[0][:-1],) + w[1:]
    assert (x[:, -1] != 0).any()
    assert (np.abs(PC.mlp_f32(x[:, :-1], short).astype(np.float64) - ref) > bound).any()


def test_the_case_list_covers_what_it_must():
    assert {c.n_envs for c in PC.CASES} == {1, 33, 65, 488}
    ref = [c for c in PC.CASES if (c.num_pots, c.h1, c.h2) == (2, 64, 64)]
    assert {(c.n_envs, c.bc_factor) for c in ref} == {(n, f) for n in (1, 33, 65, 488) for f in (0.0, 0.5, 1.0)}
    assert {(c.num_pots, PC.total_of(c.num_pots), c.h1, c.h2) for c in PC.CASES} == {(2, 96, 64, 64), (1, 76, 40, 24), (4, 136, 40, 24)}
    assert all(c.env_offset > 0 and c.step > 0 for c in PC.CASES)


# ------------------------------------------------------------------------------------------ the Python surface
def test_dense_policy_validates_shapes_and_dtypes():
    from overcooked_ai_amd.partner import DensePolicy

    w = PC.glorot(1, 96, 64, 64)
    p = DensePolicy(*w, device="cpu")
    assert (p.in_dim, p.h1, p.h2) == (96, 64, 64) and (p.struct.in_dim, p.struct.h1, p.struct.h2) == (96, 64, 64)
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(p.weights(), w))
    assert [p.struct.d_w1, p.struct.d_b1, p.struct.d_w2, p.struct.d_b2, p.struct.d_w3, p.struct.d_b3] == [t.data_ptr() for t in p.tensors()]
    import torch

    q = DensePolicy(*[torch.from_numpy(a.astype(np.float64)) for a in PC.glorot(2, 76, 40, 24)], device="cpu")  # torch, float64 in
    assert (q.in_dim, q.h1, q.h2) == (76, 40, 24) and all(t.dtype == torch.float32 and t.is_contiguous() for t in q.tensors())
    bad = [(0, w[0][:, :63]), (1, w[1][:63]), (2, w[2].T[:, :10]), (3, w[3][:-1]), (4, w[4][:, :5]), (5, w[5][:5]), (0, w[0].astype(np.int32)),
           (0, w[0].reshape(-1)), (1, w[1][:, None]), (4, np.full_like(w[4], np.nan))]
    for i, a in bad:
        args = list(w)
        args[i] = a
        with pytest.raises(ValueError):
            DensePolicy(*args, device="cpu")
    wide = PC.glorot(3, 96, 65, 64)
    with pytest.raises(ValueError):
        DensePolicy(*wide, device="cpu")


def test_the_vector_env_refuses_a_policy_it_cannot_feed():
    """(both refusals are made before the env allocates anything: no device is needed)"""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy

    p = DensePolicy(*PC.glorot(1, 96, 64, 64), device="cpu")
    with pytest.raises(ValueError, match="needs obs="):
        VecOvercookedMultiAgent("cramped_room", 4, obs="ppo", bc_policy=p, device="cpu")
    with pytest.raises(ValueError, match="feature length"):
        VecOvercookedMultiAgent("cramped_room", 4, obs="features", num_pots=1, bc_policy=p, device="cpu")
    with pytest.raises(AssertionError):  # the schedule goes through _checked_schedule
        VecOvercookedMultiAgent("cramped_room", 4, obs="features", bc_policy=p, bc_schedule=[(5, 0.5), (10, 1.0)], device="cpu")


def test_the_bc_schedule_of_the_vector_env_is_the_per_env_classes():
    """anneal_bc_factor / set_bc_factor on an object that has only what they read"""
    from overcooked_ai_amd.multi_agent import OvercookedMultiAgent, VecOvercookedMultiAgent, _checked_schedule

    sched = [(0, 1.0), (100, 0.2), (200, 0.0)]
    vec, one = object.__new__(VecOvercookedMultiAgent), object.__new__(OvercookedMultiAgent)
    vec.bc_schedule = one.bc_schedule = _checked_schedule(sched)
    for t in (0, 1, 50, 100, 150, 199, 200, 10**6):
        vec.anneal_bc_factor(t)
        one.anneal_bc_factor(t)
        assert vec.bc_factor == one.bc_factor, t
    vec.set_bc_factor(0.75)
    assert vec.bc_factor == 0.75
