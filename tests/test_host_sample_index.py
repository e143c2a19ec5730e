"""oc_sample_select / oc_sample_permute without a GPU: the exports against the header, the plan's words, every refusal (made before
any device call: this host has no device), and the restatement of tests/sample_index_cases.py itself — pi is a bijection at every
listed size and at every size from 1 to 300, it mixes (chi-square statistics of where it sends blocks of sources and of the steps
between neighbours), two epochs give two permutations, and every part of the counters reaches the keys."""
import ctypes
import os
import re

import numpy as np
import pytest

import sample_index_cases as SI
from case_support import P, ROOT

EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_prototypes_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = " ".join(_header().split())
    for name in ("oc_sample_select", "oc_sample_permute", "oc_sample_index_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert ("int oc_sample_select(int64_t n_samples, const uint8_t* d_seat, const uint8_t* d_actions, int32_t* d_ids, int64_t* d_count, "
            "uint32_t* d_block_offsets, void* stream);") in hdr
    assert ("int oc_sample_permute(const int32_t* d_ids, const int64_t* d_count, int64_t n_out, uint64_t seed, uint64_t epoch, "
            "int32_t* d_index, void* stream);") in hdr
    assert ("int oc_sample_index_plan(int64_t n_samples, int with_seat, int with_actions, int with_ids, int64_t n_out, int64_t n_learner, "
            "char* out, size_t out_size);") in hdr
    assert len(L.oc_sample_select.argtypes) == 7 and len(L.oc_sample_permute.argtypes) == 7 and len(L.oc_sample_index_plan.argtypes) == 8
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_arithmetic_the_restatement_uses():
    hdr = _header()
    for words in ("d_seat == NULL or d_seat[s >> 1] != (s & 1)", "d_actions == NULL or d_actions[s] <= 5", "d_ids[L .. S) holds -1",
                  "philox4x32_10(counter = {epoch_lo, epoch_hi, j, 0}, key = {seed_lo, seed_hi ^ 0x%08X})" % SI.SHUF, '"SHUF"',
                  "w = max(1, bit length of L - 1),  a = w >> 1,  c = w - a",
                  "v *= 0x%08X;  v ^= v >> 16;  v *= 0x%08X;  v ^= v >> 13" % (SI.MIX_1, SI.MIX_2), "top(v, q) = q ? v >> (32 - q) : 0",
                  "l = x >> c,  r = x & (2^c - 1)", "even j:  l ^= top(mix(r + k[j]), a),   odd j:  r ^= top(mix(l + k[j]), c)",
                  "x = (l << c) | r  }  until x < L", "L <= 1:  pi(0) = 0", "READ ON THE DEVICE", "not a cipher", "No atomics",
                  "P = 1024 consecutive samples"):
        assert words in hdr, words
    assert SI.SHUF == int.from_bytes(b"SHUF", "big") and SI.block_samples() == 1024


def test_the_plan_in_words():
    from overcooked_ai_amd import sample_index

    hdr = _header()
    Pb = SI.block_samples()
    S = 52428800
    rc, text = SI.plan(S, 1, 1, 1, S // 2, S // 2)
    blocks = S // Pb
    assert rc == 0 and text == (
        "select: k_sample_count<SEAT=true, ACT=true> grid=%d, 256 lanes + k_sample_scan grid=1, 256 lanes, %d pass(es) of 256 blocks, 8 passes "
        "in flight + k_sample_write<SEAT=true, ACT=true> grid=%d, 256 lanes; P = %d samples per block, scratch %d B; permute: "
        "k_sample_permute<IDS=true> grid=1024, 256 lanes (one per output, 100 output(s) per lane at most); L = 26214400: w = 25, a = 12, c = 13"
        % (blocks, blocks // 256, blocks, Pb, 4 * blocks)), text
    assert text in hdr and sample_index.plan(S, seat=True, actions=True, n_out=S // 2, n_learner=S // 2) == text
    rc, text = SI.plan()
    assert rc == 0 and text in hdr and text.startswith("select: k_sample_scan grid=1, 256 lanes, 0 pass(es) (no samples: *d_count = 0)")
    assert "scratch 4 B" in text and text.endswith("permute: nothing to launch (no output); L = 0: w = 1, a = 0, c = 1")
    for S, seat, act, ids, n_out, L in ((2, 0, 0, 0, 2, 2), (Pb + 2, 1, 0, 1, 5, 5), (300002, 0, 1, 1, 300002, 150000), (2 ** 31 - 1, 0, 1, 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        rc, text = SI.plan(S, seat, act, ids, n_out, L)
        blocks = (S + Pb - 1) // Pb
        tf = lambda v: "true" if v else "false"  # noqa: E731
        assert rc == 0 and text.startswith("select: k_sample_count<SEAT=%s, ACT=%s> grid=%d, 256 lanes + k_sample_scan grid=1, 256 lanes, %d pass(es)"
                                           % (tf(seat), tf(act), blocks, (blocks + 255) // 256)), text
        grid = min((n_out + 255) // 256, 1024)
        w, a, c = SI.widths(L)
        assert ("scratch %d B; permute: k_sample_permute<IDS=%s> grid=%d, 256 lanes (one per output, %d output(s) per lane at most); L = %d: "
                "w = %d, a = %d, c = %d" % (4 * blocks, tf(ids), grid, (n_out + grid * 256 - 1) // (grid * 256), L, w, a, c)) in text, text
        assert sample_index.scratch_bytes(S, seat) == 4 * blocks
    # the largest case of the list has more blocks than one pass of the scan, and more outputs than one trip of the permutation's grid
    assert "2 pass(es) of 256 blocks" in SI.plan(300002, 0, 1, 1, 300002, 150000)[1] and "2 output(s) per lane" in SI.plan(300002, 0, 1, 1, 300002, 150000)[1]
    assert max(SI.sizes()) == 300002 and max(SI.sizes()) > 256 * Pb and max(SI.sizes()) > 1024 * 256
    for args, why in (((-1,), "oc_sample_select: n_samples must be in 0 .. 2^31 - 1"), ((2 ** 31,), "oc_sample_select: n_samples must be in 0 .. 2^31 - 1"),
                      ((7, 1), "oc_sample_select: d_seat needs an even n_samples"), ((8, 1, 1, 1, -1), "oc_sample_permute: n_out must be in 0 .. 2^31 - 1"),
                      ((8, 1, 1, 1, 2 ** 31), "oc_sample_permute: n_out must be in 0 .. 2^31 - 1"),
                      ((8, 1, 1, 1, 8, -1), "oc_sample_index_plan: n_learner must be in 0 .. 2^31 - 1"),
                      ((8, 1, 1, 1, 8, 2 ** 31), "oc_sample_index_plan: n_learner must be in 0 .. 2^31 - 1")):
        rc, msg = SI.plan(*args)
        assert rc == EINVAL and msg == why, (args, msg)
    assert SI.plan(7, 0)[0] == 0  # (an odd S without seats is in order)
    from overcooked_ai_amd import _lib

    L = _lib.load()
    text = ctypes.create_string_buffer(64)
    assert L.oc_sample_index_plan(8, 0, 0, 0, 8, 8, None, 0) == EINVAL and L.oc_last_error() == b"oc_sample_index_plan: no output buffer"
    assert L.oc_sample_index_plan(8, 0, 0, 0, 8, 8, text, 0) == EINVAL and L.oc_last_error() == b"oc_sample_index_plan: no output buffer"
    with pytest.raises(_lib.OcAmdError, match="d_seat needs an even n_samples"):
        sample_index.plan(7, seat=True)


def test_the_entry_points_refuse_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()

    def select(S=1000, seat=P, actions=P, ids=P, count=P, scratch=P):
        rc = L.oc_sample_select(S, seat, actions, ids, count, scratch, None)
        return rc, L.oc_last_error().decode()

    def permute(ids=P, count=P, n_out=1000, index=P):
        rc = L.oc_sample_permute(ids, count, n_out, 1, 2, index, None)
        return rc, L.oc_last_error().decode()

    who = "oc_sample_select: "
    refusals = [(dict(**{f: None}), "NULL d_ids, d_count or d_block_offsets") for f in ("ids", "count", "scratch")]
    refusals += [(dict(**{f: P + off}), "d_ids and d_block_offsets must be 4-byte aligned") for f in ("ids", "scratch") for off in (1, 2, 3)]
    refusals += [(dict(count=P + off), "d_count must be 8-byte aligned") for off in (1, 4)]
    refusals += [(dict(S=-1), "n_samples must be in 0 .. 2^31 - 1"), (dict(S=2 ** 31), "n_samples must be in 0 .. 2^31 - 1"),
                 (dict(S=2 ** 40), "n_samples must be in 0 .. 2^31 - 1"), (dict(S=999), "d_seat needs an even n_samples")]
    for kw, why in refusals:
        rc, msg = select(**kw)
        assert rc == EINVAL and msg == who + why, (kw, rc, msg)
    who = "oc_sample_permute: "
    refusals = [(dict(**{f: None}), "NULL d_count or d_index") for f in ("count", "index")]
    refusals += [(dict(**{f: P + off}), "d_ids and d_index must be 4-byte aligned") for f in ("ids", "index") for off in (1, 2, 3)]
    refusals += [(dict(count=P + 4), "d_count must be 8-byte aligned")]
    refusals += [(dict(n_out=n), "n_out must be in 0 .. 2^31 - 1") for n in (-1, 2 ** 31, 2 ** 40)]
    for kw, why in refusals:
        rc, msg = permute(**kw)
        assert rc == EINVAL and msg == who + why, (kw, rc, msg)
    # accepted, and nothing to launch: no output, at the minimum alignments, with and without ids
    for kw in (dict(), dict(ids=None), dict(ids=P + 4, count=P + 8, index=P + 4)):
        assert permute(n_out=0, **kw)[0] == 0, kw


def test_the_python_surface_refuses_what_is_no_device_tensor():
    import torch

    from overcooked_ai_amd import sample_index

    seat, actions = torch.zeros(4, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)
    for bad in (lambda: sample_index.select(seat, actions, 8),  # (everything in order, but on the host: there is no CPU fallback)
                lambda: sample_index.select(seat, actions, 7), lambda: sample_index.select(seat[:3], actions, 8),
                lambda: sample_index.select(seat, actions.to(torch.int8), 8), lambda: sample_index.select(None, actions[::2], 4),
                lambda: sample_index.select(None, actions, -1), lambda: sample_index.select(None, None, 2 ** 31),
                lambda: sample_index.permute(None, -1, 0, 0), lambda: sample_index.permute(None, 2 ** 31, 0, 0),
                lambda: sample_index.permute(None, 4, 0, 0, device="cpu"), lambda: sample_index.permute(object(), 4, 0, 0),
                lambda: sample_index.permute(sample_index.LearnerSamples(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)), 5, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    for name in ("learner_samples", "learner_permutation", "learner_minibatches", "permutation", "minibatches"):
        assert callable(getattr(TrajectoryBuffer, name))


# ------------------------------------------------------------------------------------------ the restatement
def _is_bijection(p, L):
    return p.shape == (L,) and bool((np.sort(p) == np.arange(L)).all())


def test_pi_is_a_bijection_at_every_size_from_1_to_300():
    walk = {}
    for L in range(1, 301):
        seed, epoch = SI.KEYS[L % len(SI.KEYS)]
        assert _is_bijection(SI.pi(L, seed, epoch, walk=walk), L), L
        assert L <= 1 or walk["evaluations"] < 2 * L, (L, walk)
    assert SI.pi(0, 1, 2).shape == (0,) and SI.pi(1, 1, 2).tolist() == [0]
    assert [SI.widths(L) for L in (2, 3, 4, 5, 1024, 1025, 2 ** 31 - 1)] == [(1, 0, 1), (2, 1, 1), (2, 1, 1), (3, 1, 2), (10, 5, 5), (11, 5, 6), (31, 15, 16)]


@pytest.mark.parametrize("L", SI.BIJECTION_SIZES)
def test_pi_is_a_bijection_at_every_listed_size(L):
    worst = 0.0
    for seed, epoch in SI.KEYS[:2]:
        walk = {}
        assert _is_bijection(SI.pi(L, seed, epoch, walk=walk), L)
        if L > 1:
            worst = max(worst, walk["evaluations"] / L)
            assert walk["evaluations"] < 2 * L and walk["longest"] < 64, walk  # (fewer than 2 per element; no walk near the cycle's length)
    print("L = %d: %.3f evaluations of the rounds per element at most" % (L, worst))


def _z(observed, expected):
    """(chi^2 - dof) / sqrt(2 dof) of a table against its expectation, dof from the table's shape"""
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    dof = (observed.shape[0] - 1) * (observed.shape[1] - 1) if observed.ndim == 2 else observed.shape[0] - 1
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def _contingency_z(p, L, B):
    """Source block i * B // L against destination block pi(i) * B // L: the counts of a uniform permutation are the products of
    the margins over L."""
    src, dst = np.arange(L) * B // L, p * B // L
    table = np.zeros((B, B))
    np.add.at(table, (src, dst), 1)
    return _z(table, np.outer(table.sum(1), table.sum(0)) / L)


def _step_z(p, L):
    """The 16-bin histogram of (pi(i + 1) - pi(i)) mod L: of a uniform permutation every step 1 .. L - 1 is equally likely."""
    d = (p[1:] - p[:-1]) % L
    observed = np.bincount(d * 16 // L, minlength=16).astype(np.float64)
    expected = np.bincount(np.arange(1, L) * 16 // L, minlength=16).astype(np.float64)  # (L - 1 steps in all, as many as neighbours)
    return _z(observed, expected)


@pytest.mark.parametrize("L", [L for L in SI.BIJECTION_SIZES if L >= 4097])
def test_pi_mixes_blocks_and_neighbours(L):
    """z = (chi^2 - dof) / sqrt(2 dof) of three tables, each below 6: chi^2 of a uniform permutation has mean dof and variance
    2 dof, so 6 is a cap on sampling deviation, not a property of this function."""
    worst = 0.0
    for seed, epoch in SI.KEYS:
        p = SI.pi(L, seed, epoch)
        zs = (_contingency_z(p, L, 8), _contingency_z(p, L, 32), _step_z(p, L))
        print("L = %d seed %#x epoch %#x: z = %.2f (8 x 8), %.2f (32 x 32), %.2f (steps)" % ((L, seed, epoch) + zs))
        worst = max(worst, *zs)
        assert all(z < 6 for z in zs), (L, seed, epoch, zs)
    print("L = %d: largest z %.2f" % (L, worst))


def test_two_epochs_give_two_permutations_and_every_part_of_the_counters_reaches_the_keys():
    seed, epoch = SI.KEYS[2]  # (both halves of both set)
    L = 4097
    base = SI.pi(L, seed, epoch)
    for other in (epoch + 1, epoch ^ (1 << 32), epoch ^ (1 << 63)):
        assert (SI.pi(L, seed, other) != base).mean() > 0.9
    for other in (seed + 1, seed ^ (1 << 32), seed ^ (1 << 63)):
        assert (SI.pi(L, other, epoch) != base).mean() > 0.9
    assert (SI.pi(L, seed, epoch) == base).all()
    keys = SI.round_keys(seed, epoch)
    assert len(keys) == 8 and len(set(keys)) == 8 and all(0 <= k < 2 ** 32 for k in keys)
    for drop in ("seed_hi", "epoch_hi", "tweak"):  # a truncation a kernel could commit changes the keys, and the permutation
        assert SI.round_keys(seed, epoch, drop) != keys, drop
        assert (SI.pi(L, seed, epoch, drop=drop) != base).mean() > 0.9, drop
    # the wrap of the epoch's low word: 2^32 - 1 and 2^32 are two counters, and 2^32 is not 0
    assert SI.round_keys(seed, 2 ** 32) != SI.round_keys(seed, 0) and SI.round_keys(seed, 2 ** 32 - 1) != SI.round_keys(seed, 2 ** 32)
    assert SI.round_keys(seed, 2 ** 64 + 5) == SI.round_keys(seed, 5)  # (modulo 2^64)


# ------------------------------------------------------------------------------------------ the case list
def test_the_case_list_covers_what_it_must():
    Pb = SI.block_samples()
    assert SI.sizes() == (0, 2, 128, Pb - 2, Pb, Pb + 2, 2 * Pb + 2, 66562, 300002)
    cases = SI.CASES
    assert len({c.id for c in cases}) == len(cases) and len(cases) < 120
    assert {(c.n_samples, c.seat) for c in cases} >= {(S, s) for S in SI.sizes() for s in SI.SEATS}
    assert {(c.seat, c.actions) for c in cases if c.n_samples == 2 * Pb + 2} >= {(s, a) for s in SI.SEATS for a in SI.ACTIONS}
    assert {(c.n_samples, c.n_out) for c in cases} >= {(S, k) for S in SI.sizes() for k in SI.N_OUT}
    assert {(c.seed, c.epoch) for c in cases} == set(SI.KEYS) and {2 ** 32 - 1, 2 ** 32} <= {e for _, e in SI.KEYS}
    assert all(s >> 32 and s & SI.M32 for s, _ in SI.KEYS) and sum(1 for _, e in SI.KEYS if e >> 32 and e & SI.M32) >= 2
    seen_tail = seen_partial = False
    for c in cases:
        seat, actions = SI.arrays_of(c)
        ids, L, n_out, index, plain = SI.reference_of(c)
        keep = SI.selected(c.n_samples, seat, actions)
        assert L == int(keep.sum()) and (ids[:L] == np.nonzero(keep)[0]).all() and (ids[L:] == -1).all() and (np.diff(ids[:L]) > 0).all()
        m = min(L, n_out)
        assert (index[m:] == -1).all() and (plain[m:] == -1).all() and (index[:m] == ids[plain[:m]]).all()
        assert not (ids == SI.FILL).any() and not (index == SI.FILL).any()
        if n_out >= L:
            assert sorted(index[:L].tolist()) == ids[:L].tolist(), c.id
        seen_tail |= n_out > L > 0
        seen_partial |= 0 < n_out < L
        if c.actions == "all255":
            assert L == 0
        if c.seat in ("all0", "all1", "alternating") and c.actions in ("none", "valid"):
            assert L == c.n_samples // 2
        if c.seat in ("none", "all255") and c.actions in ("none", "valid"):
            assert L == c.n_samples
    assert seen_tail and seen_partial
    # the long cases run k_sample_scan beyond its first run of passes in flight: B + 1 and 2 B + 1 passes, neither a multiple of B
    per_pass, B = SI.scan_shape()
    passes = sorted({-(-(-(-c.n_samples // Pb)) // per_pass) for c in SI.LONG_CASES})
    assert (per_pass, B) == (256, 8) and passes == [B + 1, 2 * B + 1] and all(c.n_samples > 1024 * 256 * 2 for c in SI.LONG_CASES)
    assert {c.seat for c in SI.LONG_CASES} >= {"none", "random"} and {"S", "L"} <= {c.n_out for c in SI.LONG_CASES}
    for c in SI.LONG_CASES:
        assert ("%d pass(es) of %d blocks, %d passes in flight" % (-(-(-(-c.n_samples // Pb)) // per_pass), per_pass, B)) in SI.plan(c.n_samples, 0, 1, 1, 0, 0)[1]
        ids, L, n_out, index, plain = SI.reference_of(c)
        assert 0 < L <= c.n_samples and (ids[:L] == np.nonzero(SI.selected(c.n_samples, *SI.arrays_of(c)))[0]).all() and (ids[L:] == -1).all()
        m = min(L, n_out)
        assert (index[:m] == ids[plain[:m]]).all() and (index[m:] == -1).all() and len(np.unique(plain[:m])) == m
    rng = np.random.default_rng(0)
    a = SI.action_pattern("scattered", 4000, rng)
    assert {6, 255} <= set(a.tolist()) and 0.8 < (a <= 5).mean() < 0.95
    assert set(SI.seat_pattern("random", 4000, rng).tolist()) == {0, 1, 255} and SI.seat_pattern("alternating", 8, rng).tolist() == [0, 1, 0, 1]
