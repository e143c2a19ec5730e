"""The forward passes of the dense policy kernels on the device, held BIT FOR BIT to the header's fmaf chain restated in numpy
(tests/mlp_chain.py; include/oc_amd.h: OcDensePolicy "Arithmetic", OcActorCritic "Forward arithmetic"): oc_partner_logits and
oc_partner_pool_logits on the dense synthetic cases of tests/partner_dense_cases.py — every feature length, odd hidden widths, preset
seat patterns that empty tiles, wavefronts and workgroups, pool buckets at the edges of tile, pass and chunk — and oc_policy_forward
on the cases of tests/policy_cases.py.  The a-priori bound of the neighbouring tests holds for any float32 order of summation;
these comparisons are equalities (after -0 -> +0, which the header allows), and tests/test_host_partner_dense.py shows on the CPU
that more than half of the logits of numpy's own float32 order fail them.

Everything goes through the C-ABI on arrays between guard bytes at the header's minimum alignments (gpu_support.Fenced): features 16
bytes, logits 8 bytes off a 16-byte boundary, seats, members and the done mask at odd addresses, the scratch of exactly the planned
size.  Feature rows that no seat names are NaN; the logits start as a fill without integers or repeats.  Every test prints how many
logits it compared, and the running total of its entry point."""
import ctypes
import re

import numpy as np
import pytest

import mlp_chain as MC
import partner_dense_cases as D
import policy_cases as PO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import Fenced, bits, gpu  # noqa: E402, F401
from test_gpu_policy import forward  # noqa: E402

COMPARED = {"oc_partner_logits": 0, "oc_partner_pool_logits": 0, "oc_policy_forward": 0, "oc_policy_forward against oc_partner_logits": 0}


def compared(who, what, n):
    COMPARED[who] += n
    print("%s: %d logits compared bit for bit (%s: %d so far)" % (what, n, who, COMPARED[who]))


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Policy:
    """An OcDensePolicy of six host arrays, one behind the other in ONE fenced device array at 4-byte alignment (a pool of sixteen
    members is sixteen allocations, not ninety-six)"""

    def __init__(self, weights, dev):
        from overcooked_ai_amd import _lib

        self.keep = Fenced(np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in weights]), 4, dev)
        starts = np.cumsum([0] + [w.size for w in weights[:-1]])
        self.struct = _lib.OcDensePolicy(*[self.keep.ptr + 4 * int(s) for s in starts], weights[0].shape[0], weights[0].shape[1], weights[2].shape[1])

    def intact(self, weights):
        return self.keep.intact() and np.array_equal(bits(self.keep.host()), bits(np.concatenate([w.reshape(-1) for w in weights])))


def same_bits(what, got, want, where):
    """float32 got == want after -0 -> +0, or words for the first difference; where: the env of every row"""
    g, w = MC.canon(got), MC.canon(want)
    if np.array_equal(g, w):
        return
    rows = np.flatnonzero((g != w).any(-1))
    r = rows[0]
    ulps = np.abs(g.astype(np.int64) - w.astype(np.int64))
    pytest.fail("%s: %d of %d logits (%d of %d rows) are not the chain's; the first, env %d (tile %d): %s, not %s; largest distance %d ulp"
                % (what, int((g != w).sum()), g.size, len(rows), len(g), where[r], where[r] // 32, got[r].tolist(), want[r].tolist(), int(ulps.max())))


def rest_is_the_fill(what, got, fill, envs, players):
    untouched = np.ones(got.shape[:2], bool)
    untouched[envs, players] = False
    same = bits(got)[untouched] == bits(fill)[untouched]
    assert same.all(), "%s: %d logits that no seat names were written" % (what, int((~same).sum()))
    assert not (bits(got)[envs, players] == bits(fill)[envs, players]).any(), "%s: a seated logit still holds the fill" % what


# ------------------------------------------------------------------------------------------ oc_partner_logits
def partner_call(c, a, dev, fill, policy=None):
    """One oc_partner_logits call of dense case c on fenced arrays -> (logits, seats) as numpy, everything else checked here"""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    n = c.n_envs
    drawn = c.pattern == "drawn"
    policy = policy or Policy(a.weights, dev)
    feats = Fenced(a.features, 16, dev)
    seat = Fenced(np.full(n, 255, np.uint8) if drawn else a.seat, 1, dev)
    done = None if drawn else Fenced(np.zeros(n, np.uint8), 1, dev)
    logits = Fenced(fill, 8, dev)
    assert feats.ptr % 16 == 0 and logits.ptr % 16 == 8
    s = _lib.OcPartnerSeats(seat.ptr, done.ptr if done else None, D.BC_FACTOR, c.seed, c.env_offset, c.step)
    b = _lib.OcBatch(n_envs=n)
    rc = L.oc_partner_logits(ctypes.byref(b), ctypes.byref(policy.struct), ctypes.byref(s), feats.ptr, D.num_pots_of(c.in_dim), logits.ptr, stream_of(dev))
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for what, f in (("features", feats), ("seats", seat), ("done mask", done), ("logits", logits)):
        assert f is None or f.intact(), "%s: guard bytes of the %s written" % (c.id, what)
    assert policy.intact(a.weights), "%s: a weight array or its guard bytes written" % c.id
    assert np.array_equal(bits(feats.host()), bits(a.features)), "%s: the features were written" % c.id
    assert done is None or not done.host().any()
    return logits.host(), seat.host()


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.id)
def test_partner_logits_are_the_chain_bit_for_bit(c, gpu):
    a, ref = D.arrays_of(c), D.reference_of(c)
    assert ref.smallest >= MC.MIN_NORMAL
    fill = D.logits_fill(c.n_envs)
    got, seat = partner_call(c, a, gpu, fill)
    assert np.array_equal(seat, a.seat), "%s: seats %s" % (c.id, "differ from the restated draw" if c.pattern == "drawn" else "changed under an all-zero done mask")
    rest_is_the_fill(c.id, got, fill, a.seated, a.p)
    same_bits(c.id, got[a.seated, a.p], ref.out, a.seated)
    again, seat2 = partner_call(c, a, gpu, fill)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(seat2, seat), "%s: a second call gives other bytes" % c.id
    compared("oc_partner_logits", c.id, ref.out.size)


# ------------------------------------------------------------------------------------------ oc_partner_pool_logits
def pool_call(c, a, dev, fill, scratch_byte, policies):
    """One oc_partner_pool_logits call of pool case c on fenced arrays (policies: the members', which the caller checks after its
    last call) -> (logits, seats, members) as numpy"""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    n, K = c.n_envs, c.n_members
    table = (_lib.OcDensePolicy * K)(*[p.struct for p in policies])
    feats = Fenced(a.features, 16, dev)
    nobody = np.full(n, 255, np.uint8)
    seat = Fenced(nobody if c.drawn else a.seat, 1, dev)
    member = Fenced(nobody if c.drawn else a.member, 1, dev)
    done = None if c.drawn else Fenced(np.zeros(n, np.uint8), 1, dev)
    logits = Fenced(fill, 8, dev)
    pool = _lib.OcPartnerPool(ctypes.cast(table, ctypes.POINTER(_lib.OcDensePolicy)), K, None, member.ptr)
    b = _lib.OcBatch(n_envs=n)
    text = ctypes.create_string_buffer(768)
    rc = L.oc_partner_pool_plan(ctypes.byref(b), ctypes.byref(pool), D.num_pots_of(c.in_dim), text, len(text))
    assert rc == 0, L.oc_last_error().decode()
    size = int(re.search(r"scratch (\d+) B", text.value.decode()).group(1))
    assert size == 1092 + 4 * K * ((n + 255) // 256) + 4 * n
    scratch = Fenced(np.full(size, scratch_byte, np.uint8), 16, dev)
    assert scratch.ptr % 16 == 0 and logits.ptr % 16 == 8
    s = _lib.OcPartnerSeats(seat.ptr, done.ptr if done else None, D.BC_FACTOR, c.seed, c.env_offset, c.step)
    rc = L.oc_partner_pool_logits(ctypes.byref(b), ctypes.byref(pool), ctypes.byref(s), feats.ptr, D.num_pots_of(c.in_dim), logits.ptr, scratch.ptr,
                                  stream_of(dev))
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for what, f in (("features", feats), ("seats", seat), ("members", member), ("done mask", done), ("logits", logits), ("scratch", scratch)):
        assert f is None or f.intact(), "%s: guard bytes of the %s written" % (c.id, what)
    assert np.array_equal(bits(feats.host()), bits(a.features)), "%s: the features were written" % c.id
    return logits.host(), seat.host(), member.host()


@pytest.mark.parametrize("c", D.POOL_CASES, ids=lambda c: c.id)
def test_pool_logits_are_each_member_s_chain_bit_for_bit(c, gpu):
    a = D.pool_arrays_of(c)
    ref, smallest = D.pool_reference_of(c)
    assert smallest >= MC.MIN_NORMAL
    fill = D.logits_fill(c.n_envs)
    policies = [Policy(w, gpu) for w in a.weights]
    got, seat, member = pool_call(c, a, gpu, fill, 0x00, policies)
    assert np.array_equal(seat, a.seat) and np.array_equal(member, a.member), \
        "%s: seats or members %s" % (c.id, "differ from the restated draw" if c.drawn else "changed under an all-zero done mask")
    rest_is_the_fill(c.id, got, fill, a.served, a.p)  # (envs without both a seat and a member below K keep the fill)
    same_bits(c.id, got[a.served, a.p], ref, a.served)
    for byte in (0x55, 0xFF):
        again, seat2, member2 = pool_call(c, a, gpu, fill, byte, policies)
        assert np.array_equal(bits(again), bits(got)) and np.array_equal(seat2, seat) and np.array_equal(member2, member), \
            "%s: other bytes over a scratch of 0x%02X" % (c.id, byte)
    assert all(p.intact(w) for p, w in zip(policies, a.weights)), "%s: a weight array or its guard bytes written" % c.id
    compared("oc_partner_pool_logits", c.id, ref.size)


# ------------------------------------------------------------------------------------------ oc_policy_forward
EXTRA_56 = PO.Case("56_63_33-65rows-indexed-dense-chain", 65, 56, 63, 33, "indexed", "dense", 9001)
SAMPLE = 4096  # calls above this many rows are compared on their first 128 rows, their last 128 and 256 seeded ones


def rows_compared(c):
    if c.M <= SAMPLE:
        return np.arange(c.M)
    some = np.random.default_rng([c.seed, 0x5A]).choice(np.arange(128, c.M - 128), 256, replace=False)
    return np.concatenate([np.arange(128), np.sort(some), np.arange(c.M - 128, c.M)])


@pytest.mark.parametrize("c", PO.CASES + (EXTRA_56,), ids=lambda c: c.id)
def test_policy_forward_is_the_chain_bit_for_bit(c, gpu):
    a = PO.arrays_of(c)
    got = forward(c, a, gpu)
    assert not bits(got[~a.valid]).any()  # out-of-range rows: +0.0f
    at = rows_compared(c)
    at = at[a.valid[at]]
    ref = MC.evaluate(a.features[a.rows[at]], a.weights, watch=True)  # (policy_cases.rows_of, for these rows alone)
    assert ref.smallest >= MC.MIN_NORMAL and ref.out.shape == (len(at), 7)
    same_bits(c.id, got[at], ref.out, at)
    compared("oc_policy_forward", "%s (%d of %d rows)" % (c.id, len(at), c.M), 6 * len(at))


@pytest.mark.parametrize("in_dim", D.LENGTHS)
def test_policy_forward_gives_the_partner_s_logits_bit_for_bit(in_dim, gpu):
    """The same dense rows and the same six arrays through both entry points (widths (63, 33)); the value head is drawn beside them."""
    c = next(c for c in D.CASES if (c.kind, c.in_dim, c.h1, c.h2, c.pattern) == ("real", in_dim, 63, 33, "seeded"))
    a = D.arrays_of(c)
    theirs, _ = partner_call(c, a, gpu, D.logits_fill(c.n_envs))
    rng = np.random.default_rng([c.seed, 0x7A1])
    weights = a.weights + (rng.uniform(-0.4, 0.4, (c.h2,)).astype(np.float32), rng.uniform(-0.5, 0.5, (1,)).astype(np.float32))
    M = 2 * c.n_envs
    pc = PO.Case(c.id + "-as-policy", M, c.in_dim, c.h1, c.h2, "contiguous", "dense", c.seed)
    pa = PO.Arrays(weights, a.features.reshape(M, c.in_dim), None, 0, np.arange(M), np.ones(M, bool), None, None, None, None)
    mine = forward(pc, pa, gpu)[:, :6].reshape(c.n_envs, 2, 6)
    assert np.array_equal(bits(mine[a.seated, a.p]), bits(theirs[a.seated, a.p])), c.id
    same_bits(c.id, mine[a.seated, a.p], D.reference_of(c).out, a.seated)
    compared("oc_policy_forward against oc_partner_logits", c.id, 6 * len(a.seated))
