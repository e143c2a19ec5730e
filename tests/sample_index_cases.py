"""The learner's sample index (oc_sample_select, oc_sample_permute): the numpy restatement of what include/oc_amd.h states — the
selection rule and the bijection pi, operation by operation, with Philox from tests/sample_cases.py — and the case list of
tests/test_gpu_sample_index.py.  numpy only; imported like helpers.py."""
import collections
import ctypes
import functools
import re

import numpy as np

from sample_cases import philox4x32_10

M32, M64 = 0xFFFFFFFF, 2 ** 64 - 1
SHUF = 0x53485546  # "SHUF": the tweak of the key's high word
MIX_1, MIX_2 = 0x9E3779B1, 0x85EBCA6B
NO_SEAT = 255
FILL = -7  # what the output arrays of a GPU test start as: no id, index entry or count is negative but the -1 of a tail

# seeds and epochs with both halves set; an epoch on either side of the wrap of its low word
KEYS = ((0x9E3779B97F4A7C15, 2 ** 32 - 1), (0x0123456789ABCDEF, 2 ** 32), (0xC0FFEE0000000001, 0xFEDCBA9876543210), (0x8000000500000003, 0x700000007))
BIJECTION_SIZES = (1, 2, 3, 5, 17, 64, 65, 1000, 4097, 66563, 2 ** 20 + 1, 2 ** 20 + 3, 3 * 2 ** 20, 2 ** 22)


@functools.lru_cache(maxsize=None)
def plan(n_samples=0, seat=0, actions=0, ids=1, n_out=0, n_learner=0):
    """(return code, oc_sample_index_plan's words or the refusal) — no device needed"""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(1024)
    rc = L.oc_sample_index_plan(n_samples, seat, actions, ids, n_out, n_learner, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def block_samples():
    """P, the samples per block of the selection, read from the plan's words"""
    rc, text = plan()
    assert rc == 0, text
    return int(re.search(r"P = (\d+) samples per block", text).group(1))


# ------------------------------------------------------------------------------------------ the restatement
def selected(n_samples, seat=None, actions=None):
    """[S] bool: the header's selection rule"""
    s = np.arange(n_samples, dtype=np.int64)
    keep = np.ones(n_samples, bool)
    if seat is not None:
        keep &= seat[s >> 1].astype(np.int64) != (s & 1)
    if actions is not None:
        keep &= actions <= 5
    return keep


def select(n_samples, seat=None, actions=None):
    """(d_ids int32 [S]: the selected samples ascending, then -1; L)"""
    chosen = np.nonzero(selected(n_samples, seat, actions))[0]
    ids = np.full(n_samples, -1, np.int32)
    ids[:len(chosen)] = chosen
    return ids, len(chosen)


def round_keys(seed, epoch, drop=None):
    """k[0 .. 7] as python ints.  drop: None, or the part of the counters a kernel could lose — "seed_hi", "epoch_hi", "tweak"."""
    assert drop in (None, "seed_hi", "epoch_hi", "tweak")
    seed, epoch = int(seed) & M64, int(epoch) & M64
    seed_hi = 0 if drop == "seed_hi" else seed >> 32
    epoch_hi = 0 if drop == "epoch_hi" else epoch >> 32
    k1 = seed_hi ^ (0 if drop == "tweak" else SHUF)
    k = []
    for j in (0, 1):
        k += [int(x) for x in philox4x32_10(epoch & M32, epoch_hi, j, 0, seed & M32, k1)]
    return k


def widths(L):
    """(w, a, c) of L >= 2"""
    w = max(1, int(L - 1).bit_length())
    a = w >> 1
    return w, a, w - a


def mix(v):
    """u32 arithmetic that wraps, on uint64 arrays holding u32 values"""
    v = (v * np.uint64(MIX_1)) & np.uint64(M32)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(MIX_2)) & np.uint64(M32)
    v = v ^ (v >> np.uint64(13))
    return v


def top(v, q):
    return v >> np.uint64(32 - q) if q else np.zeros_like(v)


def rounds(x, k, a, c):
    """One evaluation of the eight rounds on the uint64 array x of values below 2^(a + c)"""
    l, r = x >> np.uint64(c), x & np.uint64((1 << c) - 1)
    for j in range(8):
        if j % 2 == 0:
            l = l ^ top(mix((r + np.uint64(k[j])) & np.uint64(M32)), a)
        else:
            r = r ^ top(mix((l + np.uint64(k[j])) & np.uint64(M32)), c)
    return (l << np.uint64(c)) | r


def pi(L, seed, epoch, drop=None, walk=None):
    """int64 [L]: pi(0 .. L - 1).  walk: a dict that receives `evaluations` (of the rounds, in all) and `longest` (walk of one i)."""
    if L <= 1:
        return np.zeros(L, np.int64)
    k = round_keys(seed, epoch, drop)
    _, a, c = widths(L)
    x = np.arange(L, dtype=np.uint64)
    todo = np.arange(L)
    evaluations = longest = 0
    while len(todo):
        x[todo] = rounds(x[todo], k, a, c)
        evaluations += len(todo)
        longest += 1
        todo = todo[x[todo] >= np.uint64(L)]
    if walk is not None:
        walk.update(evaluations=evaluations, longest=longest)
    return x.astype(np.int64)


def permute(ids, L, n_out, seed, epoch):
    """d_index int32 [n_out]; ids None: the identity"""
    out = np.full(n_out, -1, np.int32)
    m = min(L, n_out)
    p = pi(L, seed, epoch)[:m]
    out[:m] = p if ids is None else ids[p]
    return out


# ------------------------------------------------------------------------------------------ the cases
SEATS = ("none", "all255", "all0", "all1", "alternating", "random")
ACTIONS = ("none", "valid", "scattered", "all255")
N_OUT = ("L", "S", "zero", "L-1")
Case = collections.namedtuple("Case", "id n_samples seat actions n_out seed epoch rng")


def sizes():
    P = block_samples()
    return (0, 2, 128, P - 2, P, P + 2, 2 * P + 2, 66562, 300002)


def _cases():
    out, i = [], 0

    def add(S, seat, actions):
        nonlocal i
        seed, epoch = KEYS[i % len(KEYS)]
        out.append(Case("S%d-%s-%s-%s-k%d" % (S, seat, actions, N_OUT[(i // 4 + i) % 4], i % len(KEYS)), S, seat, actions, N_OUT[(i // 4 + i) % 4],
                        seed, epoch, 500 + i))
        i += 1

    P = block_samples()
    for S in sizes():  # every size with every seat pattern, the actions and n_out taking turns
        for j, seat in enumerate(SEATS):
            add(S, seat, ACTIONS[(j + i) % 4])
    have = {(c.seat, c.actions) for c in out if c.n_samples == 2 * P + 2}
    for seat in SEATS:  # every seat pattern with every action pattern, at more than two blocks
        for actions in ACTIONS:
            if (seat, actions) not in have:
                add(2 * P + 2, seat, actions)
    have = {(c.n_samples, c.n_out) for c in out}
    for S in sizes():  # every size with every n_out
        for kind in N_OUT:
            if (S, kind) not in have:
                while N_OUT[(i // 4 + i) % 4] != kind:
                    i += 1
                add(S, "random", "scattered")
    return tuple(out)


def seat_pattern(kind, n_samples, rng):
    n = n_samples // 2
    if kind == "none":
        return None
    if kind in ("all255", "all0", "all1"):
        return np.full(n, int(kind[3:]), np.uint8)
    if kind == "alternating":
        return (np.arange(n) & 1).astype(np.uint8)
    if kind == "random":
        return rng.choice(np.array([0, 1, NO_SEAT], np.uint8), size=n)
    raise ValueError(kind)


def action_pattern(kind, n_samples, rng):
    if kind == "none":
        return None
    if kind == "all255":
        return np.full(n_samples, 255, np.uint8)
    a = rng.integers(0, 6, size=n_samples).astype(np.uint8)
    if kind == "scattered":  # 255 (the sampler's invalid row) and 6 (the first value that is no action) here and there
        bad = rng.random(n_samples) < 0.1
        a = np.where(bad, rng.choice(np.array([255, 6], np.uint8), size=n_samples), a).astype(np.uint8)
    elif kind != "valid":
        raise ValueError(kind)
    return a


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """(seat uint8 [S / 2] or None, actions uint8 [S] or None), read-only"""
    rng = np.random.default_rng(c.rng)
    seat, actions = seat_pattern(c.seat, c.n_samples, rng), action_pattern(c.actions, c.n_samples, rng)
    for a in (seat, actions):
        if a is not None:
            a.setflags(write=False)
    return seat, actions


def n_out_of(c, L):
    return {"L": L, "S": c.n_samples, "zero": 0, "L-1": max(L - 1, 0)}[c.n_out]


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """(ids int32 [S], L, n_out, index int32 [n_out], plain int32 [n_out]: the same permutation without ids) of a case, computed
    once and shared, read-only"""
    seat, actions = arrays_of(c)
    ids, L = select(c.n_samples, seat, actions)
    n_out = n_out_of(c, L)
    plain = permute(None, L, n_out, c.seed, c.epoch)
    index = np.where(plain >= 0, ids[np.maximum(plain, 0)], -1).astype(np.int32)  # (pi evaluated once: index[i] = ids[pi(i)])
    for a in (ids, index, plain):
        a.setflags(write=False)
    return ids, L, n_out, index, plain


def scan_shape():
    """(blocks per pass of k_sample_scan, passes whose counts it holds in flight), read from the plan's words"""
    rc, text = plan(2, 0, 0, 1, 2, 2)
    assert rc == 0, text
    m = re.search(r"pass\(es\) of (\d+) blocks, (\d+) passes in flight", text)
    return int(m.group(1)), int(m.group(2))


def long_sizes():
    """Sizes at which k_sample_scan runs beyond its first run of passes in flight: one hand-over and a run of ONE pass behind it
    (B + 1 passes), two hand-overs and a run of one pass (2 B + 1 passes) — the path every pass of a 65 536-env x 400-step batch takes."""
    P = block_samples()
    per_pass, B = scan_shape()
    return (B * per_pass * P + 2 * P + 2, 2 * B * per_pass * P + P + 2)


def _long_cases():
    s1, s2 = long_sizes()
    return (Case("S%d-random-scattered-S-k2" % s1, s1, "random", "scattered", "S", *KEYS[2], 901),
            Case("S%d-none-valid-L-k1" % s2, s2, "none", "valid", "L", *KEYS[1], 902),
            Case("S%d-alternating-none-L-1-k3" % s2, s2, "alternating", "none", "L-1", *KEYS[3], 903))


CASES = _cases()
LONG_CASES = _long_cases()
