"""oc_outcome_table's case list and two numpy statements of what include/oc_amd.h says (OcOutcomeBatch): `restated`, the header's
order of summation operation by operation — what the kernel must give bit for bit —, and `reference`, a float64 table that knows
no order (math.fsum per group and column), with the sums of |x| its bound needs.  numpy only; imported like helpers.py."""
import collections
import ctypes
import functools
import math
import re

import numpy as np

NO_SEAT = 255
FILL = -7.0  # what the output arrays of a GPU test start as
COLS = 8
SUM_COLS, MIN_COL, MAX_COL = (0, 1, 2, 5, 6, 7), 3, 4
SIZES = (1, 63, 64, 65, 255, 256, 257, 488, 2100)  # (2 100: nine partials, the sum kernel's loop runs twice)
DONE_PATTERNS = ("never", "every", "equal", "first", "last", "sparse")
SEAT_PATTERNS = ("none", "all0", "all1", "mixed")
MEMBER_PATTERNS = ("none", "k1", "k2", "k3", "k16")
KINDS = ("integer", "real")
MEMBERS_OF = {"none": 1, "k1": 1, "k2": 2, "k3": 3, "k16": 16}
K16_DRAWN = (0, 3, 7, 15)  # the members a k16 case draws from: the others stay empty
K16_LONER = 9              # ... but for this one, which one env alone is given
INVALID_SEATS = (2, 7, 128, 254)


def plan_words(n_envs, n_steps, seat=False, member=False, n_members=1, env_table=False):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(512)
    rc = L.oc_outcome_plan(n_envs, n_steps, int(seat), int(member), n_members, int(env_table), out, len(out))
    assert rc == 0, L.oc_last_error().decode()
    return out.value.decode()


@functools.lru_cache(maxsize=None)
def prefetch_block():
    """The steps per prefetch block of k_outcomes, read from oc_outcome_plan's words (no device needed)."""
    return int(re.search(r"(\d+) steps per prefetch block", plan_words(65536, 400)).group(1))


@functools.lru_cache(maxsize=None)
def env_block():
    """B, the envs of one partial, read from the plan."""
    return int(re.search(r"one partial per block of (\d+) envs", plan_words(65536, 400)).group(1))


def scratch_bytes(n_envs, n_steps, seat, member, n_members):
    return int(re.search(r"scratch (\d+) B", plan_words(n_envs, n_steps, seat, member, n_members)).group(1))


def horizons():
    B = prefetch_block()
    return (1, B - 1, B, B + 1, 400)


Case = collections.namedtuple("Case", "id n_envs n_steps done seat member kind invalid seed")


def _case(n, T, done, seat, member, kind, invalid, seed):
    if seat == "none":
        member, invalid = "none", False
    return Case("n%d-T%d-%s-%s-%s-%s%s" % (n, T, done, seat, member, kind, "-invalid" if invalid else ""), n, T, done, seat, member, kind,
                invalid, seed)


def _cases():
    out, i = [], 0
    Ts = horizons()
    for n in SIZES:  # every size at every horizon, the patterns taking turns
        for T in Ts:
            out.append(_case(n, T, DONE_PATTERNS[i % 6], SEAT_PATTERNS[(i // 6 + i) % 4], MEMBER_PATTERNS[(i // 4 + i) % 5],
                             KINDS[(i // 2) % 2], i % 3 == 0, 100 + i))
            i += 1
    B = prefetch_block()
    for d in DONE_PATTERNS:  # every done pattern in both kinds above the prefetch depth, with members and invalid bytes
        for kind in KINDS:
            out.append(_case(65, B + 1, d, "mixed", "k3", kind, True, 100 + i))
            i += 1
    for s in SEAT_PATTERNS:  # every seat pattern with every member pattern
        for m in MEMBER_PATTERNS:
            out.append(_case(257, B + 1, "sparse", s, m, "real", m != "k2", 100 + i))
            i += 1
    out.append(_case(488, 400, "sparse", "mixed", "k3", "real", True, 300))
    out.append(_case(2100, 400, "sparse", "mixed", "k16", "real", True, 301))
    out.append(_case(2100, 400, "equal", "mixed", "k3", "integer", False, 302))
    out.append(_case(2100, 2 * B + 1, "every", "mixed", "k2", "real", False, 303))
    seen, unique = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            unique.append(c)
    return tuple(unique)


def done_pattern(kind, T, n, rng):
    t, e = np.arange(T)[:, None], np.arange(n)[None, :]
    if kind == "never":
        d = np.zeros((T, n), bool)
    elif kind == "every":
        d = np.ones((T, n), bool)
    elif kind == "equal":  # equal horizons: every env finishes on the same steps
        d = np.broadcast_to((t + 1) % min(7, T) == 0, (T, n))
    elif kind == "first":
        d = np.broadcast_to(t == 0, (T, n))
    elif kind == "last":
        d = np.broadcast_to(t == T - 1, (T, n))
    elif kind == "sparse":
        d = rng.random((T, n)) < 1.0 / 9.0
    else:
        raise ValueError(kind)
    return np.where(d, rng.integers(1, 256, size=(T, n)), 0).astype(np.uint8)  # (any non-zero byte reads as done)


def seat_pattern(kind, T, n, rng):
    if kind == "none":
        return None
    if kind in ("all0", "all1"):
        return np.full((T, n), int(kind[-1]), np.uint8)
    if kind == "mixed":
        return rng.choice(np.array([0, 1, NO_SEAT], np.uint8), size=(T, n))
    raise ValueError(kind)


def member_pattern(kind, seat, rng):
    if kind == "none":
        return None
    T, n = seat.shape
    K = MEMBERS_OF[kind]
    if kind == "k16":
        m = rng.choice(np.array(K16_DRAWN, np.uint8), size=(T, n))
        m[:, min(5, n - 1)] = K16_LONER
    else:
        m = rng.integers(0, K, size=(T, n)).astype(np.uint8)
    # (no partner: the library leaves 255 there; a byte that must not be looked at, so some hold anything)
    junk = rng.integers(0, 256, size=(T, n)).astype(np.uint8)
    return np.where(seat == NO_SEAT, np.where(rng.random((T, n)) < 0.5, 255, junk), m).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """(done u8 [T, N], ep_returns f32 [T, N, 4], seat u8 [T, N] or None, member u8 [T, N] or None, K) of a case, read-only.  Every
    row of ep_returns on a step that is not done holds NaN."""
    rng = np.random.default_rng(c.seed)
    T, n = c.n_steps, c.n_envs
    done = done_pattern(c.done, T, n, rng)
    seat = seat_pattern(c.seat, T, n, rng)
    member = member_pattern(c.member, seat, rng) if seat is not None else None
    K = MEMBERS_OF[c.member]
    if c.invalid:
        bad = rng.random((T, n)) < 0.06
        seat = np.where(bad, rng.choice(np.array(INVALID_SEATS, np.uint8), size=(T, n)), seat).astype(np.uint8)
        if member is not None and K < 255:
            bad = (rng.random((T, n)) < 0.06) & (seat != NO_SEAT)
            member = np.where(bad, rng.integers(K, 256, size=(T, n)), member).astype(np.uint8)
    if c.kind == "integer":  # as the env produces: sparse returns multiples of 20, shaped returns sums of 3s and 5s
        sparse = 20.0 * rng.integers(0, 12, size=(T, n, 2))
        shaped = 3.0 * rng.integers(0, 40, size=(T, n, 2)) + 5.0 * rng.integers(0, 40, size=(T, n, 2))
        ep = np.concatenate([sparse, shaped], axis=2).astype(np.float32)
    else:
        ep = (rng.standard_normal((T, n, 4)) * 100.0).astype(np.float32)
    ep[done == 0] = np.nan
    for a in (done, ep, seat, member):
        if a is not None:
            a.setflags(write=False)
    return done, ep, seat, member, K


def n_groups(seat, K):
    return 1 + 2 * K if seat is not None else 1


def groups_of(seat, member, K, shape, drop_seat_bit=False):
    """The group of every (t, e) as the header states it: G for "no group"."""
    if seat is None:
        return np.zeros(shape, np.int64)
    G = 1 + 2 * K
    s = seat.astype(np.int64)
    m = member.astype(np.int64) if member is not None else np.zeros(shape, np.int64)
    g = np.where(s == NO_SEAT, 0, np.where((s <= 1) & (m < K), 1 + 2 * m + (0 if drop_seat_bit else s), G))
    return g


def empty_table(rows):
    t = np.zeros((rows, COLS))
    t[:, MIN_COL], t[:, MAX_COL] = np.inf, -np.inf
    return t


def add_tables(acc, x):
    """"Adding" table x to the running table acc, the running table on the left."""
    out = acc.copy()
    for c in SUM_COLS:
        out[:, c] = acc[:, c] + x[:, c]
    out[:, MIN_COL] = np.fmin(acc[:, MIN_COL], x[:, MIN_COL])
    out[:, MAX_COL] = np.fmax(acc[:, MAX_COL], x[:, MAX_COL])
    return out


def _in_order(x):
    """+0.0 + x[0] + x[1] + ... one addition after the other (np.cumsum of a 1-D array adds in order)."""
    return float(np.cumsum(np.concatenate([[0.0], x]))[-1])


def restated(done, ep, seat, member, K, descending_partials=False, lanes_before_steps=False, drop_seat_bit=False, read_a_step_early=False):
    """(table f64 [G + 1, 8], env_table f64 [N, 4], partials f64 [blocks, G + 1, 8]) by the header's sentences.  The four keywords are
    the mutants the host tests must tell from the statement: the partials added in descending order; a wavefront taking its
    episodes env by env and not step by step; a group index without its seat bit; the row of the step before a done step."""
    T, n = done.shape
    B = env_block()
    G = n_groups(seat, K)
    rows = G + 1
    group = groups_of(seat, member, K, (T, n), drop_seat_bit)
    blocks = (n + B - 1) // B
    partials = np.zeros((blocks, rows, COLS))
    for b in range(blocks):
        part = empty_table(rows)
        for q in range(B // 64):
            lo, hi = b * B + 64 * q, min(b * B + 64 * q + 64, n)
            wave = empty_table(rows)
            if lo < hi:
                if lanes_before_steps:
                    e, t = np.nonzero(done[:, lo:hi].T)
                else:
                    t, e = np.nonzero(done[:, lo:hi])  # (row-major: ascending t and, within a step, ascending e)
                e = e + lo
                src = np.maximum(t - 1, 0) if read_a_step_early else t
                row = ep[src, e].astype(np.float64)   # (only rows of done steps are read)
                g = group[t, e]
                R = row[:, 0] + row[:, 1]
                RR = R * R
                for k in np.unique(g):
                    sel = g == k
                    if k == G:
                        wave[G, 0] = _in_order(np.ones(int(sel.sum())))
                        continue
                    wave[k] = (_in_order(np.ones(int(sel.sum()))), _in_order(R[sel]), _in_order(RR[sel]),
                               np.fmin.reduce(R[sel], initial=np.inf), np.fmax.reduce(R[sel], initial=-np.inf),
                               _in_order(row[sel, 2]), _in_order(row[sel, 3]), _in_order(row[sel, 0]))
            part = add_tables(part, wave)
        partials[b] = part
    table = empty_table(rows)
    for b in (range(blocks - 1, -1, -1) if descending_partials else range(blocks)):
        table = add_tables(table, partials[b])
    env = np.zeros((n, 4))
    for t in range(T):  # ascending t
        e = np.nonzero(done[t])[0]
        if len(e):
            row = ep[max(t - 1, 0) if read_a_step_early else t, e].astype(np.float64)
            R = row[:, 0] + row[:, 1]
            env[e, 0] += 1.0
            env[e, 1] += R
            env[e, 2] += R * R
            env[e, 3] += row[:, 2] + row[:, 3]
    return table, env, partials


@functools.lru_cache(maxsize=None)
def restated_of(c):
    return restated(*arrays_of(c))


def reference(done, ep, seat, member, K):
    """(table, env_table, abs_table, abs_env): the float64 tables that know no order — every sum math.fsum's, correctly rounded —
    and, in the places of the sums, the sums of |x| (elsewhere 0) that the bound n * 2^-53 * sum |x| needs; n is column 0."""
    T, n = done.shape
    G = n_groups(seat, K)
    group = groups_of(seat, member, K, (T, n))
    t, e = np.nonzero(done)
    row = ep[t, e].astype(np.float64)
    g = group[t, e]
    R = row[:, 0] + row[:, 1]
    RR = R * R
    table, mags = empty_table(G + 1), np.zeros((G + 1, COLS))
    for k in range(G):
        sel = g == k
        if not sel.any():
            continue
        cols = {1: R[sel], 2: RR[sel], 5: row[sel, 2], 6: row[sel, 3], 7: row[sel, 0]}
        table[k, 0] = int(sel.sum())
        table[k, MIN_COL], table[k, MAX_COL] = R[sel].min(), R[sel].max()
        for c, x in cols.items():
            table[k, c], mags[k, c] = math.fsum(x), math.fsum(np.abs(x))
    table[G, 0] = int((g == G).sum())
    env, env_mags = np.zeros((n, 4)), np.zeros((n, 4))
    H = row[:, 2] + row[:, 3]
    order = np.argsort(e, kind="stable")
    cuts = np.searchsorted(e[order], np.arange(n + 1))
    for i in range(n):
        idx = order[cuts[i]:cuts[i + 1]]
        if len(idx):
            env[i] = (len(idx), math.fsum(R[idx]), math.fsum(RR[idx]), math.fsum(H[idx]))
            env_mags[i] = (0.0, math.fsum(np.abs(R[idx])), math.fsum(RR[idx]), math.fsum(np.abs(H[idx])))
    return table, env, mags, env_mags


@functools.lru_cache(maxsize=None)
def reference_of(c):
    return reference(*arrays_of(c))


def within_bound(got, want, counts, mags):
    """|got - want| <= n * 2^-53 * sum |x| entry by entry (counts broadcast over the columns); where mags is 0 that is equality."""
    with np.errstate(invalid="ignore"):  # (inf - inf in the min and max of an empty group: compared by bits elsewhere)
        return np.abs(got - want) <= counts * 2.0 ** -53 * mags


def rational_table(done, ep, seat, member, K):
    """The table and the env table by a scalar loop over the episodes in exact rational arithmetic: every float as the rational it
    is — a Python int where it is an integer (the integer kind: every one), a fractions.Fraction elsewhere.  The entries come back
    as such rationals (min and max of an empty group: None)."""
    from fractions import Fraction

    T, n = done.shape
    G = n_groups(seat, K)
    table = [[0, 0, 0, None, None, 0, 0, 0] for _ in range(G + 1)]
    env = [[0] * 4 for _ in range(n)]
    for t, e in zip(*np.nonzero(done)):
        s0, s1, h0, h1 = (int(x) if x.is_integer() else Fraction(x) for x in ep[t, e].tolist())
        R = s0 + s1
        env[e] = [env[e][0] + 1, env[e][1] + R, env[e][2] + R * R, env[e][3] + h0 + h1]
        if seat is None or seat[t, e] == NO_SEAT:
            g = 0
        elif seat[t, e] <= 1 and (int(member[t, e]) if member is not None else 0) < K:
            g = 1 + 2 * (int(member[t, e]) if member is not None else 0) + int(seat[t, e])
        else:
            table[G][0] += 1
            continue
        r = table[g]
        table[g] = [r[0] + 1, r[1] + R, r[2] + R * R, R if r[3] is None else min(r[3], R), R if r[4] is None else max(r[4], R),
                    r[5] + h0, r[6] + h1, r[7] + s0]
    return table, env


def as_floats(table):
    """A rational table as float64 (every entry of the integer kind is exact there), empty min / max as +inf / -inf."""
    out = np.array([[np.nan if x is None else float(x) for x in row] for row in table])
    if out.shape[1] == COLS:
        out[:, MIN_COL] = np.where(np.isnan(out[:, MIN_COL]), np.inf, out[:, MIN_COL])
        out[:, MAX_COL] = np.where(np.isnan(out[:, MAX_COL]), -np.inf, out[:, MAX_COL])
    return out


CASES = _cases()
