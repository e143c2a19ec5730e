"""Dense synthetic cases of oc_partner_logits and oc_partner_pool_logits for the bit-for-bit comparison with the header's fmaf chain
(tests/mlp_chain.py).  Both entry points read only n_envs of the batch and take features, seats and members as plain pointers, and
a seat or member is kept where d_done[e] == 0: no env is needed, and any seat pattern can be preset.

Every case has a seed and one of two kinds of numbers:
  real  feature entries 3 * N(0, 1), about 30 % of them set to 0 and about 10 % to small integers; partner_cases.glorot weights.
        The chain test proper: another order of summation, a pair summed before it is added, a wider accumulator or a contracted
        bias add gives other bits.
  int   features in -6..6, weights in {-1, 0, 1} (density 0.5, or 1.0 where the fan-out is below 8), biases in -3..3: every partial
        sum is an integer far below 2^24, so ANY order is exact.  Where a real case fails and its int twin passes, the fault is in
        order or rounding, not in indexing.
In both kinds no feature column is 0 in every seated row (entries are put back where a column would be), and both players' rows of
an env differ.  A hidden layer of width 1 gets non-zero weights and a positive bias: its one unit has to be alive for anything behind
it to be seen.  `rows` is the dense data of every (env, player); `features`, what the device is given, holds NaN in every row that
no seat names — the other player's row of a seated env, both rows of an unseated env: none may reach a result.

A case is drawn with the next salt until it bites (`misses`: conditions on float64 evaluations of the drawn numbers alone, asserted
again by tests/test_host_partner_dense.py):
  * zeroing any one feature column changes a seated logit of some row — always;
  * zeroing any one unit of either hidden layer does — with 16 seated rows or more (a unit is dead in a row with probability 1/2,
    so with fewer rows some of 128 units are dead in all of them), and always at widths (1, 1);
  * widths >= 17: hidden units are live in 30..70 % of (row, unit); the logits of a seated row differ from those of the env's other
    player's row, and (two envs or more) from those of the next env's row, in at least half of the seated envs;
  * int, with 64 or more hidden pre-activations: some are exactly 0.
For the real kind "changes" and "differ" mean: by more than the sum of the two a-priori bounds (partner_cases.mlp_bound), so that
every float32 evaluation, the chain included, differs too.

Seat patterns (SEAT_PATTERNS) are preset under an all-zero done mask and bc_factor 0.5, so a draw would be visible."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import mlp_chain as MC
import partner_cases as PC
import pool_cases as PP

LENGTHS = (56, 76, 96, 116, 136)
WIDTHS = ((64, 64), (63, 33), (40, 24), (33, 17), (1, 1))
SIZES = (1, 31, 32, 33, 63, 64, 65, 257, 488)
KINDS = ("real", "int")
BC_FACTOR = 0.5
BITE_ROWS = 64      # the column and unit conditions look at this many seated rows at most (what bites there bites in all)
NO = PC.NO_SEAT


def num_pots_of(in_dim):
    return (in_dim - 56) // 20


# ------------------------------------------------------------------------------------------ seat patterns
def _tiles(n):
    return np.arange(n) // 32


def _p_all0(n, two):
    return np.zeros(n, np.uint8)


def _p_all1(n, two):
    return np.ones(n, np.uint8)


def _p_alternate(n, two):
    return (np.arange(n) % 2).astype(np.uint8)


def _p_one_per_tile(n, two):
    e, t = np.arange(n), _tiles(n)
    width = np.minimum(32, n - 32 * t)
    return np.where(e % 32 == (7 * t + 3) % width, two, NO).astype(np.uint8)


def _p_empty_first_tile(n, two):
    return np.where(_tiles(n) % 2 == 0, NO, two).astype(np.uint8)


def _p_empty_second_tile(n, two):
    return np.where(_tiles(n) % 2 == 1, NO, two).astype(np.uint8)


def _p_empty_waves_between(n, two):
    wave = (np.arange(n) % 256) // 64
    return np.where((wave == 1) | (wave == 2), NO, two).astype(np.uint8)


def _p_empty_workgroup_between(n, two):
    group, last = np.arange(n) // 256, (n - 1) // 256
    assert last >= 2, "three workgroups or more"
    return np.where((group > 0) & (group < last), NO, two).astype(np.uint8)


def _p_last_env_only(n, two):
    return np.where(np.arange(n) == n - 1, two, NO).astype(np.uint8)


def _p_other_bytes(n, two):
    e = np.arange(n)
    other = (2 + (e * 37) % 253).astype(np.uint8)  # 2..254
    unseated = np.flatnonzero((e // 3) % 2 == 1)
    other[unseated[0]], other[unseated[-1]] = 2, 254  # both ends among them
    return np.where((e // 3) % 2 == 0, two, other).astype(np.uint8)


def _p_seeded(n, two):
    """the shape cases' pattern: about four of five envs seated, the last one always (one env: seated)"""
    gone = np.random.default_rng([n, 0x5EA7]).random(n) < 0.2
    gone[n - 1] = False
    return np.where(gone, NO, two).astype(np.uint8)


SEAT_PATTERNS = {"all0": _p_all0, "all1": _p_all1, "alternate": _p_alternate, "one_per_tile": _p_one_per_tile,
                 "empty_first_tile": _p_empty_first_tile, "empty_second_tile": _p_empty_second_tile,
                 "empty_waves_between": _p_empty_waves_between, "empty_workgroup_between": _p_empty_workgroup_between,
                 "last_env_only": _p_last_env_only, "other_bytes": _p_other_bytes}


# ------------------------------------------------------------------------------------------ the partner cases
Case = namedtuple("Case", "id kind in_dim h1 h2 n_envs pattern seed env_offset step")
CASES = []


def case(kind, in_dim, h1, h2, n_envs, pattern):
    cid = "%s-%d_%d_%d-%denvs-%s" % (kind, in_dim, h1, h2, n_envs, pattern)
    if any(c.id == cid for c in CASES):
        return
    k = len(CASES)
    CASES.append(Case(cid, kind, in_dim, h1, h2, n_envs, pattern, 7001 + k, 5 * n_envs + 64 * k + 11, 9 + k))


for _kind in KINDS:
    # every width pair at every feature length, the sizes in turn
    for _i, _in_dim in enumerate(LENGTHS):
        for _j, (_h1, _h2) in enumerate(WIDTHS):
            case(_kind, _in_dim, _h1, _h2, SIZES[(5 * _i + _j) % len(SIZES)], "seeded")
    # every size at the reference's model
    for _n in SIZES:
        case(_kind, 96, 64, 64, _n, "seeded")
    # the seat patterns, at two workgroups (488 envs) and at three (600: another length, odd widths); a middle workgroup takes three
    for _name in SEAT_PATTERNS:
        if _name != "empty_workgroup_between":
            case(_kind, 96, 64, 64, 488, _name)
        case(_kind, 136, 63, 33, 600, _name)
    # drawn seats: d_done == NULL, against partner_cases.seats
    for _i, _in_dim in enumerate(LENGTHS):
        case(_kind, _in_dim, *WIDTHS[_i], 488, "drawn")
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def seats_of(c):
    """uint8 [n]: the seats of the case — preset, or (pattern "drawn") what the seating stream gives every env"""
    if c.pattern == "drawn":
        return PC.seats(c.seed, c.env_offset, c.step, c.n_envs, BC_FACTOR)
    two = np.random.default_rng([c.seed, 0x2]).integers(0, 2, c.n_envs).astype(np.uint8)
    fn = _p_seeded if c.pattern == "seeded" else SEAT_PATTERNS[c.pattern]
    return fn(c.n_envs, two)


def _tern(rng, shape, density):
    return (rng.choice(np.array([-1, 1]), shape) * (rng.random(shape) < density)).astype(np.float32)


def weights_of(kind, seed, in_dim, h1, h2, salt=0):
    """The six float32 arrays of a network of the kind (module docstring)"""
    if kind == "real":
        w = list(PC.glorot(seed + 7919 * salt, in_dim, h1, h2))
    else:
        rng = np.random.default_rng([seed, 0x1A7, salt])
        w = []
        for fan_in, fan_out in ((in_dim, h1), (h1, h2), (h2, 6)):
            w += [_tern(rng, (fan_in, fan_out), 1.0 if fan_out < 8 else 0.5), rng.integers(-3, 4, (fan_out,)).astype(np.float32)]
    for layer, width in ((0, h1), (1, h2)):
        if width == 1:  # the one unit must be alive: a non-zero weight behind every input, a positive bias
            w[2 * layer] = np.where(w[2 * layer] == 0, np.float32(1), w[2 * layer]).astype(np.float32)
            w[2 * layer + 1] = np.maximum(np.abs(w[2 * layer + 1]), np.float32(1 if kind == "int" else 0.125)).astype(np.float32)
    return tuple(w)


def dense_rows(kind, rng, n, in_dim, named):
    """float32 [n, 2, in_dim] of the kind; named: bool [n, 2], the rows in which no column may be 0 throughout"""
    if kind == "real":
        full = (3.0 * rng.standard_normal((n, 2, in_dim))).astype(np.float32)
        full[full == 0] = np.float32(1.5)
        x = full.copy()
        u = rng.random(x.shape)
        small = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), x.shape).astype(np.float32)
        x = np.where(u < 0.3, np.float32(0), np.where(u < 0.4, small, x)).astype(np.float32)
    else:
        full = rng.choice(np.array([-6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6]), (n, 2, in_dim)).astype(np.float32)
        x = np.where(rng.random(full.shape) < 1.0 / 13, np.float32(0), full).astype(np.float32)
    e, p = np.nonzero(named)
    for col in np.flatnonzero(~(x[e, p] != 0).any(0)):  # a column of zeros among the named rows: one entry is put back
        k = int(rng.integers(len(e)))
        x[e[k], p[k], col] = full[e[k], p[k], col]
    return x


Arrays = namedtuple("Arrays", "weights rows features seat seated p")


def _draw(c, salt):
    rng = np.random.default_rng([c.seed, 0xDE5E, salt])
    seat = seats_of(c)
    seated = np.flatnonzero(seat <= 1)
    p = seat[seated].astype(np.int64)
    named = np.zeros((c.n_envs, 2), bool)
    named[seated, p] = True
    rows = dense_rows(c.kind, rng, c.n_envs, c.in_dim, named)
    features = np.where(named[:, :, None], rows, np.float32(np.nan)).astype(np.float32)
    weights = weights_of(c.kind, c.seed, c.in_dim, c.h1, c.h2, salt)
    for a in (rows, features, seat, seated, p) + weights:
        a.setflags(write=False)
    return Arrays(weights, rows, features, seat, seated, p)


def _differs(kind, x, y, weights):
    """bool [rows]: the logits of rows x and of rows y differ in every float32 evaluation (real), or at all (int: every one is exact)"""
    fx, fy = PC.mlp_f64(x, weights)[0], PC.mlp_f64(y, weights)[0]
    if kind == "int":
        return (fx != fy).any(-1)
    return (np.abs(fx - fy) > PC.mlp_bound(x, weights) + PC.mlp_bound(y, weights)).any(-1)


def _f64_from(pre1, weights, layer):
    """float64 logits from the pre-activations of `layer` (1 or 2) on"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float32).astype(np.float64) for a in weights)
    pre2 = np.maximum(pre1, 0.0) @ w2 + b2 if layer == 1 else pre1
    return np.maximum(pre2, 0.0) @ w3 + b3


def _unbitten_by_the_chain(x, weights):
    """`unbitten` for a handful of real rows, where the a-priori bound is too coarse a sieve (a column must move one row's logits by
    a hundred times their rounding error): by the chain itself.  The columns as ONE evaluation of every row with every column
    zeroed in turn; the units — asked of so few rows at widths (1, 1) alone — with their outgoing weights zeroed (such a step adds
    an exact zero)."""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    base = MC.canon(MC.chain_f32(x, weights))
    zeroed = np.repeat(x[:, None, :], d, axis=1)
    zeroed[:, np.arange(d), np.arange(d)] = 0
    moved = (MC.canon(MC.chain_f32(zeroed, weights)) != base[:, None, :]).any(axis=(0, 2))
    units = [[], []]
    if weights[0].shape[1] == 1 and weights[2].shape[1] == 1:
        for layer in (0, 1):
            w = [a.copy() for a in weights]
            w[2 * layer + 2][0, :] = 0
            if (MC.canon(MC.chain_f32(x, w)) == base).all():
                units[layer] = [0]
    return list(np.flatnonzero(~moved)), units[0], units[1]


def unbitten(kind, x, weights):
    """(feature columns, units of layer 1, units of layer 2) whose zeroing changes no logit of rows x — in float64, for the real
    kind by more than twice the largest a-priori bound of these rows (a bound of the unchanged rows bounds the zeroed ones: a
    zeroed term only takes away from |w|^T |x|)"""
    if kind == "real" and len(x) < 16:
        return _unbitten_by_the_chain(x, weights)
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float32).astype(np.float64) for a in weights)
    x = np.asarray(x, np.float32).astype(np.float64)
    pre1 = x @ w1 + b1
    a1 = np.maximum(pre1, 0.0)
    pre2 = a1 @ w2 + b2
    base = _f64_from(pre2, weights, 2)
    margin = 0.0 if kind == "int" else 2.0 * PC.mlp_bound(x.astype(np.float32), weights).max()
    moved = lambda out: (np.abs(out - base) > margin).any(axis=(1, 2))  # noqa: E731  ([zeroed one, row, logit] -> [zeroed one])
    without = lambda pre, v, w: pre[None] - v.T[:, :, None] * w[:, None, :]  # noqa: E731  (pre without the terms of input k, for every k)
    a2 = np.maximum(pre2, 0.0)
    cols = np.flatnonzero(~moved(_f64_from(without(pre1, x, w1), weights, 1)))
    units1 = np.flatnonzero(~moved(_f64_from(without(pre2, a1, w2), weights, 2)))
    units2 = np.flatnonzero(~moved(without(base, a2, w3)))
    return cols.tolist(), units1.tolist(), units2.tolist()


Report = namedtuple("Report", "cols units1 units2 live other_row next_row zeros n_pre")


def report_of(kind, h1, h2, a_rows, x, other, nxt, weights):
    """What `misses` weighs, measured on the reference alone.  x: the seated rows; other / nxt: the other player's rows of the same
    envs and the same player's rows of the next envs (None with one env)"""
    cols, units1, units2 = unbitten(kind, x[:BITE_ROWS], weights)
    _, (a1, a2) = PC.mlp_f64(x, weights)
    w1, b1, w2, b2 = (np.asarray(a, np.float32).astype(np.float64) for a in weights[:4])
    pre1 = x.astype(np.float64) @ w1 + b1
    pre2 = a1 @ w2 + b2
    live = float(np.concatenate([(pre1 > 0).reshape(-1), (pre2 > 0).reshape(-1)]).mean())
    zeros = int((pre1 == 0).sum() + (pre2 == 0).sum())
    return Report(cols, units1, units2, live, float(_differs(kind, x, other, weights).mean()),
                  None if nxt is None else float(_differs(kind, x, nxt, weights).mean()), zeros, pre1.size + pre2.size)


def misses_of(kind, h1, h2, r, n_rows):
    """What keeps a drawn case from biting, as words (none: [])"""
    out = []
    if r.cols:
        out.append("zeroing feature column(s) %s changes nothing" % r.cols[:5])
    if (n_rows >= 16 or (h1, h2) == (1, 1)) and (r.units1 or r.units2):
        out.append("zeroing hidden unit(s) %s / %s changes nothing" % (r.units1[:5], r.units2[:5]))
    if min(h1, h2) >= 17:
        if not 0.3 <= r.live <= 0.7:
            out.append("%.2f of the hidden units are live" % r.live)
        if r.other_row < 0.5:
            out.append("only %.2f of the envs tell their two players' rows apart" % r.other_row)
        if r.next_row is not None and r.next_row < 0.5:
            out.append("only %.2f of the envs tell their row from the next env's" % r.next_row)
    if kind == "int" and r.n_pre >= 64 and r.zeros == 0:
        out.append("no pre-activation is exactly 0")
    return out


def report(c, a):
    e, p, n = a.seated, a.p, c.n_envs
    nxt = a.rows[(e + 1) % n, p] if n > 1 else None
    return report_of(c.kind, c.h1, c.h2, a.rows, a.rows[e, p], a.rows[e, 1 - p], nxt, a.weights)


def misses(c, a):
    return misses_of(c.kind, c.h1, c.h2, report(c, a), len(a.seated))


@lru_cache(maxsize=None)
def arrays_of(c):
    for salt in range(64):
        a = _draw(c, salt)
        said = misses(c, a)
        if not said:
            return a
    raise AssertionError("%s: no draw that bites: %s" % (c.id, said))


@lru_cache(maxsize=None)
def reference_of(c):
    """mlp_chain.Chain of the seated rows, in ascending env, computed once"""
    a = arrays_of(c)
    r = MC.evaluate(a.rows[a.seated, a.p], a.weights, watch=True)
    for v in r[:3]:
        v.setflags(write=False)
    return r


def logits_fill(n):
    """float32 [n, 2, 6]: no integer, no repeated value, every one finite"""
    return ((np.arange(n * 12, dtype=np.float32) + np.float32(0.5)) * np.float32(2.0 ** -10) - np.float32(3.0)).reshape(n, 2, 6)


# ------------------------------------------------------------------------------------------ the pool cases
# Seats and members are preset (an all-zero done mask) and interleaved across the envs in a seeded shuffled order, so that order[] is
# no identity.  counts: the envs of every member; beside them every case holds NULL_EACH envs of each of the kinds of NULLS — none of
# which may get logits — and plain unseated envs.
NULL_EACH = 9
NULLS = ("seat_and_member_255", "seat_and_member_beyond_the_pool", "member_and_seat_255", "member_and_another_seat_byte", "neither")
PoolCase = namedtuple("PoolCase", "id kind in_dim n_members counts drawn n_envs seed env_offset step")
POOL_CASES = []
POOL_SIZES = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)  # the tile of 32 rows, the pass of 128, the chunk of 256, two chunks + 1


def pool_case(kind, in_dim, counts, drawn=False, n_envs=None):
    k = len(POOL_CASES)
    K = len(counts)
    n = n_envs if drawn else int(sum(counts)) + NULL_EACH * len(NULLS)
    POOL_CASES.append(PoolCase("pool-%s-%d-%dmembers-%denvs%s" % (kind, in_dim, K, n, "-drawn" if drawn else ""), kind, in_dim, K, tuple(counts),
                               drawn, n, 8001 + k, 3 * n + 64 * k + 5, 21 + k))


for _kind in KINDS:
    pool_case(_kind, 56, (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 0, 2, 0, 0, 0))
    pool_case(_kind, 76, (513, 128, 0))
    pool_case(_kind, 96, (257,))
    pool_case(_kind, 116, (32, 33, 31))
    pool_case(_kind, 136, (33, 0, 1, 0, 31, 0, 64, 0, 129, 0, 0, 3, 0, 65, 0, 127))  # (empty buckets side by side; fewer rows: the longest chain)
    pool_case(_kind, 96, (0, 0, 0), drawn=True, n_envs=488)  # d_done == NULL: seats and members against pool_cases.draws
POOL_CASES = tuple(POOL_CASES)
assert len({c.id for c in POOL_CASES}) == len(POOL_CASES) and max(c.n_envs for c in POOL_CASES) < 2000
assert {c.n_members for c in POOL_CASES} == {1, 3, 16}


def pool_shapes_of(c):
    return tuple(WIDTHS[m % len(WIDTHS)] for m in range(c.n_members))


def pool_seats_of(c):
    """(seat, member) uint8 [n]"""
    if c.drawn:
        return PP.draws(c.seed, c.env_offset, c.step, c.n_envs, BC_FACTOR, PP.uniform_thresholds(c.n_members))
    rng = np.random.default_rng([c.seed, 0x9001])
    K = c.n_members
    member = np.concatenate([np.full(k, m, np.uint8) for m, k in enumerate(c.counts)] + [np.zeros(0, np.uint8)])
    seat = rng.integers(0, 2, len(member)).astype(np.uint8)
    q = NULL_EACH
    beyond = (K + (np.arange(q) * 29) % (255 - K)).astype(np.uint8)  # K..254
    beyond[0], beyond[-1] = K, 254
    extra_seat = [rng.integers(0, 2, q), rng.integers(0, 2, q), np.full(q, 255), 2 + (np.arange(q) * 31) % 253, np.full(q, 255)]
    extra_member = [np.full(q, 255), beyond, rng.integers(0, K, q), rng.integers(0, K, q), np.full(q, 255)]
    seat = np.concatenate([seat] + [np.asarray(s).astype(np.uint8) for s in extra_seat])
    member = np.concatenate([member] + [np.asarray(m).astype(np.uint8) for m in extra_member])
    order = rng.permutation(len(seat))
    return seat[order], member[order]


PoolArrays = namedtuple("PoolArrays", "weights rows features seat member served p")


def _pool_rows(c):
    rng = np.random.default_rng([c.seed, 0x9002])
    seat, member = pool_seats_of(c)
    served = np.flatnonzero((seat <= 1) & (member < c.n_members))
    p = seat[served].astype(np.int64)
    named = np.zeros((c.n_envs, 2), bool)
    named[served, p] = True
    rows = dense_rows(c.kind, rng, c.n_envs, c.in_dim, named)
    features = np.where(named[:, :, None], rows, np.float32(np.nan)).astype(np.float32)
    return PoolArrays(None, rows, features, seat, member, served, p)


def pool_member_misses(c, a, m, weights):
    """partner `misses` of member m with `weights` on the member's own rows.  A member of fewer than 16 rows is not weighed: the
    columns are put back over the case's rows together, not over every member's own, and every width is weighed at a fuller member."""
    h1, h2 = pool_shapes_of(c)[m]
    mine = a.member[a.served] == m
    e, p = a.served[mine], a.p[mine]
    if len(e) < 16:
        return []
    r = report_of(c.kind, h1, h2, a.rows, a.rows[e, p], a.rows[e, 1 - p], a.rows[(e + 1) % c.n_envs, p], weights)
    return misses_of(c.kind, h1, h2, r, len(e))


def pool_misses(c, a):
    return ["member %d: %s" % (m, s) for m in range(c.n_members) for s in pool_member_misses(c, a, m, a.weights[m])]


@lru_cache(maxsize=None)
def pool_arrays_of(c):
    """The rows are drawn once; every member's network with the next salt until it bites on the member's rows"""
    a = _pool_rows(c)
    weights = []
    for m, (h1, h2) in enumerate(pool_shapes_of(c)):
        for salt in range(64):
            w = weights_of(c.kind, c.seed + 1000 * (m + 1), c.in_dim, h1, h2, salt)
            said = pool_member_misses(c, a, m, w)
            if not said:
                break
        else:
            raise AssertionError("%s: no network of member %d that bites: %s" % (c.id, m, said))
        weights.append(w)
    a = a._replace(weights=tuple(weights))
    for v in (a.rows, a.features, a.seat, a.member, a.served, a.p) + tuple(w for ws in weights for w in ws):
        v.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def pool_reference_of(c):
    """(float32 [served, 6] logits of the served envs in ascending env, each by its own member's chain; the smallest non-zero
    magnitude any chain met)"""
    a = pool_arrays_of(c)
    out = np.zeros((len(a.served), 6), np.float32)
    small = np.inf
    for m in range(c.n_members):
        mine = a.member[a.served] == m
        if mine.any():
            r = MC.evaluate(a.rows[a.served[mine], a.p[mine]], a.weights[m], watch=True)
            out[mine] = r.out
            small = min(small, r.smallest)
    out.setflags(write=False)
    return out, small


def bucket_counts(c):
    a = pool_arrays_of(c)
    return np.bincount(a.member[a.served], minlength=c.n_members)
