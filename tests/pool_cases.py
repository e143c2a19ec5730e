"""The cases of oc_partner_pool_logits (include/oc_amd.h: OcPartnerPool; csrc/partner_pool.hpp) and the member draw restated twice.

The draw, restated: `draws` (vectorised numpy on sample_cases.philox4x32_10) and `draws_by_the_header` (one env at a time on Python
integers and the oracle's Philox, written from the header's sentences): word 2 of the SEATING block of partner_cases, counted
against the pool's thresholds.  `redraw` applies a done mask.  The network's references are partner_cases' (mlp_f64, mlp_bound),
evaluated with the weights of the env's OWN member.

Every case states, and asserts from the restatement itself, the property it is in the list for (CLAIMS)."""
from collections import namedtuple

import numpy as np

import partner_cases as PC
import sample_cases as SC

NO_MEMBER = 255
MAX_POOL = 16
SHAPES = ((64, 64), (40, 24), (1, 1))  # (h1, h2) of members 0, 1, 2, 0, ...: the reference's widths, padded ones, the narrowest


def uniform_thresholds(k):
    """ceil((m + 1) * 2^32 / k) for m < k - 1, on Python integers"""
    return [-((-(m + 1) * 2**32) // k) for m in range(k - 1)]


def words(seed, env_offset, step, n, drop=None):
    """uint32 [4][n]: the seating block of envs 0..n-1 (partner_cases.seat_words keeps words 0 and 1 of it).  drop: None, "tweak" or
    one half of a counter."""
    assert drop in (None, "t_hi", "g_hi", "seed_hi", "tweak")
    seed, step, env_offset = int(seed) & PC.M64, int(step) & PC.M64, int(env_offset) & PC.M64
    g = np.uint64(env_offset) + np.arange(n, dtype=np.uint64)
    g_lo, g_hi = g & SC.M32, g >> np.uint64(32)
    if drop == "g_hi":
        g_hi = np.zeros_like(g_hi)
    t_lo, t_hi = step & 0xFFFFFFFF, 0 if drop == "t_hi" else step >> 32
    k1 = (0 if drop == "seed_hi" else seed >> 32) ^ (0 if drop == "tweak" else PC.SEAT_TWEAK)
    return SC.philox4x32_10(np.full(n, t_lo, np.uint64), g_lo, g_hi, np.full(n, t_hi, np.uint64), seed & 0xFFFFFFFF, k1)


def members_of_words(r2, thresholds):
    """uint8: #{m : r2 >= thresholds[m]}"""
    r2 = np.asarray(r2).astype(np.uint64)
    out = np.zeros(r2.shape, np.int64)
    for t in thresholds:
        out += r2 >= np.uint64(t)
    return out.astype(np.uint8)


def draws(seed, env_offset, step, n, bc_factor, thresholds, drop=None):
    """(seat, member) uint8 [n]: what every env draws when it is reseated at `step`"""
    r = words(seed, env_offset, step, n, drop)
    u = (r[0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    has = u < np.float32(bc_factor)
    seat = np.where(has, (r[1] & np.uint32(1)).astype(np.uint8), np.uint8(PC.NO_SEAT)).astype(np.uint8)
    member = np.where(has, members_of_words(r[2], thresholds), np.uint8(NO_MEMBER)).astype(np.uint8)
    return seat, member


def draws_by_the_header(seed, env_offset, step, n, bc_factor, n_members, thresholds=None):
    """The header's sentences, one env at a time, on Python integers (thresholds None: the uniform pool's, formed here)."""
    from oracle import oracle as O

    if thresholds is None:
        thresholds = [((m + 1) * 2**32 + n_members - 1) // n_members for m in range(n_members - 1)]
    seat, member = np.empty(n, np.uint8), np.empty(n, np.uint8)
    t = step % 2**64
    for e in range(n):
        g = (env_offset + e) % 2**64
        r = O.philox4x32_10([t % 2**32, g % 2**32, g // 2**32, t // 2**32], [seed % 2**32, (seed // 2**32) ^ PC.SEAT_TWEAK])
        if float(np.float32(r[0] >> 8) * np.float32(2.0 ** -24)) < float(np.float32(bc_factor)):
            seat[e], member[e] = r[1] & 1, sum(1 for m in range(n_members - 1) if r[2] >= thresholds[m])
        else:
            seat[e], member[e] = PC.NO_SEAT, NO_MEMBER
    return seat, member


def redraw(seat, member, done, seed, env_offset, step, bc_factor, thresholds):
    """Seats and members after a call: done None — every env draws; else those whose done byte is not 0, the others keep both."""
    s, m = draws(seed, env_offset, step, len(seat), bc_factor, thresholds)
    if done is None:
        return s, m
    d = np.asarray(done) != 0
    return np.where(d, s, seat).astype(np.uint8), np.where(d, m, member).astype(np.uint8)


def chi_square_z(counts, expected):
    """(chi-square - dof) / sqrt(2 dof) of observed counts against expected ones"""
    counts, expected = np.asarray(counts, np.float64), np.asarray(expected, np.float64)
    dof = len(counts) - 1
    return float((((counts - expected) ** 2 / expected).sum() - dof) / np.sqrt(2.0 * dof))


# ------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "id table n_envs num_pots n_members bc_factor weights seed env_offset step claims")
CASES = []


def case(n_envs, n_members, bc_factor, claims, table="cramped_room", num_pots=2, weights=None, seed=None):
    k = len(CASES)
    CASES.append(Case("%s_%dpots_%denvs_%dmembers_factor%g%s" % (table, num_pots, n_envs, n_members, bc_factor, "_weighted" if weights else ""),
                      table, n_envs, num_pots, n_members, bc_factor, weights, 301 + k if seed is None else seed, 3 * n_envs + 64 * k + 37,
                      5 + k, tuple(claims)))


case(1, 3, 1.0, ("two_empty_members",))
case(33, 3, 1.0, ("every_member", "no_full_tile"))                 # one past a tile
case(33, 16, 1.0, ("an_empty_member",))
case(65, 2, 0.5, ("every_member", "unseated_envs"))
case(488, 3, 0.5, ("every_member", "ragged_buckets", "unseated_envs"))  # a ragged last block
case(488, 3, 1.0, ("every_member", "ragged_buckets"))
case(488, 16, 1.0, ("every_member", "sixteen_chunks"))             # against a grid bound of 2 + 16
case(1500, 2, 1.0, ("every_member", "three_workgroups"))
case(488, 1, 0.5, ("unseated_envs",))                              # K = 1: oc_partner_logits itself
case(488, 3, 1.0, ("every_member",), num_pots=1)                   # 76 inputs
case(488, 3, 1.0, ("every_member",), table="asymmetric_advantages", num_pots=4)  # 136 inputs
case(488, 4, 1.0, ("zero_weight_member",), weights=(1.0, 0.0, 2.0, 1.0))
case(66000, 4, 1.0, ("every_member", "more_chunks_than_cus"))      # 256 CUs: k_pool_logits takes 384 rows per workgroup, in three passes
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def far_case():
    """partner_cases.far_case()'s counters under the 488-env, three-member, factor 0.5 case."""
    f = PC.far_case()
    c = next(c for c in CASES if (c.n_envs, c.n_members, c.bc_factor, c.num_pots) == (488, 3, 0.5, 2))
    return c._replace(id=c.id + "@far", seed=f.seed, env_offset=f.env_offset, step=f.step)


def shapes_of(c):
    return tuple(SHAPES[m % len(SHAPES)] for m in range(c.n_members))


def weights_of(c):
    """One partner_cases.glorot network per member, of the member's own hidden widths"""
    return [PC.glorot((c.seed & 0xFFFFFFFF) + 1000 * (m + 1), PC.total_of(c.num_pots), h1, h2) for m, (h1, h2) in enumerate(shapes_of(c))]


def thresholds_of(c):
    """The thresholds the library uses for the case: the uniform ones, or PartnerPool's rounding of the weights, restated"""
    if c.weights is None:
        return uniform_thresholds(c.n_members)
    from fractions import Fraction

    w = [Fraction(x) for x in c.weights]
    run, out = Fraction(0), []
    for x in w[:-1]:
        run += x
        q = run * 2**32 / sum(w)
        out.append(min(int(q) + (q != int(q)), 2**32 - 1))
    return out


MI355X_CUS = 256


def chunks_of(counts, rows=256):
    """The workgroups of k_pool_logits that have rows, at `rows` rows of one member each"""
    return int(((np.asarray(counts) + rows - 1) // rows).sum())


def passes_of(counts, cus=MI355X_CUS):
    """k_pool_logits' passes of 128 rows per workgroup: two, or where the chunks of 256 rows outnumber the CUs the least number for
    which floor(T / 128) / passes + K fits them"""
    if chunks_of(counts) <= cus:
        return 2
    room = max(cus - len(counts), 1)
    return max((int(np.sum(counts)) // 128 + room - 1) // room, 2)


def first_draws(c):
    return draws(c.seed, c.env_offset, c.step, c.n_envs, c.bc_factor, thresholds_of(c))


def check_claims(c):
    """The property each case is listed for, from the restatement"""
    seat, member = first_draws(c)
    counts = np.bincount(member[member != NO_MEMBER], minlength=c.n_members)
    assert ((member == NO_MEMBER) == (seat == PC.NO_SEAT)).all() and counts.sum() == (seat != PC.NO_SEAT).sum()
    for claim in c.claims:
        ok = {"two_empty_members": lambda: (counts == 0).sum() == 2,
              "every_member": lambda: (counts > 0).all(),
              "no_full_tile": lambda: (counts < 32).all(),
              "an_empty_member": lambda: (counts == 0).any() and (counts > 0).sum() > 8,
              "unseated_envs": lambda: (seat == PC.NO_SEAT).any() and (seat != PC.NO_SEAT).any(),
              "ragged_buckets": lambda: (counts % 32 != 0).all() and c.n_envs % 256 != 0,
              "sixteen_chunks": lambda: c.n_members == 16 and int(((counts + 255) // 256).sum()) == 16 < (c.n_envs + 255) // 256 + 16,
              "three_workgroups": lambda: (counts > 512).all(),  # (every bucket spans three workgroups or more)
              "more_chunks_than_cus": lambda: chunks_of(counts) > MI355X_CUS and passes_of(counts) == 3 and chunks_of(counts, 128 * 3) <= MI355X_CUS,
              "zero_weight_member": lambda: counts[1] == 0 and (np.delete(counts, 1) > 0).all()}[claim]()
        assert ok, (c.id, claim, counts.tolist())


for _c in CASES:
    check_claims(_c)
