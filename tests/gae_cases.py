"""oc_gae's case list and two numpy restatements of the arithmetic include/oc_amd.h states (OcGaeBatch): gae_f32, the header's f32
recurrence operation by operation — what the kernel must give bit for bit —, and gae_f64, the same recurrence in float64 on the
f32-rounded rewards, with gae_bound, the a-priori bound of the difference between the two.  numpy only; imported like helpers.py."""
import collections
import ctypes
import functools
import re

import numpy as np

U = 2.0 ** -24  # the unit roundoff of f32: one rounding moves a result by at most U times its magnitude
NO_SEAT = 255
FILL = -7.0  # what the output arrays of a GPU test start as: no advantage or target of a case equals it (test_host_gae.py checks)
SIZES = (1, 63, 64, 65, 257, 488)
DONE_PATTERNS = ("none", "every", "first", "last", "horizon5", "random7")
SEAT_PATTERNS = ("none", "all0", "all1", "episode", "inconsistent")


@functools.lru_cache(maxsize=None)
def prefetch_block():
    """B, the steps per prefetch block of k_gae, read from oc_gae_plan's words (no device needed)."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    b = _lib.OcBatch(n_envs=65536)
    assert L.oc_gae_plan(ctypes.byref(b), 400, 1, 1, out, len(out)) == 0, L.oc_last_error().decode()
    return int(re.search(r"(\d+) steps per prefetch block", out.value.decode()).group(1))


def horizons():
    B = prefetch_block()
    return (1, 2, B - 1, B, B + 1, 2 * B + 1)


Case = collections.namedtuple("Case", "id n_envs n_steps done seat gamma lam last seed")


def _case(n, T, done, seat, seed, gamma=0.99, lam=0.98, last=True, tag=""):
    return Case("n%d-T%d-%s-%s%s" % (n, T, done, seat, tag), n, T, done, seat, gamma, lam, last, seed)


def _cases():
    out, i = [], 0
    Ts = horizons()
    for n in SIZES:  # every size at every horizon, the patterns taking turns
        for T in Ts:
            out.append(_case(n, T, DONE_PATTERNS[i % 6], SEAT_PATTERNS[(i // 6 + i) % 5], 100 + i))
            i += 1
    have = {(c.done, c.seat) for c in out if c.n_steps == Ts[-1]}
    for d in DONE_PATTERNS:  # every done pattern with every seat pattern, at more than two prefetch blocks
        for s in SEAT_PATTERNS:
            if (d, s) not in have:
                out.append(_case(65, Ts[-1], d, s, 100 + i))
            i += 1
    out.append(_case(65, Ts[-1], "random7", "episode", 300, last=False, tag="-nolast"))
    out.append(_case(65, Ts[-1], "random7", "episode", 301, gamma=1.0, tag="-gamma1"))
    out.append(_case(65, Ts[-1], "random7", "episode", 302, lam=0.0, tag="-lambda0"))
    out.append(_case(65, Ts[-1], "random7", "episode", 303, lam=1.0, tag="-lambda1"))
    out.append(_case(65, 400, "horizon5", "episode", 304))
    out.append(_case(65, 400, "none", "none", 305, tag="-long"))
    return tuple(out)


def done_pattern(kind, T, n, rng):
    t, e = np.arange(T)[:, None], np.arange(n)[None, :]
    if kind == "none":
        d = np.zeros((T, n), bool)
    elif kind == "every":
        d = np.ones((T, n), bool)
    elif kind == "first":
        d = np.broadcast_to(t == 0, (T, n))
    elif kind == "last":
        d = np.broadcast_to(t == T - 1, (T, n))
    elif kind == "horizon5":  # per-env staggered phases
        d = (t + e) % 5 == 4
    elif kind == "random7":
        d = rng.random((T, n)) < 1.0 / 7.0
    else:
        raise ValueError(kind)
    # (any non-zero byte reads as done)
    return np.where(d, rng.integers(1, 256, size=(T, n)), 0).astype(np.uint8)


def seat_pattern(kind, done, rng):
    T, n = done.shape
    draw = lambda size: rng.choice(np.array([0, 1, NO_SEAT], np.uint8), size=size)  # noqa: E731
    if kind == "none":
        return None
    if kind in ("all0", "all1"):
        return np.full((T, n), int(kind[-1]), np.uint8)
    if kind == "inconsistent":  # a seat that changes inside an episode: the header reads it step by step
        return draw((T, n))
    if kind == "episode":  # as the library seats: a new draw only behind a done step
        s = np.empty((T, n), np.uint8)
        s[0] = draw(n)
        for t in range(1, T):
            s[t] = np.where(done[t - 1] != 0, draw(n), s[t - 1])
        return s
    raise ValueError(kind)


def _mixed(rng, shape):
    """Numbers in +-50: quarter-integers (exact in f32) where a coin says so, uniform doubles (inexact in f32) elsewhere."""
    exact = rng.integers(-200, 201, size=shape) / 4.0
    exact = np.where(exact == FILL, FILL - 0.25, exact)  # (a done step's target is its reward: the fill itself is not drawn)
    return np.where(rng.random(shape) < 0.4, exact, rng.uniform(-50.0, 50.0, size=shape))


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """(rewards f64 [T, N, 2], values f32 [T, N, 2], done u8 [T, N], last_values f32 [N, 2] or None, seat u8 [T, N] or None) of a
    case, read-only."""
    rng = np.random.default_rng(c.seed)
    T, n = c.n_steps, c.n_envs
    rewards = _mixed(rng, (T, n, 2)).astype(np.float64)
    values = _mixed(rng, (T, n, 2)).astype(np.float32)
    last = _mixed(rng, (n, 2)).astype(np.float32) if c.last else None
    done = done_pattern(c.done, T, n, rng)
    seat = seat_pattern(c.seat, done, rng)
    # differences of quarter-integers meet every quarter-integer, the fill of the GPU tests' outputs among them: a reward whose
    # advantage or target would equal the fill moves by a quarter, until no result holds it
    for _ in range(20):
        adv, tgt = gae_f32(rewards, values, done, c.gamma, c.lam, last, seat)
        hit = (adv == FILL) | (tgt == FILL)
        if not hit.any():
            break
        rewards[hit] += 0.25
    else:
        raise AssertionError("%s: results equal to the fill remain" % c.id)
    for a in (rewards, values, last, done, seat):
        if a is not None:
            a.setflags(write=False)
    return rewards, values, done, last, seat


def gae_f32(rewards, values, done, gamma, lam, last_values=None, seat=None):
    """The header's arithmetic in np.float32, one numpy operation per rounding: (advantages, targets) f32 [T, N, 2]."""
    T, n = done.shape
    f = np.float32
    g = f(gamma)
    gl = f(f(gamma) * f(lam))
    adv, tgt = np.zeros((T, n, 2), f), np.zeros((T, n, 2), f)
    carried = np.zeros((n, 2), f)
    vn = np.zeros((n, 2), f) if last_values is None else np.asarray(last_values, f)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            r = rewards[t].astype(f)  # round to nearest
            v = values[t]
            d_end = r - v
            m = g * vn
            s = r + m
            d_run = s - v
            p = gl * carried
            a_run = d_run + p
            A = np.where(done[t][:, None] != 0, d_end, a_run)  # a select
            target = A + v
            if seat is not None:
                partner = seat[t][:, None] == np.arange(2, dtype=np.uint8)[None, :]
                A = np.where(partner, f(0), A)
                target = np.where(partner, f(0), target)
            assert A.dtype == f and target.dtype == f
            adv[t], tgt[t] = A, target
            carried, vn = A, v
    return adv, tgt


def gae_f64(rewards, values, done, gamma, lam, last_values=None, seat=None):
    """The same recurrence in float64 on the f32-rounded rewards, with the f32 constants g and gl widened, and the a-priori bound of
    |gae_f32 - gae_f64| for both outputs: (advantages, targets, bound_adv, bound_tgt) f64 [T, N, 2].
    The bound: every f32 operation returns its exact result times (1 + d), |d| <= U = 2^-24, so a result computed from operands
    that are off by e_x, e_y is off by at most e_x + e_y (scaled by a constant factor where one multiplies) plus U times (the
    magnitude of the f64 result + that incoming error).  Propagated through the header's five operations per step, and from step to
    step through the factor gl on the carried A; a done step and a partner's sample cut it as they cut the chain.  The f64 chain's
    own roundings (2^-53 each on the same magnitudes) are covered by the factor 1 + 2^-28 at the end."""
    T, n = done.shape
    g = float(np.float32(gamma))
    gl = float(np.float32(np.float32(gamma) * np.float32(lam)))
    adv, tgt = np.zeros((T, n, 2)), np.zeros((T, n, 2))
    b_adv, b_tgt = np.zeros((T, n, 2)), np.zeros((T, n, 2))
    carried, err = np.zeros((n, 2)), np.zeros((n, 2))
    vn = np.zeros((n, 2)) if last_values is None else np.asarray(last_values, np.float64)
    for t in range(T - 1, -1, -1):
        r = rewards[t].astype(np.float32).astype(np.float64)
        v = values[t].astype(np.float64)
        d_end = r - v
        e_end = U * np.abs(d_end)
        m = g * vn
        e_m = U * np.abs(m)
        s = r + m
        e_s = e_m + U * (np.abs(s) + e_m)
        d_run = s - v
        e_d = e_s + U * (np.abs(d_run) + e_s)
        p = gl * carried
        e_p = gl * err + U * (np.abs(p) + gl * err)
        a_run = d_run + p
        e_a = e_d + e_p + U * (np.abs(a_run) + e_d + e_p)
        is_done = done[t][:, None] != 0
        A = np.where(is_done, d_end, a_run)
        e_A = np.where(is_done, e_end, e_a)
        target = A + v
        e_T = e_A + U * (np.abs(target) + e_A)
        if seat is not None:
            partner = seat[t][:, None] == np.arange(2, dtype=np.uint8)[None, :]
            A, target = np.where(partner, 0.0, A), np.where(partner, 0.0, target)
            e_A, e_T = np.where(partner, 0.0, e_A), np.where(partner, 0.0, e_T)
        adv[t], tgt[t], b_adv[t], b_tgt[t] = A, target, e_A, e_T
        carried, err, vn = A, e_A, v
    k = 1.0 + 2.0 ** -28
    return adv, tgt, b_adv * k, b_tgt * k


def learner_mask(done, seat):
    """[T, N, 2] bool: the entries that are learner samples (everything without seats)."""
    T, n = done.shape
    if seat is None:
        return np.ones((T, n, 2), bool)
    return seat[:, :, None] != np.arange(2, dtype=np.uint8)[None, None, :]


def moments_f64(adv, done, seat, lo=0, hi=None):
    """(count, sum A, sum A^2, sum |A|) in float64 over the learner samples of envs [lo, hi)."""
    mask = learner_mask(done, seat)[:, lo:hi]
    x = adv[:, lo:hi].astype(np.float64)[mask]
    return int(mask.sum()), float(x.sum()), float((x * x).sum()), float(np.abs(x).sum())


def reference_of(c):
    """gae_f32 of a case, computed once and shared, read-only."""
    return _reference_of(c)


@functools.lru_cache(maxsize=None)
def _reference_of(c):
    rewards, values, done, last, seat = arrays_of(c)
    adv, tgt = gae_f32(rewards, values, done, c.gamma, c.lam, last, seat)
    adv.setflags(write=False)
    tgt.setflags(write=False)
    return adv, tgt


def first_done(done):
    """[N] the first step of every env that is done, T where there is none."""
    T = done.shape[0]
    return np.where((done != 0).any(0), (done != 0).argmax(0), T)


def poisoned(c):
    """The arrays of a case with NaN in everything behind each env's first done step — values[t + 1 ..], rewards[t + 1 ..], the last
    values — and [T, N] bool: the steps whose outputs must not change (those at or before that done step; every step of an env that
    is never done, which is left clean)."""
    rewards, values, done, last, seat = arrays_of(c)
    T, n = done.shape
    fd = first_done(done)
    later = np.arange(T)[:, None] > fd[None, :]
    rewards, values = rewards.copy(), values.copy()
    rewards[later] = np.nan
    values[later] = np.nan
    if last is not None:
        last = last.copy()
        last[fd < T] = np.nan
    return (rewards, values, done, last, seat), ~later


CASES = _cases()
