"""oc_ppo_loss's case list and two numpy restatements of the arithmetic include/oc_amd.h states (OcPpoLoss): loss_f32, the header's
f32 operations one by one, and loss_f64, the reference — the same terms, sums, stats and analytic gradients in float64 on the same
f32 inputs (the f32 constants lo, hi and the coefficients widened).  numpy only; imported like helpers.py.

Tolerances, measured here on the CPU over the whole case list (test_host_ppo_loss.py measures them again and holds them to these):
  F32_ERROR   the largest |loss_f32 - loss_f64| / max(1, |loss_f64|) of any term or gradient outside the bands: expf of a difference
              of two log-probabilities carries the error of both.
  DEVICE_TOL  4 x F32_ERROR: what the device is held to.  Its expf / logf differ from numpy's by a few ulp, which the ratio
              amplifies the same way.
  RATIO_BAND, VF_BAND   4 x the largest f32-restatement error of the ratio and of vf (relative to max(1, |x|)): a gradient is
              compared only where the f64 ratio is further than RATIO_BAND from lo and hi (the logits' gradients) and the f64 vf
              further than VF_BAND * max(1, vf_clip_param) from vf_clip_param (the values' gradient); at most BAND_CAP of a case's
              rows may lie in a band."""
import collections
import functools
import types

import numpy as np

F32_ERROR = 1.39e-6  # measured 1.382e-6 (grad_logits); the ratio alone 1.149e-6
DEVICE_TOL = 4 * F32_ERROR
RATIO_ERROR, VF_ERROR = 1.15e-6, 1.77e-7  # measured 1.149e-6 and 1.766e-7
RATIO_BAND, VF_BAND = 4 * RATIO_ERROR, 4 * VF_ERROR
BAND_CAP = 1e-3
FILL = -7.0  # what the output arrays of a GPU test start as: no result of a case equals it (test_host_ppo_loss.py checks)
NO_SEAT = 255
SIZES = (1, 63, 64, 65, 255, 256, 257, 488)
STATS = ("count", "total", "policy_loss", "vf_loss", "entropy", "kl", "clip_frac", "inv_count")

Case = collections.namedtuple("Case", "id M mode first seat moments old terms clip vf_clip vf_coeff ent kl neg_inf seed")
HYPER = ((0.05, 10.0, 1e-4, 0.2, 0.2), (0.2, 10.0, 0.5, 0.0, 0.0), (0.05, 0.5, 0.5, 0.2, 0.0), (0.2, 10.0, 1e-4, 0.0, 0.2))


@functools.lru_cache(maxsize=None)
def partial_samples():
    """P, the minibatch rows per partial, read from oc_ppo_loss_plan's words (no device needed)."""
    from overcooked_ai_amd.ppo_loss import partial_samples as P

    return P()


def _case(M, mode, i, seat, tag="", **kw):
    clip, vf_clip, vf_coeff, ent, kl = HYPER[i % 4]
    v = dict(first=0 if mode != "contiguous" else 3 + 2 * i + (i & 1), moments=bool(i & 1), old=bool(i & 2), terms=bool(i & 4) or i % 3 == 0,
             clip=clip, vf_clip=vf_clip, vf_coeff=vf_coeff, ent=ent, kl=kl, neg_inf=False, seed=500 + i)
    v.update(kw)
    if not v["old"]:
        v["kl"] = 0.0
    name = "M%d-%s-seat_%s%s%s%s%s" % (M, mode, seat, "-mom" if v["moments"] else "", "-old" if v["old"] else "",
                                      "-terms" if v["terms"] else "", tag)
    return Case(name, M, mode, v["first"], seat, v["moments"], v["old"], v["terms"], v["clip"], v["vf_clip"], v["vf_coeff"], v["ent"],
                v["kl"], v["neg_inf"], v["seed"])


def _cases():
    out, i = [], 0
    seats = ("none", "all0", "mixed")
    for M in SIZES:  # every size contiguous (first_sample > 0) and indexed, the options taking turns
        for mode in ("contiguous", "indexed"):
            out.append(_case(M, mode, i, seats[i % 3]))
            i += 1
    big = 65 * partial_samples() + 3  # more partials than the finishing wavefront has lanes
    out.append(_case(big, "indexed", 20, "mixed", moments=True, old=True, terms=True, tag="-big"))
    out.append(_case(257, "all_out", 21, "all0", terms=True, tag="-count0"))  # every row a partner's sample
    out.append(_case(65, "all_out", 22, "all0", moments=True, old=True, kl=0.2, terms=True, tag="-count0"))
    out.append(_case(488, "indexed", 23, "mixed", moments=True, old=True, terms=True, neg_inf=True, kl=0.2, tag="-neginf"))
    out.append(_case(257, "contiguous", 24, "none", terms=True, neg_inf=True, tag="-neginf"))
    out.append(_case(488, "contiguous", 25, "mixed", moments=True, terms=True, tag="-split"))  # (one call, and 200 + 288)
    out.append(_case(488, "contiguous", 26, "none", moments=False, old=False, terms=False, first=0, tag="-plain"))
    tile = partial_samples() // 4  # a workgroup walks four tiles of rows: one row into the fourth, and one row into a second workgroup
    out.append(_case(3 * tile + 1, "contiguous", 27, "mixed", moments=True, old=True, terms=True, tag="-tiles"))
    out.append(_case(4 * tile + 1, "indexed", 28, "mixed", terms=True, tag="-tiles"))
    return tuple(out)


def _log_softmax64(l):
    l = l.astype(np.float64)
    d = l - l.max(-1, keepdims=True)
    return d - np.log(np.exp(d).sum(-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """The arrays of a case, read-only, as a namespace: the batch side over S samples (actions u8 [S], logp_old, advantages, targets
    f32 [S], seat u8 [S / 2] or None, logits_old f32 [S, 6] or None, moments f64 [3] or None), the minibatch side (logits f32 [M, 6],
    values f32 [M], index i32 [M] or None, first) and sample i64 [M], the sample of every row (an out-of-range one as the index has it).
    Logits are N(0, 2), the old logits a perturbation of them by N(0, clip_param) — 0.05 under a clip of 0.05, 0.2 under one of 0.2 —,
    so about a third of the ratios lie outside the clip in every case; values are the targets + N(0, 2), so both sides of
    vf_clip_param occur."""
    rng = np.random.default_rng(c.seed)
    M = c.M
    S = c.first + M + 38 if c.mode == "contiguous" else M + 10
    S += S & 1
    logits_all = (rng.standard_normal((S, 6)) * 2).astype(np.float32)
    actions = rng.integers(0, 6, S).astype(np.uint8)
    if c.neg_inf:  # a -inf logit on an action not taken, in a tenth of the samples
        rows = np.nonzero(rng.random(S) < 0.1)[0]
        logits_all[rows, (actions[rows] + 1 + rng.integers(0, 5, len(rows))) % 6] = -np.inf
    with np.errstate(invalid="ignore"):
        old = (logits_all + c.clip * rng.standard_normal((S, 6))).astype(np.float32)
        logp_old = np.take_along_axis(_log_softmax64(old), actions[:, None].astype(np.int64), 1)[:, 0].astype(np.float32)
    bad = rng.random(S) < 0.03  # the sampler's invalid rows
    if S >= 60:
        bad[rng.integers(0, S, 2)] = True
    actions[bad] = 255
    logp_old[bad] = np.nan
    adv = (0.3 + 1.5 * rng.standard_normal(S)).astype(np.float32)
    targets = (3 * rng.standard_normal(S)).astype(np.float32)
    seat = {"none": None, "all0": np.zeros(S // 2, np.uint8), "all1": np.ones(S // 2, np.uint8),
            "mixed": rng.choice(np.array([0, 1, NO_SEAT], np.uint8), size=S // 2)}[c.seat]
    index = None
    if c.mode == "contiguous":
        sample = c.first + np.arange(M, dtype=np.int64)
    elif c.mode == "all_out":  # player 0's samples only, under seats that make every one of them the partner's
        sample = 2 * rng.integers(0, S // 2, M).astype(np.int64)
    else:  # a permutation with repeats and a few entries outside 0 .. S - 1
        sample = rng.permutation(S)[:M].astype(np.int64)
        if M >= 8:
            rep = rng.integers(0, M, max(M // 20, 2))
            sample[rep] = sample[(rep + 3) % M]
            out_of_range = np.array([-1, S, S + 5, -2 ** 31, 2 ** 31 - 1][:max(2, min(5, M // 12))], np.int64)
            sample[rng.choice(M, len(out_of_range), replace=False)] = out_of_range
    if c.mode != "contiguous":
        index = sample.astype(np.int32)
    inside = (sample >= 0) & (sample < S)
    at = np.where(inside, sample, 0)
    logits = np.where(inside[:, None], logits_all[at], (rng.standard_normal((M, 6)) * 2).astype(np.float32)).astype(np.float32)
    values = (targets[at] + 2 * rng.standard_normal(M)).astype(np.float32)
    moments = None
    if c.moments:  # as oc_gae leaves them: over the learner samples of the whole batch
        learner = np.ones(S, bool) if seat is None else seat[np.arange(S) >> 1] != (np.arange(S) & 1)
        x = adv.astype(np.float64)[learner]
        moments = np.array([learner.sum(), x.sum(), (x * x).sum()], np.float64)
    a = types.SimpleNamespace(S=S, M=M, actions=actions, logp_old=logp_old, advantages=adv, targets=targets, seat=seat,
                              logits_old=old if c.old else None, moments=moments, logits=logits, values=values, index=index,
                              first=c.first, sample=sample)
    for x in vars(a).values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a


Result = collections.namedtuple("Result", "terms grad_logits grad_values ratio vf left_out outside sums stats")


def _softmax(l):
    m = l.max(-1, keepdims=True)
    d = l - m
    w = np.exp(d)
    S = w[:, 0]
    for i in range(1, 6):
        S = S + w[:, i]
    lp = d - np.log(S)[:, None]
    p = w / S[:, None]
    return lp, p


def _sum_from_first(t):
    acc = t[:, 0]
    for i in range(1, 6):
        acc = acc + t[:, i]
    return acc


def _loss(c, a, f):
    """The header's arithmetic in dtype f, one numpy operation per rounding; the sums and stats in float64."""
    f32 = np.float32
    lo, hi = f(f32(1) - f32(c.clip)), f(f32(1) + f32(c.clip))
    vf_clip, vf_coeff, ent, klc = f(f32(c.vf_clip)), f(f32(c.vf_coeff)), f(f32(c.ent)), f(f32(c.kl))
    s = a.sample
    inside = (s >= 0) & (s < a.S)
    at = np.where(inside, s, 0)
    act = a.actions[at]
    left_out = ~inside | (act > 5)
    if a.seat is not None:
        left_out |= a.seat[at >> 1] == (at & 1)
    with np.errstate(all="ignore"):
        lp, p = _softmax(a.logits.astype(f))
        logp = np.take_along_axis(lp, np.minimum(act, 5)[:, None].astype(np.int64), 1)[:, 0]
        lpo = a.logp_old[at].astype(f)
        ratio = np.exp(logp - lpo)
        Ah = a.advantages[at].astype(f)
        if a.moments is not None and a.moments[0] >= 1:
            n, m1, m2 = (float(x) for x in a.moments)
            mean = m1 / n
            std = max(np.sqrt(max(m2 / n - mean * mean, 0.0)), 1e-4)
            Ah = ((a.advantages[at].astype(np.float64) - mean) / std).astype(f)  # (rounded to f32 by the restatement, not by the reference)
        s1 = ratio * Ah
        s2 = np.minimum(np.maximum(ratio, lo), hi) * Ah
        surr = np.minimum(s1, s2)
        H = -_sum_from_first(np.where(p == 0, f(0), p * lp))
        dv = a.values.astype(f) - a.targets[at].astype(f)
        vf = dv * dv
        vfc = np.minimum(vf, vf_clip)
        if a.logits_old is not None:
            lq, q = _softmax(a.logits_old[at].astype(f))
            kl = _sum_from_first(np.where(q == 0, f(0), q * (lq - lp)))
        else:
            kl = lpo - logp
        g = np.where(s1 <= s2, -s1, f(0))
        onehot = (np.arange(6)[None, :] == act[:, None]).astype(f)
        gl = g[:, None] * (onehot - p) + np.where(p == 0, f(0), (ent * p) * (lp + H[:, None]))
        if a.logits_old is not None:
            gl = gl + klc * (p - q)
        gv = vf_coeff * np.where(vf <= vf_clip, f(2) * dv, f(0))
        outside = (ratio < lo) | (ratio > hi)
    terms = np.where(left_out[:, None], f(0), np.stack([surr, vfc, H, kl], 1))
    gl = np.where(left_out[:, None], f(0), gl)
    gv = np.where(left_out, f(0), gv)
    assert terms.dtype == f and gl.dtype == f and gv.dtype == f and ratio.dtype == f
    keep = ~left_out
    t64 = terms.astype(np.float64)[keep]
    sums = np.array([keep.sum(), -t64[:, 0].sum(), t64[:, 1].sum(), t64[:, 2].sum(), t64[:, 3].sum(), (outside & keep).sum()], np.float64)
    return Result(terms, gl, gv, ratio, vf, left_out, outside & keep, sums, stats_of(sums, c))


def stats_of(sums, c):
    """d_stats of the six sums, as k_ppo_loss_stats derives them."""
    n = sums[0]
    if not n > 0:
        return np.zeros(8)
    f32 = np.float32
    policy, vf, H, kl = (sums[i] / n for i in (1, 2, 3, 4))
    total = ((policy + float(f32(c.vf_coeff)) * vf) - float(f32(c.ent)) * H) + float(f32(c.kl)) * kl
    return np.array([n, total, policy, vf, H, kl, sums[5] / n, 1.0 / n], np.float64)


def loss_f32(c, a=None):
    return _loss(c, arrays_of(c) if a is None else a, np.float32)


def loss_f64(c, a=None):
    return _loss(c, arrays_of(c) if a is None else a, np.float64)


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """loss_f64 of a case, computed once and shared, read-only."""
    r = loss_f64(c)
    for x in r:
        x.setflags(write=False)
    return r


def bands(c, ref=None):
    """(rows whose f64 ratio is within RATIO_BAND of lo or hi, rows whose f64 vf is within VF_BAND of vf_clip_param) among the
    rows that are not left out: bool [M] each."""
    ref = reference_of(c) if ref is None else ref
    lo, hi = float(np.float32(1) - np.float32(c.clip)), float(np.float32(1) + np.float32(c.clip))
    vf_clip = float(np.float32(c.vf_clip))
    with np.errstate(invalid="ignore"):
        near_ratio = (np.abs(ref.ratio - lo) <= RATIO_BAND) | (np.abs(ref.ratio - hi) <= RATIO_BAND)
        near_vf = np.abs(ref.vf - vf_clip) <= VF_BAND * max(1.0, vf_clip)
    return near_ratio & ~ref.left_out, near_vf & ~ref.left_out


def rel_error(got, ref, rows=None):
    """The largest |got - ref| / max(1, |ref|) over rows (all of them by default); 0 where there is none.  Equal infinities agree."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.where(got == ref, 0.0, np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))
    return float(err.max())  # (a NaN where the reference has a number is an error of NaN, and fails every comparison)


def poisoned(c):
    """The arrays of a case with NaN in every input of the left-out samples — their logp_old, advantage, target and old logits on the
    batch side, the logits and values of the rows that name them or name no sample — as a namespace of writable copies."""
    a = arrays_of(c)
    b = types.SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(a).items()})
    s_all = np.arange(a.S)
    out = a.actions > 5
    if a.seat is not None:
        out |= a.seat[s_all >> 1] == (s_all & 1)
    for x in (b.logp_old, b.advantages, b.targets):
        x[out] = np.nan
    if b.logits_old is not None:
        b.logits_old[out] = np.nan
    rows = reference_of(c).left_out
    b.logits[rows] = np.nan
    b.values[rows] = np.nan
    return b


CASES = _cases()
