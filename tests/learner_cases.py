"""The cases of oc_adam_step and oc_ppo_update (include/oc_amd.h: OcAdam, OcPpoUpdate; csrc/adam.hpp, csrc/update_chain.hpp) and two
numpy statements of the step: `adam_f32`, the header's operations one by one — the order of the norm's sum included —, which the
device must equal as BIT PATTERNS, and `adam_f64`, the reference: the same step in float64 on the same float32 inputs (the
hyperparameters widened from float32, the norm a plain float64 sum).  numpy only; imported like helpers.py.

A case is a shape, a pattern and three consecutive steps, so that moments and clock carry; a pattern says what the gradients of a
step are and what d_grad_scale is.

Errors.  rel(x, ref) = max_i |x_i - ref_i| / max_i |ref_i| over the flat concatenation of the eight arrays (0 where both are zeros):
an error relative to the largest element, because a moment that cancels to nearly nothing has no relative accuracy of its own.
F32_ERROR is the largest rel of adam_f32's parameters and moments against adam_f64's over every step of every case, measured on the
CPU (tests/test_host_learner.py measures it again); the device through another path (torch's gradients, torch's order of
operations) is held to DEVICE_FACTOR times it, the project's convention.

The bound of G7 (one PPOLearner.update against the float64 chain).  With zero moments the first Adam step moves parameter i by
  delta_i = -lr * f(c g_i),  f(x) = x / (|x| + eps)       (the bias corrections cancel: m^ = g, sqrt(v^) = |g|)
and f' = eps / (|x| + eps)^2 <= eps / (max(|x| - d, 0) + eps)^2 on [x - d, x + d].  A device gradient that lies within
d_i = DEVICE_FACTOR * policy_cases.F32_ERROR * scale_i of the float64 one (policy_cases' scaled error; here without clipping, c = 1)
therefore moves the step by at most lr * d_i * eps / (max(|g_i| - d_i, 0) + eps)^2, and never by more than 2 lr (|f| < 1); the float32
Adam adds DEVICE_FACTOR * F32_ERROR * max |p|, H1's measure of the parameters.  `update_bound` is that sum."""
import collections
import functools

import numpy as np

NAMES = ("w1", "b1", "w2", "b2", "wp", "bp", "wv", "bv")
LANES = 256
F32_ERROR = 2.7e-7   # measured 2.68e-7 (136_64_64-scale_count, third step): see test_h1_the_recorded_error_is_the_measured_one
DEVICE_FACTOR = 4
FILL = -7.0          # guard rows
CLOCK0 = np.array([0.0, 1.0, 1.0, 0.0])
SHAPES = ((56, 1, 1), (96, 33, 17), (96, 64, 64), (136, 64, 64))
PATTERNS = ("below", "above", "off", "zero", "nan", "inf", "scale0", "scale_count")
STEPS = 3

Hyper = collections.namedtuple("Hyper", "lr beta1 beta2 eps max_grad_norm")  # max_grad_norm None: no clipping
Case = collections.namedtuple("Case", "id in_dim h1 h2 pattern hyper seed")
Step = collections.namedtuple("Step", "grads scale good")  # eight f32 arrays; the f64 d_grad_scale or None; whether the step is taken


def shapes(in_dim, h1, h2):
    return ((in_dim, h1), (h1,), (h1, h2), (h2,), (h2, 6), (6,), (h2,), (1,))


def n_of(in_dim, h1, h2):
    return sum(int(np.prod(s)) for s in shapes(in_dim, h1, h2))


def _cases():
    out = []
    for k, (in_dim, h1, h2) in enumerate(SHAPES):
        for j, pattern in enumerate(PATTERNS):
            clip = {"below": 10.0, "above": 0.1, "off": None, "zero": 0.1, "nan": 0.1, "inf": None, "scale0": 0.5, "scale_count": 0.1}[pattern]
            # two learning rates taking turns, and other betas and eps on every other shape
            hyper = Hyper(1e-3 if j % 2 == 0 else 5e-5, 0.9 if k % 2 == 0 else 0.5, 0.999 if k % 2 == 0 else 0.9, 1e-8 if k % 2 == 0 else 1e-5, clip)
            out.append(Case("%d_%d_%d-%s" % (in_dim, h1, h2, pattern), in_dim, h1, h2, pattern, hyper, 900 + 8 * k + j))
    return tuple(out)


CASES = _cases()


def split(flat, in_dim, h1, h2):
    out, at = [], 0
    for s in shapes(in_dim, h1, h2):
        size = int(np.prod(s))
        out.append(flat[at:at + size].reshape(s))
        at += size
    return out


def flat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays])


@functools.lru_cache(maxsize=None)
def inputs_of(c):
    """(the eight float32 parameter arrays, the STEPS steps), read-only.  The gradients of pattern
      below / above   N(0, 1e-3) / N(0, 1): a norm far below max_grad_norm = 10 / far above 0.1
      off             N(0, 1e-2), no clipping
      zero            a drawn step, then all-zero gradients twice (the momentum alone moves the parameters)
      nan / inf       the second step has one NaN / one +inf (in w2, or in the only array that is long enough)
      scale0          raw gradients N(0, 1) with d_grad_scale = 1 / 37; 0 in the second step
      scale_count     raw gradients N(0, 1) with d_grad_scale = 1 / 37, 1 / 38, 1 / 39"""
    rng = np.random.default_rng(c.seed)
    dims = (c.in_dim, c.h1, c.h2)
    n = n_of(*dims)
    params = split((0.3 * rng.standard_normal(n)).astype(np.float32), *dims)
    sigma = {"below": 1e-3, "above": 1.0, "off": 1e-2, "zero": 1e-2, "nan": 1e-2, "inf": 1e-2, "scale0": 1.0, "scale_count": 1.0}[c.pattern]
    steps = []
    for t in range(STEPS):
        g = (sigma * rng.standard_normal(n)).astype(np.float32)
        scale, good = None, True
        if c.pattern == "zero" and t > 0:
            g[:] = 0
        if c.pattern in ("nan", "inf") and t == 1:
            g[(n * 2) // 3] = np.nan if c.pattern == "nan" else np.inf
            good = False
        if c.pattern in ("scale0", "scale_count"):
            scale = 1.0 / (37 + t)
        if c.pattern == "scale0" and t == 1:
            scale, good = 0.0, False
        steps.append(Step(tuple(split(g, *dims)), scale, good))
    for a in list(params) + [g for s in steps for g in s.grads]:
        a.setflags(write=False)
    return tuple(params), tuple(steps)


State = collections.namedtuple("State", "params m v clock")  # three flat arrays and the clock [4] f64


def state0(params, dtype=np.float32):
    p = flat(params).astype(dtype)
    return State(p, np.zeros_like(p), np.zeros_like(p), CLOCK0.copy())


def norm_f32(g):
    """The header's norm of the flat float32 gradients: the lanes' sums in ascending i, the fixed tree, (float)sqrt."""
    q = g.astype(np.float64)
    q = q * q
    pad = (-len(q)) % LANES
    rows = np.concatenate([q, np.zeros(pad)]).reshape(-1, LANES)  # (+0.0 adds nothing to a sum that is never -0.0)
    s = np.zeros(LANES)
    for row in rows:
        s = s + row
    k = LANES // 2
    while k >= 1:
        s[:k] = s[:k] + s[k:2 * k]
        k //= 2
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.sqrt(s[0]))


def adam_f32(state, grads, hyper, scale=None):
    """(the State after the step, info [4] f64): include/oc_amd.h's arithmetic (OcAdam), one numpy operation per rounding."""
    f32, f64 = np.float32, np.float64
    with np.errstate(all="ignore"):
        gs = f32(f64(scale)) if scale is not None else f32(1)
        g = flat(grads).astype(f32) * gs
        norm = norm_f32(g)
        mg = f32(hyper.max_grad_norm) if hyper.max_grad_norm is not None else f32(0)
        clip = bool(np.isfinite(mg) and mg > 0)
        c = f32(1)
        if clip:
            c = min(mg / (norm + f32(1e-6)), f32(1))
        if not np.isfinite(norm) or (scale is not None and f64(scale) == 0.0):
            clock = state.clock.copy()
            clock[3] += 1.0
            return State(state.params, state.m, state.v, clock), np.array([f64(norm), 0.0, f64(gs), 1.0])
        if clip:
            g = g * c
        beta1, beta2, eps, lr = f32(hyper.beta1), f32(hyper.beta2), f32(hyper.eps), f32(hyper.lr)
        steps, p1, p2, skipped = state.clock
        p1, p2 = p1 * f64(beta1), p2 * f64(beta2)
        bc1, bc2s = 1.0 - p1, np.sqrt(1.0 - p2)
        step_size, rbc2s = f32(f64(lr) / bc1), f32(bc2s)
        omb1, omb2 = f32(1) - beta1, f32(1) - beta2
        m = state.m + (g - state.m) * omb1
        v = state.v * beta2 + (g * g) * omb2
        den = np.sqrt(v) / rbc2s + eps
        p = state.params - step_size * (m / den)
        assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32 and den.dtype == f32 and isinstance(c, f32)
    return State(p, m, v, np.array([steps + 1.0, p1, p2, skipped])), np.array([f64(norm), f64(c), f64(gs), 0.0])


def adam_f64(state, grads, hyper, scale=None):
    """The reference: the same step in float64 (state: float64 arrays), the float32 inputs and hyperparameters widened."""
    f32, f64 = np.float32, np.float64
    with np.errstate(all="ignore"):
        gs = f64(f32(f64(scale))) if scale is not None else 1.0
        g = flat(grads).astype(f64) * gs
        norm = np.sqrt((g * g).sum())
        mg = f64(f32(hyper.max_grad_norm)) if hyper.max_grad_norm is not None else 0.0
        clip = bool(np.isfinite(mg) and mg > 0)
        c = min(mg / (norm + f64(f32(1e-6))), 1.0) if clip else 1.0
        if not np.isfinite(norm) or (scale is not None and f64(scale) == 0.0):
            clock = state.clock.copy()
            clock[3] += 1.0
            return State(state.params, state.m, state.v, clock), np.array([norm, 0.0, gs, 1.0])
        g = g * c
        beta1, beta2, eps, lr = (f64(f32(x)) for x in (hyper.beta1, hyper.beta2, hyper.eps, hyper.lr))
        steps, p1, p2, skipped = state.clock
        p1, p2 = p1 * beta1, p2 * beta2
        m = state.m + (g - state.m) * (1.0 - beta1)
        v = state.v * beta2 + (g * g) * (1.0 - beta2)
        den = np.sqrt(v) / np.sqrt(1.0 - p2) + eps
        p = state.params - (lr / (1.0 - p1)) * (m / den)
    return State(p, m, v, np.array([steps + 1.0, p1, p2, skipped])), np.array([norm, c, gs, 0.0])


@functools.lru_cache(maxsize=None)
def trajectory_of(c):
    """[(State, info)] after each of the case's steps by adam_f32, computed once and shared, read-only."""
    params, steps = inputs_of(c)
    s, out = state0(params), []
    for st in steps:
        s, info = adam_f32(s, st.grads, c.hyper, st.scale)
        for a in tuple(s) + (info,):
            a.setflags(write=False)
        out.append((s, info))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """The same by adam_f64, from the same float32 parameters."""
    params, steps = inputs_of(c)
    s, out = state0(params, np.float64), []
    for st in steps:
        s, info = adam_f64(s, st.grads, c.hyper, st.scale)
        out.append((s, info))
    return tuple(out)


def rel(x, ref):
    x, ref = np.asarray(x, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    top = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(x - ref).max() if ref.size else 0.0
    return 0.0 if err == 0.0 else float(err / top) if top > 0 else float("inf")


def state_error(s, ref):
    """The largest rel of parameters, first and second moments of State s against State ref"""
    return max(rel(s.params, ref.params), rel(s.m, ref.m), rel(s.v, ref.v))


def update_bound(g64, scale, lr, eps, p64):
    """G7's bound of |device step - float64 step| per flat element (the module's docstring): g64 the float64 gradients, scale the
    sums of |input| |delta| that policy_cases' scaled error is relative to, both already divided by the count."""
    import policy_cases as PC

    d = PC.DEVICE_FACTOR * PC.F32_ERROR * scale
    slope = eps / (np.maximum(np.abs(g64) - d, 0.0) + eps) ** 2
    return np.minimum(2.0 * lr, lr * d * slope) + DEVICE_FACTOR * F32_ERROR * np.abs(p64).max()
