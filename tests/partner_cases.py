"""The cases of oc_partner_logits (include/oc_amd.h: OcDensePolicy, OcPartnerSeats; csrc/partner.hpp: k_partner_logits), the seating
stream restated twice, and the network's float64 reference with its a-priori error bound.

The seating stream, restated: `seats` (vectorised numpy on sample_cases.philox4x32_10) and `seats_by_the_header` (one env at a time
on Python integers and the oracle's Philox, written from the header's sentences).  `reseat` applies a done mask.

The network: `mlp_f64` is the reference — float64 numpy on the float32 inputs and weights — and `mlp_bound` the forward error bound
that holds for ANY float32 evaluation of it, whatever the summation order, with or without fused multiply-add (Higham, Accuracy and
Stability of Numerical Algorithms, §3.1: an inner product of n terms plus a bias has |error| <= gamma_{n+1} * (|w|^T |x| + |b|),
gamma_n = n u / (1 - n u), u = 2^-24), pushed through the layers:
    e1 = gamma_{in_dim+1} (|W1|^T |x| + |b1|)
    e2 = gamma_{h1+1} (|W2|^T (|h1*| + e1) + |b2|) + |W2|^T e1          h1* = the reference's hidden activations
    e3 = gamma_{h2+1} (|W3|^T (|h2*| + e2) + |b3|) + |W3|^T e2
(ReLU is 1-Lipschitz: an input error passes through it no larger.)  Nothing in it comes from a result of the code under test.

Weights are Glorot-uniform from a seeded numpy generator; features are real ones: the env's own feature buffer after STEPS_BEFORE
random steps from drawn start states (tests/test_gpu_partner.py)."""
from collections import namedtuple

import numpy as np

import sample_cases as SC

SEAT_TWEAK = 0x53454154  # "SEAT"
NO_SEAT = 255
U = 2.0 ** -24
STEPS_BEFORE = 10
M64 = 2**64 - 1


# ------------------------------------------------------------------------------------------ the seating stream, twice
def seat_words(seed, env_offset, step, n, drop=None):
    """(r0, r1) uint32 [n]: words 0 and 1 of the seating block of envs 0..n-1.  drop: None, or one part of the counters a kernel could
    lose — "t_hi", "g_hi", "carry" (g_hi taken from env_offset alone), "seed_hi", "tweak"."""
    assert drop in (None, "t_hi", "g_hi", "carry", "seed_hi", "tweak")
    seed, step, env_offset = int(seed) & M64, int(step) & M64, int(env_offset) & M64
    g = np.uint64(env_offset) + np.arange(n, dtype=np.uint64)
    g_lo, g_hi = g & SC.M32, g >> np.uint64(32)
    if drop == "g_hi":
        g_hi = np.zeros_like(g_hi)
    if drop == "carry":
        g_hi = np.full_like(g_hi, env_offset >> 32)
    t_lo, t_hi = step & 0xFFFFFFFF, 0 if drop == "t_hi" else step >> 32
    k1 = (0 if drop == "seed_hi" else seed >> 32) ^ (0 if drop == "tweak" else SEAT_TWEAK)
    r = SC.philox4x32_10(np.full(n, t_lo, np.uint64), g_lo, g_hi, np.full(n, t_hi, np.uint64), seed & 0xFFFFFFFF, k1)
    return r[0], r[1]


def seats(seed, env_offset, step, n, bc_factor, drop=None):
    """uint8 [n]: the seat every env draws when it is reseated at `step`"""
    r0, r1 = seat_words(seed, env_offset, step, n, drop)
    u = (r0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(u < np.float32(bc_factor), (r1 & np.uint32(1)).astype(np.uint8), np.uint8(NO_SEAT)).astype(np.uint8)


def reseat(seat, done, seed, env_offset, step, bc_factor):
    """The seats after a call: done None — every env is reseated; else those whose done byte is not 0, the others keep theirs."""
    drawn = seats(seed, env_offset, step, len(seat), bc_factor)
    return drawn if done is None else np.where(np.asarray(done) != 0, drawn, seat).astype(np.uint8)


def seats_by_the_header(seed, env_offset, step, n, bc_factor):
    """The header's sentences, one env at a time, on Python integers."""
    from oracle import oracle as O

    out = np.empty(n, np.uint8)
    t = step % 2**64
    for e in range(n):
        g = (env_offset + e) % 2**64
        r = O.philox4x32_10([t % 2**32, g % 2**32, g // 2**32, t // 2**32], [seed % 2**32, (seed // 2**32) ^ SEAT_TWEAK])
        u = float(np.float32(r[0] >> 8) * np.float32(2.0 ** -24))
        out[e] = (r[1] & 1) if u < float(np.float32(bc_factor)) else NO_SEAT
    return out


# ------------------------------------------------------------------------------------------ the network
def glorot(seed, in_dim, h1, h2):
    """(w1, b1, w2, b2, w3, b3) float32, Keras layout: Glorot-uniform kernels; the biases too are drawn (a trained model's are not 0)."""
    rng = np.random.default_rng([seed, in_dim, h1, h2])
    out = []
    for fan_in, fan_out in ((in_dim, h1), (h1, h2), (h2, 6)):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        out += [rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), rng.uniform(-0.5, 0.5, (fan_out,)).astype(np.float32)]
    return tuple(out)


def mlp_f64(x, weights):
    """float64 [..., 6] logits of float32 rows x [..., in_dim], and the hidden activations (h1*, h2*)"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float32).astype(np.float64) for a in weights)
    x = np.asarray(x, np.float32).astype(np.float64)
    a1 = np.maximum(x @ w1 + b1, 0.0)
    a2 = np.maximum(a1 @ w2 + b2, 0.0)
    return a2 @ w3 + b3, (a1, a2)


def gamma(n):
    return n * U / (1.0 - n * U)


def mlp_bound(x, weights):
    """float64 [..., 6]: the forward error bound of the module docstring for every logit of rows x"""
    w1, b1, w2, b2, w3, b3 = (np.abs(np.asarray(a, np.float32).astype(np.float64)) for a in weights)
    _, (a1, a2) = mlp_f64(x, weights)
    ax = np.abs(np.asarray(x, np.float32).astype(np.float64))
    e1 = gamma(w1.shape[0] + 1) * (ax @ w1 + b1)
    e2 = gamma(w2.shape[0] + 1) * ((np.abs(a1) + e1) @ w2 + b2) + e1 @ w2
    return gamma(w3.shape[0] + 1) * ((np.abs(a2) + e2) @ w3 + b3) + e2 @ w3


def mlp_f32(x, weights):
    """A float32 evaluation (np.matmul: some other summation order than the kernel's)"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float32) for a in weights)
    x = np.asarray(x, np.float32)
    a1 = np.maximum(np.matmul(x, w1) + b1, np.float32(0))
    a2 = np.maximum(np.matmul(a1, w2) + b2, np.float32(0))
    return np.matmul(a2, w3) + b3


def total_of(num_pots):
    return 2 * (num_pots * 10 + 26) + 4


# ------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "id table n_envs num_pots h1 h2 bc_factor seed env_offset step")
CASES = []


def case(table, n_envs, num_pots, h1, h2, bc_factor):
    k = len(CASES)
    CASES.append(Case("%s_%dpots_%dx%d_%denvs_factor%g" % (table, num_pots, h1, h2, n_envs, bc_factor), table, n_envs, num_pots, h1, h2,
                      bc_factor, 101 + k, 3 * n_envs + 64 * k + 37, 5 + k))


SIZES = (1, 33, 65, 256 + 232)  # one env; one past a 32-env tile; one past a wavefront; a ragged last workgroup of two
for _n in SIZES:
    for _f in (0.0, 0.5, 1.0):
        case("cramped_room", _n, 2, 64, 64, _f)  # the reference's model: 96 -> 64 -> 64 -> 6
for _n in SIZES:
    case("cramped_room", _n, 1, 40, 24, 0.5)            # 76 inputs (38 K steps), hidden widths padded 40 -> 64, 24 -> 64
    case("asymmetric_advantages", _n, 4, 40, 24, 1.0)   # 136 inputs
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def far_case():
    """At the far corner of the counter space (tests/far_cases.py): a seed with both halves set, an env offset whose low word wraps
    inside the batch, a step above 2^32."""
    import far_cases as F

    c = next(c for c in CASES if c.n_envs == SIZES[-1] and c.bc_factor == 0.5 and c.num_pots == 2)
    return c._replace(id=c.id + "@far", seed=F.FAR_SEED, env_offset=F.far_env_offset(c.n_envs), step=2**32 + 2**31 + 9)


def weights_of(c):
    return glorot(c.seed, total_of(c.num_pots), c.h1, c.h2)


def logits_fill(n):
    """float32 [n, 2, 6]: a distinct finite value per element, every row a valid row of logits for the sampler"""
    return (np.arange(n * 12, dtype=np.float32) * np.float32(2.0 ** -10) - np.float32(2.0)).reshape(n, 2, 6)


def synthetic_features(c, rows=64):
    """float32 [rows, in_dim] in the range of featurize_state's entries (indicators, small counts, signed distances): for the CPU
    tests of the bound, which have no env to take real rows from"""
    rng = np.random.default_rng([c.seed, 0xFEA7])
    x = rng.integers(-6, 7, size=(rows, total_of(c.num_pots))).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0
    return x
