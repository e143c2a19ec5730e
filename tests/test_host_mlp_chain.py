"""tests/mlp_chain.py, the numpy restatement of the header's fmaf chain that the device is held to bit for bit
(tests/test_gpu_mlp_chain.py), against rational arithmetic: fma32 on seeded triples with cancellations and ties, on the triple at
which the two-rounding form fails; chain_f32 against a scalar loop of exact fused multiply-adds; the ReLU of a NaN; canon and
no_subnormals."""
from fractions import Fraction

import numpy as np
import pytest

import mlp_chain as MC

F32 = np.float32


def round_f32(q):
    """The float32 nearest to the rational q, ties to even (gradual underflow below 2^-126; no overflow in these tests)"""
    if q == 0:
        return F32(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(q, quantum)
    n = int(n)
    if rem * 2 > quantum or (rem * 2 == quantum and n % 2):
        n += 1
    return F32(sign * float(n * quantum))  # (n * quantum has 24 bits or is 2^(e + 1): exact as a double)


def fma_exact(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def triples(n, seed=20240):
    """float32 (a, b, c) [n]: random mantissas and exponents; a third with c near -a * b (heavy cancellation), among them exact
    cancellations; a third with few-bit operands, whose sums land on ties of the second rounding"""
    rng = np.random.default_rng(seed)

    def rand(k, lo=-20, hi=20):
        return (rng.uniform(1, 2, k) * rng.choice([-1.0, 1.0], k) * 2.0 ** rng.integers(lo, hi, k)).astype(F32)

    third = n // 3
    a, b, c = rand(n), rand(n), rand(n, -40, 40)
    prod = a.astype(np.float64) * b.astype(np.float64)
    c[:third] = (-prod[:third] * (1 + rng.integers(-4, 5, third) * 2.0 ** -24)).astype(F32)
    few = slice(third, 2 * third)
    a[few] = (rng.integers(1, 64, third) * 2.0 ** rng.integers(-12, 0, third)).astype(F32)  # 6-bit operands: exact products in float32
    b[few] = (rng.integers(1, 64, third) * 2.0 ** rng.integers(-12, 0, third)).astype(F32)
    c[few] = -(a[few] * b[few])
    c[third:third + third // 2] += F32(1.0)  # (half of them cancel exactly, half sit beside 1 with a tail of low bits)
    tie = slice(2 * third, 2 * third + third // 2)  # the family of the constructed triple: a * b = 2^-23 - 2^-69, c = 2^k + 2^(k - 23)
    j = rng.integers(1, 23, third // 2)
    a[tie] = (2.0 ** -12 * (1 + 2.0 ** -j)).astype(F32)
    b[tie] = (2.0 ** -11 * (1 - 2.0 ** -j)).astype(F32)
    c[tie] = (2.0 + 2.0 ** -22 * rng.integers(1, 9, third // 2)).astype(F32)
    return a, b, c


def test_fma32_equals_rational_arithmetic_on_seeded_triples():
    a, b, c = triples(12000)
    got = MC.fma32(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F32)
    wrong = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert wrong.size == 0, (wrong[:5], a[wrong[:5]], b[wrong[:5]], c[wrong[:5]])
    exact_zero = int(((a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)) == 0).sum())
    plain = MC.fma32_plain(a, b, c)
    unfused = a * b + c
    print("%d triples, %d cancel exactly; the two-rounding form differs on %d, the unfused float32 form on %d"
          % (len(a), exact_zero, (plain != want).sum(), (unfused != want).sum()))
    assert exact_zero >= 100 and (unfused != want).sum() > len(a) // 10 and (plain != want).sum() > 0


def test_fma32_on_the_triple_that_rounds_twice():
    """a * b = 2^-23 (1 - 2^-46) lies just below half an ulp of c = 2 + 2^-22: the sum rounds to c.  In float64 the sum is first
    rounded to c + 2^-23 exactly — a tie at 24 bits — and then to even, c + 2^-22."""
    a, b, c = F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -11 * (1 - 2.0 ** -23)), F32(2 + 2.0 ** -22)
    assert fma_exact(a, b, c) == c
    assert MC.fma32(a, b, c) == c
    assert MC.fma32_plain(a, b, c) == F32(c + F32(2.0 ** -22)) != c


def test_fma32_broadcasts_and_keeps_special_values():
    x = np.array([[1.5], [2.0]], F32)
    w = np.array([[3.0, -1.0, 0.0]], F32)
    assert MC.fma32(x, w, F32(0.25)).tolist() == [[4.75, -1.25, 0.25], [6.25, -1.75, 0.25]]
    assert MC.fma32(x, w, F32(0.25)).dtype == np.float32
    assert np.isnan(MC.fma32(F32(np.nan), F32(1), F32(1))) and np.isnan(MC.fma32(F32(np.inf), F32(0), F32(1)))
    assert MC.fma32(F32(np.inf), F32(1), F32(1)) == np.inf and MC.fma32(F32(3e38), F32(3e38), F32(1)) == np.inf
    assert MC.fma32(F32(1), F32(1), F32(-1)) == 0 and MC.fma32(F32(2.0 ** -100), F32(2.0 ** -100), F32(0)) == 0  # (underflow to 0)
    assert MC.fma32(F32(2.0 ** -70), F32(2.0 ** -70), F32(0)) == F32(2.0 ** -140)  # a subnormal result, exact


def scalar_chain(x, weights):
    """The header's sentences one unit at a time on exact fused multiply-adds"""
    w1, b1, w2, b2, w3, b3 = MC.head(weights)

    def layer(v, w, b, relu):
        out = []
        for j in range(w.shape[1]):
            acc = b[j]
            for k in range(w.shape[0]):
                acc = fma_exact(v[k], w[k, j], acc)
            out.append(max(acc, F32(0)) if relu else acc)
        return out

    return np.array([layer(layer(layer(r, w1, b1, True), w2, b2, True), w3, b3, False) for r in x], F32)


@pytest.mark.parametrize("n_arrays", (6, 8))
def test_chain_f32_is_the_scalar_chain(n_arrays):
    rng = np.random.default_rng(5 + n_arrays)
    d, h1, h2 = 9, 5, 3
    w = [rng.standard_normal(s).astype(F32) for s in ((d, h1), (h1,), (h1, h2), (h2,), (h2, 6), (6,))]
    if n_arrays == 8:
        w += [rng.standard_normal((h2,)).astype(F32), rng.standard_normal((1,)).astype(F32)]
    x = (3 * rng.standard_normal((4, 2, d))).astype(F32)
    got = MC.chain_f32(x, w)
    assert got.shape == (4, 2, 6 if n_arrays == 6 else 7) and got.dtype == np.float32
    want = scalar_chain(x.reshape(-1, d), w).reshape(got.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    r = MC.evaluate(x.reshape(-1, d), w)
    assert (r.pre1 > 0).any() and (r.pre1 < 0).any() and np.array_equal(r.out.reshape(got.shape), got)
    # another order of layer 1 is another result
    assert (MC.chain_f32(x, w, order=list(range(d))[::-1]) != got).any()


def test_the_relu_of_a_nan_is_zero():
    w = [np.ones((2, 2), F32), np.zeros(2, F32), np.ones((2, 1), F32), np.ones(1, F32), np.ones((1, 6), F32), np.zeros(6, F32)]
    out = MC.chain_f32(np.array([[np.nan, 1.0]], F32), w)
    assert (out == 1.0).all()  # both hidden units NaN -> 0; the second layer's unit is its bias
    assert MC.relu(np.array([np.nan, -1.0, -0.0, 2.0], F32)).tolist() == [0.0, 0.0, 0.0, 2.0]


def test_canon_and_no_subnormals():
    a = np.array([-0.0, 0.0, 1.0, -1.0], F32)
    assert MC.canon(a).tolist() == [0, 0, 0x3F800000, 0xBF800000]
    w = [np.full((2, 1), 2.0 ** -70, F32), np.zeros(1, F32), np.ones((1, 1), F32), np.zeros(1, F32), np.ones((1, 6), F32), np.zeros(6, F32)]
    MC.no_subnormals(np.array([[1.0, 0.0]], F32), w)  # 2^-70 and exact zeros
    with pytest.raises(AssertionError, match="2\\^-126"):
        MC.no_subnormals(np.array([[2.0 ** -70, 0.0]], F32), w)  # a product of 2^-140
    assert MC.evaluate(np.array([[1.0, 1.0]], F32), w, watch=True).smallest == 2.0 ** -70
