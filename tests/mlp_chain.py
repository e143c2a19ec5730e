"""The forward arithmetic of the dense policy kernels (include/oc_amd.h: OcDensePolicy "Arithmetic", OcActorCritic "Forward
arithmetic"), restated in numpy so that a device result can be held to it bit for bit: every unit an f32 fmaf chain over its inputs
in ascending index that starts from the bias, one rounding per step, hidden units followed by max(., 0).

`fma32(a, b, c)` is round_f32(a * b + c), exactly.  The product of two float32 has 48 significant bits and is exact in float64; the
float64 sum p + c is rounded once, TwoSum (Knuth) gives its error exactly, and where the sum is inexact it is re-rounded TO ODD (of
the two float64 neighbours of the exact value, the one whose last bit is set).  A value rounded to odd at 53 bits rounds to
nearest-even at 24 bits (or at a subnormal's fewer) exactly as the unrounded value does (Boldo & Melquiond, "Emulation of a FMA and
correctly rounded sums: proved algorithms using rounding to odd": two bits more than the target are enough).  The plain
f32(f64(a) * f64(b) + f64(c)) rounds twice to nearest and is wrong on ties of the second rounding (tests/test_host_mlp_chain.py
holds one such triple).

`chain_f32(x, weights)` applies it in ascending k from the broadcast bias; `evaluate` also returns the hidden pre-activations and
the smallest non-zero magnitude among all products and partial sums, which `no_subnormals` holds to 2^-126: the header is silent
on subnormal numbers, so no case may come near one.  `canon` maps -0 to +0 before a bit comparison (the header allows either).
numpy only; imported like helpers.py."""
from collections import namedtuple

import numpy as np

MIN_NORMAL = 2.0 ** -126


def fma32(a, b, c):
    """float32 round_f32(a * b + c) of float32 arrays (broadcast), with ONE rounding"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                      # exact: 24 + 24 bits
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)  # TwoSum: p + c = s + err exactly
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(1)) == 0
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))  # the neighbour on the exact value's side
        return np.where(inexact & even, other, s).astype(np.float32)


def fma32_plain(a, b, c):
    """The tempting form: two roundings to nearest.  NOT an fma (kept for the test that shows it)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def head(weights):
    """Six arrays (w1, b1, w2, b2, w3, b3) as they are; eight (.., wp, bp, wv, bv) with the value head as the seventh output column"""
    weights = tuple(np.asarray(w, np.float32) for w in weights)
    if len(weights) == 6:
        return weights
    w1, b1, w2, b2, wp, bp, wv, bv = weights
    return (w1, b1, w2, b2, np.concatenate([wp, wv.reshape(-1, 1)], 1), np.concatenate([bp, bv.reshape(1)]))


def _smallest(v, so_far):
    v = np.abs(np.asarray(v, np.float64))
    v = v[v != 0]
    return min(so_far, float(v.min())) if v.size else so_far


def _layer(x, w, b, order, watch):
    """[rows, H] float32: the chain of every unit over the inputs k in `order`, from the bias"""
    acc = np.broadcast_to(b, (x.shape[0], w.shape[1])).astype(np.float32)
    small = watch
    for k in order:
        xk, wk = x[:, k:k + 1], w[k][None, :]
        acc = fma32(xk, wk, acc)
        if watch is not None:
            small = _smallest(xk.astype(np.float64) * wk.astype(np.float64), _smallest(acc, small))
    return acc, small


def relu(acc):
    return np.where(acc > 0, acc, np.float32(0)).astype(np.float32)  # (max(., 0) of a NaN is 0)


Chain = namedtuple("Chain", "out pre1 pre2 smallest")


def evaluate(x, weights, order=None, watch=False):
    """Chain(out float32 [rows, 6 or 7], the hidden pre-activations, the smallest non-zero |product| or |partial sum| (watch=True))
    of float32 rows x [rows, in_dim].  order: the k order of LAYER 1 where it is not 0, 1, .. in_dim - 1 (for mutants of the chain)."""
    w1, b1, w2, b2, w3, b3 = head(weights)
    x = np.asarray(x, np.float32).reshape(-1, w1.shape[0])
    small = np.inf if watch else None
    pre1, small = _layer(x, w1, b1, range(w1.shape[0]) if order is None else order, small)
    pre2, small = _layer(relu(pre1), w2, b2, range(w2.shape[0]), small)
    out, small = _layer(relu(pre2), w3, b3, range(w3.shape[0]), small)
    return Chain(out, pre1, pre2, small)


def chain_f32(x, weights, order=None):
    """float32 [..., 6] logits (six arrays) or [..., 7] logits and value (eight) of float32 rows x [..., in_dim]"""
    out = evaluate(x, weights, order).out
    return out.reshape(np.shape(x)[:-1] + (out.shape[-1],))


def no_subnormals(x, weights):
    """No product and no partial sum of the chain on rows x, other than an exact 0, is below 2^-126 in magnitude"""
    small = evaluate(x, weights, watch=True).smallest
    assert small >= MIN_NORMAL, "a product or partial sum of magnitude %.3g < 2^-126" % small


def canon(a):
    """uint32 bit patterns of float32 a with -0 as +0"""
    a = np.asarray(a, np.float32)
    return np.ascontiguousarray(np.where(a == 0, np.float32(0), a)).view(np.uint32)
