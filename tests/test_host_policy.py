"""oc_policy_forward / oc_policy_backward without a GPU: the exports and the structs against the header, the plan's words and their
numbers, every refusal (made before any device call: this host has no device), the references of tests/policy_cases.py against
each other and against torch autograd in float64, the share of rows a case had to silence, the recorded float32 error, the
exact cases (their precondition, their premise in two float32 orders of summation, that they bite, the dealing rule of the partials),
the backward plan of every feature length, and ActorCritic's own refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import partner_cases as PTC
import policy_cases as PC
from case_support import P, ROOT

EINVAL = -1
LDS_MAX = 160 * 1024


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_structs_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_policy_forward", "oc_policy_backward", "oc_policy_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    for struct, words in (("OcActorCritic", r"d_\w+|in_dim|h1|h2"), ("OcPolicyRows", r"d_\w+|n_feature_rows|first_row|n_rows"), ("OcPolicyGrads", r"d_\w+")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(%s)\b" % words, body) == [f[0] for f in getattr(_lib, struct)._fields_], struct
    A, R, G = _lib.OcActorCritic, _lib.OcPolicyRows, _lib.OcPolicyGrads
    assert [getattr(A, f).offset for f, _ in A._fields_] == list(range(0, 64, 8)) + [64, 68, 72] and ctypes.sizeof(A) == 80
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 32] and ctypes.sizeof(R) == 40
    assert ctypes.sizeof(G) == 64
    assert "int oc_policy_forward(const OcActorCritic* policy, const OcPolicyRows* rows, float* d_logits, float* d_values, void* stream);" in hdr
    assert ("int oc_policy_backward(const OcActorCritic* policy, const OcPolicyRows* rows, const float* d_grad_logits, const float* d_grad_values,\n"
            "                       const OcPolicyGrads* grads, float* d_partials, void* stream);") in hdr
    assert "int oc_policy_plan(int64_t n_rows, int with_index, int in_dim, int h1, int h2, int backward, char* out, size_t out_size);" in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_arithmetic():
    hdr = _header()
    for words in ("a1 = relu(x W1 + b1)", "pre1_j = fmaf(x_{in_dim-1}, w1[in_dim-1][j]", "bit for bit on the same weights and row",
                  "delta2_u = pre2_u > 0 ? fmaf(wv[u], gv, fmaf(wp[u][5], gl_5", "is > 0 and 0 elsewhere", "torch's convention",
                  "a wavefront adds its tiles in ascending order and the rows of a tile in ascending order", "((w0 + w1) + w2) + w3",
                  "d_partials[0] + d_partials[1] + ... in ascending order", "No floating-point atomics", "OVERWRITTEN", "+0.0f logits and value"):
        assert words in hdr, words


def test_the_plans_words_carry_their_numbers():
    from overcooked_ai_amd import policy as POL

    hdr = _header()
    rc, fwd = PC.plan(2 ** 17, 0, 96, 64, 64, 0)
    rc2, bwd = PC.plan(2 ** 17, 1, 96, 64, 64, 1)
    assert rc == 0 and rc2 == 0 and fwd in hdr and bwd in hdr, (fwd, bwd)
    assert POL.plan(2 ** 17) == fwd and POL.plan(2 ** 17, index=True, backward=True) == bwd
    assert PC.plan(0, 0, 96, 64, 64, 0) == (0, "nothing to launch (no rows)")
    rc, none = PC.plan(0, 1, 96, 64, 64, 1)
    assert rc == 0 and none in hdr and PC.plan_numbers(none)["partials"] == 0 and PC.plan_numbers(none)["size"] == 10823
    assert POL.partials_shape(2 ** 17, 96, 64, 64) == (256, 10823) and POL.partials_shape(0, 96, 64, 64) == (0, 10823)
    for in_dim, h1, h2 in ((56, 64, 64), (76, 40, 24), (96, 64, 64), (96, 1, 1), (96, 33, 17), (116, 64, 64), (136, 64, 64), (136, 33, 17)):
        size = in_dim * h1 + h1 + h1 * h2 + h2 + h2 * 6 + 6 + h2 + 1
        for n_rows in (1, 31, 32, 33, 129, 4096, PC.one_pass(in_dim, h1, h2) + 33, 2 ** 20):
            for backward in (0, 1):
                rc, text = PC.plan(n_rows, backward, in_dim, h1, h2, backward)
                assert rc == 0, text
                n = PC.plan_numbers(text)
                waves = n["lanes"] // 64
                assert n["lanes"] in (192, 256) and n["per_pass"] == 32 * waves and n["lds"] <= LDS_MAX, text
                tiles = (n_rows + 31) // 32
                assert n["grid"] == min((tiles + waves - 1) // waves, 256), text
                assert ("index=yes" if backward else "index=no") in text
                if backward:
                    assert n["partials"] == n["grid"] and n["size"] == size and n["sum_grid"] == (size + 255) // 256, text
                    assert ("k_policy_backward<F0=3" in text) == (in_dim > 96), text
                else:
                    assert "partial" not in text and "K %d -> 64 -> 64 -> 32 (h1 = %d, h2 = %d" % (in_dim, h1, h2) in text
    # one pass of the persistent grid stays a few tens of thousands of rows: the cases one pass + 33 rows long stay quick
    assert PC.one_pass(96) == 256 * 128 and PC.one_pass(136) == 256 * 96 and PC.BIG == 32801 and PC.BIG_136 == 24609
    from overcooked_ai_amd import _lib

    L = _lib.load()
    assert L.oc_policy_plan(4, 0, 96, 64, 64, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_policy_plan: no output buffer"
    for backward, who in ((0, "oc_policy_forward: "), (1, "oc_policy_backward: ")):
        for args, why in (((-1, 0, 96, 64, 64), "n_rows < 0"), ((2 ** 40 + 1, 0, 96, 64, 64), "n_rows above 2^40"),
                          ((4, 0, 97, 64, 64), "policy.in_dim must be a feature length"), ((4, 0, 36, 64, 64), "policy.in_dim must be a feature length"),
                          ((4, 0, 156, 64, 64), "policy.in_dim must be a feature length"), ((4, 0, 96, 0, 64), "policy.h1 and policy.h2 must be in 1..64"),
                          ((4, 0, 96, 64, 65), "policy.h1 and policy.h2 must be in 1..64")):
            rc, msg = PC.plan(*args, backward)
            assert rc == EINVAL and msg.startswith(who + why), (args, msg)
    with pytest.raises(_lib.OcAmdError, match="oc_policy_backward: n_rows < 0"):
        POL.plan(-1, backward=True)


def test_the_entry_points_refuse_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    weights = [f for f, _ in _lib.OcActorCritic._fields_[:8]]

    def call(backward, pol=(), rows=(), grads=(), **kw):
        v = dict({f: P for f in weights}, in_dim=96, h1=64, h2=64, d_features=P, n_feature_rows=4000, d_index=P, first_row=10, n_rows=1000,
                 d_logits=P, d_values=P, d_grad_logits=P, d_grad_values=P, d_partials=P, **{"g_" + f: P for f in weights})
        v.update(kw)
        pol = _lib.OcActorCritic(*[v[f] for f in weights], v["in_dim"], v["h1"], v["h2"]) if pol == () else pol
        rows = _lib.OcPolicyRows(v["d_features"], v["n_feature_rows"], v["d_index"], v["first_row"], v["n_rows"]) if rows == () else rows
        grads = _lib.OcPolicyGrads(*[v["g_" + f] for f in weights]) if grads == () else grads
        ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
        if backward:
            rc = L.oc_policy_backward(ref(pol), ref(rows), v["d_grad_logits"], v["d_grad_values"], ref(grads), v["d_partials"], None)
        else:
            rc = L.oc_policy_forward(ref(pol), ref(rows), v["d_logits"], v["d_values"], None)
        return rc, L.oc_last_error().decode()

    contiguous = "first_row .. first_row + n_rows must lie inside 0 .. n_feature_rows without d_index"
    shared = [(dict(pol=None), "policy is NULL"), (dict(rows=None), "rows is NULL")]
    shared += [({f: None}, "NULL weight or bias array") for f in weights]
    shared += [({f: P + 2}, "weight and bias arrays must be 4-byte aligned") for f in weights]
    shared += [(dict(d_features=None), "rows.d_features is NULL"), (dict(d_features=P + 8), "rows.d_features must be 16-byte aligned"),
               (dict(d_index=P + 2), "rows.d_index must be 4-byte aligned"), (dict(n_rows=-1), "n_rows < 0"),
               (dict(in_dim=100), "policy.in_dim must be a feature length"), (dict(h1=0), "policy.h1 and policy.h2 must be in 1..64"),
               (dict(h2=65), "policy.h1 and policy.h2 must be in 1..64"), (dict(n_feature_rows=-1), "rows.n_feature_rows < 0"),
               (dict(n_feature_rows=2 ** 31), "rows.n_feature_rows must be below 2^31 with d_index")]
    shared += [(dict(d_index=None, **kw), contiguous) for kw in (dict(first_row=3001), dict(first_row=-1), dict(first_row=4001, n_rows=0),
                                                                 dict(n_feature_rows=999, first_row=0), dict(first_row=2 ** 62, n_rows=2 ** 37))]
    forward = [(dict(d_logits=None), "NULL d_logits or d_values"), (dict(d_values=None), "NULL d_logits or d_values"),
               (dict(d_logits=P + 4), "d_logits must be 8-byte aligned"), (dict(d_values=P + 2), "d_values must be 4-byte aligned")]
    backward = [(dict(d_grad_logits=None), "NULL d_grad_logits or d_grad_values"), (dict(d_grad_values=None), "NULL d_grad_logits or d_grad_values"),
                (dict(d_grad_logits=P + 4), "d_grad_logits must be 8-byte aligned"), (dict(d_grad_values=P + 2), "d_grad_values must be 4-byte aligned"),
                (dict(grads=None), "grads is NULL"), (dict(d_partials=None), "d_partials is NULL"), (dict(d_partials=P + 2), "d_partials must be 4-byte aligned")]
    backward += [({"g_" + f: None}, "NULL gradient array") for f in weights]
    backward += [({"g_" + f: P + 1}, "gradient arrays must be 4-byte aligned") for f in weights]
    for which, who, own in ((0, "oc_policy_forward: ", forward), (1, "oc_policy_backward: ", backward)):
        for kw, why in shared + own:
            rc, msg = call(which, **kw)
            assert rc == EINVAL and msg.startswith(who + why), (which, kw, rc, msg)
    # accepted, and nothing to launch (forward only: the backward call of no rows zeroes the gradients, a device call): no rows;
    # no index; the minimum alignments; an index with the most feature rows it can name; the whole array contiguous
    for kw in (dict(), dict(d_index=None), dict(d_features=P + 16, d_index=P + 4, d_logits=P + 8, d_values=P + 4, d_w1=P + 4, d_bv=P + 12),
               dict(n_feature_rows=2 ** 31 - 1), dict(d_index=None, n_feature_rows=2 ** 40, first_row=2 ** 40), dict(in_dim=136, h1=1, h2=1)):
        assert call(0, n_rows=0, **kw)[0] == 0, kw


# ------------------------------------------------------------------------------------------ the references
def test_the_forward_reference_is_the_partners_with_a_value_column():
    c = next(c for c in PC.CASES if c.id == "136_33_17-%drows-contiguous-zero_tiles" % PC.BIG_136)
    a = PC.arrays_of(c)
    x = a.features
    six = a.weights[:6]
    pre1, pre2, out = PC.forward_f64(x, a.weights)
    logits, (a1, a2) = PTC.mlp_f64(x, six)
    # (a product with seven columns and one with six may round their float64 sums differently: 1e-13, not bit for bit)
    close = lambda p, q: np.allclose(p, q, rtol=1e-13, atol=1e-13)  # noqa: E731
    assert close(out[:, :6], logits) and np.array_equal(np.maximum(pre1, 0), a1) and np.array_equal(np.maximum(pre2, 0), a2)
    assert close(out[:, 6], a2 @ PC.f64(a.weights[6]) + PC.f64(a.weights[7])[0])
    bound = PC.forward_bound(x, a.weights)
    assert bound.shape == out.shape and close(bound[:, :6], PTC.mlp_bound(x, six)) and (bound[:, 6] > 0).all()
    # the bounds of the hidden pre-activations are the ones inside mlp_bound: pushed through the last layer they give it again
    e1, e2 = PC.hidden_bounds(x, a.weights)
    w3, b3 = np.abs(PC.f64(PC.head(a.weights)[4])), np.abs(PC.f64(PC.head(a.weights)[5]))
    assert close(PTC.gamma(w3.shape[0] + 1) * ((np.abs(a2) + e2) @ w3 + b3) + e2 @ w3, bound)
    # and a float32 evaluation lies inside them
    f32 = PTC.mlp_f32(x, PC.head(a.weights))
    assert (np.abs(f32 - out) <= bound).all()


def _torch_autograd(a):
    import torch

    w = [torch.tensor(PC.f64(t), requires_grad=True) for t in a.weights]
    x = torch.tensor(PC.f64(PC.rows_of(a)))
    a1 = torch.relu(x @ w[0] + w[1])
    a2 = torch.relu(a1 @ w[2] + w[3])
    logits, values = a2 @ w[4] + w[5], a2 @ w[6] + w[7]
    up = PC.upstream(a).astype(np.float64)
    ((logits * torch.tensor(up[:, :6])).sum() + (values * torch.tensor(up[:, 6])).sum()).backward()
    return [t.grad.numpy() for t in w]


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.M <= 488], ids=lambda c: c.id)
def test_the_reference_gradients_are_torch_autograd_s(c):
    a = PC.arrays_of(c)
    _, _, ref = PC.reference_of(c)
    for name, mine, theirs in zip(PC.NAMES, ref.grads, _torch_autograd(a)):
        assert mine.shape == theirs.shape or mine.size == theirs.size, name
        assert np.abs(mine.reshape(theirs.shape) - theirs).max() <= 1e-12 * max(1.0, np.abs(theirs).max()), (c.id, name)


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_few_rows_are_silenced_and_no_result_equals_the_sentinel(c):
    a = PC.arrays_of(c)
    out, bound, ref = PC.reference_of(c)
    live = int(a.valid.sum())
    assert a.unstable.sum() <= PC.UNSTABLE_CAP * c.M, (c.id, int(a.unstable.sum()), c.M)
    assert not a.grad_logits[a.unstable].any() and not a.grad_values[a.unstable].any()
    assert not (out == PC.FILL).any() and not np.isnan(out).any() and not out[~a.valid].any() and (bound[a.valid] > 0).all()
    for g in ref.grads:
        assert np.isfinite(g).all() and not (g == PC.FILL).any()
    if c.M >= 32 and live:
        assert all(np.abs(g).max() > 0 for g in ref.grads[4:]), c.id  # (there are gradients to compare)


def test_the_recorded_error_is_the_measured_one():
    """F32_ERROR is the largest scaled error of the float32 numpy restatement over the case list: no smaller than what is measured
    here, and no more than twice it (np.matmul's order of summation may differ between builds)."""
    worst, where = 0.0, None
    for c in PC.CASES:
        _, _, ref = PC.reference_of(c)
        errs = PC.scaled_errors(PC.backward_f32(c).grads, ref)
        if max(errs) > worst:
            worst, where = max(errs), (c.id, PC.NAMES[int(np.argmax(errs))])
    print("largest scaled error of backward_f32 over %d cases: %.4g (%s, %s)" % (len(PC.CASES), worst, *where))
    assert PC.F32_ERROR / 2 <= worst <= PC.F32_ERROR, (worst, PC.F32_ERROR)
    assert PC.DEVICE_FACTOR == 4


def test_the_case_list_covers_what_it_must():
    cases = PC.CASES
    sizes = {c.M for c in cases}
    assert sizes >= {1, 31, 32, 33, 64, 65, 257, 488, PC.BIG}
    for M in PC.SIZES:
        assert {c.mode for c in cases if c.M == M and (c.in_dim, c.h1, c.h2) == (96, 64, 64)} >= {"contiguous", "indexed"}
    assert {(c.h1, c.h2) for c in cases} >= {(64, 64), (1, 1), (33, 17)} and {c.in_dim for c in cases} == {56, 76, 96, 116, 136}
    for in_dim in (76, 116):
        assert {c.mode for c in cases if c.in_dim == in_dim} == {"contiguous", "indexed"}, in_dim
    for c in cases:
        rc, text = PC.plan(c.M, c.mode == "indexed", c.in_dim, c.h1, c.h2, 1)
        assert rc == 0 and ("k_policy_backward<F0=3" in text) == (c.in_dim in (116, 136)), (c.id, text)
    assert {c.pattern for c in cases} == {"dense", "zero_tiles", "at_zero"}
    for c in cases:
        a = PC.arrays_of(c)
        if c.mode == "contiguous":
            assert a.first > 0 and a.index is None and a.valid.all()
        elif c.M >= 8:
            inside = a.rows[a.valid]
            assert (~a.valid).sum() >= 2 and len(np.unique(inside)) < len(inside) and a.nan_row not in inside, c.id
        if c.pattern == "zero_tiles":
            up = PC.upstream(a).reshape(-1)
            tiles = [up[7 * 32 * t:7 * 32 * (t + 1)] for t in range((c.M + 31) // 32)]
            assert any(not t.any() for t in tiles) and any(t.any() for t in tiles), c.id
            assert any(0 < np.count_nonzero(t.reshape(-1, 7).any(1)) <= 1 for t in tiles), c.id  # a tile with one live row
        if c.pattern == "at_zero":
            # all-zero feature rows under non-zero upstream gradients, zero hidden biases: every hidden pre-activation is exactly 0 in
            # any arithmetic, and the derivative there is 0: such a row reaches the last layer's biases alone
            xs, up = PC.rows_of(a), PC.upstream(a)
            zero = a.valid & ~xs.any(1)
            assert zero.sum() >= 3 and up[zero].all(1).any() and not a.weights[1].any() and not a.weights[3].any()
            pre1, pre2, _ = PC.forward_f64(xs[zero], a.weights)
            assert not pre1.any() and not pre2.any() and not a.unstable[zero].any()
            only = PC._backward(xs[zero], a.weights, up[zero], np.float64).grads
            assert not any(g.any() for g in only[:5]) and not only[6].any() and only[5].any() and only[7].any()


# ------------------------------------------------------------------------------------------ the exact cases
EXACT = pytest.mark.parametrize("c", PC.EXACT_CASES, ids=lambda c: c.id)


def test_the_exact_case_list_covers_what_it_must():
    cases = PC.EXACT_CASES
    small = [c for c in cases if c.kind == "small"]
    assert {(c.in_dim, c.M) for c in small} == {(d, M) for d in (56, 76, 96, 116, 136) for M in (1, 33, 257)} and len(small) == 15
    for in_dim in (56, 76, 96, 116, 136):
        mine = [c for c in small if c.in_dim == in_dim]
        assert {c.mode for c in mine} == {"contiguous", "indexed"} and any(c.h1 < 64 and c.h2 < 64 for c in mine), in_dim
    assert {(c.h1, c.h2) for c in small} == set(PC.EXACT_WIDTHS)
    three = [c for c in cases if c.kind == "three_pass"]
    assert [(c.in_dim, c.h1, c.h2, c.mode) for c in three] == [(96, 64, 64, "indexed"), (96, 64, 64, "contiguous"), (116, 64, 64, "indexed"),
                                                             (136, 33, 17, "contiguous"), (76, 40, 24, "indexed")]
    assert [c.M for c in three] == [65825, 65825, 65825, 49377, 65825]
    for c in three:
        # the third pass: two full workgroups, one full tile more, and a tile of ONE row
        grid, waves = PC.backward_plan_of(c)
        assert grid == 256 and c.M == 2 * PC.one_pass(c.in_dim) + 2 * 32 * waves + 33
        owner = PC.owner_of_rows(c.M, grid, waves)
        third = owner[2 * PC.one_pass(c.in_dim):]
        assert np.array_equal(np.unique(third), [0, 1, 2]) and (third == 2).sum() == 33 and (np.bincount(owner)[3:] == 2 * 32 * waves).all()
    for c in cases:
        a = PC.exact_arrays_of(c)
        assert not a.unstable.any()
        if c.mode == "contiguous":
            assert a.first == PC.FIRST and a.index is None and a.valid.all() and len(a.features) == a.first + c.M + 5
        else:
            inside = a.rows[a.valid]
            assert len(a.features) == PC.EXACT_ROWS and (~a.valid).sum() == c.M // 16 and a.nan_row not in inside and a.valid[-1], c.id
            assert not PC.upstream(a)[~a.valid].any() and (c.M < 16 or np.concatenate([a.grad_logits, a.grad_values[:, None]], 1)[~a.valid].any())


def test_the_owner_of_a_row_is_the_kernels_dealing():
    """tile = (pass * grid + workgroup) * wavefronts + wavefront, written out as the loops of k_policy_backward"""
    for M, grid, waves in ((1, 1, 4), (33, 1, 4), (257, 3, 3), (2 * 5 * 3 * 32 + 100, 5, 3), (3 * 7 * 4 * 32 - 31, 7, 4)):
        want = np.full(M, -1, np.int64)
        n_tiles = (M + 31) // 32
        for block in range(grid):
            for wave in range(waves):
                for t in range(block * waves + wave, n_tiles, grid * waves):
                    want[32 * t:32 * (t + 1)] = block
        assert np.array_equal(PC.owner_of_rows(M, grid, waves), want), (M, grid, waves)


@EXACT
def test_the_precondition_of_exactness(c):
    """Integer inputs, and no sum of absolute values of the terms of any sum reaches 2^24: a condition on the reference alone"""
    a = PC.exact_arrays_of(c)
    for t in a.weights + (a.features, a.grad_logits, a.grad_values):
        assert t.dtype == np.float32 and np.array_equal(t, np.rint(t)), c.id
    assert all(np.abs(w).max() <= 1 for w in a.weights) and np.abs(a.features).max() <= 6 and np.abs(a.grad_logits).max() <= 1
    sums = PC.exact_sums(c)
    assert set(sums) == {"pre1", "pre2", "out", "delta2", "delta1"} | {"g" + n for n in PC.NAMES}
    print("%s: largest sum of |terms| %.6g (%s) of 2^24 = %d; %s" % (c.id, max(sums.values()), max(sums, key=sums.get), 2 ** 24,
                                                                    ", ".join("%s %.6g" % kv for kv in sums.items())))
    assert max(sums.values()) < 2 ** 24, (c.id, sums)


def _f32_other_order(a):
    """(out [M, 7], the eight gradients) in float32 in ANOTHER order of summation than np.matmul's: every K loop descending (the
    operands flipped along K), the rows of the call in four interleaved groups added last group first"""
    f = np.float32
    w1, b1, w2, b2, w3, b3 = PC.head(a.weights)
    x, d3 = PC.rows_of(a), PC.upstream(a)
    dot = lambda p, q: np.matmul(np.ascontiguousarray(p[:, ::-1]), np.ascontiguousarray(q[::-1]))  # noqa: E731
    pre1 = dot(x, w1) + b1
    a1 = np.maximum(pre1, f(0))
    pre2 = dot(a1, w2) + b2
    a2 = np.maximum(pre2, f(0))
    out = dot(a2, w3) + b3
    d2 = np.where(pre2 > 0, dot(d3, w3.T), f(0))
    d1 = np.where(pre1 > 0, dot(d2, w2.T), f(0))
    total = None
    for k in (3, 2, 1, 0):
        r = slice(k, None, 4)
        g3 = dot(a2[r].T, d3[r])
        part = [dot(x[r].T, d1[r]), d1[r][::-1].sum(0), dot(a1[r].T, d2[r]), d2[r][::-1].sum(0), g3[:, :6], d3[r][::-1, :6].sum(0), g3[:, 6], d3[r][::-1, 6:].sum(0)]
        assert all(p.dtype == f for p in part)
        total = part if total is None else [t + p for t, p in zip(total, part)]
    assert out.dtype == f and all(t.dtype == f for t in total)
    return np.where(a.valid[:, None], out, f(0)), total


@EXACT
def test_the_premise_any_f32_evaluation_of_an_exact_case_is_the_f64_reference(c):
    a = PC.exact_arrays_of(c)
    out, ref = PC.exact_reference_of(c)
    xs = PC.rows_of(a)
    f32 = PC._backward(xs, a.weights, PC.upstream(a), np.float32)
    out32 = np.where(a.valid[:, None], PTC.mlp_f32(xs, PC.head(a.weights)), np.float32(0))
    out_other, grads_other = _f32_other_order(a)
    assert out32.dtype == np.float32 and np.array_equal(out32, out) and np.array_equal(out_other, out), c.id
    for name, g64, g32, other in zip(PC.NAMES, ref.grads, f32.grads, grads_other):
        assert g32.dtype == np.float32 and np.array_equal(g32, g64) and np.array_equal(other.reshape(g64.shape), g64), (c.id, name)
    # the reference's own pieces agree: the flat layout, the sum of the workgroups' partials
    flat = PC.flat_grads(PC.exact_terms_of(c))
    lay = PC.layout_of(c)
    assert all(np.array_equal(flat[lay[n]], g.reshape(-1)) for n, g in zip(PC.NAMES, ref.grads)) and np.array_equal(flat, PC.flat(ref.grads))
    partials = PC.exact_partials_of(c)
    assert partials.shape == (PC.backward_plan_of(c)[0], len(flat)) and np.array_equal(partials.sum(0), flat)
    # every result is an integer, so none holds the exact cases' sentinel (FILL itself is one: -7 is a logit of these cases)
    assert np.array_equal(out, np.rint(out)) and np.array_equal(partials, np.rint(partials)) and PC.EXACT_FILL != np.rint(PC.EXACT_FILL)


@pytest.mark.parametrize("c", [c for c in PC.EXACT_CASES if c.kind == "small"], ids=lambda c: c.id)
def test_the_exact_reference_gradients_are_torch_autograd_s(c):
    a = PC.exact_arrays_of(c)
    _, ref = PC.exact_reference_of(c)
    for name, mine, theirs in zip(PC.NAMES, ref.grads, _torch_autograd(a)):
        assert np.array_equal(mine.reshape(theirs.shape), theirs), (c.id, name)  # (integers in float64: exactly)


@EXACT
def test_the_exact_cases_bite(c):
    a = PC.exact_arrays_of(c)
    assert PC.exact_misses(c, a) == [], c.id
    t = PC.exact_terms_of(c)
    pre = np.concatenate([t.pre1[a.valid].reshape(-1), t.pre2[a.valid].reshape(-1)])
    live = a.valid & PC.upstream(a).any(1)
    at_zero = ((t.pre1 == 0).any(1) | (t.pre2 == 0).any(1)) & live
    print("%s: %.3f of the hidden pre-activations positive, %.3f exactly 0, %d live rows with one at 0" % (c.id, (pre > 0).mean(), (pre == 0).mean(), at_zero.sum()))
    assert 0.3 <= (pre > 0).mean() <= 0.7 and at_zero.any()
    _, ref = PC.exact_reference_of(c)
    assert all(g.any() for g in ref.grads), c.id
    if c.kind == "three_pass":
        lay = PC.layout_of(c)
        third, last = PC.flat_grads(t, slice(2 * PC.one_pass(c.in_dim), None)), PC.flat_grads(t, slice(c.M - 1, None))
        assert all(third[lay[n]].any() and last[lay[n]].any() for n in PC.NAMES), c.id
        # a pass, a workgroup's share of it or the last row left out is another answer
        owner = PC.owner_of_rows(c.M, *PC.backward_plan_of(c))
        assert all(PC.flat_grads(t, np.flatnonzero(owner == p)).any() for p in (0, 1, 2, 255))


def test_the_backward_plan_of_every_feature_length():
    """Lanes and LDS bytes as oc_policy_plan states them: four wavefronts wherever their images fit 160 KB, which leaves out 136
    inputs alone (116 inputs: 832 bytes to spare)."""
    table = {56: (256, 120320, 2, None), 76: (256, 132416, 3, None), 96: (256, 147456, 3, None), 116: (256, 163008, 3, 1), 136: (192, 151456, 3, 2)}
    for in_dim, (lanes, lds, nf, more) in table.items():
        rc, text = PC.plan(2 ** 20, 1, in_dim, 64, 64, 1)
        n = PC.plan_numbers(text)
        assert rc == 0 and (n["lanes"], n["lds"], n["grid"]) == (lanes, lds, 256) and lds <= LDS_MAX, (in_dim, text)
        assert "k_policy_backward<F0=0,NF=%d,REST>" % nf in text and "%d wavefronts x 32-row tiles" % (lanes // 64) in text
        assert ("k_policy_backward<F0=3,NF=%s>" % more in text) if more else ("F0=3" not in text), text
        assert PC.one_pass(in_dim) == 256 * 32 * (lanes // 64) and PC.per_pass(in_dim) == 32 * (lanes // 64)
    with open(os.path.join(ROOT, "overcooked_ai_amd", "csrc", "policy.hpp")) as f:
        src = f.read()
    assert "else three (136 inputs)" in src and "else three (116 and 136 inputs)" not in src
    assert "With 136 inputs a backward workgroup has three wavefronts" in _header()


# ------------------------------------------------------------------------------------------ the Python surface
def test_actor_critic_validates_its_arguments():
    import torch

    from overcooked_ai_amd.policy import NAMES, ActorCritic, shapes

    pol = ActorCritic(96, 40, 24, seed=3)
    assert [tuple(p.shape) for p in pol.parameters()] == list(shapes(96, 40, 24)) and [n for n, _ in pol.named_parameters()] == list(NAMES)
    assert all(p.dtype == torch.float32 and p.requires_grad for p in pol.parameters())
    lim = np.sqrt(6.0 / (96 + 40))
    assert float(pol.w1.detach().abs().max()) <= lim and float(pol.w1.detach().abs().max()) > 0.9 * lim and not pol.b1.any() and not pol.bv.any()
    again = ActorCritic(96, 40, 24, seed=3)
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), again.parameters())) and not torch.equal(pol.w1, ActorCritic(96, 40, 24, seed=4).w1)
    for bad in (lambda: ActorCritic(97), lambda: ActorCritic(96, 0, 64), lambda: ActorCritic(96, 64, 65)):
        with pytest.raises(ValueError):
            bad()
    w = [p.detach().numpy() for p in pol.parameters()]
    twin = ActorCritic.from_weights(*w, device="cpu")
    assert all(torch.equal(p, q) for p, q in zip(pol.parameters(), twin.parameters()))
    for k, wrong in ((0, w[0].astype(np.int32)), (1, w[1][:-1]), (4, w[4][:, :5]), (6, w[6][:, None]), (7, np.zeros(2, np.float32)), (0, w[0][0])):
        with pytest.raises(ValueError):
            ActorCritic.from_weights(*[wrong if i == k else t for i, t in enumerate(w)], device="cpu")
    x = torch.zeros((12, 2, 96))
    index = torch.zeros(5, dtype=torch.int32)
    bad = [(dict(features=x.double()), "features must be a contiguous float32 [..., 96]"),
           (dict(features=torch.zeros((12, 95))), "features must be a contiguous float32 [..., 96]"),
           (dict(features=torch.zeros((96, 12)).t()), "features must be a contiguous float32 [..., 96]"),
           (dict(features=torch.zeros(96)), "features must be a contiguous float32 [..., 96]"),
           (dict(features=x.clone().requires_grad_(True)), "features must not require a gradient"),
           (dict(features=torch.zeros(12 * 96 + 1)[1:].view(12, 96)), "features must be 16-byte aligned"),
           (dict(index=index.long()), "index must be a contiguous int32 [5]"), (dict(index=index.view(5, 1)), "index must be a contiguous int32 [M]"),
           (dict(index=torch.zeros(10, dtype=torch.int32)[::2]), "index must be a contiguous int32 [5]"),
           (dict(first=25), "first = 25 lies outside"), (dict(first=-1), "first = -1 lies outside"),
           # (the last three: everything in order, but on the host — there is no CPU fallback)
           (dict(), "no CPU fallback"), (dict(index=index), "no CPU fallback"), (dict(first=3), "no CPU fallback")]
    for kw, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            pol(**dict(dict(features=x), **kw))
    for kw, words in ((dict(features=x[:, 0]), "features must be a contiguous float32 [N, 2, 96]"), (dict(features=x.view(24, 96)), "[N, 2, 96]"),
                      (dict(features=x, out=(torch.zeros((12, 2, 5)), torch.zeros((12, 2)))), "out[0] must be a contiguous float32 [12, 2, 6]"),
                      (dict(features=x, out=(torch.zeros((12, 2, 6)), torch.zeros((12, 2)).double())), "out[1] must be a contiguous float32 [12, 2]"),
                      (dict(features=x), "no CPU fallback")):
        with pytest.raises(ValueError, match=re.escape(words)):
            pol.act(**kw)
    pol.w2.data = pol.w2.data.double()
    with pytest.raises(ValueError, match=re.escape("ActorCritic.w2 must be a contiguous float32 [40, 24]")):
        pol(x)
