"""oc_bc_epoch_fused without a GPU: the planner's words, every refusal before the first launch (with stand-in pointers: a call that got
past its checks would fault at its launch, and this host has no device), K = 0, the learner's refusals, the ABI against the header,
and the case list of tests/bc_fused_cases.py held to what numpy says of it."""
import ctypes
import os
import re

import numpy as np
import pytest

import bc_fused_cases as FC

EINVAL = -1
P = 0x10000  # a stand-in pointer, 64 KiB aligned


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oc_amd.h")).read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_struct_match_the_header():
    from overcooked_ai_amd import _lib

    L, hdr = _lib.load(), _header()
    for name in ("oc_bc_epoch_fused", "oc_bc_epoch_fused_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    E = _lib.OcBcEpochFused
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct OcBcEpochFused \{(.*?)\} OcBcEpochFused;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(d_\w+|n_feature_rows|n_index|minibatch)\b", body) == [f[0] for f in E._fields_]
    assert [getattr(E, f).offset for f, _ in E._fields_] == list(range(0, 56, 8)) and ctypes.sizeof(E) == 56
    assert "int oc_bc_epoch_fused(const OcActorCritic* policy, const OcBcLoss* loss, const OcAdam* adam, const OcBcEpochFused* epoch, void* stream);" in hdr
    assert L.oc_abi_version() == 6
    for words in ("BIT FOR BIT", "minibatch 1..128; in_dim 56, 76 or 96", "at most 64 minibatches", "NO scratch"):
        assert words in hdr, words


# ------------------------------------------------------------------------------------------ the plan
def test_the_plans_words_carry_their_numbers():
    from overcooked_ai_amd import _lib, bc

    hdr = _header()
    per = FC.per_launch()
    assert per == 64 and "at most %d minibatches" % per in hdr
    assert bc.plan_bc_epoch_fused(25600, 64) in hdr
    assert bc.plan_bc_epoch_fused(0, 64) in hdr and bc.plan_bc_epoch_fused(0, 64).startswith("nothing to launch (no index)")
    lds = {}
    for n, M, in_dim, h1, h2 in ((1, 1, 96, 64, 64), (150, 64, 56, 40, 24), (150, 64, 76, 64, 64), (25600, 64, 96, 64, 64), (8193, 128, 96, 64, 64),
                                 (per + 1, 1, 76, 40, 24), (per, 1, 56, 1, 1), (100, 128, 96, 33, 17)):
        text = bc.plan_bc_epoch_fused(n, M, in_dim, h1, h2, class_weights=bool(n & 1))
        K, rows = (n + M - 1) // M, min(n, M)
        nf = (in_dim + 31) // 32
        size = in_dim * h1 + h1 + h1 * h2 + h2 + 6 * h2 + 6 + h2 + 1
        assert text.startswith("k_bc_epoch_fused<NF=%d> grid=1, 256 lanes (4 wavefronts x one 32-row tile), %d minibatch(es) of %d rows (the last %d), "
                               "at most %d minibatches per launch: %d launch(es), no host synchronisation" % (nf, K, rows, n - (K - 1) * M, per, -(-K // per))), text
        assert "%d accumulator tiles per wavefront, %d elements (%d per lane) in Adam's phases, class_weights=%s" % (2 * nf + 6, size, -(-size // 256), "yes" if n & 1 else "no") in text
        assert text.endswith("no scratch; out: stats %d x 8 f64, info %d x 4 f64" % (K, K))
        lds[in_dim] = int(re.search(r"(\d+) B LDS", text).group(1))
    # the LDS: the f64 words, oc_policy_plan's backward figure (four wavefronts) and the last forward layer's operand and bias, within 160 KB
    from overcooked_ai_amd import policy

    for in_dim, got in lds.items():
        backward = int(re.search(r"(\d+) B LDS", policy.plan(64, index=True, in_dim=in_dim, backward=True)).group(1))
        assert got == backward + 8 * (256 + 16 + 8) + 4 * (32 * 64 + 32) and got <= 160 * 1024, (in_dim, got, backward)
    assert lds[96] == 158016
    L = _lib.load()
    assert L.oc_bc_epoch_fused_plan(10, 5, 96, 64, 64, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_bc_epoch_fused_plan: no output buffer"


SERVED = "minibatch must be in 1..128"
DIMS = "policy.in_dim must be 56, 76 or 96"


def test_the_plan_refuses_what_is_not_served():
    from overcooked_ai_amd import _lib, bc

    L = _lib.load()
    out = ctypes.create_string_buffer(1024)
    cases = [((-1, 5, 96, 64, 64), "n_index < 0"), ((2 ** 31, 5, 96, 64, 64), "n_index must be below 2^31"), ((10, 0, 96, 64, 64), SERVED),
             ((10, -3, 96, 64, 64), SERVED), ((1000, 129, 96, 64, 64), SERVED), ((10, 4096, 96, 64, 64), SERVED), ((10, 5, 116, 64, 64), DIMS),
             ((10, 5, 136, 64, 64), DIMS), ((10, 5, 97, 64, 64), DIMS), ((10, 5, 36, 64, 64), DIMS), ((10, 5, 96, 0, 64), "policy.h1 and policy.h2 must be in 1..64"),
             ((10, 5, 96, 64, 65), "policy.h1 and policy.h2 must be in 1..64")]
    for args, why in cases:
        assert L.oc_bc_epoch_fused_plan(*args, 0, out, len(out)) == EINVAL and L.oc_last_error().decode().startswith("oc_bc_epoch_fused: " + why), (args, why)
        with pytest.raises(ValueError, match=re.escape("oc_bc_epoch_fused: " + why)):
            bc.plan_bc_epoch_fused(*args)
    for why in (SERVED, DIMS):  # the messages say what is served, and by what the rest is
        L.oc_bc_epoch_fused_plan(10, 129, 116, 64, 64, 0, out, len(out)) if why is SERVED else L.oc_bc_epoch_fused_plan(10, 5, 116, 64, 64, 0, out, len(out))
        assert "oc_bc_update serves" in L.oc_last_error().decode()


# ------------------------------------------------------------------------------------------ the refusals of the call
def _call(pol=(), loss=(), ad=(), ep=(), **kw):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    ptrs = ctypes.c_void_p * 8
    v = dict(w=[P] * 8, in_dim=96, h1=64, h2=64, m=[P] * 8, v=[P] * 8, d_clock=P, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.5,
             d_actions=P + 1, d_class_weights=P, n_samples=3000, d_features=P, n_feature_rows=3000, d_index=P, n_index=250, minibatch=100, d_stats=P, d_info=P)
    v.update(kw)
    polc = _lib.OcActorCritic(*v["w"], v["in_dim"], v["h1"], v["h2"]) if pol == () else pol
    q = _lib.OcBcLoss(v["d_actions"], v["d_class_weights"], v["n_samples"], None, None, 0, 0, None, None, None, None, None) if loss == () else loss
    adam = _lib.OcAdam(ptrs(*v["m"]), ptrs(*v["v"]), v["d_clock"], None, None, v["lr"], v["beta1"], v["beta2"], v["eps"], v["max_grad_norm"]) if ad == () else ad
    e = _lib.OcBcEpochFused(v["d_features"], v["n_feature_rows"], v["d_index"], v["n_index"], v["minibatch"], v["d_stats"], v["d_info"]) if ep == () else ep
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return L.oc_bc_epoch_fused(ref(polc), ref(q), ref(adam), ref(e), None), L.oc_last_error().decode()


def test_every_refusal_is_made_before_the_first_launch():
    def but(i, x, base=P):
        return [x if k == i else base for k in range(8)]

    cases = [(dict(pol=None), "policy is NULL"), (dict(loss=None), "loss is NULL"), (dict(ad=None), "adam is NULL"), (dict(ep=None), "epoch is NULL"),
             (dict(n_index=-1), "n_index < 0"), (dict(n_index=2 ** 31), "n_index must be below 2^31"), (dict(minibatch=0), SERVED), (dict(minibatch=129), SERVED),
             (dict(minibatch=129, n_index=5), SERVED), (dict(in_dim=116), DIMS), (dict(in_dim=136), DIMS), (dict(h1=0), "policy.h1 and policy.h2 must be in 1..64"),
             (dict(h2=65), "policy.h1 and policy.h2 must be in 1..64"),
             (dict(d_index=None), "epoch.d_index is NULL"), (dict(d_stats=None), "NULL epoch.d_stats or epoch.d_info"), (dict(d_info=None), "NULL epoch.d_stats or epoch.d_info"),
             (dict(d_stats=P + 4), "epoch.d_stats and epoch.d_info must be 8-byte aligned"), (dict(d_info=P + 4), "epoch.d_stats and epoch.d_info must be 8-byte aligned"),
             (dict(w=but(3, None)), "NULL weight or bias array"), (dict(w=but(7, P + 2)), "weight and bias arrays must be 4-byte aligned"),
             (dict(d_features=None), "rows.d_features is NULL"), (dict(d_features=P + 8), "rows.d_features must be 16-byte aligned"),
             (dict(d_index=P + 2), "rows.d_index must be 4-byte aligned"), (dict(n_feature_rows=-1), "rows.n_feature_rows < 0"),
             (dict(n_feature_rows=2 ** 31), "rows.n_feature_rows must be below 2^31 with d_index"),
             (dict(d_actions=None), "loss.d_actions is NULL"), (dict(d_class_weights=P + 2), "loss.d_class_weights must be 4-byte aligned"),
             (dict(n_samples=-1), "n_samples < 0"), (dict(n_samples=2 ** 31), "n_samples must be below 2^31 with d_index"),
             (dict(m=but(2, None)), "NULL moment array"), (dict(v=but(5, None)), "NULL moment array"), (dict(m=but(0, P + 2)), "moment arrays must be 4-byte aligned"),
             (dict(d_clock=None), "adam.d_clock is NULL"), (dict(d_clock=P + 4), "adam.d_clock, adam.d_grad_scale and adam.d_info must be 8-byte aligned"),
             (dict(lr=-1.0), "adam.lr must be finite and >= 0"), (dict(lr=float("inf")), "adam.lr must be finite and >= 0"),
             (dict(beta1=1.0), "adam.beta1 and adam.beta2 must be in [0, 1)"), (dict(eps=0.0), "adam.eps must be positive"),
             (dict(max_grad_norm=float("nan")), "adam.max_grad_norm is NaN")]
    for kw, why in cases:
        rc, msg = _call(**kw)
        assert rc == EINVAL and msg.startswith("oc_bc_epoch_fused: " + why), (kw, rc, msg)


def test_no_index_launches_nothing_and_is_checked_all_the_same():
    assert _call(n_index=0)[0] == 0 and _call(n_index=0, minibatch=1)[0] == 0 and _call(n_index=0, d_class_weights=None)[0] == 0
    assert _call(n_index=0, lr=-1.0) == (EINVAL, "oc_bc_epoch_fused: adam.lr must be finite and >= 0")
    assert _call(n_index=0, minibatch=129)[0] == EINVAL


# ------------------------------------------------------------------------------------------ the Python surface
def test_the_learner_refuses_what_is_not_served_with_the_librarys_message():
    import torch

    from overcooked_ai_amd.bc import BCLearner
    from overcooked_ai_amd.policy import ActorCritic

    acts, index = torch.zeros(300, dtype=torch.uint8), torch.zeros(258, dtype=torch.int32)
    learner = BCLearner(ActorCritic(96, 40, 24, seed=3))
    with pytest.raises(ValueError, match=re.escape("oc_bc_epoch_fused: " + SERVED)):
        learner.epoch(torch.zeros((300, 96)), acts, index, 129, fused=True)
    with pytest.raises(ValueError, match=re.escape("oc_bc_epoch_fused: " + SERVED)):
        learner.update(torch.zeros((300, 96)), acts, index[:129], fused=True)
    wide = BCLearner(ActorCritic(116, 64, 64, seed=3))
    with pytest.raises(ValueError, match=re.escape("oc_bc_epoch_fused: " + DIMS)):
        wide.epoch(torch.zeros((300, 116)), acts, index, 64, fused=True)
    # a served shape on host tensors comes as far as every other call: there is no CPU fallback
    for call in (lambda: learner.epoch(torch.zeros((300, 96)), acts, index, 64, fused=True), lambda: learner.update(torch.zeros((300, 96)), acts, index[:128], fused=True),
                 lambda: learner.epoch(torch.zeros((300, 96)), acts, index, 129)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    assert learner._scratch == {}


# ------------------------------------------------------------------------------------------ the case list
def test_the_case_list_covers_what_it_says():
    cases = FC.CASES
    assert len({c.id for c in cases}) == len(cases)
    plain = [c for c in cases if not c.special]
    assert {c.M for c in plain if c.n == c.M} == {1, 31, 32, 33, 64, 96, 97, 128}
    assert {(c.in_dim, c.h1, c.h2) for c in plain if c.n == 150 and c.M == 64} == {(d, *h) for d in FC.SERVED_IN_DIMS for h in ((64, 64), (40, 24))}
    assert {(c.weights, c.clip) for c in plain if c.n == 130} == {(w, k) for w in ("off", "on", "zero") for k in (False, True)}
    assert all(c.M <= FC.MAX_ROWS and c.in_dim in FC.SERVED_IN_DIMS for c in cases)
    assert {c.special for c in cases} == {"", "middle_out", "nan_left_out", "nan_kept", "chain"}
    for c in cases:
        feats, actions, index, cw, weights = FC.arrays_of(c)
        R = len(actions)
        assert feats.shape == (R, c.in_dim) and index.shape == (c.n,) and index.dtype == np.int32 and actions.dtype == np.uint8
        assert (cw is None) == (c.weights == "off") and (cw is None or ((cw == 0).sum() == (c.weights == "zero") and (cw >= 0).all()))
        assert [w.shape for w in weights] == [(c.in_dim, c.h1), (c.h1,), (c.h1, c.h2), (c.h2,), (c.h2, 6), (6,), (c.h2, 1), (1,)] or \
            [w.size for w in weights] == [c.in_dim * c.h1, c.h1, c.h1 * c.h2, c.h2, c.h2 * 6, 6, c.h2, 1]
        out, mbs = FC.left_out(c), FC.minibatches(c)
        assert len(mbs) == -(-c.n // c.M) and mbs[-1][1] == c.n and FC.kept_counts(c) == [int((~out[lo:hi]).sum()) for lo, hi in mbs]
        ix = index.astype(np.int64)
        want = np.array([not (0 <= i < R) or actions[i] > 5 for i in ix])
        assert (out == want).all()
        if c.n >= 64 and c.special in ("", "nan_kept"):  # repeats, out of range on both sides, actions above 5 that are named
            assert len(np.unique(ix)) < c.n and (ix < 0).any() and (ix >= R).any() and (actions[ix[(ix >= 0) & (ix < R)]] > 5).any(), c.id
        if not c.special:
            assert np.isfinite(feats).all()
    c = next(c for c in cases if c.special == "middle_out")
    assert FC.kept_counts(c)[1] == 0 and min(FC.kept_counts(c)[0], FC.kept_counts(c)[2]) > 0 and len(FC.minibatches(c)) == 3
    c = next(c for c in cases if c.special == "nan_left_out")
    feats, actions, index, _, _ = FC.arrays_of(c)
    assert c.M == 64 and FC.left_out(c)[32:].all() and not FC.left_out(c)[:32].any() and np.isnan(feats[index[32:]]).any(axis=1).all() \
        and np.isfinite(feats[index[:32]]).all()
    c = next(c for c in cases if c.special == "nan_kept")
    feats, actions, index, _, _ = FC.arrays_of(c)
    rows = [i for i in range(c.n) if 0 <= index[i] < len(actions) and np.isnan(feats[index[i]]).any()]
    assert rows and all(c.M <= i < 2 * c.M for i in rows) and not FC.left_out(c)[rows].all()
    c = next(c for c in cases if c.special == "chain")
    assert c.n == FC.per_launch() + 1 and c.M == 1
