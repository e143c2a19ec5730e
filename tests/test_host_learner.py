"""oc_adam_step / oc_ppo_update without a GPU: the restatement of tests/learner_cases.py against its float64 reference (H1) and
against torch's clip_grad_norm_ + torch.optim.Adam on CPU tensors (H2), the plans, every refusal — made before any device call: this
host has no device —, the structs against the header (H3), the clock's running products against beta ** t (H4), and the Python
surface's own refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import learner_cases as LC
from case_support import P, ROOT

EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ H1, H2, H4: the arithmetic
def test_h1_the_recorded_error_is_the_measured_one():
    """F32_ERROR is the largest error of adam_f32's parameters and moments against adam_f64's over every step of every case: no
    smaller than what is measured here, and no more than twice it."""
    worst, where = 0.0, None
    for c in LC.CASES:
        for t, ((s32, i32), (s64, i64)) in enumerate(zip(LC.trajectory_of(c), LC.reference_of(c))):
            err = LC.state_error(s32, s64)
            if err > worst:
                worst, where = err, (c.id, t)
            assert np.array_equal(s32.clock, s64.clock), (c.id, t)  # the clock is float64 in both
            assert i32[3] == i64[3] == (0.0 if LC.inputs_of(c)[1][t].good else 1.0), (c.id, t)
            if np.isfinite(i64[0]):
                assert abs(i32[0] - i64[0]) <= 1e-6 * i64[0] and abs(i32[1] - i64[1]) <= 1e-6, (c.id, t, i32, i64)
    print("largest error of adam_f32 over %d cases x %d steps: %.4g (%s, step %d)" % (len(LC.CASES), LC.STEPS, worst, *where))
    assert LC.F32_ERROR / 2 <= worst <= LC.F32_ERROR, (worst, LC.F32_ERROR)
    assert LC.DEVICE_FACTOR == 4


def test_h1_the_cases_cover_what_they_must():
    assert {(c.in_dim, c.h1, c.h2) for c in LC.CASES} == {(56, 1, 1), (96, 33, 17), (96, 64, 64), (136, 64, 64)}
    assert {c.pattern for c in LC.CASES} == {"below", "above", "off", "zero", "nan", "inf", "scale0", "scale_count"}
    assert [LC.n_of(*s) for s in ((56, 1, 1), (96, 64, 64), (136, 64, 64))] == [73, 10823, 13383]
    for c in LC.CASES:
        params, steps = LC.inputs_of(c)
        traj = LC.trajectory_of(c)
        assert len(steps) == 3 and [tuple(p.shape) for p in params] == list(LC.shapes(c.in_dim, c.h1, c.h2))
        infos = [i for _, i in traj]
        if c.pattern == "below":
            assert all(i[0] < 0.1 * c.hyper.max_grad_norm and i[1] == 1.0 for i in infos), c.id
        if c.pattern == "above":
            assert all(i[0] > 10 * c.hyper.max_grad_norm and i[1] < 0.1 for i in infos), c.id
        if c.pattern in ("off", "inf"):
            assert c.hyper.max_grad_norm is None and all(i[1] == 1.0 for i in infos if i[3] == 0), c.id
        if c.pattern == "zero":
            assert infos[1][0] == 0.0 and infos[2][0] == 0.0 and infos[1][3] == 0.0
            assert not np.array_equal(traj[1][0].params, traj[2][0].params) or c.h1 == 1  # the momentum moves them
        if c.pattern in ("nan", "inf", "scale0"):
            assert [i[3] for i in infos] == [0.0, 1.0, 0.0], c.id
            (a, _), (b, _), (d, _) = traj
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a.clock[:3], b.clock[:3])
            assert b.clock[3] == 1.0 and d.clock[0] == 2.0 and d.clock[3] == 1.0
            assert np.isnan(infos[1][0]) if c.pattern == "nan" else np.isinf(infos[1][0]) if c.pattern == "inf" else infos[1][0] == 0.0
        if c.pattern == "scale_count":
            assert [i[2] for i in infos] == [float(np.float32(1.0 / (37 + t))) for t in range(3)]
        if c.pattern not in ("nan", "inf", "scale0"):
            assert traj[-1][0].clock.tolist()[0] == 3.0 and traj[-1][0].clock[3] == 0.0
        for s, _ in traj:
            assert np.isfinite(s.params).all() and np.isfinite(s.m).all() and np.isfinite(s.v).all() and not (s.params == LC.FILL).any()


def _torch_steps(c, n_steps, seed):
    """(adam_f32's States, torch's States) over n_steps steps of fresh N(0, sigma) gradients"""
    import torch

    params, _ = LC.inputs_of(c)
    rng = np.random.default_rng(seed)
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    h = c.hyper
    # (torch takes its hyperparameters as Python floats: it is given the float32 values the C call takes, widened — with a beta2 of
    #  0.999 as typed, its 1 - beta2 would differ from the float32 one by 1.3e-5 of itself, a difference of inputs, not of arithmetic)
    w = lambda x: float(np.float32(x))  # noqa: E731
    opt = torch.optim.Adam(tp, lr=w(h.lr), betas=(w(h.beta1), w(h.beta2)), eps=w(h.eps))
    s, mine, theirs = LC.state0(params), [], []
    for t in range(n_steps):
        sigma = 10.0 ** rng.integers(-3, 1)
        grads = [(sigma * rng.standard_normal(p.shape)).astype(np.float32) for p in params]
        s, _ = LC.adam_f32(s, grads, h, None)
        for p, g in zip(tp, grads):
            p.grad = torch.from_numpy(g.copy())
        if h.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(tp, w(h.max_grad_norm))
        opt.step()
        theirs.append(LC.State(LC.flat([p.detach().numpy() for p in tp]), LC.flat([opt.state[p]["exp_avg"].numpy() for p in tp]),
                               LC.flat([opt.state[p]["exp_avg_sq"].numpy() for p in tp]), None))
        mine.append(s)
    return mine, theirs


@pytest.mark.parametrize("c", [c for c in LC.CASES if c.pattern in ("below", "above", "off")], ids=lambda c: c.id)
def test_h2_the_restatement_is_torch_s_clip_grad_norm_and_adam(c):
    mine, theirs = _torch_steps(c, 10, c.seed + 5000)
    worst = max(LC.state_error(a, b) for a, b in zip(mine, theirs))
    print("%s: largest error against torch over 10 steps / (4 * F32_ERROR) %.3g" % (c.id, worst / (LC.DEVICE_FACTOR * LC.F32_ERROR)))
    assert worst <= LC.DEVICE_FACTOR * LC.F32_ERROR, (c.id, worst)
    assert LC.rel(mine[-1].params, mine[0].params) > 100 * LC.F32_ERROR  # (the steps moved the parameters)


def test_h4_the_running_products_are_the_powers():
    """The clock's p *= (double)beta against beta ** t in float64: t roundings of half an ulp each bound the running product's
    relative error by t * 2^-53 (first order), and pow's own is below an ulp.  Of these betas only 0.9 reaches the subnormal range
    within 10 000 steps, where a product is rounded to a multiple of 2^-1074 instead: at most half of that per step, shrinking by 0.9
    per later step — 0.5 / (1 - 0.9) = 5 of them in all."""
    for beta in (0.9, 0.999, 0.5, 0.0, 0.99999):
        b = float(np.float32(beta))
        p = 1.0
        for t in range(1, 10001):
            p *= b
            want = b ** t
            if want > 0:
                assert abs(p - want) <= (t + 2) * 2.0 ** -53 * want + 5 * 2.0 ** -1074, (beta, t)
            else:
                assert p == 0.0 or p < 1e-300, (beta, t)


# ------------------------------------------------------------------------------------------ H3: the ABI, the plans, the refusals
def test_h3_exports_and_structs_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_adam_step", "oc_adam_plan", "oc_ppo_update", "oc_ppo_update_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    A, U = _lib.OcAdam, _lib.OcPpoUpdate
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct OcAdam \{(.*?)\} OcAdam;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(d_\w+|lr|beta1|beta2|eps|max_grad_norm)\b", body) == [f[0] for f in A._fields_]
    assert [getattr(A, f).offset for f, _ in A._fields_] == [0, 64, 128, 136, 144, 152, 156, 160, 164, 168] and ctypes.sizeof(A) == 176
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct OcPpoUpdate \{(.*?)\} OcPpoUpdate;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(d_\w+|n_feature_rows|n_index|minibatch|grads)\b", body) == [f[0] for f in U._fields_]
    assert [getattr(U, f).offset for f, _ in U._fields_] == list(range(0, 96, 8)) + [152, 160] and ctypes.sizeof(U) == 168
    assert "int oc_adam_step(const OcActorCritic* params, const OcPolicyGrads* grads, const OcAdam* adam, void* stream);" in hdr
    assert "int oc_adam_plan(int in_dim, int h1, int h2, char* out, size_t out_size);" in hdr
    assert "int oc_ppo_update(const OcActorCritic* policy, const OcPpoLoss* loss, const OcAdam* adam, const OcPpoUpdate* update, void* stream);" in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr
    for words in ("i % 256 == l in", "s[l] += s[l + k] for k = 128, 64, ..., 1", "norm = (float)sqrt(s[0])", "c = min(max_grad_norm / (norm + 1e-6f), 1.0f)",
                  "The step is skipped if norm is not finite", "increments skipped", "running products, not pow",
                  "m_i = m_i + (g_i - m_i) * (1 - beta1)", "v_i = v_i * beta2 + (g_i * g_i) * (1 - beta2)", "den = sqrtf(v_i) / rbc2s + eps",
                  "p_i = p_i - step_size * (m_i / den)", "No atomics", "on those RAW gradients", "before the FIRST launch"):
        assert words in hdr, words


def test_h3_the_plans_words_carry_their_numbers():
    from overcooked_ai_amd import _lib, learner, policy, ppo_loss

    hdr = _header()
    assert learner.plan_adam() in hdr
    for in_dim, h1, h2 in LC.SHAPES + ((76, 40, 24),):
        n = LC.n_of(in_dim, h1, h2)
        text = learner.plan_adam(in_dim, h1, h2)
        assert text.startswith("k_adam_step grid=1, 256 lanes, %d elements (%d per lane)" % (n, (n + 255) // 256)), text
    whole = learner.plan_update(16 * 4096, 4096)
    assert whole.startswith("16 minibatch(es) of 4096 rows (the last 4096), no host synchronisation")
    for quoted in (policy.plan(4096, index=True), ppo_loss.plan_ppo_loss(4096, index=True), policy.plan(4096, index=True, backward=True), learner.plan_adam()):
        assert "[" + quoted + "]" in whole, quoted
    assert whole.endswith("scratch: logits 4096 x 6 f32, values 4096 f32, grad_logits 4096 x 6 f32, grad_values 4096 f32, loss partials 4 x 6 f64, "
                          "policy partials 32 x 10823 f32, gradients 10823 f32; out: stats 16 x 8 f64, info 16 x 4 f64")
    for n, M, in_dim in ((1, 1, 96), (33, 33, 56), (1000, 488, 96), (70000, 32801, 96), (5, 4096, 136), (12000, 2000, 136)):
        text = learner.plan_update(n, M, in_dim, 64, 64, seat=True, moments=True, old_logits=True)
        K, rows = (n + M - 1) // M, min(n, M)
        assert text.startswith("%d minibatch(es) of %d rows (the last %d)" % (K, rows, n - (K - 1) * M)), text
        assert "k_ppo_loss<OLD=true>" in text and "seat=yes moments=yes" in text
        assert learner.scratch_rows(n, M, in_dim, 64, 64) == (rows, (rows + ppo_loss.partial_samples() - 1) // ppo_loss.partial_samples(),
                                                             *policy.partials_shape(rows, in_dim, 64, 64)), text
        assert "out: stats %d x 8 f64, info %d x 4 f64" % (K, K) in text
    assert learner.plan_update(0, 4096).startswith("nothing to launch (no index); scratch: ")
    L = _lib.load()
    out = ctypes.create_string_buffer(2048)
    assert L.oc_adam_plan(96, 64, 64, None, 0) == EINVAL and L.oc_last_error() == b"oc_adam_plan: no output buffer"
    assert L.oc_ppo_update_plan(10, 5, 96, 64, 64, 0, 0, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_ppo_update_plan: no output buffer"
    for args, why in (((97, 64, 64), "policy.in_dim must be a feature length"), ((96, 0, 64), "policy.h1 and policy.h2 must be in 1..64"),
                      ((96, 64, 65), "policy.h1 and policy.h2 must be in 1..64")):
        assert L.oc_adam_plan(*args, out, len(out)) == EINVAL and L.oc_last_error().decode().startswith("oc_adam_step: " + why)
        assert L.oc_ppo_update_plan(10, 5, *args, 0, 0, 0, out, len(out)) == EINVAL and L.oc_last_error().decode().startswith("oc_ppo_update: " + why)
    for n, M, why in ((-1, 5, "n_index < 0"), (2 ** 31, 5, "n_index must be below 2^31"), (10, 0, "minibatch < 1"), (10, -3, "minibatch < 1")):
        assert L.oc_ppo_update_plan(n, M, 96, 64, 64, 0, 0, 0, out, len(out)) == EINVAL and L.oc_last_error().decode() == "oc_ppo_update: " + why


_W = ("d_w1", "d_b1", "d_w2", "d_b2", "d_wp", "d_bp", "d_wv", "d_bv")


def _adam_structs(v):
    from overcooked_ai_amd import _lib

    ptrs = ctypes.c_void_p * 8
    pol = _lib.OcActorCritic(*[v[f] for f in _W], v["in_dim"], v["h1"], v["h2"])
    grads = _lib.OcPolicyGrads(*[v["g_" + f] for f in _W])
    ad = _lib.OcAdam(ptrs(*v["m"]), ptrs(*v["v"]), v["d_clock"], v["d_grad_scale"], v["d_info"], v["lr"], v["beta1"], v["beta2"], v["eps"], v["max_grad_norm"])
    return pol, grads, ad


def _defaults():
    return dict({f: P for f in _W}, **{"g_" + f: P for f in _W}, m=[P] * 8, v=[P] * 8, in_dim=96, h1=64, h2=64, d_clock=P, d_grad_scale=P, d_info=P,
                lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.1)


def _adam_refusals():
    nan, inf = float("nan"), float("inf")
    out = [({f: None}, "NULL weight or bias array") for f in _W] + [({f: P + 2}, "weight and bias arrays must be 4-byte aligned") for f in _W]
    out += [({"g_" + f: None}, "NULL gradient array") for f in _W] + [({"g_" + f: P + 1}, "gradient arrays must be 4-byte aligned") for f in _W]
    for k in range(8):
        for which in ("m", "v"):
            out.append(({which: [None if j == k else P for j in range(8)]}, "NULL moment array"))
            out.append(({which: [P + 2 if j == k else P for j in range(8)]}, "moment arrays must be 4-byte aligned"))
    out += [(dict(d_clock=None), "adam.d_clock is NULL")]
    out += [({f: P + 4}, "adam.d_clock, adam.d_grad_scale and adam.d_info must be 8-byte aligned") for f in ("d_clock", "d_grad_scale", "d_info")]
    out += [(dict(in_dim=100), "policy.in_dim must be a feature length"), (dict(h1=0), "policy.h1 and policy.h2 must be in 1..64"),
            (dict(h2=65), "policy.h1 and policy.h2 must be in 1..64")]
    out += [(dict(lr=x), "adam.lr must be finite and >= 0") for x in (-1e-3, nan, inf)]
    out += [(kw, "adam.beta1 and adam.beta2 must be in [0, 1)") for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=nan))]
    out += [(dict(eps=x), "adam.eps must be positive") for x in (0.0, -1e-8, nan)]
    out += [(dict(max_grad_norm=nan), "adam.max_grad_norm is NaN")]
    return out


def test_h3_oc_adam_step_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()

    def call(pol=(), grads=(), ad=(), **kw):
        v = _defaults()
        v.update(kw)
        s = _adam_structs(v)
        pol, grads, ad = (s[0] if pol == () else pol), (s[1] if grads == () else grads), (s[2] if ad == () else ad)
        ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        return L.oc_adam_step(ref(pol), ref(grads), ref(ad), None), L.oc_last_error().decode()

    cases = [(dict(pol=None), "params is NULL"), (dict(grads=None), "grads is NULL"), (dict(ad=None), "adam is NULL")] + _adam_refusals()
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith("oc_adam_step: " + why), (kw, rc, msg)


def test_h3_oc_ppo_update_makes_every_refusal_of_every_stage_before_its_first_launch():
    """With stand-in pointers and more than one minibatch: a refusal behind the first launch would come behind a fault, and this host
    has no device.  The stages' refusals come in their own words under oc_ppo_update's name."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    loss_fields = [f for f, _ in _lib.OcPpoLoss._fields_]
    upd_fields = [f for f, _ in _lib.OcPpoUpdate._fields_ if f != "grads"]

    def call(pol=(), loss=(), ad=(), upd=(), **kw):
        v = _defaults()
        v.update(d_grad_scale=None, d_info=None)
        q = dict(d_actions=P, d_logp_old=P, d_advantages=P, d_targets=P, d_seat=P, d_logits_old=P, d_moments=P, n_samples=3000, d_logits=None,
                 d_values=None, d_index=None, first_sample=0, n_minibatch=0, d_grad_logits=None, d_grad_values=None, d_partials=None, d_stats=None,
                 d_terms_out=None, clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.1, kl_coeff=0.2)
        u = dict(d_features=P, n_feature_rows=3000, d_index=P, n_index=2500, minibatch=1000, d_logits=P, d_values=P, d_grad_logits=P, d_grad_values=P,
                 d_loss_partials=P, d_policy_partials=P, d_stats=P, d_info=P)
        for k, x in kw.items():
            if k.startswith("q_"):
                q[k[2:]] = x
            elif k.startswith("u_"):
                u[k[2:]] = x
            else:
                v[k] = x
        s = _adam_structs(v)
        pol, ad = (s[0] if pol == () else pol), (s[2] if ad == () else ad)
        loss = _lib.OcPpoLoss(*[q[f] for f in loss_fields]) if loss == () else loss
        if upd == ():
            upd = _lib.OcPpoUpdate(**{f: u[f] for f in upd_fields}, grads=s[1])
        ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        return L.oc_ppo_update(ref(pol), ref(loss), ref(ad), ref(upd), None), L.oc_last_error().decode()

    cases = [(dict(pol=None), "policy is NULL"), (dict(loss=None), "loss is NULL"), (dict(ad=None), "adam is NULL"), (dict(upd=None), "update is NULL"),
             (dict(u_n_index=-1), "n_index < 0"), (dict(u_n_index=2 ** 31), "n_index must be below 2^31"), (dict(u_minibatch=0), "minibatch < 1"),
             (dict(u_d_index=None), "update.d_index is NULL"), (dict(u_d_stats=None), "NULL update.d_stats or update.d_info"),
             (dict(u_d_info=None), "NULL update.d_stats or update.d_info"), (dict(u_d_loss_partials=None), "update.d_loss_partials is NULL"),
             (dict(u_d_info=P + 4), "update.d_info must be 8-byte aligned"),
             # oc_policy_forward's
             (dict(u_d_features=None), "rows.d_features is NULL"), (dict(u_d_features=P + 8), "rows.d_features must be 16-byte aligned"),
             (dict(u_d_index=P + 2), "rows.d_index must be 4-byte aligned"), (dict(u_n_feature_rows=-1), "rows.n_feature_rows < 0"),
             (dict(u_n_feature_rows=2 ** 31), "rows.n_feature_rows must be below 2^31 with d_index"),
             (dict(u_d_logits=None), "NULL d_logits or d_values"), (dict(u_d_values=None), "NULL d_logits or d_values"),
             (dict(u_d_values=P + 2), "d_values must be 4-byte aligned"),
             # oc_ppo_loss's
             (dict(q_d_actions=None), "NULL d_actions, d_logp_old"), (dict(u_d_grad_logits=None), "NULL d_actions, d_logp_old"),
             (dict(q_d_logp_old=P + 2), "d_logp_old, d_advantages, d_targets, d_values, d_index and d_grad_values must be 4-byte aligned"),
             (dict(q_d_moments=P + 4), "d_logits_old, d_moments, d_partials and d_stats must be 8-byte aligned"),
             (dict(u_d_stats=P + 4), "d_logits_old, d_moments, d_partials and d_stats must be 8-byte aligned"),
             (dict(u_d_logits=P + 8), "d_logits, d_grad_logits and d_terms_out must be 16-byte aligned"),
             (dict(u_d_grad_logits=P + 8), "d_logits, d_grad_logits and d_terms_out must be 16-byte aligned"),
             (dict(q_n_samples=-1), "n_samples < 0"), (dict(q_n_samples=3001), "n_samples must be even with d_seat"),
             (dict(q_n_samples=2 ** 31), "n_samples must be below 2^31 with d_index"), (dict(q_clip_param=0.0), "clip_param must be finite and positive"),
             (dict(q_vf_clip_param=float("inf")), "vf_clip_param must be finite and positive"),
             (dict(q_entropy_coeff=-0.1), "vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0"), (dict(q_d_logits_old=None), "kl_coeff > 0 needs d_logits_old"),
             # oc_policy_backward's
             (dict(u_d_grad_values=P + 2), "d_logp_old, d_advantages, d_targets, d_values, d_index and d_grad_values must be 4-byte aligned"),
             (dict(u_d_policy_partials=None), "d_partials is NULL"), (dict(u_d_policy_partials=P + 2), "d_partials must be 4-byte aligned")]
    # oc_adam_step's (d_grad_scale and d_info are the call's own)
    cases += [(kw, why) for kw, why in _adam_refusals() if not set(kw) & {"d_grad_scale", "d_info"}]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith("oc_ppo_update: " + why), (kw, rc, msg)
    # accepted, and nothing to launch: no index entries (every check is made all the same: see the refusal below)
    assert call(u_n_index=0)[0] == 0 and call(u_n_index=0, u_minibatch=1)[0] == 0
    rc, msg = call(u_n_index=0, lr=-1.0)
    assert rc == EINVAL and msg == "oc_ppo_update: adam.lr must be finite and >= 0"


# ------------------------------------------------------------------------------------------ the Python surface
def test_the_python_surface_validates_its_arguments():
    import torch

    from overcooked_ai_amd.learner import Adam, PPOLearner
    from overcooked_ai_amd.policy import NAMES, ActorCritic
    from overcooked_ai_amd.ppo_loss import LearnerBatch

    pol = ActorCritic(96, 40, 24, seed=3)
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(max_grad_norm=0.0),
               dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            Adam(pol, **kw)
    with pytest.raises(ValueError, match="must be an ActorCritic"):
        Adam(torch.nn.Linear(2, 2))
    opt = Adam(pol, lr=1e-3, max_grad_norm=0.1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        opt.step()
    state = opt.state_dict()
    assert list(state["m"]) == list(NAMES) and state["clock"].tolist() == [0.0, 1.0, 1.0, 0.0] and state["max_grad_norm"] == 0.1
    assert all(not t.any() and t.shape == p.shape for t, p in zip(state["m"].values(), pol.parameters()))
    state["clock"][0] = 5.0
    state["lr"] = 3e-4
    other = Adam(pol)
    other.load_state_dict(state)
    assert other.lr == 3e-4 and other.clock.tolist()[0] == 5.0 and other.state_dict()["clock"].tolist() == state["clock"].tolist()
    with pytest.raises(ValueError, match="clock must be a float64"):
        other.load_state_dict(dict(state, clock=torch.zeros(3, dtype=torch.float64)))
    with pytest.raises(ValueError, match=re.escape("m[w2] must be a float32 [40, 24]")):
        other.load_state_dict(dict(state, m=dict(state["m"], w2=torch.zeros(40, 23))))
    for p in pol.parameters():
        p.grad = torch.ones_like(p)
    opt.zero_grad()
    assert all(p.grad is not None and not p.grad.any() for p in pol.parameters())
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in pol.parameters())
    good = dict(lr=1e-3, clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.1)
    for kw in (dict(clip_param=0.0), dict(vf_clip_param=float("inf")), dict(entropy_coeff=-1.0), dict(kl_coeff=-0.1)):
        with pytest.raises(ValueError):
            PPOLearner(pol, **dict(good, **kw))
    learner = PPOLearner(pol, **good, max_grad_norm=0.1)
    assert PPOLearner(pol, 1e-3, 0.05, 10.0, 0.5, 0.1, 0.0, 0.1).hyper == learner.hyper  # (positionally, in the documented order)
    assert learner.adam.max_grad_norm == 0.1 and learner.adam.lr == 1e-3
    S = 24
    batch = LearnerBatch(torch.zeros(S, dtype=torch.uint8), torch.zeros(S), torch.zeros(S), torch.zeros(S), None, None, None)
    with pytest.raises(ValueError, match="no CPU fallback"):
        learner.update(torch.zeros((S, 96)), batch, torch.zeros(5, dtype=torch.int32))


def test_trajectory_buffer_permutation_is_what_minibatches_cuts():
    import types

    import torch

    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    buf = TrajectoryBuffer.__new__(TrajectoryBuffer)
    buf.tenv, buf.T, buf.n_envs, buf.values = types.SimpleNamespace(_torch=torch), 5, 7, torch.zeros((5, 7, 2))
    perm = buf.permutation(generator=torch.Generator().manual_seed(4))
    assert perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(70))
    cut = list(buf.minibatches(32, generator=torch.Generator().manual_seed(4)))
    assert [len(x) for x in cut] == [32, 32, 6] and torch.equal(torch.cat(cut), perm)
