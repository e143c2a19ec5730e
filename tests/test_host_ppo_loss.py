"""oc_ppo_loss without a GPU: the exports and the struct against the header, the plan's words, every refusal (made before any device
call: this host has no device), the two restatements of tests/ppo_loss_cases.py against each other and the tolerances recorded
there, the reference's analytic gradients against torch autograd in float64, the bands, and the Python surface's own refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import ppo_loss_cases as PC
from case_support import P, ROOT

EINVAL = -1
WHO = "oc_ppo_loss: "


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_struct_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_ppo_loss", "oc_ppo_loss_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    body = re.search(r"typedef struct OcPpoLoss \{(.*?)\} OcPpoLoss;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(d_\w+|n_samples|first_sample|n_minibatch|clip_param|vf_clip_param|vf_loss_coeff|entropy_coeff|kl_coeff)\b", body)
    Q = _lib.OcPpoLoss
    assert names == [f[0] for f in Q._fields_]
    # seven pointers, an int64, three pointers, two int64, five pointers, five floats
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == list(range(0, 144, 8)) + [144, 148, 152, 156, 160] and ctypes.sizeof(Q) == 168
    assert "int oc_ppo_loss(const OcPpoLoss* q, void* stream);" in hdr
    assert ("int oc_ppo_loss_plan(int64_t n_minibatch, int with_index, int with_seat, int with_moments, int with_old_logits, "
            "int with_terms, char* out, size_t out_size);") in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_arithmetic_the_references_restate():
    hdr = _header()
    for words in ("S = ((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5", "lp_i = d_i - logf(S);  p_i = w_i / S;  logp = lp_a",
                  "ratio = expf(logp - d_logp_old[s])", "std = max(sqrt(max(s2 / n - mean * mean, 0)), 1e-4)",
                  "s2 = min(max(ratio, lo), hi) * A^", "t_i = 0 where p_i == 0", "vfc = min(vf, vf_clip_param)",
                  "g = (s1 <= s2) ? -s1 : 0", "(entropy_coeff * p_i) * (lp_i + H)", "kl_coeff * (p_i - q_i)",
                  "d_seat[s >> 1] == (s & 1)", "+0.0f", "by a select", "added in ascending k", "No floating-point atomics"):
        assert words in hdr, words


def _plan(M, *flags):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    rc = L.oc_ppo_loss_plan(M, *(list(flags) + [0] * (5 - len(flags))), out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def test_the_plan_in_words_and_the_partial_size():
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.ppo_loss import plan_ppo_loss

    Pn = PC.partial_samples()
    assert Pn == 1024
    rc, text = _plan(2 ** 22, 1, 1, 1, 1, 0)
    assert rc == 0 and text == ("k_ppo_loss<OLD=true> grid=4096, 256 lanes (one per sample, 4 tiles of 256), 1024 samples per partial, "
                                "index=yes seat=yes moments=yes terms=no + k_ppo_loss_stats grid=1, 64 lanes, 4096 partial(s) (with d_stats)"), text
    assert text in _header() and plan_ppo_loss(2 ** 22, index=True, seat=True, moments=True, old_logits=True) == text
    for M, flags in ((1, (0, 0, 0, 0, 0)), (256, (0, 1, 0, 0, 1)), (257, (1, 0, 1, 0, 0)), (65 * Pn + 3, (1, 1, 1, 1, 1))):
        rc, text = _plan(M, *flags)
        yn = ["yes" if f else "no" for f in flags]
        grid = (M + Pn - 1) // Pn
        assert rc == 0 and text.startswith("k_ppo_loss<OLD=%s> grid=%d, 256 lanes" % ("true" if flags[3] else "false", grid)), text
        assert "index=%s seat=%s moments=%s terms=%s" % (yn[0], yn[1], yn[2], yn[4]) in text and "%d partial(s)" % grid in text
    assert _plan(0) == (0, "nothing to launch (no samples)") and _plan(0, 1, 1, 1, 1, 1) == (0, "nothing to launch (no samples)")
    rc, msg = _plan(-1)
    assert rc == EINVAL and msg == WHO + "n_minibatch < 0"
    with pytest.raises(_lib.OcAmdError, match="oc_ppo_loss: n_minibatch < 0"):
        plan_ppo_loss(-1)
    L = _lib.load()
    assert L.oc_ppo_loss_plan(4, 0, 0, 0, 0, 0, None, 0) == EINVAL and L.oc_last_error() == b"oc_ppo_loss_plan: no output buffer"


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    fields = [f for f, _ in _lib.OcPpoLoss._fields_]
    pointers = [f for f in fields if f.startswith("d_")]

    def call(q=(), **kw):
        if q == ():
            v = dict({f: P for f in pointers}, n_samples=4000, first_sample=10, n_minibatch=1000, clip_param=0.05, vf_clip_param=10.0,
                     vf_loss_coeff=0.5, entropy_coeff=0.1, kl_coeff=0.2)
            v.update(kw)
            q = _lib.OcPpoLoss(*[v[f] for f in fields])
        rc = L.oc_ppo_loss(ctypes.byref(q) if q is not None else None, None)
        return rc, L.oc_last_error().decode()

    required = "NULL d_actions, d_logp_old, d_advantages, d_targets, d_logits, d_values, d_grad_logits or d_grad_values"
    aligned4 = "d_logp_old, d_advantages, d_targets, d_values, d_index and d_grad_values must be 4-byte aligned"
    aligned8 = "d_logits_old, d_moments, d_partials and d_stats must be 8-byte aligned"
    aligned16 = "d_logits, d_grad_logits and d_terms_out must be 16-byte aligned"
    contiguous = "first_sample .. first_sample + n_minibatch must lie inside 0 .. n_samples without d_index"
    inf, nan = float("inf"), float("nan")
    refusals = [(dict(q=None), "loss is NULL")]
    refusals += [({f: None}, required) for f in ("d_actions", "d_logp_old", "d_advantages", "d_targets", "d_logits", "d_values",
                                                 "d_grad_logits", "d_grad_values")]
    refusals += [({f: P + 2}, aligned4) for f in ("d_logp_old", "d_advantages", "d_targets", "d_values", "d_index", "d_grad_values")]
    refusals += [({f: P + 4}, aligned8) for f in ("d_logits_old", "d_moments", "d_partials", "d_stats")]
    refusals += [({f: P + 8}, aligned16) for f in ("d_logits", "d_grad_logits", "d_terms_out")]
    refusals += [(dict(n_minibatch=-1), "n_minibatch < 0"), (dict(n_samples=-1), "n_samples < 0")]
    refusals += [(dict(n_samples=2 ** 31), "n_samples must be below 2^31 with d_index"), (dict(n_samples=3999), "n_samples must be even with d_seat")]
    refusals += [(dict(d_index=None, **kw), contiguous) for kw in (dict(first_sample=3001), dict(first_sample=-1), dict(first_sample=4001, n_minibatch=0),
                                                                   dict(n_samples=998, first_sample=0), dict(first_sample=2 ** 62, n_minibatch=2 ** 37))]
    refusals += [(dict(clip_param=x), "clip_param must be finite and positive") for x in (0.0, -0.1, inf, nan)]
    refusals += [(dict(vf_clip_param=x), "vf_clip_param must be finite and positive") for x in (0.0, -10.0, inf, nan)]
    refusals += [({f: x}, "vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0") for f in ("vf_loss_coeff", "entropy_coeff", "kl_coeff")
                 for x in (-1e-3, nan)]
    refusals += [(dict(d_logits_old=None), "kl_coeff > 0 needs d_logits_old"), (dict(d_partials=None), "d_stats needs d_partials")]
    for kw, why in refusals:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith(WHO + why), (kw, rc, msg)
    # accepted, and nothing to launch (no stats asked for: zeroing them is a device call): no rows; the optional arrays absent; the
    # minimum alignments; actions and seats at odd addresses; an index with the most samples it can name; the whole batch contiguous
    for kw in (dict(), dict(d_seat=None, d_moments=None, d_terms_out=None, d_index=None), dict(d_logits_old=None, kl_coeff=0.0),
               dict(d_logp_old=P + 4, d_values=P + 12, d_index=P + 4, d_grad_values=P + 4, d_logits_old=P + 8, d_moments=P + 8,
                    d_logits=P + 16, d_grad_logits=P + 48, d_terms_out=P + 16), dict(d_actions=P + 1, d_seat=P + 3),
               dict(n_samples=2 ** 31 - 1, d_seat=None), dict(d_index=None, n_samples=2 ** 40, first_sample=2 ** 40),
               dict(vf_loss_coeff=0.0, entropy_coeff=0.0, kl_coeff=0.0)):
        assert call(n_minibatch=0, d_partials=None, d_stats=None, **kw)[0] == 0, kw


# ------------------------------------------------------------------------------------------ the arithmetic
def test_a_hand_computed_sample():
    """Uniform logits (p_i = 1/6, H = ln 6), logp_old = ln(1/6) - ln 2 so that the ratio is 2, advantage 3, clip 0.2: s1 = 6,
    s2 = 1.2 * 3 = 3.6, surr = 3.6 and no policy gradient; vf = (1 - 4)^2 = 9 under a clip of 10."""
    a = types.SimpleNamespace(S=2, M=1, actions=np.array([2, 0], np.uint8), logp_old=np.array([np.log(1 / 12), 0], np.float32),
                              advantages=np.array([3, 0], np.float32), targets=np.array([4, 0], np.float32), seat=None, logits_old=None,
                              moments=None, logits=np.zeros((1, 6), np.float32), values=np.array([1], np.float32), index=None, first=0,
                              sample=np.array([0], np.int64))
    c = PC.Case("hand", 1, "contiguous", 0, "none", False, False, True, 0.2, 10.0, 0.5, 0.25, 0.0, False, 0)
    r = PC.loss_f64(c, a)
    assert abs(r.ratio[0] - 2) < 1e-6 and abs(r.terms[0, 0] - 3 * float(np.float32(1.2))) < 1e-6 and r.terms[0, 1] == 9
    assert abs(r.terms[0, 2] - np.log(6)) < 1e-12 and abs(r.terms[0, 3] - (a.logp_old[0] - np.log(1 / 6))) < 1e-12
    assert np.abs(r.grad_logits).max() < 1e-15  # (clipped: no policy gradient; uniform: no entropy gradient)
    assert r.grad_values[0] == 0.5 * 2 * (1 - 4) and r.sums.tolist()[:1] == [1] and r.sums[5] == 1
    assert abs(r.stats[1] - (-r.terms[0, 0] + 0.5 * 9 - 0.25 * np.log(6))) < 1e-12 and r.stats[6] == 1 and r.stats[7] == 1
    # the advantage -3: s1 = -6 <= s2 = -3.6, the unclipped branch, gradient -A^ ratio ([i == a] - p_i)
    a.advantages = np.array([-3, 0], np.float32)
    r = PC.loss_f64(c, a)
    assert abs(r.terms[0, 0] + 6) < 1e-5 and abs(r.grad_logits[0, 2] - 6 * (1 - 1 / 6)) < 1e-5 and abs(r.grad_logits[0, 0] + 6 / 6) < 1e-5
    # vf beyond its clip: no value gradient; the partner's sample: zeros and no count
    c2 = c._replace(vf_clip=8.0)
    r = PC.loss_f64(c2, a)
    assert r.terms[0, 1] == 8 and r.grad_values[0] == 0
    a.seat = np.array([0], np.uint8)
    r = PC.loss_f32(c, a)
    assert not r.terms.any() and not r.grad_logits.any() and not r.grad_values.any() and not r.stats.any() and r.left_out.all()
    assert not np.signbit(r.grad_logits).any() and r.terms.dtype == np.float32


def test_the_recorded_tolerances_are_the_measured_ones():
    """The figures of the cases file are what loss_f32 and loss_f64 give over the case list: none smaller than what is measured here.
    numpy's f32 exp and log differ by an ulp between its SIMD paths, so the lower side is only that a recorded figure is no more than
    twice the measured one.  The device is held to four times the largest."""
    worst = dict(ratio=0.0, vf=0.0, all=0.0)
    for c in PC.CASES:
        r32, r64 = PC.loss_f32(c), PC.reference_of(c)
        assert np.array_equal(r32.left_out, r64.left_out)
        keep = ~r64.left_out
        near_ratio, near_vf = PC.bands(c)
        worst["ratio"] = max(worst["ratio"], PC.rel_error(r32.ratio, r64.ratio, keep))
        worst["vf"] = max(worst["vf"], PC.rel_error(r32.vf, r64.vf, keep))
        worst["all"] = max(worst["all"], PC.rel_error(r32.terms, r64.terms), PC.rel_error(r32.grad_logits, r64.grad_logits, ~near_ratio),
                           PC.rel_error(r32.grad_values, r64.grad_values, ~near_vf))
    print("largest |loss_f32 - loss_f64| / max(1, |loss_f64|) over %d cases: %.4g (ratio %.4g, vf %.4g)"
          % (len(PC.CASES), worst["all"], worst["ratio"], worst["vf"]))
    for key, recorded in (("all", PC.F32_ERROR), ("ratio", PC.RATIO_ERROR), ("vf", PC.VF_ERROR)):
        assert recorded / 2 <= worst[key] <= recorded, (key, worst[key], recorded)
    assert PC.DEVICE_TOL == 4 * PC.F32_ERROR and PC.RATIO_BAND == 4 * PC.RATIO_ERROR and PC.VF_BAND == 4 * PC.VF_ERROR


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_the_bands_hold_few_rows_and_no_result_equals_the_sentinel(c):
    ref = PC.reference_of(c)
    near_ratio, near_vf = PC.bands(c)
    assert near_ratio.sum() <= PC.BAND_CAP * c.M and near_vf.sum() <= PC.BAND_CAP * c.M, (int(near_ratio.sum()), int(near_vf.sum()))
    for x in (ref.terms, ref.grad_logits, ref.grad_values, ref.sums, ref.stats):  # an element that still holds the fill was not written
        assert not (x == PC.FILL).any() and not np.isnan(x).any(), c.id
    assert not ref.terms[ref.left_out].any() and not ref.grad_logits[ref.left_out].any() and not ref.grad_values[ref.left_out].any()
    assert ref.sums[0] == (~ref.left_out).sum()


def _torch_textbook(c, a, rows):
    """The textbook expression in torch float64 on rows `rows` (learner samples): per-sample -surr + vf_coeff * vfc - ent * H +
    kl_coeff * kl with torch.min, torch.clamp and log_softmax -> its sum's gradients with respect to logits and values.  A -inf
    logit is given as -1e300: its probability is exactly 0 all the same and its log-probability finite, so autograd meets no 0 * inf
    (the limit, which is what the header's selects give)."""
    import torch

    f32 = np.float32
    s = a.sample[rows]
    logits = torch.tensor(np.where(np.isinf(a.logits[rows]), -1e300, a.logits[rows].astype(np.float64)), requires_grad=True)
    values = torch.tensor(a.values[rows].astype(np.float64), requires_grad=True)
    act = torch.tensor(a.actions[s].astype(np.int64))
    A = a.advantages[s].astype(np.float64)
    if a.moments is not None:
        n, m1, m2 = (float(x) for x in a.moments)
        mean = m1 / n
        A = (A - mean) / max(np.sqrt(max(m2 / n - mean * mean, 0.0)), 1e-4)
    A = torch.tensor(A)
    lp = torch.log_softmax(logits, -1)
    logp = lp.gather(1, act[:, None])[:, 0]
    ratio = torch.exp(logp - torch.tensor(a.logp_old[s].astype(np.float64)))
    lo, hi = float(f32(1) - f32(c.clip)), float(f32(1) + f32(c.clip))
    surr = torch.min(ratio * A, torch.clamp(ratio, lo, hi) * A)
    H = -(lp.exp() * lp).sum(-1)
    vf = (values - torch.tensor(a.targets[s].astype(np.float64))) ** 2
    vfc = torch.clamp(vf, max=float(f32(c.vf_clip)))
    if a.logits_old is not None:
        lq = torch.log_softmax(torch.tensor(np.where(np.isinf(a.logits_old[s]), -1e300, a.logits_old[s].astype(np.float64))), -1)
        kl = (lq.exp() * (lq - lp)).sum(-1)
    else:
        kl = torch.tensor(a.logp_old[s].astype(np.float64)) - logp
    per = -surr + float(f32(c.vf_coeff)) * vfc - float(f32(c.ent)) * H + float(f32(c.kl)) * kl
    per.sum().backward()
    return per.detach().numpy(), logits.grad.numpy(), values.grad.numpy()


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.M <= 488], ids=lambda c: c.id)
def test_the_reference_gradients_are_torch_autograd_s(c):
    a, ref = PC.arrays_of(c), PC.reference_of(c)
    rows = np.nonzero(~ref.left_out)[0]
    if len(rows) == 0:
        assert ref.sums[0] == 0 and not ref.stats.any()
        return
    per, g_logits, g_values = _torch_textbook(c, a, rows)
    f32 = np.float32
    t = ref.terms[rows]
    mine = -t[:, 0] + float(f32(c.vf_coeff)) * t[:, 1] - float(f32(c.ent)) * t[:, 2] + float(f32(c.kl)) * t[:, 3]
    assert PC.rel_error(mine, per) <= 1e-12
    near_ratio, near_vf = (b[rows] for b in PC.bands(c))
    assert PC.rel_error(ref.grad_logits[rows], g_logits, ~near_ratio) <= 1e-12
    assert PC.rel_error(ref.grad_values[rows], g_values, ~near_vf) <= 1e-12
    assert abs(ref.stats[1] - per.sum() / len(rows)) <= 1e-12 * max(1.0, np.abs(per).sum() / len(rows))


def test_the_case_list_covers_what_it_must():
    Pn = PC.partial_samples()
    cases = PC.CASES
    assert {c.M for c in cases} >= set(PC.SIZES) | {65 * Pn + 3} and len({c.id for c in cases}) == len(cases)
    for M in PC.SIZES:
        assert {c.mode for c in cases if c.M == M} >= {"contiguous", "indexed"}
    assert all(c.first > 0 for c in cases if c.mode == "contiguous" and not c.id.endswith("-plain"))
    assert {c.seat for c in cases} >= {"none", "all0", "mixed"} and any(PC.reference_of(c).sums[0] == 0 and c.M > 64 for c in cases)
    for flag in ("moments", "old", "terms", "neg_inf"):
        assert {getattr(c, flag) for c in cases} == {False, True}, flag
    assert {c.clip for c in cases} == {0.05, 0.2} and {c.vf_clip for c in cases} >= {10.0} and {c.vf_coeff for c in cases} == {1e-4, 0.5}
    assert {c.ent for c in cases} == {0.0, 0.2} and {c.kl for c in cases} == {0.0, 0.2}
    for c in cases:
        a, ref = PC.arrays_of(c), PC.reference_of(c)
        keep = ~ref.left_out
        if keep.sum() >= 100:  # both policy branches and both value branches
            assert ref.outside.any() and not ref.outside[keep].all(), c.id
            assert (ref.vf[keep] > c.vf_clip).any() and (ref.vf[keep] <= c.vf_clip).any(), c.id
        if c.mode == "indexed" and c.M >= 8:
            inside = (a.sample >= 0) & (a.sample < a.S)
            assert (~inside).sum() >= 2 and len(np.unique(a.sample[inside])) < inside.sum(), c.id
        if a.S >= 60:
            bad = a.actions == 255
            assert bad.any() and np.isnan(a.logp_old[bad]).all() and not np.isnan(a.logp_old[~bad]).any(), c.id
        if c.neg_inf:
            rows = np.isinf(a.logits).any(1) & keep
            assert rows.any() and not np.isinf(a.logits[np.arange(c.M), np.minimum(a.actions[np.where(keep, a.sample, 0)], 5)][keep]).any()
    # NaN in every input of the left-out samples changes nothing in the restatement either
    c = next(c for c in cases if c.id.endswith("-neginf") and c.seat == "mixed")
    clean, dirty = PC.loss_f32(c), PC.loss_f32(c, PC.poisoned(c))
    for x, y in zip(clean, dirty):
        if x.dtype != bool and x.ndim and x.shape[0] == c.M and x is not clean.ratio and x is not clean.vf:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(clean.stats, dirty.stats) and np.isnan(PC.poisoned(c).logits).any()


# ------------------------------------------------------------------------------------------ the Python surface
def _stub_env(n, bc=False):
    import torch

    return types.SimpleNamespace(n_envs=n, venv=types.SimpleNamespace(device=torch.device("cpu")), bc_policy=object() if bc else None,
                                 obs_kind="features", _torch=torch)


@pytest.mark.parametrize("n", (1, 33, 65))
def test_learner_batch_and_minibatches_of_a_trajectory_buffer(n):
    import torch

    from overcooked_ai_amd import trajectory_buffer as TB
    from overcooked_ai_amd.ppo_loss import LearnerBatch

    T, S = 5, 5 * n * 2
    buf = TB.TrajectoryBuffer(_stub_env(n, bc=True), T, keep_logits=True)
    assert buf.logits.shape == (T, n, 2, 6) and buf.logits.dtype == torch.float32
    values, logits = torch.zeros((n, 2)), torch.arange(n * 12, dtype=torch.float32).view(n, 2, 6)
    row = buf.row(3, values, logits)
    assert torch.equal(buf.logits[3], logits) and not buf.logits[2].any() and row.rewards.data_ptr() == buf.rewards[3].data_ptr()
    adv, tgt = torch.rand((T, n, 2)), torch.rand((T, n, 2))
    mom = torch.zeros(3, dtype=torch.float64)
    batch = buf.learner_batch(adv, tgt, mom)
    assert isinstance(batch, LearnerBatch) and batch.moments is mom
    for name, whole, shape in (("actions", buf.actions, (S,)), ("logp_old", buf.logp, (S,)), ("advantages", adv, (S,)), ("targets", tgt, (S,)),
                               ("seat", buf.seat, (S // 2,)), ("logits_old", buf.logits, (S, 6))):
        part = getattr(batch, name)
        assert part.data_ptr() == whole.data_ptr() and tuple(part.shape) == shape and part.is_contiguous(), name
    s = ((2 * n + n // 2) * 2 + 1)  # sample (t = 2, e = n // 2, p = 1)
    buf.logp[2, n // 2, 1] = 7.0
    assert batch.logp_old[s] == 7.0
    plain = TB.TrajectoryBuffer(_stub_env(n), T)
    assert plain.logits is None and plain.row(0, values).seat is None
    b2 = plain.learner_batch(adv, tgt)
    assert b2.seat is None and b2.logits_old is None and b2.moments is None
    for bad in (lambda: buf.row(0, values), lambda: plain.row(0, values, logits), lambda: buf.row(0, values, logits[:, :1]),
                lambda: buf.row(0, values, logits.long()), lambda: buf.learner_batch(adv[:-1], tgt), lambda: buf.learner_batch(adv, tgt.double()),
                lambda: buf.learner_batch(adv, tgt, mom.float()), lambda: list(buf.minibatches(0))):
        with pytest.raises(ValueError):
            bad()
    gen = torch.Generator().manual_seed(5)
    size = max(S // 3, 1) + 1
    parts = list(buf.minibatches(size, generator=gen))
    assert [len(p) for p in parts] == [size] * (S // size) + ([S % size] if S % size else [])
    assert all(p.dtype == torch.int32 and p.is_contiguous() and p.data_ptr() % 4 == 0 for p in parts)
    assert sorted(torch.cat(parts).tolist()) == list(range(S))
    again = list(buf.minibatches(size, generator=torch.Generator().manual_seed(5)))
    assert all(torch.equal(x, y) for x, y in zip(parts, again))


def test_ppo_loss_validates_its_tensors():
    import torch

    from overcooked_ai_amd.ppo_loss import LearnerBatch, ppo_loss

    S, M = 40, 12
    batch = LearnerBatch(torch.zeros(S, dtype=torch.uint8), torch.zeros(S), torch.zeros(S), torch.zeros(S), torch.zeros(S // 2, dtype=torch.uint8),
                         torch.zeros((S, 6)), torch.zeros(3, dtype=torch.float64))
    ok = dict(logits=torch.zeros((M, 6)), values=torch.zeros(M), batch=batch, index=torch.zeros(M, dtype=torch.int32), clip_param=0.05,
              vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.1, kl_coeff=0.2)
    # every entry with the words of the check it is there for: all of these tensors are on the host, so a lost check would end at the
    # "no CPU fallback" refusal, which matches none of them
    nan, inf = float("nan"), float("inf")
    hyper = "clip_param and vf_clip_param must be finite and positive"
    coeff = "vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0"
    bad = [(dict(logits=ok["logits"].double()), "logits must be a contiguous float32 [12, 6]"),
           (dict(logits=torch.zeros((M, 5))), "logits must be a contiguous float32 [M, 6]"),
           (dict(logits=torch.zeros((6, M)).t()), "logits must be a contiguous float32 [12, 6]"),
           (dict(logits=torch.zeros(M * 6)), "logits must be a contiguous float32 [M, 6]"),
           (dict(values=torch.zeros((M, 1))), "values must be a contiguous float32 [12]"),
           (dict(values=torch.zeros(M, dtype=torch.float64)), "values must be a contiguous float32 [12]"),
           (dict(values=torch.zeros(2 * M)[::2]), "values must be a contiguous float32 [12]"),
           (dict(index=torch.zeros(M, dtype=torch.int64)), "index must be a contiguous int32 [12]"),
           (dict(index=torch.zeros(M - 1, dtype=torch.int32)), "index must be a contiguous int32 [12]"),
           (dict(index=torch.zeros(2 * M, dtype=torch.int32)[::2]), "index must be a contiguous int32 [12]"),
           (dict(index=None, first=S - M + 1), "lie outside the batch's 0 .. 39"), (dict(index=None, first=-1), "lie outside the batch's 0 .. 39"),
           (dict(batch=tuple(batch)), "batch must be a LearnerBatch"),
           (dict(batch=batch._replace(actions=batch.actions.long())), "batch.actions must be a contiguous uint8 [40]"),
           (dict(batch=batch._replace(actions=torch.zeros((S // 2, 2), dtype=torch.uint8))), "batch.actions must be a contiguous uint8 [S]"),
           (dict(batch=batch._replace(logp_old=torch.zeros(S + 1))), "batch.logp_old must be a contiguous float32 [40]"),
           (dict(batch=batch._replace(advantages=torch.zeros((S // 2, 2)))), "batch.advantages must be a contiguous float32 [40]"),
           (dict(batch=batch._replace(targets=torch.zeros(S, dtype=torch.float64))), "batch.targets must be a contiguous float32 [40]"),
           (dict(batch=batch._replace(seat=torch.zeros(S, dtype=torch.uint8))), "batch.seat must be a contiguous uint8 [20]"),
           (dict(batch=batch._replace(logits_old=torch.zeros((S, 5)))), "batch.logits_old must be a contiguous float32 [40, 6]"),
           (dict(batch=batch._replace(logits_old=torch.zeros((6, S)).t())), "batch.logits_old must be a contiguous float32 [40, 6]"),
           (dict(batch=batch._replace(moments=torch.zeros(3))), "batch.moments must be a contiguous float64 [3]"),
           (dict(batch=batch._replace(logits_old=None)), "kl_coeff > 0 needs the batch's old logits"),
           (dict(clip_param=0.0), hyper), (dict(clip_param=nan), hyper), (dict(vf_clip_param=inf), hyper), (dict(vf_clip_param=-1.0), hyper),
           (dict(vf_loss_coeff=-1.0), coeff), (dict(entropy_coeff=nan), coeff), (dict(kl_coeff=-0.1), coeff),
           # (the last two: everything in order, but on the host — there is no CPU fallback)
           (dict(), "no CPU fallback"), (dict(index=None, first=3), "no CPU fallback")]
    for kw, words in bad:
        with pytest.raises(ValueError, match=re.escape(words)):
            ppo_loss(**dict(ok, **kw))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ppo_loss(**ok)
