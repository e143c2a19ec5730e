"""oc_gae without a GPU: the exports and the struct against the header, the plan's words and the prefetch block, every refusal
(made before any device call: this host has no device), the two restatements of tests/gae_cases.py against each other within an
a-priori bound, a hand-computed case, the properties the header states (a done step isolates, a partner's sample is zero and
cuts the chain), the TrajectoryBuffer's row addresses and the Python surface's own refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import gae_cases as GC
from case_support import P, ROOT

EINVAL = -1
WHO = "oc_gae: "


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


def _batch(n):
    from overcooked_ai_amd import _lib

    return _lib.OcBatch(n_envs=n)


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_struct_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_gae", "oc_gae_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    body = re.search(r"typedef struct OcGaeBatch \{(.*?)\} OcGaeBatch;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(d_\w+|n_steps|gamma|lambda)\b", body)
    assert [{"lambda": "lam"}.get(x, x) for x in names] == [f[0] for f in _lib.OcGaeBatch._fields_]
    G = _lib.OcGaeBatch  # nine pointers, an int64, two floats
    assert ctypes.sizeof(G) == 88 and [getattr(G, f).offset for f, _ in G._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84]
    assert "int oc_gae(const OcBatch* batch, const OcGaeBatch* g, void* stream);" in hdr
    assert "int oc_gae_plan(const OcBatch* batch, int64_t n_steps, int with_seat, int with_moments, char* out, size_t out_size);" in hdr
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_the_arithmetic_the_references_restate():
    hdr = _header()
    for words in ("gl = gamma * lambda (one f32 product, formed on the host)", "r = (float)d_rewards[t][e][p] (round to nearest)",
                  "if d_done[t][e] != 0:  delta = r - v;  A = delta", "a select, not a multiplication by 0",
                  "delta = (r + g * vn) - v;  A = delta + gl * A_carried", "target = A + v", "d_seat[t][e] == p", "+0.0f",
                  "sum of the partials in ascending k", "No floating-point atomics"):
        assert words in hdr, words


def _plan(b, n_steps, seat=0, moments=0):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    rc = L.oc_gae_plan(ctypes.byref(b) if b is not None else None, n_steps, seat, moments, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def test_the_plan_in_words_and_the_prefetch_block():
    from overcooked_ai_amd.gae import plan_gae

    B = GC.prefetch_block()
    assert B in (8, 16)
    rc, text = _plan(_batch(65536), 400, 1, 1)
    assert rc == 0 and text == ("k_gae<SEAT=true, MOM=true> grid=256, 256 lanes (one per env, both players), %d steps per prefetch block, "
                                "%d block(s) + k_gae_moments grid=1, 64 lanes" % (B, (400 + B - 1) // B)), text
    assert text in _header() and plan_gae(65536, 400, seat=True, moments=True) == text
    for n, T, seat, mom in ((1, 1, 0, 0), (257, B + 1, 0, 1), (488, 2 * B + 1, 1, 0)):
        rc, text = _plan(_batch(n), T, seat, mom)
        assert rc == 0 and text.startswith("k_gae<SEAT=%s, MOM=%s> grid=%d, 256 lanes" % (GC_tf(seat), GC_tf(mom), (n + 255) // 256)), text
        assert ("%d block(s)" % ((T + B - 1) // B)) in text and text.endswith("k_gae_moments grid=1, 64 lanes") == bool(mom)
    assert _plan(_batch(0), 400) == (0, "nothing to launch (no envs)")
    assert _plan(_batch(0), 0) == (0, "nothing to launch (no envs)")
    assert _plan(_batch(65), 0, 1, 1) == (0, "nothing to launch (no steps)")
    for b, T, why in ((None, 4, "batch is NULL"), (_batch(-1), 4, "batch.n_envs < 0"), (_batch(4), -1, "n_steps < 0")):
        rc, msg = _plan(b, T)
        assert rc == EINVAL and msg.startswith(WHO + why), (why, msg)
    with pytest.raises(Exception, match="oc_gae: n_steps < 0"):
        plan_gae(4, -1)


def GC_tf(v):
    return "true" if v else "false"


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at its launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    fields = [f for f, _ in _lib.OcGaeBatch._fields_]

    def call(b=(), g=(), **kw):
        b = _batch(1000) if b == () else b
        if g == ():
            v = dict(d_rewards=P, d_values=P, d_last_values=P, d_done=P, d_seat=P, d_advantages=P, d_targets=P, d_partials=P, d_moments=P,
                     n_steps=12, gamma=0.99, lam=0.98)
            v.update(kw)
            g = _lib.OcGaeBatch(*[v[f] for f in fields])
        rc = L.oc_gae(ctypes.byref(b) if b is not None else None, ctypes.byref(g) if g is not None else None, None)
        return rc, L.oc_last_error().decode()

    required = "NULL d_rewards, d_values, d_done, d_advantages or d_targets"
    aligned8 = "d_values, d_last_values, d_advantages and d_targets must be 8-byte aligned"
    refusals = [(dict(b=None), "batch is NULL"), (dict(g=None), "gae batch is NULL")]
    refusals += [({f: None}, required) for f in ("d_rewards", "d_values", "d_done", "d_advantages", "d_targets")]
    refusals += [(dict(d_rewards=P + 8), "d_rewards must be 16-byte aligned")]
    refusals += [({f: P + 4}, aligned8) for f in ("d_values", "d_last_values", "d_advantages", "d_targets")]
    refusals += [({f: P + 4}, "d_partials and d_moments must be 8-byte aligned") for f in ("d_partials", "d_moments")]
    refusals += [(dict(n_steps=-1), "n_steps < 0"), (dict(b=_batch(-1)), "batch.n_envs < 0")]
    refusals += [(dict(gamma=x), "gamma must be in [0, 1]") for x in (-0.001, 1.001, float("nan"), float("inf"))]
    refusals += [(dict(lam=x), "lambda must be in [0, 1]") for x in (-0.001, 1.001, float("nan"), float("-inf"))]
    refusals += [(dict(d_partials=None), "d_moments needs d_partials")]
    for kw, why in refusals:
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith(WHO + why), (kw, rc, msg)
    # accepted, and nothing to launch (no moments asked for: zeroing them is a device call): no envs, no steps; the optional
    # arrays absent; the minimum alignments; both ends of gamma and lambda; done and seat at odd addresses
    for kw in (dict(), dict(d_last_values=None), dict(d_seat=None), dict(d_rewards=P + 16, d_values=P + 8, d_advantages=P + 8, d_targets=P + 24),
               dict(gamma=0.0, lam=0.0), dict(gamma=1.0, lam=1.0), dict(d_done=P + 1, d_seat=P + 3)):
        assert call(b=_batch(0), d_partials=None, d_moments=None, **kw)[0] == 0, kw
        assert call(n_steps=0, d_partials=None, d_moments=None, **kw)[0] == 0, kw


# ------------------------------------------------------------------------------------------ the arithmetic
def test_a_hand_computed_three_step_case():
    """One env, quantities exact in f32 (gamma = lambda = 0.5, so g = 0.5 and gl = 0.25): player 0 runs through, player 1 is done at
    step 1, and the next episode's value (100, behind the done step) must not reach it."""
    rewards = np.array([[[1.0, 2.0]], [[0.5, 4.0]], [[2.0, 1.0]]])
    values = np.array([[[0.5, 1.0]], [[1.0, 2.0]], [[2.0, 100.0]]], np.float32)
    last = np.array([[4.0, 8.0]], np.float32)
    # player 0: t=2: delta = 2 + 0.5*4 - 2 = 2, A = 2; t=1: delta = 0.5 + 0.5*2 - 1 = 0.5, A = 0.5 + 0.25*2 = 1;
    #           t=0: delta = 1 + 0.5*1 - 0.5 = 1, A = 1 + 0.25*1 = 1.25
    adv, tgt = GC.gae_f32(rewards, values, np.zeros((3, 1), np.uint8), 0.5, 0.5, last)
    assert adv[:, 0, 0].tolist() == [1.25, 1.0, 2.0] and tgt[:, 0, 0].tolist() == [1.75, 2.0, 4.0]
    # player 1 with done at step 1: t=2: delta = 1 + 0.5*8 - 100 = -95; t=1 (done): A = 4 - 2 = 2; t=0: delta = 2 + 0.5*2 - 1 = 2,
    #           A = 2 + 0.25*2 = 2.5
    done = np.array([[0], [9], [0]], np.uint8)
    adv, tgt = GC.gae_f32(rewards, values, done, 0.5, 0.5, last)
    assert adv[:, 0, 1].tolist() == [2.5, 2.0, -95.0] and tgt[:, 0, 1].tolist() == [3.5, 4.0, 5.0]
    assert adv[:, 0, 0].tolist() == [0.875, -0.5, 2.0]  # (player 0 of the same env: t=1 done: 0.5 - 1; t=0: 1 + 0.25 * -0.5)
    # the partner plays player 1 during step 1: zeros there, nothing carried to step 0, player 0 as before
    seat = np.array([[255], [1], [255]], np.uint8)
    adv2, tgt2 = GC.gae_f32(rewards, values, np.zeros((3, 1), np.uint8), 0.5, 0.5, last, seat)
    assert adv2[:, 0, 0].tolist() == [1.25, 1.0, 2.0]
    assert adv2[1, 0, 1] == 0 and tgt2[1, 0, 1] == 0 and not np.signbit(adv2[1, 0, 1]) and not np.signbit(tgt2[1, 0, 1])
    assert adv2[0, 0, 1] == 2.0 + 0.5 * 2.0 - 1.0 and adv2[2, 0, 1] == -95.0  # (t=0: delta only; t=2 untouched)
    # without last values the horizon end bootstraps from 0
    adv3, _ = GC.gae_f32(rewards, values, np.zeros((3, 1), np.uint8), 0.5, 0.5, None)
    assert adv3[2, 0].tolist() == [0.0, -99.0]
    for a in (adv, adv2, adv3, tgt, tgt2):
        assert a.dtype == np.float32


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_the_f32_restatement_stays_within_the_a_priori_bound_of_the_f64_one(c):
    rewards, values, done, last, seat = GC.arrays_of(c)
    adv, tgt = GC.reference_of(c)
    adv64, tgt64, b_adv, b_tgt = GC.gae_f64(rewards, values, done, c.gamma, c.lam, last, seat)
    live = GC.learner_mask(done, seat)
    assert (b_adv[live] > 0).any() or not live.any()
    assert not adv[~live].any() and not tgt[~live].any() and not b_adv[~live].any()
    e_adv, e_tgt = np.abs(adv.astype(np.float64) - adv64), np.abs(tgt.astype(np.float64) - tgt64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = max(float(np.nan_to_num(e_adv / b_adv).max()), float(np.nan_to_num(e_tgt / b_tgt).max()))
    print("%s: largest error / bound %.4f (largest bound %.3g)" % (c.id, ratio, float(b_adv.max())))
    assert (e_adv <= b_adv).all() and (e_tgt <= b_tgt).all(), ratio
    # the bound is a rounding bound, not slack: a chain one step short, or gamma in lambda's place, leaves it
    if c.n_steps > 1 and c.done not in ("every",) and c.seat in ("none", "episode") and c.gamma != c.lam and c.lam > 0:
        wrong, _ = GC.gae_f32(rewards, values, done, c.lam, c.gamma, last, seat)
        assert (np.abs(wrong.astype(np.float64) - adv64) > b_adv).any()


def test_the_largest_error_to_bound_ratio_over_the_case_list():
    worst = 0.0
    for c in GC.CASES:
        rewards, values, done, last, seat = GC.arrays_of(c)
        adv, tgt = GC.reference_of(c)
        adv64, tgt64, b_adv, b_tgt = GC.gae_f64(rewards, values, done, c.gamma, c.lam, last, seat)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nan_to_num(np.abs(adv - adv64) / b_adv).max()), float(np.nan_to_num(np.abs(tgt - tgt64) / b_tgt).max()))
    print("largest |gae_f32 - gae_f64| / bound over %d cases: %.4f" % (len(GC.CASES), worst))
    assert 0 < worst <= 1


@pytest.mark.parametrize("c", [c for c in GC.CASES if c.done in ("horizon5", "random7", "first")][:8], ids=lambda c: c.id)
def test_a_done_step_isolates_what_lies_before_it(c):
    """The restatement itself has the property the kernel is held to: NaN behind an env's first done step changes nothing at or
    before it, and a (1 - done) product in the select's place would."""
    clean_adv, clean_tgt = GC.reference_of(c)
    (rewards, values, done, last, seat), keep = GC.poisoned(c)
    adv, tgt = GC.gae_f32(rewards, values, done, c.gamma, c.lam, last, seat)
    assert np.array_equal(adv[keep].view(np.uint32), clean_adv[keep].view(np.uint32))
    assert np.array_equal(tgt[keep].view(np.uint32), clean_tgt[keep].view(np.uint32))
    if (~keep).any():
        live = GC.learner_mask(done, seat)
        assert np.isnan(adv[~keep & live.all(-1)]).all()


def test_the_case_list_covers_what_it_must():
    B = GC.prefetch_block()
    Ts = {1, 2, B - 1, B, B + 1, 2 * B + 1}
    assert {(c.n_envs, c.n_steps) for c in GC.CASES} >= {(n, T) for n in GC.SIZES for T in Ts}
    assert {(c.done, c.seat) for c in GC.CASES if c.n_steps >= 2 * B + 1} >= {(d, s) for d in GC.DONE_PATTERNS for s in GC.SEAT_PATTERNS}
    assert any(c.n_steps == 400 and c.n_envs == 65 for c in GC.CASES)
    assert any(not c.last for c in GC.CASES) and {1.0} <= {c.gamma for c in GC.CASES} and {0.0, 1.0} <= {c.lam for c in GC.CASES}
    assert len({c.id for c in GC.CASES}) == len(GC.CASES)
    for c in GC.CASES:  # an output element that still holds the fill was not written: no result may equal it, and none is NaN
        for a in GC.reference_of(c):
            assert not (a == GC.FILL).any() and not np.isnan(a).any(), c.id
    c = next(c for c in GC.CASES if c.n_envs == 488 and c.n_steps == 2 * B + 1)
    rewards, values, done, last, seat = GC.arrays_of(c)
    assert rewards.dtype == np.float64 and values.dtype == np.float32 and done.dtype == np.uint8
    assert np.abs(rewards).max() <= 50 and np.abs(values).max() <= 50
    exact = rewards == rewards.astype(np.float32)
    assert exact.any() and not exact.all()  # members that are exact in f32 and members that are not
    # the patterns are what their names say
    rng = np.random.default_rng(0)
    d = GC.done_pattern("horizon5", 12, 7, rng)
    assert all((d[:, e] != 0).tolist() == [(t + e) % 5 == 4 for t in range(12)] for e in range(7))
    d = GC.done_pattern("random7", 400, 65, rng)
    assert abs((d != 0).mean() - 1 / 7) < 5 * np.sqrt(1 / 7 * 6 / 7 / d.size)
    s = GC.seat_pattern("episode", d, rng)
    changed = s[1:] != s[:-1]
    assert changed.any() and not (changed & (d[:-1] == 0)).any() and set(np.unique(s)) == {0, 1, GC.NO_SEAT}
    s = GC.seat_pattern("inconsistent", d, rng)
    assert ((s[1:] != s[:-1]) & (d[:-1] == 0)).any()


# ------------------------------------------------------------------------------------------ the Python surface
def _stub_env(n, bc=False, obs_kind="features"):
    import torch

    return types.SimpleNamespace(n_envs=n, venv=types.SimpleNamespace(device=torch.device("cpu")), bc_policy=object() if bc else None,
                                 obs_kind=obs_kind, _torch=torch)


@pytest.mark.parametrize("n", (1, 63, 65, 257, 487))
def test_every_row_of_the_trajectory_buffer_meets_the_alignment_the_step_asks_for(n):
    import torch

    from overcooked_ai_amd import trajectory_buffer as TB

    T = 7
    for name in ("rewards", "done", "actions", "logp", "values", "seat"):
        offs = TB.row_offsets(name, T, n)
        assert offs == [t * n * TB.ROW_BYTES[name] for t in range(T)] and all(o % TB.ROW_ALIGN[name] == 0 for o in offs), name
    assert TB.ROW_ALIGN == dict(rewards=16, done=1, actions=2, logp=8, values=8, seat=1)  # include/oc_amd.h: d_shaped, OcActionSampler, OcGaeBatch
    buf = TB.TrajectoryBuffer(_stub_env(n, bc=True), T)
    assert buf.rewards.shape == (T, n, 2) and buf.rewards.dtype == torch.float64 and buf.done.shape == (T, n) and buf.done.dtype == torch.uint8
    assert buf.actions.shape == (T, n, 2) and buf.actions.dtype == torch.uint8 and buf.logp.shape == buf.values.shape == (T, n, 2)
    assert buf.logp.dtype == buf.values.dtype == buf.last_values.dtype == torch.float32 and buf.last_values.shape == (n, 2)
    assert buf.seat.shape == (T, n) and buf.seat.dtype == torch.uint8 and bool((buf.seat == 255).all())
    values = torch.arange(2 * n, dtype=torch.float32).view(n, 2)
    for t in range(T):
        row = buf.row(t, values + t)
        for name in ("rewards", "done", "actions", "logp", "seat"):
            whole, part = getattr(buf, name), getattr(row, name)
            assert part.is_contiguous() and part.data_ptr() == whole.data_ptr() + TB.row_offsets(name, T, n)[t]
            assert part.data_ptr() % TB.ROW_ALIGN[name] == 0 and part.shape == whole.shape[1:]
        assert torch.equal(buf.values[t], values + t) and buf.values[t].data_ptr() % 8 == 0
    assert TB.TrajectoryBuffer(_stub_env(n), T).seat is None and TB.TrajectoryBuffer(_stub_env(n), T).row(0, values).seat is None
    for bad in (lambda: buf.row(T, values), lambda: buf.row(-1, values), lambda: buf.row(0, values[:, :1]), lambda: buf.row(0, values.long()),
                lambda: TB.TrajectoryBuffer(_stub_env(n), 0), lambda: TB.TrajectoryBuffer(_stub_env(n, obs_kind="bc"), 2, keep_obs=True)):
        with pytest.raises(ValueError):
            bad()


def test_gae_validates_its_tensors():
    import torch

    from overcooked_ai_amd.gae import gae

    T, n = 3, 5
    ok = dict(rewards=torch.zeros((T, n, 2), dtype=torch.float64), values=torch.zeros((T, n, 2)), done=torch.zeros((T, n), dtype=torch.uint8),
              gamma=0.99, lam=0.98)
    bad = [dict(rewards=ok["rewards"].float()), dict(rewards=ok["rewards"][:, :, 0]), dict(values=ok["values"].double()),
           dict(values=ok["values"][:2]), dict(done=ok["done"].bool()), dict(done=ok["done"][:, :4]), dict(gamma=1.5), dict(lam=-0.1),
           dict(gamma=float("nan")), dict(last_values=torch.zeros((n, 3))), dict(last_values=torch.zeros((n, 2), dtype=torch.float64)),
           dict(seat=torch.zeros((T, n), dtype=torch.int8)), dict(seat=torch.zeros((n, T), dtype=torch.uint8)),
           dict(values=torch.zeros((T, 2, n)).transpose(1, 2)), dict(out=(torch.zeros((T, n, 2)), torch.zeros((T, n, 1)))),
           dict()]  # (the last: everything in order, but on the host — there is no CPU fallback)
    for kw in bad:
        with pytest.raises(ValueError):
            gae(**dict(ok, **kw))
