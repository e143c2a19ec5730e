"""tests/sample_cases.py kept honest without a GPU: every case is planned (oc_multi_agent_step_sample_plan) onto what it names, the
SAMPLE = true instances csrc/train_dispatch.hpp instantiates are those the list covers, the entry points refuse what they must before
any device call (this host has none to make), the numpy Philox is the oracle's, each part of the far counters reaches a draw, and on
the references alone each case contains what it claims and the float32 restatement of the sampler equals the float64 reference
outside the boundary band."""
import ctypes
import os
import re

import numpy as np
import pytest

import sample_cases as SC
import train_cases as TC
from case_support import CSRC, P, check_census, synthetic_batch, table_of, train_selector

ALL = SC.CASES + (SC.far_case(),)
EINVAL = -1  # OC_EINVAL


def _plan(b, horizon=11, with_obs=0, obs_dtype=None, with_features=0, num_pots=2, options=0, use_phi=1, event_sink=0, start=None):
    """oc_multi_agent_step_sample_plan of a batch -> (rc, text or the refusal's message)"""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(400)
    rc = L.oc_multi_agent_step_sample_plan(ctypes.byref(b) if b is not None else None, horizon, with_obs,
                                           _lib.OBS_U8 if obs_dtype is None else obs_dtype, with_features, num_pots, options, use_phi,
                                           event_sink, ctypes.byref(start) if start is not None else None, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


# ------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_the_planner_gives_the_case_what_it_names(case):
    """... and its words are those of the same call with an actions array, with SAMPLE=true in the step kernel's name or behind
    k_sample_actions."""
    from overcooked_ai_amd import _lib, dispatch

    plan = SC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    base = dispatch.multi_agent_featurize_plan(
        table_of(case.table), case.n_envs, horizon=case.horizon, obs_dtype=_lib.OBS_F32 if case.obs == "f32" else _lib.OBS_U8,
        with_obs=case.obs in ("u8", "f32"), with_features=case.obs == "features", num_pots=case.num_pots,
        options=_lib.OPT_ONE_KERNEL if case.one_kernel else 0, use_phi=case.use_phi, event_sink=case.events, start=SC.start_spec_of(case))
    fused = base.split("<")[0] in ("k_train_step_obs", "k_train_step_feat", "k_train_step1")
    assert fused == (SC.instance_of(case) is not None), (case.id, base)
    if fused:
        head, tail = base.split(">", 1)
        assert plan == head + ", SAMPLE=true>" + tail
    else:
        assert plan == "k_sample_actions + " + base


def test_the_instances_of_the_sources_are_those_the_list_covers():
    with open(os.path.join(CSRC, "train_dispatch.hpp")) as f:
        src = f.read()
    assert "k_train_step_obs<MP, T, NW, true, SampleArgs>" in src and "k_train_step1<U, MP, LL, true, SampleArgs>" in src
    assert "k_train_step_feat<MP, true, SampleArgs>" in src
    # the selector lines the plain censuses read (tests/test_host_train_instances.py, tests/test_host_train_featurize.py), wherever
    # their last template argument is SAMPLE: train_selector holds those selectors to be instantiated for SAMPLE = true as well
    (obs, s_obs), (lean, s_lean), (feat, s_feat), (_, s_general) = (train_selector(k) for k in ("obs", "step1", "feat", "step"))
    assert s_obs and s_lean and s_feat and not s_general
    found = [SC.obs_k(int(mp), {"uint8_t": "u8", "float": "f32"}[t], int(w)) for mp, t, w, _ in obs]
    found += [SC.step1(u == "true", int(mp), ll == "true") for u, mp, ll, _ in lean]
    found += [SC.feat_k(int(mp)) for mp, _ in feat]
    reached = {SC.instance_of(c) for c in ALL} - {None}
    check_census(found, SC.INSTANCES, SC.UNREACHABLE, reached, 14, "SAMPLE = true instances")
    # each is the SAMPLE form of an instance the step's own launch code has (tests/train_cases.py, tests/train_featurize_cases.py)
    import train_featurize_cases as FC

    plain = {i.replace(", SAMPLE=true", "") for i in SC.INSTANCES}
    assert plain == {i for i in TC.INSTANCES if not i.startswith("k_train_step<")} | set(FC.INSTANCES)
    assert {i.replace(", SAMPLE=true", "") for i in SC.UNREACHABLE} == set(TC.UNREACHABLE)
    with open(os.path.join(CSRC, "sample.hpp")) as f:
        sampler = f.read()
    assert sampler.count("void sample_row(") == 1 and "k_sample_actions" in sampler  # one device function, behind both paths
    for name in ("shaping.hpp", "train_obs.hpp", "train_feat.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert f.read().count("if constexpr (SAMPLE) in.a01 = sample_env(") == 1, name


def test_the_cases_cover_what_the_issue_lists():
    fused = [c for c in SC.CASES if SC.instance_of(c) and not c.greedy]
    small = [c for c in fused if not c.expect.startswith("k_train_step_obs<")]
    assert {c.n_envs for c in small} >= {1, 33, 65, 256 + 232, 300} and {c.table for c in small} >= {"mix5", "cramped_room_old"}
    assert any(c.table == "mix5" and c.start == "regen" and "UNIFORM=false" in c.expect for c in small)
    assert {c.use_phi for c in small} == {True, False}
    assert all(c.steps == 25 and c.horizon == 11 and c.start != "standard" and c.env_offset > 0 for c in small)
    big = {(c.expect, c.n_envs) for c in fused if c.expect.startswith("k_train_step_obs<")}
    assert big >= {(SC.obs_k(1, "u8", 16), TC.N_OBS + 232), (SC.obs_k(2, "u8", 8), TC.N_OBS + 1), (SC.obs_k(2, "f32", 8), TC.N_OBS + 65)}
    assert all(c.steps == 9 and c.horizon == 4 for c in fused if c.expect.startswith("k_train_step_obs<"))
    other = [c for c in SC.CASES if not SC.instance_of(c)]
    assert {c.table for c in other} >= {"marshmallow_experiment", "seven_pots"} and any(c.events for c in other)
    assert table_of("marshmallow_experiment").n_cells == 65
    assert any(c.greedy and SC.instance_of(c) for c in SC.CASES) and any(c.greedy and not SC.instance_of(c) for c in SC.CASES)
    for c in SC.CASES:
        assert c.horizon < c.steps / 2 and c.env_offset > 0 and c.steps % c.horizon >= 1, c.id
    far = SC.far_case()
    assert far.seed >> 32 and far.seed & 0xFFFFFFFF and far.env_offset < 2**32 < far.env_offset + far.n_envs
    assert far.step0 < 2**32 < far.step0 + far.steps


# ------------------------------------------------------------------------------------------ refusals (no device call: none exists here)
def test_the_plan_refuses_what_the_entry_point_refuses():
    from overcooked_ai_amd import _lib

    who = "oc_multi_agent_step_sample: "
    ok = synthetic_batch(5, 4, 1000)
    assert _plan(ok)[0] == 0 and _plan(ok, with_features=1)[0] == 0
    for kw, b, why in ((dict(with_features=1, num_pots=5), ok, "num_pots must be in 0..4"),
                       (dict(with_features=1), synthetic_batch(5, 4, 1000, flags=0), "d_features needs 2-player layouts"),
                       (dict(options=_lib.OPT_AUTO_RESET), ok, "options other than OC_OPT_ONE_KERNEL"),
                       (dict(horizon=0), ok, "horizon must be in 1..65535"),
                       (dict(horizon=0, with_features=1), ok, "horizon must be in 1..65535"),
                       (dict(start=_lib.OcStartSpec(1, 0, 1, 1, 1.5, 0, 0)), ok, "start.rnd_obj_prob_thresh must be in [0, 1]")):
        rc, msg = _plan(b, **kw)
        assert rc != 0 and msg.startswith(who + why), (kw, msg)
    assert _plan(synthetic_batch(5, 4, 0))[1] == "nothing to launch (no envs)"
    assert _plan(synthetic_batch(5, 4, 0), with_features=1)[1] == "nothing to launch (no envs)"


def _sampler(logits=P, actions=P, logp=P, mode=0):
    from overcooked_ai_amd import _lib

    return _lib.OcActionSampler(logits, actions, logp, 7, 0, 0, mode)


SAMPLER_REFUSALS = ((None, "sampler is NULL"), (dict(logits=None), "NULL sampler.d_logits or sampler.d_actions_out"),
                    (dict(actions=None), "NULL sampler.d_logits or sampler.d_actions_out"),
                    (dict(logits=P + 8), "sampler.d_logits must be 16-byte aligned"),
                    (dict(actions=P + 1), "sampler.d_actions_out must be 2-byte aligned"),
                    (dict(logp=P + 4), "sampler.d_logp_out must be 8-byte aligned"), (dict(mode=2), "unknown sampler.mode"))


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at the first launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    who = "oc_multi_agent_step_sample: "

    def call(b, sampler=(), features=None, tables=(None, None), num_pots=2, options=0, horizon=11, done=P, shaped=P, phi=(P, P, P, P, P, P)):
        plan_blob, plan_off, phi_tables, phi_next, phi_cur, phi_start = phi
        s = _sampler() if sampler == () else sampler
        rc = L.oc_multi_agent_step_sample(ctypes.byref(b), P, ctypes.byref(s) if s is not None else None, P, P, P, P, plan_blob, plan_off,
                                          phi_tables, phi_next, phi_cur, phi_start, 0.5, shaped, done, None, _lib.OBS_U8, horizon, tables[0],
                                          tables[1], features, num_pots, options, None, None, None)
        return rc, L.oc_last_error().decode()

    ok = synthetic_batch(5, 4, 1000)
    for kw, why in SAMPLER_REFUSALS:
        rc, msg = call(ok, sampler=None if kw is None else _sampler(**kw))
        assert rc == EINVAL and msg.startswith(who + why), (kw, rc, msg)  # (OC_EINVAL)
    for kw, b, why in ((dict(features=P + 8, tables=(P, P)), ok, "d_features must be 16-byte aligned"),
                       (dict(features=P, tables=(P, P), num_pots=5), ok, "num_pots must be in 0..4"),
                       (dict(features=P, tables=(P, P)), synthetic_batch(5, 4, 1000, flags=0), "d_features needs 2-player layouts"),
                       (dict(options=0x40), ok, "options other than OC_OPT_ONE_KERNEL"),
                       (dict(features=P, tables=(None, P)), ok, "d_features needs the feature plan tables"),
                       # the step's own refusals, with and without features, under this entry point's name
                       (dict(done=None), ok, "d_done is required"),
                       (dict(done=None, features=P, tables=(P, P)), ok, "d_done is required"),
                       (dict(horizon=70000), ok, "horizon must be in 1..65535"),
                       (dict(shaped=P + 8), ok, "d_shaped must be 16-byte aligned"),
                       (dict(phi=(None, P, P, P, P, P)), ok, "use_phi needs the plan tables and the three phi buffers")):
        rc, msg = call(b, **kw)
        assert rc == EINVAL and msg.startswith(who + why), (kw, rc, msg)
    assert call(synthetic_batch(5, 4, 0))[0] == 0 and call(synthetic_batch(5, 4, 0), features=P, tables=(P, P))[0] == 0  # no envs


def test_oc_sample_actions_refuses_before_any_device_call():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    ok = synthetic_batch(5, 4, 1000)
    for kw, why in SAMPLER_REFUSALS:
        s = None if kw is None else _sampler(**kw)
        rc = L.oc_sample_actions(ctypes.byref(ok), ctypes.byref(s) if s is not None else None, None)
        assert rc == EINVAL and L.oc_last_error().decode().startswith("oc_sample_actions: " + why), (kw, L.oc_last_error())
    assert L.oc_sample_actions(None, ctypes.byref(_sampler()), None) == EINVAL
    assert L.oc_sample_actions(ctypes.byref(synthetic_batch(5, 4, 0)), ctypes.byref(_sampler()), None) == 0  # no envs: nothing to do


def test_the_header_states_the_sampler_the_references_restate():
    from case_support import ROOT

    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        hdr = f.read()
    for words in ("{t_lo, g_lo, g_hi, t_hi}", "seed_hi ^ 0x53414D50", "(float)(r[p] >> 8) * 2^-24", "the number of i with c_i <= x",
                  "logp = (l_a - m) - logf(S)", "the action is 255", "#define OC_SAMPLE_ARGMAX      1u"):
        assert words in hdr, words
    assert SC.KEY_TWEAK == 0x53414D50 == int.from_bytes(b"SAMP", "big")


# ------------------------------------------------------------------------------------------ the stream
def test_the_numpy_philox_is_the_oracles():
    from oracle import oracle as O

    rng = np.random.default_rng(5)
    words = rng.integers(0, 2**32, size=(64, 6), dtype=np.uint64)
    words[0] = 0
    words[1] = 0xFFFFFFFF
    got = np.stack(SC.philox4x32_10(*(words[:, i] for i in range(6))), axis=1)
    for row, g in zip(words, got):
        assert tuple(int(x) for x in g) == O.philox4x32_10([int(x) for x in row[:4]], [int(x) for x in row[4:]])


def test_the_uniforms_are_the_headers_counters():
    from oracle import oracle as O

    c = SC.far_case()
    n, t = c.n_envs, c.step0 + 5  # (above the wrap of t_lo)
    u = SC.uniforms(c.seed, c.env_offset, t, n)
    assert u.dtype == np.float32 and u.shape == (n, 2) and (u >= 0).all() and (u < 1).all()
    for e in (0, n // 2 + 36, n // 2 + 37, n - 1):  # both sides of the wrap of g_lo
        g = c.env_offset + e
        r = O.philox4x32_10([t & 0xFFFFFFFF, g & 0xFFFFFFFF, g >> 32, t >> 32], [c.seed & 0xFFFFFFFF, (c.seed >> 32) ^ 0x53414D50])
        assert [float(x) for x in u[e]] == [(r[0] >> 8) / 2.0**24, (r[1] >> 8) / 2.0**24]
    assert (c.env_offset + n // 2 + 36) >> 32 == 0 and (c.env_offset + n // 2 + 37) >> 32 == 1


@pytest.mark.parametrize("drop", ("t_hi", "g_hi", "carry", "tweak"))
def test_at_the_far_counters_every_part_of_them_reaches_a_draw(drop):
    """Dropping t_hi, g_hi, the carry from g_lo into g_hi or the key's tweak changes uniforms of the far case — and, through them,
    actions the reference draws."""
    c = SC.far_case()
    changed = 0
    for t in range(c.steps):
        u, v = SC.uniforms_of(c, t), SC.uniforms(c.seed, c.env_offset, c.step0 + t, c.n_envs, drop=drop)
        rows = (u != v).any(axis=1)
        if drop == "t_hi":
            assert rows.any() == (c.step0 + t >= 2**32)
        if drop in ("g_hi", "carry"):
            assert rows[: c.n_envs // 2 + 37].sum() == 0 and rows[c.n_envs // 2 + 37:].mean() > 0.99  # (the envs above the wrap)
        logits = SC.logits_of(c, t)
        changed += int((SC.sample_f64(logits, u)[0] != SC.sample_f64(logits, v)[0]).sum())
    assert changed > 0


# ------------------------------------------------------------------------------------------ the references
def test_the_sampler_on_rows_written_out_by_hand():
    inf, nan = np.inf, np.nan
    l = np.array([[[0, 0, 0, 0, 0, 0], [-inf, 0, -inf, 0, -inf, -inf]],
                  [[1, 2, 2, 1, 2, 0], [-inf, -inf, -inf, -inf, -inf, 5]],
                  [[-inf] * 6, [0, inf, 0, 0, 0, 0]],
                  [[0, 0, nan, 0, 0, 0], [0, 0, 0, 0, 0, 0]]], np.float32)
    u = np.array([[0.5, 0.0], [0.95, 0.0], [0.5, 0.5], [0.5, 1 - 2.0**-24]], np.float32)
    for sample in (SC.sample_f32, SC.sample_f64):
        a, logp = sample(l, u)[:2]
        assert a.tolist() == [[3, 1], [4, 5], [255, 255], [255, 5]]  # (row 0: x = 3.0 and c_0..c_2 = 1, 2, 3 <= x)
        assert np.isnan(logp[2]).all() and np.isnan(logp[3, 0])
        assert np.allclose(logp[0], [-np.log(6), -np.log(2)]) and logp[1, 1] == 0
        a, logp = sample(l, u, greedy=True)[:2]
        assert a.tolist() == [[0, 1], [1, 5], [255, 255], [255, 0]]  # the lowest index holding the maximum
    assert np.allclose(SC.logp_f64(l[:2], np.array([[3, 1], [4, 5]])), SC.sample_f64(l[:2], u[:2])[1])


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_the_reference_run_of_the_case_holds_what_it_claims(case):
    """The float64 reference's actions stepped through OracleTrainStep; and, on the same samples, the float32 restatement: the same
    actions outside the boundary band, the band's share under its cap, logp within LOGP_TOL."""
    run = SC.oracle_of(case)
    restarts = np.zeros((case.n_envs,), np.int64)
    drawn = np.zeros((2, 6), np.int64)
    sparse = masked = nan_last = in_band = samples = 0
    for t in range(case.steps):
        logits, u = SC.logits_of(case, t), SC.uniforms_of(case, t)
        assert logits.shape == (case.n_envs, 2, 6) and logits.dtype == np.float32 and logits.flags.c_contiguous
        assert not np.isneginf(logits).all(axis=-1).any() and not np.isposinf(logits).any()
        a, logp, band = SC.sample_f64(logits, u, case.greedy)
        a32, logp32 = SC.sample_f32(logits, u, case.greedy)
        assert np.array_equal(a32[~band], a[~band]), (case.id, t)
        valid = a != 255
        assert np.array_equal(a32 == 255, ~valid) and np.isnan(logp32[~valid]).all() and np.isnan(logp[~valid]).all()
        agree = valid & (a32 == a)
        assert np.abs(logp32[agree] - logp[agree]).max() <= SC.LOGP_TOL and np.abs(logp[valid]).max() < 32
        assert np.array_equal(~valid, np.isnan(logits).any(axis=-1)) and (~valid).sum() == len(SC.nan_rows(case, t))
        in_band += int(band.sum())
        samples += band.size
        # a masked action is never drawn; greedy: the lowest-index maximum
        assert np.isfinite(np.take_along_axis(logits, np.minimum(a, 5).astype(np.int64)[..., None], axis=-1)[..., 0][valid]).all()
        if case.greedy:
            assert np.array_equal(a[valid], np.argmax(logits, axis=-1)[valid])
        masked += int(np.isneginf(logits).sum())
        for p in range(2):
            drawn[p] += np.bincount(a[:, p][valid[:, p]], minlength=6)[:6]
        run.step(a, case.factor)
        assert np.array_equal((run.flags & 2) != 0, (~valid).any(axis=1))
        restarts += run.done != 0
        sparse += int((run.rewards[:, :2] != 0).sum())
        nan_last = int((~valid).sum())
    assert in_band <= SC.BAND_CAP * samples, (case.id, in_band, samples)
    held = {"restarts": int(restarts.min()) >= 2, "all_actions": bool((drawn > 0).all()), "masked": masked > 0, "nan_last": nan_last > 0,
            "sparse": sparse > 0}
    assert set(case.claims) <= set(held)
    assert all(held[k] for k in case.claims), (case.id, {k: held[k] for k in case.claims})
