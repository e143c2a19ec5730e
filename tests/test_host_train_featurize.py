"""tests/train_featurize_cases.py kept honest without a GPU: every case is planned (oc_multi_agent_step_featurize_plan) onto what it
names, the k_train_step_feat instances csrc/train_dispatch.hpp instantiates are those the list covers, the entry point refuses what it must
before any device call (this host has none to make), and on the oracle alone each case contains what it claims."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_cases as TC
import train_featurize_cases as FC
from case_support import CSRC, P, check_census, ledger, synthetic_batch, table_of, train_selector

ALL = FC.CASES + (FC.far_case(),)


def _plan(b, horizon=11, with_obs=0, obs_dtype=None, with_features=1, num_pots=2, options=0, use_phi=1, event_sink=0, start=None):
    """oc_multi_agent_step_featurize_plan of a batch -> (rc, text or the refusal's message)"""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    rc = L.oc_multi_agent_step_featurize_plan(ctypes.byref(b) if b is not None else None, horizon, with_obs,
                                              _lib.OBS_U8 if obs_dtype is None else obs_dtype, with_features, num_pots, options, use_phi,
                                              event_sink, ctypes.byref(start) if start is not None else None, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


# ------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_the_planner_gives_the_case_what_it_names(case):
    plan = FC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    if case.expect.startswith("k_train_step_feat<"):
        assert re.fullmatch(r"k_train_step_feat<MAXP=[12]> G=(32|16|8), grid=%d, \d+ B LDS" % -(-case.n_envs // 256), plan), plan
    else:  # oc_multi_agent_plan's words for the same call, then oc_featurize_plan's
        from overcooked_ai_amd import _lib, dispatch

        step = dispatch.multi_agent_plan(table_of(case.table), case.n_envs, horizon=case.horizon,
                                         obs_dtype=_lib.OBS_U8 if case.obs_dtype == "u8" else _lib.OBS_F32, with_obs=case.obs == "both",
                                         use_phi=case.use_phi, event_sink=case.events, start=FC.start_spec_of(case))
        b = dispatch.batch_for(table_of(case.table), case.n_envs)
        out = ctypes.create_string_buffer(320)
        assert _lib.load().oc_featurize_plan(ctypes.byref(b), case.num_pots, out, len(out)) == 0
        assert plan == step + " + " + out.value.decode()


def test_the_default_plan_takes_the_kernel_from_the_threshold_on():
    c = FC.default_plan_case()
    assert FC.plan_of_case(c).startswith(c.expect)
    below = FC.plan_of_case(c, c.n_envs - 1)
    assert "k_train_step_feat" not in below and below.startswith(FC.two_launches(TC.step1(True, 1, True))), below
    assert c.n_envs % 256 == 0 and c.horizon < c.steps / 2  # whole workgroups; two restarts per env


def test_four_pot_blocks_get_smaller_images_and_the_plan_says_so():
    by_id = {c.id: c for c in FC.CASES}
    g = lambda c: int(re.search(r" G=(\d+),", FC.plan_of_case(c)).group(1))  # noqa: E731
    assert g(by_id["feat_four_pot_blocks_smaller_images"]) < 32 == g(by_id["feat_two_pots_ragged_last_workgroup"])
    for c in FC.CASES:  # the LDS figure is the shape calculation's: rows, header, two records, rewards, eight images of whole 16 bytes
        if c.expect.startswith("k_train_step_feat<"):
            plan, t = FC.plan_of_case(c), table_of(c.table)
            image = (g(c) * 2 * (FC.total_of(c.num_pots) + 2) * 2 + 15) // 16 * 16
            assert int(re.search(r", (\d+) B LDS", plan).group(1)) == (t.n_planes - 1 + 4) * 256 * 16 + 8 * image <= 150 * 1024, plan


def test_the_instances_of_the_sources_are_those_the_list_covers():
    with open(os.path.join(CSRC, "train_dispatch.hpp")) as f:
        src = f.read()
    assert "k_train_step_feat<MP>" in src
    found = [FC.feat_k(int(p)) for p, _ in train_selector("feat")[0]]  # one line of select_train_feat each
    reached = {c.expect for c in ALL if c.expect.startswith("k_train_step_feat<")}
    check_census(found, FC.INSTANCES, {}, reached, 2, "k_train_step_feat instances")
    led = ledger(ALL, lambda c: c.expect)
    assert all(len(led[i]) >= 2 for i in FC.INSTANCES)


def test_the_cases_cover_what_the_issue_lists():
    forced = [c for c in FC.CASES if c.expect.startswith("k_train_step_feat<")]
    other = [c for c in FC.CASES if not c.expect.startswith("k_train_step_feat<")]
    assert {c.n_envs for c in forced} >= {1, 33, 65, 256 + 232} and all(c.one_kernel for c in forced)
    assert {c.table for c in forced} >= {"cramped_room", "asymmetric_advantages", "coordination_ring", "cramped_room_old"}
    assert {c.num_pots for c in forced} == {0, 1, 2, 4} and {c.counter_goals for c in forced} == {"all", "none"}
    assert {c.use_phi for c in forced} == {True, False} and {c.factor for c in forced} >= {0.37, "anneal"}
    assert {c.start for c in forced} == {"standard", "drawn"}
    assert {(c.obs, c.obs_dtype) for c in other} >= {("both", "u8"), ("both", "f32")} and any(c.events for c in other)
    assert {c.table for c in other} >= {"mix5", "marshmallow_experiment", "seven_pots"} and any(c.start == "regen" for c in other)
    assert any(not c.one_kernel and c.obs == "features" and not c.events and c.table == "cramped_room" for c in other)
    assert table_of("marshmallow_experiment").n_cells == 65
    for c in FC.CASES:
        assert c.horizon < c.steps / 2 and c.env_offset > 0 and c.steps % c.horizon >= 3, c.id
    far = FC.far_case()
    assert far.seed >> 32 and far.seed & 0xFFFFFFFF and far.env_offset < 2**32 < far.env_offset + far.n_envs


# ------------------------------------------------------------------------------------------ refusals (no device call: none exists here)
def test_features_off_is_oc_multi_agent_plan_word_for_word():
    from overcooked_ai_amd import _lib, dispatch

    for name, n, obs in (("cramped_room", 65536, True), ("cramped_room", 200, False), ("mix5", 3000, True), ("seven_pots", 1500, True)):
        got = dispatch.multi_agent_featurize_plan(table_of(name), n, with_obs=obs, with_features=False, obs_dtype=_lib.OBS_U8)
        assert got == dispatch.multi_agent_plan(table_of(name), n, with_obs=obs, obs_dtype=_lib.OBS_U8), (name, got)


def test_the_plan_refuses_what_the_entry_point_refuses():
    from overcooked_ai_amd import _lib

    who = "oc_multi_agent_step_featurize: "
    ok = synthetic_batch(5, 4, 1000)
    assert _plan(ok)[0] == 0
    for kw, b, why in ((dict(num_pots=5), ok, "num_pots must be in 0..4"), (dict(num_pots=-1), ok, "num_pots must be in 0..4"),
                       (dict(), synthetic_batch(5, 4, 1000, flags=0), "d_features needs 2-player layouts"),
                       (dict(options=_lib.OPT_AUTO_RESET), ok, "options other than OC_OPT_ONE_KERNEL"),
                       (dict(options=_lib.OPT_ONE_KERNEL | _lib.OPT_FLAGS_TILED8), ok, "options other than OC_OPT_ONE_KERNEL"),
                       (dict(horizon=0), ok, "horizon must be in 1..65535"),  # oc_multi_agent_step's own, under the new name
                       (dict(start=_lib.OcStartSpec(1, 0, 1, 1, 1.5, 0, 0)), ok, "start.rnd_obj_prob_thresh must be in [0, 1]")):
        rc, msg = _plan(b, **kw)
        assert rc != 0 and msg.startswith(who + why), (kw, msg)
    rc, msg = _plan(ok, options=_lib.OPT_AUTO_RESET, with_features=0)  # (the options are this entry point's, features or not)
    assert rc != 0 and msg.startswith(who)
    assert _plan(synthetic_batch(5, 4, 0))[1] == "nothing to launch (no envs)"


def test_the_entry_point_refuses_before_any_device_call():
    """With stand-in pointers: a call that got past its checks would fault at the first launch, and this host has no device."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    who = "oc_multi_agent_step_featurize: "

    def call(b, features=P, tables=(P, P), num_pots=2, options=0, horizon=11, done=P, shaped=P, phi=(P, P, P, P, P, P), obs=None):
        plan_blob, plan_off, phi_tables, phi_next, phi_cur, phi_start = phi
        rc = L.oc_multi_agent_step_featurize(ctypes.byref(b), P, P, P, P, P, P, plan_blob, plan_off, phi_tables, phi_next, phi_cur, phi_start,
                                             0.5, shaped, done, obs, _lib.OBS_U8, horizon, tables[0], tables[1], features, num_pots, options,
                                             None, None, None)
        return rc, L.oc_last_error().decode()

    ok = synthetic_batch(5, 4, 1000)
    for kw, b, why in ((dict(features=P + 8), ok, "d_features must be 16-byte aligned"),
                       (dict(num_pots=5), ok, "num_pots must be in 0..4"),
                       (dict(), synthetic_batch(5, 4, 1000, flags=0), "d_features needs 2-player layouts"),
                       (dict(options=0x40), ok, "options other than OC_OPT_ONE_KERNEL"),
                       (dict(tables=(None, P)), ok, "d_features needs the feature plan tables"),
                       (dict(tables=(P, None), phi=(None,) * 6), ok, "d_features needs the feature plan tables"),  # (also with use_phi off)
                       # oc_multi_agent_step's own refusals, under the new name
                       (dict(done=None), ok, "d_done is required"),
                       (dict(horizon=70000), ok, "horizon must be in 1..65535"),
                       (dict(shaped=P + 8), ok, "d_shaped must be 16-byte aligned"),
                       (dict(phi=(None, P, P, P, P, P)), ok, "use_phi needs the plan tables and the three phi buffers")):
        rc, msg = call(b, **kw)
        assert rc != 0 and msg.startswith(who + why), (kw, msg)
    # no features: the call is oc_multi_agent_step, refusals and their name included; and no envs: nothing to do
    rc, msg = call(ok, features=None, done=None)
    assert rc != 0 and msg.startswith("oc_multi_agent_step: d_done is required"), msg
    assert call(synthetic_batch(5, 4, 0))[0] == 0 and call(synthetic_batch(5, 4, 0), features=None)[0] == 0


# ------------------------------------------------------------------------------------------ the oracle's run holds what the case claims
@pytest.mark.parametrize("case", ALL + (FC.DEFAULT_PLAN,), ids=lambda c: c.id)
def test_the_reference_run_of_the_case_holds_what_it_claims(case):
    if case.n_envs is None:
        case = FC.default_plan_case()
    run = TC.oracle_of(case)
    restarts = np.zeros((case.n_envs,), np.int64)
    sparse = phi_moves = feat_moves = counter_object = last_illegal = 0
    prev = FC.features_of(case, run)
    assert prev.shape == (case.n_envs, 2, FC.total_of(case.num_pots))
    for t in range(case.steps):
        phi_before = run.phi_cur.copy()
        run.step(FC.actions_of(case, t), TC.factor_at(case, t))
        restarts += run.done != 0
        sparse += int((run.rewards[:, :2] != 0).sum())
        phi_moves += int((run.phi_next != phi_before).any()) if case.use_phi else 0
        feats = FC.features_of(case, run)
        assert np.array_equal(feats, np.round(feats)) and np.abs(feats).max() < 2**15  # small integers: exact in f32 (and in the int16 image)
        feat_moves += int((feats != prev).any())
        prev = feats
        if case.counter_goals == "all":
            # (own block 8..17: the closest onion, tomato, dish and soup with its counts — not 20, 21, the closest EMPTY counter)
            counter_object += int((feats[..., 8:18] != FC.features_of(case, run, "none")[..., 8:18]).any())
        last_illegal = int(((run.flags & 2) != 0).sum())
    held = {"restarts": int(restarts.min()) >= 2, "sparse": sparse > 0, "phi": phi_moves > 0, "illegal_last": last_illegal > 0,
            "features_move": feat_moves > 0, "counter_object": counter_object > 0}
    assert set(case.claims) <= set(held)
    assert all(held[k] for k in case.claims), (case.id, {k: held[k] for k in case.claims})
