"""tests/train_cases.py kept honest without a GPU: every case is planned (oc_multi_agent_plan) onto the path or kernel instance it
names, the cases and the named exclusions cover every training-step kernel instance csrc/train_dispatch.hpp instantiates, and on the
reference alone each case contains what it is there for — restarts, sparse and shaped rewards, a changing potential, illegal
actions, event counters, re-drawn layouts.  A change to plan_train (csrc/train_dispatch.hpp) that moves a case to another kernel
fails here, by the case's name, instead of silently changing what a GPU test runs."""
import os

import numpy as np
import pytest

import train_cases as TC
from case_support import CSRC, check_census, ledger, print_ledger, train_kernels_named_in_launch_code, train_selector


def _ledger():
    """instance or sequence (oc_multi_agent_plan's words) -> ids of the cases that are there for it"""
    return ledger(TC.CASES, lambda c: c.expect)


def _instantiated():
    """The training-step kernel instances the selectors of csrc/train_dispatch.hpp name (one line each), in oc_multi_agent_plan's
    words."""
    with open(os.path.join(CSRC, "train_dispatch.hpp")) as f:
        src = f.read()
    kinds = {"uint8_t": "u8", "float": "f32"}
    (obs, _), (lean, _), (general, sampled) = train_selector("obs"), train_selector("step1"), train_selector("step")
    assert not sampled  # k_train_step has no SAMPLE parameter
    assert "k_train_step<U, 2, U, false, EV>" in src and "k_train_step1<U, MP, LL>" in src and "k_train_step_obs<MP, T, NW>" in src
    found = [TC.obs_k(int(p), kinds[t], int(w)) for p, t, w, _ in obs]
    found += [TC.step1(u == "true", int(p), ll == "true") for u, p, ll, _ in lean]
    found += [TC.step_k(u == "true", ev == "true") for u, ev in general]
    return found


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_instance_it_names(case):
    plan = TC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    if case.expect.startswith("k_"):  # the observation: inside k_train_step_obs, else the kernel after the step's
        assert plan.endswith(" + oc_encode_lossless") == (case.obs is not None and not case.expect.startswith("k_train_step_obs")), plan


def test_cases_keep_the_restart_path_inside_the_run():
    for c in TC.CASES:
        assert c.horizon < c.steps / 2 and c.env_offset > 0 or c.start == "standard", c.id
        assert c.steps % c.horizon >= 1 and c.n_envs >= TC.N_BAD * c.steps + 2, c.id  # (room for one illegal action per env)
    assert any(c.env_offset % 256 and c.n_envs >= 131072 + 232 for c in TC.CASES)
    assert {c.n_envs for c in TC.CASES} >= {TC.N_OBS - 1, TC.N_OBS, TC.N_OBS + 1, TC.N_OBS + 65}


def test_every_training_step_instance_of_the_sources_has_a_case_or_a_named_exclusion():
    check_census(_instantiated(), TC.INSTANCES, TC.UNREACHABLE, {text for text in _ledger() if text.startswith("k_")}, 16, "training-step kernels")
    # the sequence: drawn and standard starts, and oc_regen_layouts inside it
    seq = [text for text in _ledger() if text.startswith("sequence:")]
    assert any("oc_regen_layouts" in t for t in seq) and any("oc_reset_random" in t for t in seq) and any(t.endswith("oc_reset, oc_encode_lossless") for t in seq)


def test_each_training_step_instance_is_named_in_one_place():
    """Outside the four launch templates of csrc/train_dispatch.hpp — each reached through its selector alone (train_selector) — no
    source of the library names a training-step kernel with template arguments: nothing else can launch one."""
    assert sorted(train_kernels_named_in_launch_code()) == sorted(("train_dispatch.hpp", k) for k in (
        "k_train_step_obs<MP, T, NW>", "k_train_step_obs<MP, T, NW, true, SampleArgs>", "k_train_step_feat<MP>",
        "k_train_step_feat<MP, true, SampleArgs>", "k_train_step1<U, MP, LL>", "k_train_step1<U, MP, LL, true, SampleArgs>",
        "k_train_step<U, 2, U, false, EV>"))
    for kind in ("obs", "feat", "step1", "step"):
        train_selector(kind)


def test_the_named_exclusions_hold():
    """f32 observations never get 16 wavefronts: whatever the planner answers for an f32 call, it is not such an instance."""
    from overcooked_ai_amd import _lib, dispatch

    for name in ("cramped_room", "cramped_room_two_pots", "scenario2_s", "coordination_ring", "asymmetric_advantages"):
        plan = dispatch.multi_agent_plan(TC.table_of(name), 65536, obs_dtype=_lib.OBS_F32)
        assert not any(plan.startswith(text) for text in TC.UNREACHABLE), (name, plan)


def test_ledger():
    """instance -> case ids, one line per instance (shown by `pytest -s -k test_ledger`)."""
    led = _ledger()
    print_ledger(TC.INSTANCES, led, TC.UNREACHABLE)
    for text in sorted(t for t in led if t.startswith("sequence:")):
        print("%s\n%30s%s" % (text, "<- ", ", ".join(led[text])))
    assert len([t for t in led if t.startswith("k_")]) + len(TC.UNREACHABLE) == len(TC.INSTANCES) == 16


def test_the_cases_cover_what_the_paths_differ_in():
    cs = TC.CASES
    assert {c.use_phi for c in cs} == {True, False} and {c.obs for c in cs} == {"u8", "f32", None}
    assert {c.factor for c in cs} >= {0.37, "anneal"} and {c.start for c in cs} == {"standard", "drawn", "regen"}
    anneal = next(c for c in cs if c.factor == "anneal")
    assert TC.factor_at(anneal, 0) == 1.0 and TC.factor_at(anneal, anneal.steps - 1) == 0.663 == 1.0 * (1 - 337 / 1000) and TC.anneal_at(anneal) % anneal.horizon
    for path in ("k_train_step_obs<", "k_train_step1<", "k_train_step<", "sequence:"):  # old dynamics on every path
        assert any(c.expect.startswith(path) and c.table.endswith("_old") for c in cs), path
        assert all(s.old_dynamics for c in cs if c.table.endswith("_old") for s in TC.table_of(c.table).specs)
    big = TC.table_of("marshmallow_experiment")
    assert big.n_cells > 64 and TC.table_of("big_4").n_cells > 64 and len(TC.table_of("canonical_5_x8")) > 32


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_the_reference_run_of_the_case_is_not_vacuous(case):
    """On the reference alone: every env restarts steps // horizon times, drawn starts earn sparse rewards, the potential changes
    on most steps (use_phi), illegal actions are flagged, event cases publish counters, regen cases move most envs to another
    layout, and some env finishes an episode on a step whose factor * dense is not zero."""
    run = TC.oracle_of(case)
    lid0 = None if run.layout_id is None else run.layout_id.copy()
    restarts = flagged = moving = done_with_dense = 0
    sparse = 0.0
    for t in range(case.steps):
        run.step(TC.actions_of(case, t), TC.factor_at(case, t))
        restarts += int(run.done.sum())
        flagged += int(((run.flags & 2) != 0).sum())
        sparse += float(run.rewards[:, :2].sum())
        moving += int((run.dense != 0).any())
        done_with_dense += int(((TC.factor_at(case, t) * run.dense != 0).any(axis=1) & (run.done != 0)).sum())
    assert restarts == case.n_envs * (case.steps // case.horizon)
    assert flagged == TC.N_BAD * case.steps + 1
    if case.start != "standard":
        assert sparse > 0
    if case.use_phi:
        assert moving > case.steps / 2
    assert done_with_dense > 0
    if case.events:
        assert run.counts_done.sum() > 0 and run.counts.sum() > 0
    if case.start == "regen":
        assert (run.layout_id != lid0).mean() > 0.5
