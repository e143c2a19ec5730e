"""tests/rollout_cases.py kept honest without a GPU: every case is planned (oc_rollout_plan) onto the kernel instance it names,
the cases reach every instance the sources list, and on the oracle alone each case contains what it is there for — restarts,
shaped rewards, deliveries, events, re-drawn layouts.  A change to choose_launch (csrc/rollout_dispatch.hpp) that moves a case to another
kernel fails here, by the case's name, instead of silently changing what a GPU test runs."""
import itertools
import os
import re

import pytest

import rollout_cases as RC
from case_support import CSRC, ledger

# Instances no real table reaches, by name, each with the condition of choose_launch that excludes it (at most two)
UNREACHABLE = {}


def _ledger():
    """instance (oc_rollout_plan's words) -> ids of the cases that are there for it"""
    return ledger(RC.CASES, lambda c: c.expect)


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_instance_it_names(case):
    plan = RC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)


def test_cases_keep_the_restart_path_inside_the_launch():
    for c in RC.CASES:
        assert c.horizon < c.n_steps / 2 and c.env_offset > 0 or c.start == "standard", c.id
        assert c.n_steps <= 96 or c.t0 & 7, c.id  # (long launches: the off-grid split only)


def test_every_k_rollout4_instance_of_the_sources_has_a_case():
    """The universe is R4Instances in csrc/shared.hpp, less the six recording instances (oc_rollout_plan plans no recording
    call; tests/test_gpu_rollout_record*.py name them)."""
    with open(os.path.join(CSRC, "shared.hpp")) as f:
        body = re.search(r"using R4Instances = R4List<(.*?)>;", f.read(), re.S).group(1)
    names = [nm.strip() for nm in body.split(",")]
    plain = [nm for nm in names if not nm.startswith("R4Rec")]
    assert len(names) == len(set(names)) and len(names) - len(plain) == 6
    reached = {text for text in _ledger() if text.startswith("k_rollout4<")}
    missing = sorted(set(plain) - {RC.R4_NAME.get(t) for t in reached} - set(UNREACHABLE))
    assert not missing, "no case reaches %s" % missing
    assert len(reached) + len([nm for nm in UNREACHABLE if nm.startswith("R4")]) == len(plain) == len(RC.R4)
    assert sorted(RC.R4) == sorted(plain)


def test_every_k_rollout5_instance_has_a_case():
    """k_rollout5's instances: four table kinds x {tiled flags, flat flags, no output arrays} x {new, old dynamics}
    (with_r5 / with_r5_table, csrc/rollout4.hip)."""
    kinds = ((True, False, False), (False, False, False), (True, True, False), (True, False, True))  # (LAY_LDS, BIG, EV)
    outs = (dict(FT8=True), dict(), dict(NOOUT=True))
    universe = {RC.r5(LAY_LDS=k[0], BIG=k[1], EV=k[2], OLD=old, **o) for k, o, old in itertools.product(kinds, outs, (False, True))}
    assert len(universe) == 24
    with open(os.path.join(CSRC, "rollout4.hip")) as f:
        src = f.read()
    assert len(re.findall(r"with_r5_table<(?:true|false), (?:true|false), (?:true|false)>\(s, f\)", src)) == len(kinds)
    assert len(re.findall(r"f\(R5<LAY_LDS, (?:true|false), (?:true|false), BIG, EV, (?:true|false)>\(\)\)", src)) == 2 * len(outs)
    reached = {text for text in _ledger() if text.startswith("k_rollout5<")}
    assert reached | set(UNREACHABLE) >= universe, "no case reaches %s" % sorted(universe - reached)
    assert reached <= universe, "not an instance: %s" % sorted(reached - universe)


def test_ledger():
    """instance -> case ids, one line per instance (shown by `pytest -s -k test_ledger`)."""
    led = _ledger()
    print()
    for text in sorted(led, key=lambda t: (t.startswith("k_rollout5"), list(RC.R4).index(RC.R4_NAME[t]) if t in RC.R4_NAME else t)):
        print("%-28s %s\n%30s%s" % (RC.R4_NAME.get(text, "k_rollout5"), text, "<- ", ", ".join(led[text])))
    assert len(led) + len(UNREACHABLE) == len(RC.R4) + 24


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_the_oracle_run_of_the_case_is_not_vacuous(case):
    """On the reference alone: every env restarts n_steps // horizon times inside the launch, shaped rewards are earned, drawn
    starts lead to deliveries (under old dynamics a soup exists only because a pot started cooking by itself with its third
    item), event cases publish counters, regen cases move most envs to another layout."""
    run = RC.oracle_launch_of(case)
    lid0 = None if run.layout_id is None else run.layout_id.copy()
    restarts = shaped = sparse = 0
    for _, rew, fl, masks in run.chunks(case.n_steps, t0=case.t0):
        restarts += int(((fl & 4) != 0).sum())
        sparse += float(rew[..., :2].sum())
        shaped += float(rew[..., 2:].sum())
    assert restarts == case.n_envs * (case.n_steps // case.horizon)
    assert shaped > 0
    if case.start != "standard":
        assert sparse > 0
    if case.events:
        assert run.counts_done.sum() > 0
    if case.start == "regen":
        assert (run.layout_id != lid0).mean() > 0.5
