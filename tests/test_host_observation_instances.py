"""tests/obs_cases.py kept honest without a GPU: every case is planned (oc_observation_plan) onto the kernel instance it names, the
cases and the named exclusions cover the 13 observation kernel instances csrc/observation_dispatch.hpp instantiates, the exclusions hold for every
grid the single kernel takes, and on the oracle alone each case contains what it is there for — urgent and other envs in one
sub-group, restarts inside the launch, crowded and sparse sub-groups side by side, every kind of object, flagged illegal actions.
A change to plan_encode / plan_rollout_encode (csrc/observation_plan.hpp) that moves a case to another kernel fails here, by the
case's name, instead of silently changing what a GPU test runs."""
import os
import re

import numpy as np
import pytest

import obs_cases as OC
from case_support import CSRC, check_census, function_body as _function, ledger, observation_plan as plan, pot_kinds, print_ledger, synthetic_batch as batch
from overcooked_ai_amd import _lib

U8, F32, ONE_KERNEL = _lib.OBS_U8, _lib.OBS_F32, _lib.OPT_ONE_KERNEL
ROLLOUTS = [c for c in OC.CASES if c.call != "encode"]
SINGLE = [c for c in ROLLOUTS if c.expect.startswith("k_rollout_encode<")]
ENCODES = [c for c in OC.CASES if c.call == "encode"]


def _ledger():
    """instance (oc_observation_plan's words) -> ids of the cases that are there for it"""
    return ledger(OC.CASES, OC.instance_of)


def _instantiated():
    """The observation kernel instances launch_encode and launch_rollout_encode (csrc/observation_dispatch.hpp) launch, and the ones
    rollout_encode_lds asks the runtime about, in oc_observation_plan's words."""
    with open(os.path.join(CSRC, "observation_dispatch.hpp")) as f:
        src = f.read()
    kinds = {"uint8_t": "u8", "float": "f32"}
    enc = _function(src, "launch_encode")
    assert "hipLaunchKernelGGL((k_encode<T, LAY_LDS>)" in enc
    found = [OC.uniform(0, 0, 0).split(">")[0] + ">" for _ in re.findall(r"hipLaunchKernelGGL\(\(k_encode_uniform<uint8_t>\)", enc)]
    found += [OC.generic(kinds[t], ll == "true") for t, ll in re.findall(r"\bgeneric\((uint8_t|float)\(\), std::(true|false)_type\(\)\)", enc)]
    ro = _function(src, "launch_rollout_encode")
    assert "hipLaunchKernelGGL((k_rollout_encode<2, FAST, T, NW>)" in ro
    types = re.findall(r"\bgo\(fast, (uint8_t|float)\(\), nw\)", ro)  # go_t's body: one go per observation type
    shapes = re.findall(r"\bgo_t\(integral_constant<int, (\d)>\(\), integral_constant<int, (\d)>\(\)\)", ro)
    found += [OC.single(int(f), kinds[t], int(w)) for f, w in shapes for t in types]
    asked = [OC.single(int(f), kinds[t], int(w)) for f, t, w in
             re.findall(r"k_rollout_encode<2, (\d), (uint8_t|float), (\d)>", _function(src, "rollout_encode_lds"))]
    return found, asked


@pytest.mark.parametrize("case", OC.CASES, ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_instance_it_names(case):
    text = OC.plan_of_case(case)
    assert text.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, text, case.expect)
    assert OC.instance_of(case) in OC.INSTANCES, case.id
    if case in SINGLE:  # every row of the trajectory a multiple of 16 bytes, or one buffer: the env class hands the call to the library
        assert case.call in ("rollout_single_buffer", "step_encode") or case.n_envs * OC.env_bytes(case) % 16 == 0, case.id


def test_every_observation_instance_of_the_sources_has_a_case_or_a_named_exclusion():
    found, asked = _instantiated()
    reached = set(_ledger())
    check_census(found, OC.INSTANCES, OC.UNREACHABLE, reached, 13, "observation kernels")
    assert set(asked) <= set(found) and len(asked) == 4  # (the budget is asked of one instance per FAST and T)
    assert len(reached) == 9 and len(OC.UNREACHABLE) == 4
    # the paths that are no instance: oc_step_encode on the single kernel, and both step-by-step entry points
    assert {c.call for c in OC.CASES} == set(OC.CALLS)
    assert {c.expect.split(" + ")[0] for c in OC.CASES if c.expect.startswith("step by step")} == {"step by step: oc_rollout_random", "step by step: oc_step"}


def test_ledger():
    """instance -> case ids, one line per instance (shown by `pytest -s -k test_ledger`)."""
    led = _ledger()
    print_ledger(OC.INSTANCES, led, OC.UNREACHABLE)
    assert len(led) + len(OC.UNREACHABLE) == len(OC.INSTANCES) == 13


def test_the_named_exclusions_hold():
    """For every grid the single kernel takes (W, H >= 3, at most 48 cells), with and without the two-players hint: the f32 plan
    names eight wavefronts on 3x3 only, the u8 plan never names four.  And every two-player registry layout of at most 48 cells (one
    or two pots) is planned onto an instance that is not excluded."""
    from overcooked_ai_amd import _lib, dispatch
    from overcooked_ai_amd.layouts import LayoutTable, layout_names, spec_from_name

    for w in range(3, 17):
        for h in range(3, 17):
            if w * h > 48:
                continue
            for flags in (_lib.BATCH_TWO_PLAYERS, 0):
                for pots in (1, 2):
                    rc, f32 = plan(batch(w, h, 260, max_pots=pots, flags=flags), F32, 2, ONE_KERNEL)
                    assert rc == 0 and f32.startswith("k_rollout_encode<") and ("NW=8>" in f32) == ((w, h) == (3, 3)), (w, h, f32)
                    rc, u8 = plan(batch(w, h, 260, max_pots=pots, flags=flags), U8, 2, ONE_KERNEL)
                    assert rc == 0 and u8.startswith("k_rollout_encode<") and "NW=4>" not in u8, (w, h, u8)
    seen = 0
    for name in layout_names():
        spec = spec_from_name(name)
        if spec.num_players != 2 or spec.width * spec.height > 48:
            continue
        table = LayoutTable([spec])
        for code in (_lib.OBS_U8, _lib.OBS_F32):
            text = dispatch.observation_plan(table, 260, 2, code, options=_lib.OPT_ONE_KERNEL)
            assert text.startswith("k_rollout_encode<") == (1 <= table.max_pots <= 2), (name, text)
            assert not any(text.startswith(x) for x in OC.UNREACHABLE), (name, text)
            seen += text.startswith("k_rollout_encode<")
    assert seen >= 40
    # a 3x3 grid seats one player at most, and the oracle refuses to encode a one-player layout
    from oracle import oracle as O

    one = spec_from_name("cramped_room_single")
    assert one.num_players == 1
    with pytest.raises(AssertionError, match="2 players"):
        O.Oracle([O.mdp_from_layout_dict(one.to_layout_dict())]).encode_lossless(np.zeros((3, 1, 16), np.uint8))


def _derived(w, h, f32, budget):
    """(NW, unit, G, LDS bytes) of k_rollout_encode for a W x H grid within `budget`, from the rules at the head of
    tests/test_host_observation_plan.py"""
    cells = w * h
    n_obj, env = (cells + 15) // 16, 2 * cells * 26 * (4 if f32 else 1)
    unit = 1
    while env * unit % 16:
        unit *= 2
    fixed = 8192 * n_obj + unit * env + 4096 + 7424
    nw, gmax = 8, min(64, (budget - fixed) // (8 * env))
    if gmax < (8 if f32 else 4) or gmax < unit:
        nw, gmax = 4, min(64, (budget - fixed) // (4 * env))
    span = 32 if nw == 8 else 64
    parts = -(-span // gmax)
    even = -(-span // parts)
    g = -(-even // unit) * unit  # up to whole templates ...
    if g > gmax:
        g = gmax - gmax % unit   # ... or what fits, down to whole templates
    return nw, unit, g, fixed + nw * g * env, g > even


def test_the_single_kernel_shape_of_every_grid_follows_the_rules():
    """For every grid the single kernel takes, u8 and f32: the wavefronts, the unit, G and the LDS bytes the planner names are the
    ones the rules give for the budget it names (rounding G the other way, or to no whole template, fails here on 6x3 and 7x3)."""
    rounded_up = []
    for w in range(3, 17):
        for h in range(3, 17):
            if w * h > 48:
                continue
            for dtype, t in ((U8, "u8"), (F32, "f32")):
                rc, text = plan(batch(w, h, 260, max_pots=2), dtype, 2, ONE_KERNEL)
                budget = int(text.rsplit("budget ", 1)[1].split(" B ")[0])
                nw, unit, g, lds, up = _derived(w, h, dtype == F32, budget)
                assert rc == 0 and text.startswith(OC.single(3, t, nw, unit, g, lds) + ", budget"), (w, h, text, (nw, unit, g, lds))
                assert g % unit == 0 and g >= unit and lds <= budget
                rounded_up += [(w, h)] if up else []
    assert (7, 3) in rounded_up, rounded_up  # (obs_cases' seven_by_three: G = 12 for any budget)


def test_the_hand_written_tables():
    six, eight, seven = OC.table_of("six_by_five"), OC.table_of("eight_by_four"), OC.table_of("seven_by_three")
    assert (seven.width, seven.height, seven.max_pots, seven.n_cells % 2) == (7, 3, 2, 1)
    assert (six.width, six.height, six.max_pots) == (6, 5, 2) and six.n_cells % 4 == 2
    assert (eight.width, eight.height, eight.max_pots, eight.n_planes) == (8, 4, 2, 3)
    assert len(eight.specs[0].cells_of("X")) + len(eight.specs[0].cells_of("P")) > OC.LIST_CAP
    for t in (six, eight, seven):
        assert t.specs[0].num_players == 2
    # no registry layout of at most 48 cells has observation rows of 8 mod 16 bytes
    from overcooked_ai_amd.layouts import layout_names, spec_from_name

    for name in layout_names():
        s = spec_from_name(name)
        assert s.width * s.height > 48 or s.width * s.height % 4 != 2, name


def test_the_streamed_case_really_crosses_the_threshold():
    """k_encode takes its streaming-store branch when env_bytes * n_envs > 320 MiB (csrc/encode.hpp): the streamed case is above it,
    by less than three envs, and every other encode case is below it — the one listed before it among them."""
    with open(os.path.join(CSRC, "encode.hpp")) as f:
        src = f.read()
    m = re.findall(r"if \(env_bytes \* \(size_t\)n > \(\(size_t\)(\d+) << (\d+)\)\)", src)
    assert m == [("320", "20")], m
    limit = int(m[0][0]) << int(m[0][1])
    c = OC.STREAMED
    assert OC.instance_of(c).startswith("k_encode<") and c.n_envs * OC.env_bytes(c) > limit >= (c.n_envs - 3) * OC.env_bytes(c)
    before = OC.CASES[OC.CASES.index(c) - 1]
    assert before.call == "encode" and before.dtype == "f32" and before.n_envs * OC.env_bytes(before) <= limit
    assert all(x.n_envs * OC.env_bytes(x) <= limit for x in ENCODES if x is not c)


def _urgent(state, horizon):
    """bool [n_envs]: the envs in their last 40 steps (mdp.py:2446-2447), from the packed timestep."""
    t = state[0, :, 6].astype(np.int64) | (state[0, :, 7].astype(np.int64) << 8)
    return horizon - t < 40


def _groups(n_envs, span, g):
    """(first, last + 1) of every set of envs encoded together: `g` consecutive envs within `span` (a wavefront's 64; the batch)."""
    return [(a, min(a + g, w + span, n_envs)) for w in range(0, n_envs, span) for a in range(w, min(w + span, n_envs), g)]


def _objects(state):
    """int [n_envs]: objects on each env's grid, soups in pots included — what k_rollout_encode's compact lists count"""
    return (state[1:] != 0).sum(axis=(0, 2))


def _pot_kinds(case, state):
    return pot_kinds(OC.table_of(case.table), OC.layout_ids(case), state)


@pytest.mark.parametrize("case", ROLLOUTS, ids=lambda c: c.id)
def test_the_reference_run_of_a_rollout_case_is_not_vacuous(case):
    """On the oracle alone.  The states the run starts from hold idle, cooking and ready pots and held soups; at every step some
    sub-group (G consecutive envs of a 64-env wavefront; step by step: a block or group of the encode kernel) holds urgent and other
    envs; at least n_envs / 8 restarts fall inside the call; illegal actions are flagged, one by one.  Crowded cases: on at least a
    third of the steps one sub-group's largest object count is above the list's capacity and another's is not, and counts of
    exactly 14 and 15 both occur."""
    text = OC.plan_of_case(case)
    groups = _groups(case.n_envs, 64 if case in SINGLE else case.n_envs, OC.group_envs(case, text))
    run = OC.OracleRun(case)
    assert all(v > 0 for v in _pot_kinds(case, run.state)), (case.id, _pot_kinds(case, run.state))
    restarts = flagged = both = 0
    counts = set()
    for k in range(case.n_steps):
        _, fl = run.step(k)
        restarts += int(((fl & 4) != 0).sum())
        flagged += int(((fl & 2) != 0).sum())
        urgent = _urgent(run.state, case.horizon)
        assert any(urgent[a:b].any() and not urgent[a:b].all() for a, b in groups), (case.id, k)
        n_obj = _objects(run.state)
        counts |= set(n_obj.tolist())
        largest = [int(n_obj[a:b].max()) for a, b in groups]
        both += max(largest) > OC.LIST_CAP and min(largest) <= OC.LIST_CAP
    assert restarts >= case.n_envs / 8, (case.id, restarts)
    assert flagged == (OC.n_illegal(case) if run.actions is not None else 0), (case.id, flagged)
    if case.fill is OC.THIRDS:
        assert both >= case.n_steps / 3 and {OC.LIST_CAP, OC.LIST_CAP + 1} <= counts, (case.id, both, sorted(counts))


@pytest.mark.parametrize("case", ENCODES, ids=lambda c: c.id)
def test_the_states_of_an_encode_case_are_not_vacuous(case):
    """Urgent and other envs fall in the same block (k_encode: epb envs) or group (k_encode_uniform: unit * upg envs) — with blocks
    of one env: in the batch —, its ragged last one included where there is one; every kind of object (onion, tomato, dish, soup)
    lies on a counter somewhere, and the pots are idle, cooking and ready."""
    text = OC.plan_of_case(case)
    g = OC.group_envs(case, text)
    state = OC.states_of(case)
    urgent = _urgent(state, case.horizon)
    groups = _groups(case.n_envs, case.n_envs, g) if g > 1 else [(0, case.n_envs)]
    assert any(urgent[a:b].any() and not urgent[a:b].all() for a, b in groups), case.id
    if g > 2 and case.n_envs % g > 1:
        a, b = groups[-1]
        assert urgent[a:b].any() and not urgent[a:b].all(), case.id
    assert all(v > 0 for v in _pot_kinds(case, state)), case.id
    table, lid = OC.table_of(case.table), OC.layout_ids(case)
    kinds = set()
    for l, spec in enumerate(table.specs):
        st = state if lid is None else state[:, lid == l]
        for x, y in spec.cells_of("X"):
            cell = y * spec.width + x
            kinds |= {min(int(o), 0x80) for o in np.unique(st[1 + (cell >> 4), :, cell & 15]) if o}
    assert kinds == {1, 2, 3, 0x80}, (case.id, kinds)


def test_the_cases_cover_what_the_paths_differ_in():
    by_id = {c.id: c for c in OC.CASES}
    units = {(c.call == "encode", int(re.search(r"unit=(\d)", c.expect).group(1))) for c in OC.CASES if "unit=" in c.expect and not c.expect.startswith("step")}
    assert units >= {(True, 1), (True, 2), (True, 4), (False, 1), (False, 2), (False, 4)}
    assert {c.dtype for c in SINGLE if not c.hint} == {"u8", "f32"} and {c.dtype for c in SINGLE if c.fill} == {"u8"}
    assert by_id["rollout_u8_unit2_single_buffer"].n_envs % 64 == 1 and by_id["rollout_u8_unit2"].n_envs % 64 == 2
    assert OC.table_of("eight_by_four").n_planes - 1 <= 2 < OC.table_of("asymmetric_advantages").n_planes - 1  # (8 / 16 dword slots)
    assert all(c.t0 > 0 for c in OC.CASES if c.call in ("rollout", "rollout_single_buffer"))
    assert all(c.horizon - 40 > 0 and c.n_steps == 14 for c in ROLLOUTS)
    assert {c.start for c in SINGLE} == {"standard", "drawn"}
