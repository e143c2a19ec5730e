"""tests/derived_cases.py kept honest without a GPU: every case is planned (oc_potential_plan / oc_featurize_plan) onto the kernel
instance it names, the cases cover the four kernel instances csrc/derived_dispatch.hpp launches for oc_potential and oc_featurize, the
planners' selection boundaries and refusals hold, the states of every case hold the situations the case lists — at least one
wavefront's worth of envs each, and one in every whole workgroup —, and the set orders those states ask for on the new layouts are
the running interpreter's.  A change to the planners that moves a case to another kernel fails here, by the case's name, instead of
silently changing what a GPU test runs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import derived_cases as DC
from case_support import CSRC, check_census, function_body as _function, ledger, print_ledger, synthetic_batch as batch

NEW_TABLES = ("three_pots", "eight_pots_serve_ring", "one_player_two_pots", "mdp_test_tomato")


def _ledger():
    return ledger(DC.CASES, lambda c: c.expect)


def _instantiated():
    """The kernel instances oc_potential and oc_featurize (csrc/derived_dispatch.hpp) launch, in their planners' words."""
    with open(os.path.join(CSRC, "derived_dispatch.hpp")) as f:
        src = f.read()
    pot = _function(src, "oc_potential")
    found = re.findall(r"hipLaunchKernelGGL\((k_potential2?),", pot)
    tf = re.findall(r"\blaunch_featurize<(true|false)>\(", _function(src, "oc_featurize"))
    assert "hipLaunchKernelGGL((k_featurize<LAY_LDS>)" in _function(src, "launch_featurize")
    found += ["k_featurize<LAY_LDS=%s>" % v for v in tf]
    # ... and nothing else launches them (the fused training kernels call potential2_core, not the kernels)
    everything = ""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(CSRC, name)) as f:
                everything += f.read()
    assert len(re.findall(r"hipLaunchKernelGGL\(\(?k_(?:potential|featurize)", everything)) == 3
    return found


def test_every_derived_instance_of_the_sources_has_a_case_or_a_named_exclusion():
    check_census(_instantiated(), DC.INSTANCES, DC.UNREACHABLE, set(_ledger()), 4, "potential and featurize kernels")


def test_ledger():
    """instance -> case ids (shown by `pytest -s -k test_ledger`)."""
    led = _ledger()
    print_ledger(DC.INSTANCES, led, DC.UNREACHABLE)
    assert len(led) + len(DC.UNREACHABLE) == len(DC.INSTANCES) == 4


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_instance_it_names(case):
    """... with the grid and the dynamic LDS bytes include/oc_amd.h documents."""
    text = DC.plan_of_case(case)
    table = DC.table_of(case.table)
    if case.kind == "potential":
        assert text == "%s grid=%d" % (case.expect, -(-case.n_envs // 256)), (case.id, text)
    else:
        lds = 128 * (16 * table.n_planes + 4 * (2 * (case.num_pots * 10 + 26) + 6))
        assert text == "%s grid=%d, %d B LDS" % (case.expect, -(-case.n_envs // 128), lds), (case.id, text)


def test_the_cases_cover_what_the_list_promises():
    by = {c.id: c for c in DC.CASES}
    plans = {c.id: DC.plan_of_case(c) for c in DC.CASES}
    assert DC.N_ENVS == 9 * 256 + 3 == 18 * 128 + 3
    assert plans["featurize_eight_pots"].endswith(", 84992 B LDS") and plans["featurize_largest_lds"].endswith(", 89088 B LDS")
    assert {by["featurize_%s" % n].n_envs for n in ("1_env", "127_envs", "129_envs")} == {1, 127, 129}
    # the tables: what each is there for
    t = {name: DC.table_of(name) for name in {c.table for c in DC.CASES}}
    pots = lambda name: [len(s.cells_of("P")) for s in t[name].specs]  # noqa: E731
    assert pots("three_pots") == [3] and pots("seven_pots") == [7] and pots("eight_pots_serve_ring") == [8]
    assert sorted(set(pots("seven_and_scenario2_s"))) == [1, 2, 7] and sorted(set(pots("mix5"))) == [1, 2]
    assert len(t["canonical_5_x8"]) == 40 and len(t["mix5"]) == 5
    eight = t["eight_pots_serve_ring"].specs[0]
    assert (eight.width, eight.height, t["eight_pots_serve_ring"].n_planes) == (10, 9, 7) and len(eight.cells_of("S")) == 21
    assert bool(eight.cells_of("T")) and eight.recipe_config == dict(onion_time=3, tomato_time=5, onion_value=7, tomato_value=4)
    assert len(t["you_shall_not_pass"].specs[0].cells_of("S")) == 16 and t["corridor"].n_cells == 126 and t["corridor"].n_planes == 9
    assert t["asymmetric_advantages"].width == 9
    one = t["one_player_two_pots"].specs[0]
    assert one.num_players == 1 and pots("one_player_two_pots") == [2]
    from overcooked_ai_amd.potential import phi_record, potential_params

    assert [potential_params(t["mdp_test_tomato"].specs[0], 0.99)[k] for k in ("max_delivery_steps", "max_pickup_steps", "pot_onion_steps",
                                                                              "pot_tomato_steps")] == [4, 4, 5, 6]
    assert phi_record(eight, 0.99)[456] == 255 and phi_record(t["you_shall_not_pass"].specs[0], 0.99)[456] == 255  # (the terrain scan)
    assert phi_record(t["three_pots"].specs[0], 0.99)[456] == 1
    # the same states under both potential kernels
    a, b = by["potential2_two_pots"], by["potential_hints_withheld"]
    assert a.expect == "k_potential2" and b.expect == "k_potential" and not b.hints and DC.states_of(a) is DC.states_of(b)
    # every situation has a case per kernel that can meet it
    pot2 = set().union(*(c.situations for c in DC.CASES if c.expect == "k_potential2"))
    pot = set().union(*(c.situations for c in DC.CASES if c.expect == "k_potential"))
    common = set(DC._ANY + DC._TWO_PLAYERS + DC._TWO_POTS + DC._TWO_OF_EACH) | set(DC._BITS) | {"mixed_completion"}
    assert pot2 == common | {"dish_unreachable", "soup_unservable"}  # (no layout of more than two pots here has unreachable cells)
    assert pot == common | {"three_or_four_partial", "set_resize", "set_resize_all_eight"}
    feat = {v: set().union(*(c.situations for c in DC.CASES if c.expect == "k_featurize<LAY_LDS=%s>" % v)) for v in ("true", "false")}
    counters = set(DC._COUNTERS) | {"counter_unreachable"}
    assert feat["false"] == set(DC._HELD) | set(DC._pots(2)) | {"pot1_absent", "pot2_absent"} | counters | {"counter_soup_tomato"}
    assert feat["true"] == set(DC._HELD) | set(DC._pots(4)) | {"pot%d_absent" % r for r in (1, 2, 3, 4)} | counters | {"counter_soup_tomato"}
    assert {c.counter_goals for c in DC.CASES if c.kind == "featurize"} == {"none", "all", "half"}
    assert {c.num_pots for c in DC.CASES if c.kind == "featurize"} == {0, 2, 3, 4}
    half = DC.counter_goals_of(by["featurize_counter_list"])
    for s in t["mix5"].specs:  # about half of each layout's counters
        assert 0.3 <= len(set(half) & set(s.cells_of("X"))) / len(s.cells_of("X")) <= 0.7


def _plan(b, num_pots=None):
    from overcooked_ai_amd import _lib

    L, out = _lib.load(), ctypes.create_string_buffer(320)
    br = ctypes.byref(b) if b is not None else None
    rc = L.oc_potential_plan(br, out, len(out)) if num_pots is None else L.oc_featurize_plan(br, num_pots, out, len(out))
    return rc, out.value.decode() if rc == 0 else L.oc_last_error().decode()


def test_the_selection_boundaries():
    from overcooked_ai_amd import _lib

    TWO = _lib.BATCH_TWO_PLAYERS
    for max_pots, want in ((0, "k_potential"), (1, "k_potential2"), (2, "k_potential2"), (3, "k_potential"), (8, "k_potential")):
        for flags in (TWO, 0):  # (phi is defined for one player; the flag changes nothing)
            for n_layouts in (1, 33):
                assert _plan(batch(9, 5, 2307, n_layouts, max_pots, flags)) == (0, want + " grid=10"), (max_pots, flags, n_layouts)
    for n_envs, grid in ((1, 1), (256, 1), (257, 2), (65536, 256)):
        assert _plan(batch(5, 4, n_envs)) == (0, "k_potential2 grid=%d" % grid)
    for n_layouts, want in ((1, "true"), (32, "true"), (33, "false"), (65536, "false")):
        for max_pots in (0, 1, 3):  # (the pot hint changes nothing)
            assert _plan(batch(9, 5, 2307, n_layouts, max_pots), 4) == (0, "k_featurize<LAY_LDS=%s> grid=19, 78848 B LDS" % want)  # (the header's example)
    # the documented formula over num_pots and the state planes
    for (w, h), num_pots in (((5, 4), 0), ((5, 4), 4), ((14, 9), 4), ((16, 8), 1)):
        planes = 1 + -(-w * h // 16)
        lds = 128 * 16 * planes + 128 * 2 * (2 * (num_pots * 10 + 26) + 4 + 2) * 2
        assert _plan(batch(w, h, 129), num_pots) == (0, "k_featurize<LAY_LDS=true> grid=2, %d B LDS" % lds)
    assert _plan(batch(14, 9, 2307), 4)[1].endswith(", 89088 B LDS")  # the largest request
    for num_pots in (-1, 5):
        assert _plan(batch(5, 4, 300), num_pots) == (-1, "oc_featurize: num_pots must be in 0..4")
    assert _plan(batch(5, 4, 300, flags=0), 2) == (-1, "oc_featurize: needs 2-player layouts")
    one = DC.table_of("one_player_two_pots")
    from overcooked_ai_amd import dispatch

    assert _plan(dispatch.batch_for(one, 300), 2) == (-1, "oc_featurize: needs 2-player layouts")
    assert _plan(dispatch.batch_for(one, 300)) == (0, "k_potential2 grid=2")
    for num_pots in (None, 2):
        assert _plan(batch(5, 4, 0), num_pots) == (0, "nothing to launch (no envs)")
        assert _plan(None, num_pots) == (-1, "batch is NULL")
        assert _plan(batch(40, 40, 8), num_pots) == (-1, "grid shape out of range (3x3 .. 128 cells)")
        assert _plan(batch(5, 4, -1), num_pots) == (-1, "batch.n_envs < 0")
        b = batch(5, 4, 8, n_layouts=2)
        b.d_layout_id = None
        assert _plan(b, num_pots) == (-1, "d_layout_id required when n_layouts > 1")


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.situations], ids=lambda c: c.id)
def test_the_states_of_a_case_hold_what_it_lists(case):
    """From the states and the host planner alone: every listed situation in at least FLOOR envs, and in every whole GROUP."""
    cen = DC.census(case)
    short = {s: cen.get(s, (0, 0)) for s in case.situations if cen.get(s, (0, 0))[0] < DC.FLOOR or cen.get(s, (0, 0))[1] < 1}
    assert not short, "%s: (envs, fewest per whole workgroup) %s" % (case.id, short)
    assert DC.FLOOR == 64 and DC.GROUP == 256 and case.n_envs == DC.N_ENVS


def test_the_states_are_valid_and_shared():
    """Players on distinct floor cells, objects only on counters and pots, ticks within the cook time; computed once, read-only."""
    for case in DC.CASES:
        st, table, lid = DC.states_of(case), DC.table_of(case.table), DC.layout_ids(case)
        assert st.shape == (table.n_planes, case.n_envs, 16) and not st.flags.writeable and DC.states_of(case) is st
        for l, spec in enumerate(table.specs):
            sub = st if lid is None else st[:, lid == l]
            W = spec.width
            terrain = np.array([ord(ch) for row in spec.terrain_mtx for ch in row])
            floor = terrain == ord(" ")
            assert floor[sub[0, :, 0]].all()
            if spec.num_players == 2:
                assert floor[sub[0, :, 3]].all() and (sub[0, :, 0] != sub[0, :, 3]).all()
            else:
                assert (sub[0, :, 3] == 0xFF).all()
            objs = np.moveaxis(sub[1:], 1, 0).reshape(sub.shape[1], -1)[:, :len(terrain)]
            assert not objs[:, ~np.isin(terrain, [ord("X"), ord("P")])].any()
            for k, (x, y) in enumerate(spec.cells_of("P")):
                o, tk = objs[:, y * W + x].astype(int), sub[0, :, 8 + k].astype(int)
                assert ((o == 0) | (o >= 0x88)).all() and (tk[o == 0] == 0).all()
                for code in np.unique(o[o != 0]):
                    n, n_t = (code >> 3) & 3, bin(code & 7).count("1")
                    assert 1 <= n <= 3 and n_t <= n and (code & 7) < (1 << n)
                    assert (tk[o == code] <= spec.recipe_time((n - n_t, n_t)) + 1).all()


def test_set_orders_of_the_new_layouts_match_the_interpreter():
    """Every (pots with one item, pots with two items) pair of insertion lists the cases' states produce on the new layouts — what
    get_partially_full_pots hands to `set().union` (mdp.py:1882-1890) —: the oracle's py_set_order and potential.py's give
    `list(set().union(...))` of the running interpreter; all 8-pot subsets that resize the set are among them."""
    from oracle import oracle as O
    from overcooked_ai_amd.potential import py_set_order

    if not (3, 8) <= sys.version_info[:2] <= (3, 12):
        pytest.skip("set/tuple-hash internals restated for CPython 3.8-3.12")
    seen = {}
    for case in DC.CASES:
        if case.kind != "potential" or case.table not in NEW_TABLES:
            continue
        table, st = DC.table_of(case.table), DC.states_of(case)
        ctx = DC._ctx(table.specs[0], "none")
        for e in range(case.n_envs):
            pots = DC._pot_view(ctx, st, e)
            lists = tuple(tuple(ctx.pots[k] for k, p in enumerate(pots) if p[0] == items) for items in (1, 2))
            if len(lists[0]) + len(lists[1]) >= 2:
                seen.setdefault(case.table, set()).add(lists)
    assert set(seen) == set(NEW_TABLES)
    assert any(len(a) + len(b) == 8 for a, b in seen["eight_pots_serve_ring"]) and len(seen["eight_pots_serve_ring"]) > 300
    assert sum(len(a) + len(b) >= 5 for a, b in seen["eight_pots_serve_ring"]) > 150
    assert {len(a) + len(b) for a, b in seen["three_pots"]} == {2, 3}
    for name, pairs in seen.items():
        W = DC.table_of(name).width
        for a, b in pairs:
            xy = lambda cells: [(c % W, c // W) for c in cells]  # noqa: E731
            want = list(set().union(xy(a), xy(b)))
            assert xy(O.py_set_order(W, list(a + b))) == want, (name, a, b)
            assert py_set_order(xy(a + b)) == want, (name, a, b)
