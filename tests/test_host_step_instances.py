"""tests/step_cases.py kept honest without a GPU: every case is planned (oc_step_plan) onto the kernel instance it names, the cases
cover the 29 kernel instances csrc/step_dispatch.hpp lists for oc_step, oc_step_many and oc_step_server_*, the coverage the list
promises holds, the planner's rules and refusals hold over a sweep of synthetic batches, and on the oracle alone each case contains
what it is there for — restarts at different steps within a wavefront, flagged illegal actions, every event type its table can
produce, every kind of pot, re-drawn layouts.  A change to choose_step (csrc/step_dispatch.hpp) that moves a case to another kernel fails
here, by the case's name, instead of silently changing what a GPU test runs."""
import ctypes
import itertools
import os
import re

import pytest

import step_cases as SC
from case_support import CSRC, check_census, event_bits, function_body as _function, ledger, pot_kinds, print_ledger, synthetic_batch as batch

AUTO_RESET = 1  # OC_OPT_AUTO_RESET


def _ledger():
    """instance (oc_step_plan's words) -> ids of the cases that are there for it"""
    return ledger(SC.CASES, SC.instance_of)


def _instantiated():
    """The kernel instances launch_step_as (csrc/step_dispatch.hpp) and sv_launch (csrc/step_server_host.hpp) launch, in
    oc_step_plan's words: the StepRow lines of the four row lists of step_dispatch.hpp, each walked (launch_row) with the one lambda
    that names its kernel with the row's template arguments; k_step1 / k_step3 / k_step once without and once with EVENTS (launch_step_from picks
    the template)."""
    with open(os.path.join(CSRC, "step_dispatch.hpp")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "step_server_host.hpp")) as f:
        sv = _function(f.read(), "sv_launch")
    tf = {"true": True, "false": False}

    def rows(name, n_args):
        """the (UNIFORM, MAXP, LAY_LDS[, FAST]) of every row of `using <name> = StepRows<...>;`, one row per line"""
        text = re.search(r"^using %s = StepRows<[^\n]*\n(.*?>>);\n" % name, src, re.S | re.M).group(1)
        found = re.findall(r"^\s+StepRow<(true|false), (\d), (true|false)(?:, (true|false))?>[,>]$", text, re.M)
        assert len(found) == len(text.splitlines()) and all((f != "") == (n_args == 4) for *_, f in found), text  # nothing but rows
        return [(tf[u], int(mp), tf[ll]) + ((tf[f],) if n_args == 4 else ()) for u, mp, ll, f in found]

    # each kernel is named once, with the row's template arguments, in the lambda that the walk of its row list is given; the
    # lambdas of launch_step_as launch through its `launch`, sv_launch's launches itself
    body = _function(src, "launch_step_as")
    assert body.count("hipLaunchKernelGGL(kernel, ") == 1 and sv.count("hipLaunchKernelGGL(kernel, ") == 1
    for kernel, args, walk, where in (("k_step1", "row.UNIFORM, row.MAXP, row.LAY_LDS, EVENTS", "Step1Rows", body),
                                      ("k_step3", "row.UNIFORM, row.MAXP, row.LAY_LDS, row.FAST, EVENTS", "Step3Rows", body),
                                      ("k_step", "row.UNIFORM, row.MAXP, row.LAY_LDS, EVENTS", "PredicateRows", body),
                                      ("k_step_server", "row.UNIFORM, row.MAXP, row.LAY_LDS", "ServerRows", sv)):
        assert re.findall(r"\b%s<[^>]*>" % kernel, where) == ["%s<%s>" % (kernel, args)], kernel
        assert where.count("launch_row(%s(), ch, " % walk) == 1, kernel
        if where is sv:
            assert re.search(r"launch_row\(ServerRows\(\), ch, \[&\]\(auto row\) \{\n[^}]*\bk_step_server<[^}]*hipLaunchKernelGGL\(kernel, ", sv), kernel
        else:
            (name, _), = [(n, text) for n, text in re.findall(r"const auto (\w+) = \[&\]\(auto row\) \{\n(.*?)\n    \};", body, re.S)
                          if kernel + "<" in text and re.search(r"\blaunch\(", text)]
            assert "launch_row(%s(), ch, %s)" % (walk, name) in body, kernel
    go = _function(src, "launch_step_from")
    assert "ch.events ? launch_step_as<true> : launch_step_as<false>" in go
    found = []
    for ev in (False, True):
        found += [SC.step1(*row, ev) for row in rows("Step1Rows", 3)]
        found += [SC.step3(*row, ev) for row in rows("Step3Rows", 4)]
        found += [SC.pred(*row, ev) for row in rows("PredicateRows", 3)]
    found += [SC.server(*row) for row in rows("ServerRows", 3)]
    return found


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_instance_it_names(case):
    text = SC.plan_of_case(case)
    assert text.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, text, case.expect)
    assert SC.instance_of(case) in SC.INSTANCES, case.id
    assert ("EVENTS=true" in case.expect) == (case.events != "none") or case.entry == "server", case.id
    assert " grid=%d, " % -(-case.n_envs // 256) in text and text.endswith(" B LDS"), text


def test_every_step_instance_of_the_sources_has_a_case_or_a_named_exclusion():
    check_census(_instantiated(), SC.INSTANCES, SC.UNREACHABLE, set(_ledger()), 29, "caller-actions kernels")
    assert {c.entry for c in SC.CASES} == set(SC.ENTRIES)


def test_ledger():
    """instance -> case ids, one line per instance (shown by `pytest -s -k test_ledger`)."""
    led = _ledger()
    print_ledger(SC.INSTANCES, led, SC.UNREACHABLE)
    assert len(led) + len(SC.UNREACHABLE) == len(SC.INSTANCES) == 29


def _where(**kw):
    return [c for c in SC.CASES if all(getattr(c, k) == v for k, v in kw.items())]


def test_the_cases_cover_what_the_list_promises():
    led = _ledger()
    inst = {c.id: SC.instance_of(c) for c in SC.CASES}

    def on(table, instance, **kw):
        return [c for c in _where(table=table, **kw) if inst[c.id] == instance]

    # one case per instance, on the tables the rows are named for, each k_step1 / k_step3 / k_step row with and without events
    rows1 = dict(zip(("cramped_room", "asymmetric_advantages", "seven_pots", "mix5", "canonical_5_x8", "seven_and_scenario2_s"), SC.STEP1_ROWS))
    for table, row in rows1.items():
        for ev in (False, True):
            assert on(table, SC.step1(*row, EVENTS=ev), entry="step"), (table, ev)
    many = dict(zip(("cramped_room", "asymmetric_advantages", "mix5", "seven_pots"), SC.STEP3_ROWS))
    for table, row in many.items():
        for ev in (False, True):
            assert led.get(SC.step3(*row, EVENTS=ev)), (row, ev)
        assert on(table, SC.step3(*row), entry="step_many"), table
    assert [c for c in _where(table="canonical_5_x8", entry="step_many") if inst[c.id].startswith(SC.step3(False, 8, False, False)[:50])]
    general = SC.step3(False, 2, True, False)
    assert on("big_4", general, entry="step") and on("corridor", general, entry="step")
    assert on("small_corridor", SC.step3(False, 2, True, False, True), entry="step", events="both")  # (one layout, 65 cells, events)
    for table, row in zip(("asymmetric_advantages", "seven_pots", "mix5"), SC.PRED_ROWS):
        for ev in (False, True):
            assert [c for c in on(table, SC.pred(*row, EVENTS=ev), predicate=True) if c.entry != "step_many"], (table, ev)
    assert [c for c in _where(entry="step_many", predicate=True) if c.expect.startswith("step by step: oc_step + k_step<")]
    for table, row in zip(("cramped_room", "mix5", "seven_pots"), SC.SERVER_ROWS):
        assert on(table, SC.server(*row), entry="server", hints=True), table
    # k_step1 out of place: with drawn restarts, with events, on the 64-cell grid
    oop = [c for c in _where(entry="step_out_of_place") if inst[c.id].startswith("k_step1<")]
    assert len(oop) >= 3 and any(c.start == "drawn" for c in oop) and any(c.events == "both" for c in oop)
    assert any(c.table == "eight_by_eight" for c in oop)
    # k_step1's grid edges, in place
    assert SC.table_of("four_by_four").n_planes == 2 and SC.table_of("eight_by_eight").n_planes == 5
    for table in ("four_by_four", "eight_by_eight"):
        assert [c for c in _where(table=table, entry="step") if inst[c.id].startswith("k_step1<")], table
    # k_step3's action queue: its fill edges on a FAST and on a general instance
    for row in (SC.STEP3_ROWS[0], SC.STEP3_ROWS[2]):
        assert {c.n_steps for c in _where(entry="step_many") if inst[c.id] == SC.step3(*row)} >= {7, 8, 9, 17}, row
    # layout re-draws on both tables through both entry points
    for table in ("mix5", "seven_and_scenario2_s"):
        assert {c.entry for c in _where(table=table, start="regen")} >= {"step", "step_many"}, table
    # one player
    assert SC.table_of("cramped_room_single").specs[0].num_players == 1
    assert on("cramped_room_single", SC.step1(True, 1, True), entry="step")
    assert [c for c in _where(table="cramped_room_single", entry="step_many") if "UNIFORM=false" in c.expect]
    # withheld hints: the MAXP=8 / non-FAST instances on a table that earns MAXP=1 and FAST
    held = {c.entry: c for c in _where(table="cramped_room", hints=False)}
    assert set(held) == {"step", "step_many", "server"}
    assert all("MAXP=8" in c.expect and "FAST=true" not in c.expect for c in held.values())
    # event sinks of either half alone, for k_step1 and for k_step3; no episode returns once per table-driven kernel
    for kernel in ("k_step1<", "k_step3<"):
        assert {c.events for c in SC.CASES if inst[c.id].startswith(kernel)} >= {"none", "masks", "counts", "both"}, kernel
    for kernel in ("k_step1<", "k_step3<", "k_step_server<"):
        assert [c for c in _where(returns=False) if inst[c.id].startswith(kernel)], kernel
    # the server: 10 steps in one play, a sync, 11 single steps; one case with drawn starts
    servers = _where(entry="server")
    assert all(c.n_steps == 21 and SC.SERVER_SPLIT == 10 and c.events == "none" for c in servers) and any(c.start == "drawn" for c in servers)
    # the shapes: ten workgroups (no multiple of 8), a last wavefront of 3 envs; runs in which roughly every env restarts
    assert SC.N_ENVS == 9 * 256 + 3 and all(c.n_envs % 64 == 3 and c.n_envs <= 4096 for c in SC.CASES)
    assert all(c.n_steps >= c.horizon or c.n_steps in (7, 8, 9) for c in SC.CASES)


def _plan(b, entry, n_steps=1, options=AUTO_RESET, masks=0, counts=0, start=None, horizon=400):
    from overcooked_ai_amd import _lib

    out = ctypes.create_string_buffer(320)
    rc = _lib.load().oc_step_plan(ctypes.byref(b), entry, horizon, options, n_steps, masks, counts,
                                  ctypes.byref(start) if start is not None else None, out, len(out))
    return rc, out.value.decode() if rc == 0 else _lib.load().oc_last_error().decode()


def test_the_planners_rules_hold_over_a_sweep_of_batches():
    """choose_step's rules, restated: UNIFORM = one layout; LAY_LDS = at most 32 layouts; small = 1 or 2 pots; FAST = two players
    everywhere and at most 64 cells.  k_step1 (one step, at most 64 cells): (T,1,T) / (T,2,T) / (T,8,T) for one layout by pots, else
    (F,2,T) small in LDS, (F,2,F) small, (F,8,F).  k_step3: (T,1,T,T) / (T,2,T,T) for one FAST layout, (F,2,T,F) small in LDS, else
    (F,8,F,F).  k_step: (T,2,T) / (T,8,T) for one layout, else (F,8,F).  k_step_server: (T,2,T) one small layout, (F,2,T) small in
    LDS, else (F,8,F)."""
    from overcooked_ai_amd import _lib

    seen = set()
    shapes = ((8, 8), (9, 7), (13, 5), (5, 4), (4, 4))  # 64, 63, 65, 20, 16 cells
    for (w, h), pots, layouts, two, n_steps, ev, predicate in itertools.product(shapes, (0, 1, 2, 3), (1, 2, 32, 33), (True, False), (1, 2),
                                                                                (False, True), (False, True)):
        b = batch(w, h, 2307, max_pots=pots, flags=_lib.BATCH_TWO_PLAYERS if two else 0, n_layouts=layouts)
        n_obj = -(-w * h // 16)
        uniform, lds, small, fast = layouts == 1, layouts <= 32, pots in (1, 2), two and w * h <= 64
        options = AUTO_RESET | (_lib.OPT_PREDICATE_INTERACT if predicate else 0)
        for entry in (0, 1):
            rc, text = _plan(b, entry, n_steps, options, masks=int(ev))
            K = n_steps if entry == 1 else 1
            if predicate and entry == 1 and ev:
                assert rc != 0 and text.startswith("oc_step_many: "), text
                continue
            assert rc == 0, text
            lds_bytes = n_obj * 8192
            if predicate:
                want = SC.pred(True, 2 if small else 8, True, ev) if uniform else SC.pred(False, 8, False, ev)
                want = ("step by step: oc_step + " if entry == 1 else "") + want
            elif K == 1 and w * h <= 64:
                lds_bytes = n_obj * 4096
                if uniform:
                    want = SC.step1(True, 1 if pots == 1 else 2 if small else 8, True, ev)
                else:
                    want = SC.step1(False, 2, True, ev) if lds and small else SC.step1(False, 2, False, ev) if small else SC.step1(False, 8, False, ev)
            elif uniform and fast and small:
                want = SC.step3(True, pots, True, True, ev)
            else:
                want = SC.step3(False, 2, True, False, ev) if lds and small else SC.step3(False, 8, False, False, ev)
            assert text == "%s grid=10, %d B LDS" % (want, lds_bytes), ((w, h), pots, layouts, two, n_steps, ev, predicate, entry, text)
            seen.add(want.split(" + ")[-1])
        rc, text = _plan(b, 2, n_steps, AUTO_RESET, masks=int(ev))
        want = SC.server(True, 2, True) if uniform and small else SC.server(False, 2, True) if lds and small else SC.server(False, 8, False)
        assert rc == 0 and text == "%s grid=10, %d B LDS" % (want, n_obj * 8192), text
        seen.add(want)
    assert seen == set(SC.INSTANCES), sorted(set(SC.INSTANCES) - seen)  # (the sweep itself reaches every instance)
    b = batch(5, 4, 0, max_pots=1)
    assert _plan(b, 0) == (0, "nothing to launch (no envs)") and _plan(b, 1, 4) == (0, "nothing to launch (no envs)")
    assert _plan(batch(5, 4, 7, max_pots=1), 1, 0) == (0, "nothing to launch (no steps)")


def test_the_planners_refusals_carry_the_entry_points_name():
    from overcooked_ai_amd import _lib

    P = _lib.OPT_PREDICATE_INTERACT
    b = batch(5, 4, 300, max_pots=1)
    sp = _lib.OcStartSpec(1, 0, 1, 1, 0.35, 0, 0)
    rc, msg = _plan(b, 0, options=AUTO_RESET | P, start=sp)
    assert rc != 0 and msg.startswith("oc_step: drawn start states need the table-driven kernel"), msg
    rc, msg = _plan(b, 0, options=AUTO_RESET | P, counts=1)
    assert rc != 0 and msg.startswith("oc_step: event counters need the table-driven kernel"), msg
    assert _plan(b, 0, options=AUTO_RESET | P, masks=1)[0] == 0  # (per-step masks: k_step writes them)
    for kw in (dict(start=sp), dict(counts=1), dict(masks=1)):
        rc, msg = _plan(b, 1, 4, options=AUTO_RESET | P, **kw)
        assert rc != 0 and msg.startswith("oc_step_many: drawn start states / event logging need the table-driven kernel"), msg
    rc, msg = _plan(b, 1, -1)
    assert rc != 0 and msg == "oc_step_many: n_steps < 0", msg
    rc, msg = _plan(b, 2, options=AUTO_RESET | P)
    assert rc != 0 and msg == "oc_step_server_open: the only option is OC_OPT_AUTO_RESET", msg
    rc, msg = _plan(batch(5, 4, 0, max_pots=1), 2)
    assert rc != 0 and msg == "oc_step_server_open: no envs", msg
    for entry, who in enumerate(("oc_step", "oc_step_many", "oc_step_server_open")):
        rc, msg = _plan(b, entry, 3, horizon=0)
        assert rc != 0 and msg == who + ": horizon must be in 1..65535", msg
        rc, msg = _plan(b, entry, 3, start=_lib.OcStartSpec(1, 0, 1, 1, 1.5, 0, 0))
        assert rc != 0 and msg.startswith(who + ": start.rnd_obj_prob_thresh"), msg
    rc, msg = _plan(b, 3)
    assert rc != 0 and msg.startswith("oc_step_plan: entry must be"), msg


def _event_names(masks):
    from overcooked_ai_amd.mdp import EVENT_TYPES

    seen = event_bits(masks).any(axis=(0, 2))
    return {EVENT_TYPES[i] for i in range(25) if seen[i]}


def _pot_kinds(case, state):
    return pot_kinds(SC.table_of(case.table), SC.layout_ids(case), state)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_the_reference_run_of_a_case_is_not_vacuous(case):
    """On the oracle alone.  The states the run starts from hold idle, cooking and ready pots and held soups; at least n_envs / 8
    restarts fall inside the run, and at some step some but not all envs of one 64-env wavefront restart; exactly the planted
    illegal actions are flagged; with an event sink every event type the table can produce occurs, and no other; re-draws move at
    least n_envs / 8 envs to another layout; on the 64-cell grid an object lies in the fourth object plane at the start and on a step
    where its env is stepped (out of place where the case is)."""
    table = SC.table_of(case.table)
    run = SC.OracleRun(case)
    assert all(v > 0 for v in _pot_kinds(case, run.state)), (case.id, _pot_kinds(case, run.state))
    if table.n_planes == 5:
        assert run.state[4].any(), case.id
    restarts = flagged = moved = 0
    partial = fourth = False
    events = set()
    for k in range(case.n_steps):
        before = None if run.layout_id is None else run.layout_id.copy()
        _, fl, masks = run.step(k)
        restarted = (fl & 4) != 0
        restarts += int(restarted.sum())
        flagged += int(((fl & 2) != 0).sum())
        assert not (restarted & ((fl & 2) != 0)).any()
        partial = partial or any(restarted[a:a + 64].any() and not restarted[a:a + 64].all() for a in range(0, case.n_envs, 64))
        events |= _event_names(masks)
        if before is not None:
            moved += int((before != run.layout_id).sum())
            assert case.start == "regen" or moved == 0
        if table.n_planes == 5:  # an env whose fourth object plane is occupied takes a legal step and keeps the plane occupied
            legal = (fl & 2) == 0
            fourth = fourth or bool((run.prev_state[4].any(axis=1) & run.state[4].any(axis=1) & legal & ~restarted).any())
    assert restarts >= case.n_envs / 8 and partial, (case.id, restarts, partial)
    assert flagged == SC.n_illegal(case), (case.id, flagged)
    if case.events != "none":
        possible = SC.possible_events(table)
        assert events == possible, (case.id, "missing", sorted(possible - events), "not expected", sorted(events - possible))
    if case.start == "regen":
        assert moved >= case.n_envs / 8, (case.id, moved)
    if table.n_planes == 5:
        assert fourth, case.id


def test_the_hand_written_tables():
    four, eight = SC.table_of("four_by_four"), SC.table_of("eight_by_eight")
    assert (four.width, four.height, four.max_pots, four.n_planes) == (4, 4, 1, 2)
    assert (eight.width, eight.height, eight.max_pots, eight.n_planes) == (8, 8, 2, 5)
    assert four.specs[0].num_players == 2 and eight.specs[0].num_players == 2
    with open(os.path.join(CSRC, "step_one.hpp")) as f:
        assert "constexpr int STEP1_MAX_PLANES = 4;" in f.read()
    # no registry layout has 16 or 64 cells
    from overcooked_ai_amd.layouts import layout_names, spec_from_name

    assert all(spec_from_name(nm).width * spec_from_name(nm).height not in (16, 64) for nm in layout_names())
