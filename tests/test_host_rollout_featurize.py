"""oc_rollout_featurize without a GPU: plan_rollout_featurize (csrc/observation_plan.hpp) through oc_rollout_featurize_plan — the
conditions of the single kernel one at a time, every refusal before any device call, the empty calls, the instances the planner can
name against the ones csrc/observation_dispatch.hpp instantiates — and tests/featurize_rollout_cases.py kept honest: every case is planned onto
the path it names, and on the oracle alone its run contains what it claims."""
import ctypes
import os
import re

import pytest

import featurize_rollout_cases as FC
from case_support import CSRC, P, check_census, function_body, ledger, synthetic_batch as batch
from overcooked_ai_amd import _lib

AUTO, ONE = _lib.OPT_AUTO_RESET, _lib.OPT_ONE_KERNEL
FILL = 256 * 64  # the fill rule on a host without a GPU: (1 024 SIMDs / 4) * 64 envs
STEPS = "step by step: oc_rollout_random + k_featurize<LAY_LDS=true>"


def plan(b, num_pots=2, n_steps=12, options=AUTO, actions=0, outputs=1, start=None, horizon=400):
    """oc_rollout_featurize_plan of a batch -> (rc, text or the refusal's message)"""
    L = _lib.load()
    out = ctypes.create_string_buffer(320)
    rc = L.oc_rollout_featurize_plan(ctypes.byref(b) if b is not None else None, num_pots, horizon, options, n_steps, actions, outputs,
                                     ctypes.byref(start) if start is not None else None, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def test_the_single_kernel_conditions_one_at_a_time():
    """One layout, two players, one or two pots by the table's hint, at most 64 cells, and OC_OPT_ONE_KERNEL or a batch that fills
    the GPU with at least two steps: each condition alone sends the call step by step."""
    rc, text = plan(batch(5, 4, 200), options=AUTO | ONE)
    assert rc == 0 and text == FC.ONE_KERNEL + " G=32, grid=1, 70656 B LDS", text  # 2 * 8192 + 4096 + 4 * (32 * 2 * 98 * 2)
    for pots in (1, 2):
        assert plan(batch(8, 8, 200, max_pots=pots), options=AUTO | ONE)[1].startswith(FC.ONE_KERNEL)
    # the largest: four images of 32 envs of 136-float rows beside four object planes, 32768 + 4096 + 4 * 17664 = 107520 bytes;
    # an image holds 32 envs whatever the batch
    rc, text = plan(batch(8, 8, 321, max_pots=2), num_pots=4, options=AUTO | ONE)
    assert rc == 0 and text == FC.ONE_KERNEL + " G=32, grid=2, 107520 B LDS", text
    assert plan(batch(8, 8, 65537, max_pots=2), num_pots=4)[1] == FC.ONE_KERNEL + " G=32, grid=257, 107520 B LDS"
    assert plan(batch(9, 5, 131072, max_pots=2))[1] == FC.ONE_KERNEL + " G=32, grid=512, 78848 B LDS"
    assert plan(batch(5, 4, 65537))[1] == FC.ONE_KERNEL + " G=32, grid=257, 70656 B LDS"
    for what, b in (("two layouts", batch(5, 4, 200, n_layouts=2)), ("three pots", batch(5, 4, 200, max_pots=3)),
                    ("no hint of the pots", batch(5, 4, 200, max_pots=0)), ("65 cells", batch(13, 5, 200))):
        rc, text = plan(b, options=AUTO | ONE)
        assert rc == 0 and text.startswith(STEPS), (what, text)
    # a one-player table is refused, as oc_featurize refuses it
    rc, text = plan(batch(5, 4, 200, flags=_lib.BATCH_NEW_DYNAMICS), options=AUTO | ONE)
    assert rc == -1 and text == "oc_rollout_featurize: needs 2-player layouts"
    # without OC_OPT_ONE_KERNEL: the fill rule and at least two steps
    assert plan(batch(5, 4, FILL), n_steps=2)[1].startswith(FC.ONE_KERNEL + " G=32, grid=64,")
    assert plan(batch(5, 4, FILL), n_steps=1)[1].startswith(STEPS)
    assert plan(batch(5, 4, FILL), n_steps=1, options=AUTO | ONE)[1].startswith(FC.ONE_KERNEL)
    assert plan(batch(5, 4, FILL - 1), n_steps=12)[1].startswith(STEPS)
    # caller actions: oc_step is the one-step entry point; a table of more than 32 layouts is read through L2
    assert plan(batch(5, 4, 200), actions=1)[1].startswith("step by step: oc_step + k_featurize<LAY_LDS=true> grid=2, ")
    assert plan(batch(5, 4, 200, n_layouts=40), actions=1)[1].startswith("step by step: oc_step + k_featurize<LAY_LDS=false> grid=2, ")
    assert plan(batch(5, 4, 200))[1] == STEPS + " grid=2, 56320 B LDS"  # 128 * (16 * 3 + 4 * 98), oc_featurize_plan's own words


def test_every_refusal_comes_with_a_message_and_before_any_device_call():
    """Stand-in pointers everywhere and no GPU: a refusal that came after a device call could not be had here."""
    L = _lib.load()
    b = batch(5, 4, 200)
    other = _lib.OcStartSpec(3, 77, 1, 1, 0.35, 0, 0)  # (env_offset 77; the plan describes a call whose env_offset is the spec's)
    for what, kw, message in (
            ("num_pots", dict(num_pots=-1), "num_pots must be in 0..4"), ("num_pots", dict(num_pots=5), "num_pots must be in 0..4"),
            ("option bit", dict(options=AUTO | 0x8), "options other than OC_OPT_AUTO_RESET / OC_OPT_ONE_KERNEL"),
            ("option bit", dict(options=0x40), "options other than"),
            ("actions without outputs", dict(actions=1, outputs=0), "caller actions need the rewards and flags arrays"),
            ("horizon", dict(horizon=0), "horizon must be in 1..65535"), ("horizon", dict(horizon=65536), "horizon must be in 1..65535"),
            ("n_steps", dict(n_steps=-1), "n_steps must be in 0..2^30"),
            ("start spec", dict(start=_lib.OcStartSpec(3, 0, 1, 1, 1.5, 0, 0)), "start.rnd_obj_prob_thresh")):
        rc, text = plan(b, **kw)
        assert rc == -1 and text.startswith("oc_rollout_featurize: ") and message in text, (what, rc, text)
    # the entry point itself: the same checks, and the ones of its arrays
    br, sp = ctypes.byref(b), ctypes.byref(other)

    def call(blob=P, state=P, actions=None, rewards=None, flags=None, feats=P, stride=0, num_pots=2, horizon=400, options=AUTO,
             env_offset=0, n_steps=12, start=None):
        rc = L.oc_rollout_featurize(br, blob, P, state, actions, rewards, flags, None, feats, stride, num_pots, horizon, options, 3,
                                    env_offset, 5, n_steps, start, None)
        return rc, L.oc_last_error().decode()

    for what, kw, message in (
            ("start.env_offset", dict(start=sp, env_offset=78), "start.env_offset differs from env_offset"),
            ("no plan blob", dict(blob=None), "NULL plan / state / features pointer"), ("no state", dict(state=None), "NULL plan / state / features"),
            ("no features", dict(feats=None), "NULL plan / state / features"),
            ("features off 16 bytes", dict(feats=P + 4), "multiples of 16 bytes"), ("stride off 16 bytes", dict(stride=200 * 2 * 96 * 4 + 8), "multiples of 16 bytes"),
            ("negative stride", dict(stride=-16), "multiples of 16 bytes"),
            ("actions without rewards", dict(actions=P, flags=P), "caller actions need"), ("num_pots", dict(num_pots=7), "num_pots must be in 0..4"),
            ("option bit", dict(options=AUTO | 0x4), "options other than"), ("horizon", dict(horizon=70000), "horizon must be in 1..65535")):
        rc, text = call(**kw)
        assert rc == -1 and text.startswith("oc_rollout_featurize: ") and message in text, (what, rc, text)
    assert L.oc_rollout_featurize(None, P, P, P, None, None, None, None, P, 0, 2, 400, AUTO, 3, 0, 5, 12, None, None) == -1
    assert b"batch is NULL" in L.oc_last_error()
    wide = batch(40, 40, 4)
    assert plan(wide)[0] == -1 and "grid shape" in plan(wide)[1]
    text = ctypes.create_string_buffer(320)
    assert L.oc_rollout_featurize_plan(br, 2, 400, AUTO, 12, 0, 1, None, None, 0) == -1 and b"oc_rollout_featurize_plan: no output buffer" in L.oc_last_error()
    assert L.oc_rollout_featurize_plan(None, 2, 400, AUTO, 12, 0, 1, None, text, len(text)) == -1 and text.value == b""


def test_empty_calls_plan_and_launch_nothing():
    L = _lib.load()
    assert plan(batch(5, 4, 0)) == (0, "nothing to launch (no envs)")
    assert plan(batch(5, 4, 200), n_steps=0) == (0, "nothing to launch (no steps)")
    for b, k in ((batch(5, 4, 0), 12), (batch(5, 4, 200), 0)):  # (stand-in pointers: a launch would fault)
        assert L.oc_rollout_featurize(ctypes.byref(b), P, P, P, None, None, None, None, P, 0, 2, 400, AUTO | ONE, 3, 0, 5, k, None, None) == 0
    # refused before the empty-batch exit
    assert plan(batch(5, 4, 0), num_pots=9)[0] == -1 and plan(batch(5, 4, 0), horizon=0)[0] == -1


def _instantiated():
    """The instances launch_rollout_featurize (csrc/observation_dispatch.hpp) launches, in oc_rollout_featurize_plan's words."""
    with open(os.path.join(CSRC, "observation_dispatch.hpp")) as f:
        src = f.read()
    body = function_body(src, "launch_rollout_featurize")
    found = ["k_rollout_featurize<MAXP=%s, FAST=%s>" % mf for mf in re.findall(r"hipLaunchKernelGGL\(\(k_rollout_featurize<(\d), (\d)>\)", body)]
    everywhere = re.findall(r"hipLaunchKernelGGL\(\(k_rollout_featurize<", "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))
                                                                                 if f.endswith((".hip", ".hpp"))))
    assert len(everywhere) == len(found)  # no other launch site
    return found, body


def test_the_instances_the_planner_names_are_the_ones_the_sources_instantiate():
    found, body = _instantiated()
    led = ledger([c for c in FC.CASES if c.one_kernel] + [FC.LAUNCH_SIZE, FC.far_case()], lambda c: c.expect)
    check_census(found, FC.INSTANCES, {}, set(led), 1, "oc_rollout_featurize kernels")
    # every text the planner gives for a grid the kernel takes names that instance; the step-by-step path has no launch site of
    # k_featurize of its own: it calls the entry point
    for w, h in ((3, 3), (5, 4), (9, 5), (8, 8), (16, 4)):
        for pots in (1, 2):
            for num_pots in range(5):
                rc, text = plan(batch(w, h, 260, max_pots=pots), num_pots=num_pots, options=AUTO | ONE)
                assert rc == 0 and text[:text.index(">") + 1] in found, (w, h, text)
                lds = int(re.search(r", (\d+) B LDS$", text).group(1))
                assert " G=32, grid=2," in text, text
                big = plan(batch(w, h, 65537, max_pots=pots), num_pots=num_pots)[1]
                assert big == text.replace("grid=2,", "grid=257,"), big  # (the batch size changes the grid alone)
                assert lds + 4608 + 64 <= 160 * 1024, text  # (4 608 bytes of static LDS)
    # (rollout_featurize_step_by_step: the loop it shares with oc_rollout_encode, with oc_featurize as the observation of a step)
    src = open(os.path.join(CSRC, "observation_dispatch.hpp")).read()
    steps, loop = function_body(src, "rollout_featurize_step_by_step"), function_body(src, "rollout_step_by_step")
    assert "hipLaunchKernelGGL" not in steps and re.search(r"\boc_featurize\(", steps) and "return rollout_step_by_step(c, " in steps
    assert "hipLaunchKernelGGL" not in loop and "oc_step(" in loop and "oc_rollout_random(" in loop and "observe(k)" in loop


@pytest.mark.parametrize("case", FC.CASES + (FC.far_case(),), ids=lambda c: c.id)
def test_the_planner_gives_the_case_the_path_it_names(case):
    text = FC.plan_of_case(case)
    assert text.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, text, case.expect)
    table = FC.table_of(case.table)
    if not case.one_kernel and len(table) == 1 and 1 <= table.max_pots <= 2:  # its twin runs the same inputs through the kernel
        twin = next(c for c in FC.CASES + (FC.far_case(),) if c.id == case.id[:-len("/steps")])
        assert twin._replace(id=case.id, one_kernel=False, expect=case.expect) == case


def test_the_launch_size_case_is_the_smallest_batch_the_fill_rule_accepts():
    c = FC.LAUNCH_SIZE
    assert not c.one_kernel
    assert FC.plan_of_case(c, FILL).startswith(FC.ONE_KERNEL + " G=32, grid=64,") and FC.plan_of_case(c, FILL - 1).startswith(STEPS)


@pytest.mark.parametrize("case", [c for c in FC.CASES if c.one_kernel or c.table in ("mix5", "three_pots")] + [FC.far_case()], ids=lambda c: c.id)
def test_the_reference_run_of_a_case_is_not_vacuous(case):
    """On the oracle alone: for both players at least one (step, env) of every situation the case claims, at least n_envs restarts
    inside the launch, and every illegal action flagged."""
    import far_cases as F

    far = case.id.endswith("@far")
    traj = FC.oracle_trajectory(case, FC.far_epoch0(case) if far else 1)
    found = FC.check_claims(case, traj)
    assert case.n_steps < 12 or {"restarts", "held_soup"} <= set(case.claims), case.id
    flagged = int(((traj.flags & 2) != 0).sum())
    assert flagged == ((FC.N_BAD * case.n_steps + 1) if case.call == "actions" else 0), (case.id, flagged)
    assert int(traj.features.max()) < 255 and int(traj.features.min()) > -128  # small integers: exact in the int16 image and in float32
    if far:  # the counters wrap where the case says: inside the batch, inside the launch, between restarts
        assert case.seed >> 32 and case.seed & 0xFFFFFFFF and case.env_offset < 2**32 < case.env_offset + case.n_envs
        assert (case.t0 >> 3) < 2**32 <= ((case.t0 + case.n_steps - 1) >> 3) and case.t0 == F.FAR_T0_SHORT
        e0 = FC.far_epoch0(case)
        assert e0 < 2**32 < e0 + case.n_steps - 1
        restart_steps = [k for k in range(case.n_steps) if (traj.flags[k] & 4).any()]
        assert any(e0 + k < 2**32 for k in restart_steps) and any(e0 + k >= 2**32 for k in restart_steps)
    assert found["restarts"][0] >= (case.n_envs if case.n_steps >= 12 else 1), case.id


def test_the_cases_cover_what_the_paths_differ_in():
    one = [c for c in FC.CASES if c.one_kernel]
    assert {c.n_envs for c in one} == {200, 321} and {c.call for c in one} == set(FC.CALLS)
    assert {c.num_pots for c in one} >= {0, 2, 4} and {c.counter_goals for c in one} == {"none", "all"}
    assert {FC.table_of(c.table).n_planes - 1 for c in one} == {2, 3, 4} and {FC.table_of(c.table).max_pots for c in one} == {1, 2}
    assert any(FC.table_of(c.table).specs[0].old_dynamics for c in one)
    assert {(c.n_steps, c.t0) for c in one} >= {(1, 5), (3, 5), (12, 5)} and all(c.horizon == 8 for c in FC.CASES)
    eight = FC.table_of("featurize_eight_by_seven")
    assert 49 <= eight.n_cells <= 64 and eight.n_planes == 5 and eight.specs[0].num_players == 2
    steps_only = [c for c in FC.CASES if not c.one_kernel and c.id[:-len("/steps")] not in {o.id for o in one}]
    assert {(len(FC.table_of(c.table)), FC.table_of(c.table).max_pots) for c in steps_only} == {(5, 2), (1, 3)}
