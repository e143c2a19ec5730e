"""Every kernel instance of oc_potential and oc_featurize against the C oracle alone, by name: the cases of tests/derived_cases.py
(held to the planners, to the sources' instances and to the situations their states promise by tests/test_host_derived_instances.py),
each asked of oc_potential_plan / oc_featurize_plan on this device, then run as VecOvercookedEnv.potential / .featurize on the
case's states.

The tolerance is zero, and it is derived, not chosen: phi is a float64 sum of products of table entries taken in the reference's
operand order without contraction (csrc/potential.hpp), the features are small integers, exact in float32.  So every array is
compared with np.array_equal; no case's reference holds a nan (asserted).  The output is a slice of a larger array pre-filled with
a value no result holds, with guard rows before its first env and after its last that must come back untouched."""
import numpy as np
import pytest

import derived_cases as DC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import GUARD, gpu, guarded, guards_untouched  # noqa: E402, F401

SENTINEL = -7.0  # the fill of the whole array; the guards are compared with it, the rows between them with the oracle


def _output_between_guards(rows, row_shape, dtype, gpu):
    """The output between GUARD rows on either side.  GUARD feature rows are a multiple of 32 bytes and GUARD potentials of 8, so the
    slice keeps the alignment the entry points ask for."""
    out, guards = guarded(rows, row_shape, dtype, SENTINEL, gpu, before=GUARD)
    assert out.is_contiguous() and out.data_ptr() % (16 if row_shape else 8) == 0
    return out, guards


def _situations(case, e):
    goals = DC.counter_goals_of(case) if case.kind == "featurize" else "none"
    st = DC.states_of(case)[:, e:e + 1]
    lid = DC.layout_ids(case)
    return DC.situations_of_states(DC.table_of(case.table), None if lid is None else lid[e:e + 1], st, case.kind, goals, case.num_pots or 0)[0]


def _new_env(case, gpu, hints=None):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    kw = DC.env_kwargs(case)
    if hints is not None:
        kw["withhold_hints"] = not hints
    env = VecOvercookedEnv(DC.table_of(case.table), case.n_envs, device=gpu, **kw)
    env.set_packed_state(np.array(DC.states_of(case)))
    return env


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.id)
def test_every_derived_instance_against_the_oracle(case, gpu):
    n, lid = case.n_envs, DC.layout_ids(case)
    env = _new_env(case, gpu)
    context = lambda e: ", situations %s" % sorted(_situations(case, e))  # noqa: E731

    # 1. the plan of the call, on this device: the instance the case is there for
    plan = env.potential_plan() if case.kind == "potential" else env.featurize_plan(case.num_pots)
    assert plan.startswith(case.expect + " grid="), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    assert plan == DC.plan_of_case(case)

    # 2. the launch, into a guarded slice, against the oracle
    if case.kind == "potential":
        for gamma in DC.GAMMAS:
            want = DC.oracle_run(case, gamma)
            assert want.dtype == np.float64 and np.isfinite(want).all() and (want > 0).all()
            out, guards = _output_between_guards(n, (), torch.float64, gpu)
            assert env.potential(gamma, out=out).data_ptr() == out.data_ptr()
            got = out.cpu().numpy()
            compare(case, None, "phi at gamma %s" % gamma, got, want, lid, context=context)
            guards_untouched(case, "potentials", guards, SENTINEL)
            if case.id == "potential_hints_withheld":  # ... and k_potential2 on the same states: the two kernels agree
                env2 = _new_env(case, gpu, hints=True)
                assert env2.potential_plan().startswith("k_potential2 grid=")
                assert np.array_equal(env2.potential(gamma).cpu().numpy(), got)
    else:
        total = 2 * (case.num_pots * 10 + 26) + 4
        want = DC.oracle_run(case)
        assert want.dtype == np.float32 and want.shape == (n, 2, total) and np.isfinite(want).all()
        out, guards = _output_between_guards(n, (2, total), torch.float32, gpu)
        assert env.featurize(case.num_pots, DC.counter_goals_of(case), out=out).data_ptr() == out.data_ptr()
        compare(case, None, "features", out.cpu().numpy(), want, lid, context=context)
        guards_untouched(case, "features", guards, SENTINEL)
