"""Every path of oc_multi_agent_step_featurize against the plain reference, by name: the cases of tests/train_featurize_cases.py
(held to the planner and to the sources' instances by tests/test_host_train_featurize.py), each asked of
oc_multi_agent_step_featurize_plan on this device, then stepped as a VecOvercookedMultiAgent(obs="features" / "both") beside
train_cases.OracleTrainStep, with oracle.featurize of the reference's states after each step.

The tolerance is zero, and it is derived, not chosen: the transition, the restart draws, the layout draws, the event counters, the
lossless observation and the features are integer work; the rewards and every feature (flags, counts, deltas on a grid of at most
128 cells, cook time left < 255) are small integers, exact in f32 and in the kernels' int16 image; phi is the same sequence of IEEE
float64 operations on both sides (`#pragma clang fp contract(off)` in every training kernel, -ffp-contract=off for the oracle), and
shaped = (sparse0 + sparse1) + factor * dense is one sum, one product and one sum of float64 on both sides.  So every array is
compared with np.array_equal, the float64 ones as bit patterns."""
import numpy as np
import pytest

import train_cases as TC
import train_featurize_cases as FC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import GUARD, gpu, guards_untouched, packed_counters  # noqa: E402, F401

FILL = -12345.0  # no feature holds it


def guarded_features(env, case, device):
    """The env's persistent feature buffer replaced by rows [GUARD, GUARD + n_envs) of an array filled with FILL: guard rows before and
    behind the output."""
    whole = torch.full((GUARD + case.n_envs + GUARD, 2, FC.total_of(case.num_pots)), FILL, dtype=torch.float32, device=device)
    env._feat = whole[GUARD:GUARD + case.n_envs]
    assert env._feat.data_ptr() % 16 == 0 and env._feat.is_contiguous()
    return whole[:GUARD], whole[GUARD + case.n_envs:]


def run_case(case, gpu, epoch0=None, collect=False):
    """Steps the case beside the reference, every output compared at every step; collect: also returns every step's outputs
    (numpy), for a comparison of two paths."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    plan = FC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    table = TC.table_of(case.table)
    dt = {"u8": torch.uint8, "f32": torch.float32, None: None}[case.obs_dtype]
    env = VecOvercookedMultiAgent(table, case.n_envs, device=gpu, obs_dtype=dt, **FC.env_kwargs(case))
    assert env.plan() == plan, (case.id, env.plan(), plan)  # (the env's own batch and arrays give the plan the case was listed for)
    guards = guarded_features(env, case, gpu)
    ref = TC.oracle_of(case)
    v = env.venv
    if epoch0 is not None:
        v._epoch = ref.epoch = epoch0
    lid = lambda: None if ref.layout_id is None else ref.layout_id  # noqa: E731
    compare(case, -1, "state", v.get_packed_state(), ref.state, lid(), env_axis=1)  # (the packed state is [plane][env][16])
    if case.use_phi:
        compare(case, -1, "phi_cur", env.phi_cur.cpu().numpy(), ref.phi_cur, lid())
    trace = []
    for t in range(case.steps):
        if case.factor == "anneal" and t == TC.anneal_at(case):
            env.anneal_reward_shaping_factor(TC.ANNEAL_TIMESTEPS)
        assert env.reward_shaping_factor == TC.factor_at(case, t)
        a = FC.actions_of(case, t)
        obs, shaped, done, infos = env.step(torch.from_numpy(a).to(gpu))
        ref.step(a, TC.factor_at(case, t))
        lossless, feats = obs if case.obs == "both" else (None, obs)
        assert feats.data_ptr() == env._feat.data_ptr() and feats.shape == (case.n_envs, 2, FC.total_of(case.num_pots)) and feats.dtype == torch.float32
        fields = [("state", v.get_packed_state(), ref.state), ("rewards", v.rewards, ref.rewards), ("flags", v.flags, ref.flags),
                  ("ep_returns", v.ep_returns, ref.ep_returns), ("infos[ep_returns]", infos["ep_returns"], ref.ep_out),
                  ("shaped", shaped, ref.shaped), ("done", done, ref.done)]
        if case.use_phi:
            fields += [("phi_next", infos["phi_s_prime"], ref.phi_next), ("phi_cur", env.phi_cur, ref.phi_cur)]
        if ref.layout_id is not None:
            fields.append(("layout_id", v.layout_ids(), ref.layout_id))
        fields.append(("features", feats, FC.features_of(case, ref)))
        got_all = {}
        for field, got, want in fields:
            got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
            compare(case, t, field, got, want, lid(), env_axis=1 if field == "state" else 0)
            got_all[field] = got.copy()
        if case.events:
            for field, got, want in (("event counters, running", v.event_counts, ref.counts), ("event counters, published", v.event_counts_done, ref.counts_done)):
                compare(case, t, field, packed_counters(got), want, lid())
        if lossless is not None:
            assert lossless.dtype == dt and lossless.shape == (case.n_envs, 2, table.width, table.height, 26)
            compare(case, t, "observation", lossless.cpu().numpy(), ref.obs(0, case.n_envs), lid())
        guards_untouched(case, "features", guards, FILL)
        trace.append(got_all)
    assert (ref.flags & 2).any()  # (the last step, like every step of the larger batches, carries illegal actions)
    return trace if collect else None


@pytest.mark.parametrize("case", FC.CASES, ids=lambda c: c.id)
def test_every_path_of_the_training_step_with_features_against_the_reference(case, gpu):
    run_case(case, gpu)


def test_the_far_counter_case_against_the_reference(gpu):
    c = FC.far_case()
    run_case(c, gpu, epoch0=FC.far_epoch0(c))


def test_the_default_plan_at_the_smallest_batch_it_gives_the_kernel(gpu):
    c = FC.default_plan_case()
    assert "k_train_step_feat" not in FC.plan_of_case(c, c.n_envs - 1)
    run_case(c, gpu)


def test_the_kernel_and_the_two_launches_agree_bit_for_bit(gpu):
    """A forced case run a second time through oc_multi_agent_step's own path + k_featurize on the same inputs: every output of
    every step is bit-equal (both runs are also held to the reference)."""
    one = next(c for c in FC.CASES if c.id == "feat_two_pots_ragged_last_workgroup")
    two = one._replace(id=one.id + "/two_launches", one_kernel=False, expect=FC.two_launches(TC.step1(True, 2, True)))
    a, b = run_case(one, gpu, collect=True), run_case(two, gpu, collect=True)
    assert len(a) == len(b) == one.steps
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for field in x:
            u, w = (np.ascontiguousarray(z).view(np.uint8) for z in (x[field], y[field]))
            assert np.array_equal(u, w), (t, field)
