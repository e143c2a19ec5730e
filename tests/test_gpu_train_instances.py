"""Every path and kernel instance of oc_multi_agent_step against the plain reference, by name: the cases of tests/train_cases.py
(held to the planner and to the sources' instances by tests/test_host_train_instances.py), each asked of oc_multi_agent_plan on
this device, then stepped as a VecOvercookedMultiAgent beside OracleTrainStep.

The tolerance is zero, and it is derived, not chosen: the transition, the restart draws, the layout draws, the event counters
and the observation are integer work; the rewards are small integers in f32; phi is the same sequence of IEEE float64
operations on both sides (`#pragma clang fp contract(off)` in every training kernel, -ffp-contract=off for the oracle; the suite
holds oc_potential to bit identity already), and shaped = (sparse0 + sparse1) + factor * dense is one sum, one product and one
sum of float64 on both sides.  So every array is compared with np.array_equal, the float64 ones as bit patterns."""
import pytest

import train_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import gpu, packed_counters  # noqa: E402, F401

OBS_CHUNK = 16384  # envs per comparison of the observation: the oracle's int32 image of 16 384 cramped_room envs is 68 MB


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_every_training_step_instance_against_the_reference(case, gpu):
    training_case_against_the_reference(case, gpu)


def training_case_against_the_reference(case, gpu, epoch0=None):
    """epoch0: the epoch the first step draws from (the env's own counter, set after its construction; the reference's likewise)."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    plan = TC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    table = TC.table_of(case.table)
    dt = {"u8": torch.uint8, "f32": torch.float32, None: None}[case.obs]
    env = VecOvercookedMultiAgent(table, case.n_envs, device=gpu, obs_dtype=dt, **TC.env_kwargs(case))
    assert env.plan() == plan, (case.id, env.plan(), plan)  # (the env's own batch and arrays give the plan the case was listed for)
    ref = TC.oracle_of(case)
    v = env.venv
    if epoch0 is not None:
        v._epoch = ref.epoch = epoch0
    lid = lambda: None if ref.layout_id is None else ref.layout_id  # noqa: E731
    compare(case, -1, "state", v.get_packed_state(), ref.state, lid(), env_axis=1)  # (the packed state is [plane][env][16])
    if case.use_phi:
        compare(case, -1, "phi_cur", env.phi_cur.cpu().numpy(), ref.phi_cur, lid())
    big = case.n_envs >= 131072
    for t in range(case.steps):
        if case.factor == "anneal" and t == TC.anneal_at(case):
            env.anneal_reward_shaping_factor(TC.ANNEAL_TIMESTEPS)
        assert env.reward_shaping_factor == TC.factor_at(case, t)
        a = TC.actions_of(case, t)
        obs, shaped, done, infos = env.step(torch.from_numpy(a).to(gpu))
        ref.step(a, TC.factor_at(case, t))
        fields = [("state", v.get_packed_state(), ref.state), ("rewards", v.rewards, ref.rewards), ("flags", v.flags, ref.flags),
                  ("ep_returns", v.ep_returns, ref.ep_returns), ("infos[ep_returns]", infos["ep_returns"], ref.ep_out),
                  ("shaped", shaped, ref.shaped), ("done", done, ref.done)]
        if case.use_phi:
            fields += [("phi_next", infos["phi_s_prime"], ref.phi_next), ("phi_cur", env.phi_cur, ref.phi_cur)]
        if ref.layout_id is not None:
            fields.append(("layout_id", v.layout_ids(), ref.layout_id))
        for field, got, want in fields:
            compare(case, t, field, got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want, lid(), env_axis=1 if field == "state" else 0)
        if case.events:
            for field, got, want in (("event counters, running", v.event_counts, ref.counts), ("event counters, published", v.event_counts_done, ref.counts_done)):
                compare(case, t, field, packed_counters(got), want, lid())
        # the observation of the states the next step starts from, in env chunks (the batch of >= 131 072 envs: the first, the
        # last and every restart-bearing step)
        if case.obs is not None and (not big or t in (0, case.steps - 1) or ref.done.any()):
            assert obs.dtype == dt and obs.shape == (case.n_envs, 2, table.width, table.height, 26)
            for a0 in range(0, case.n_envs, OBS_CHUNK):
                a1 = min(case.n_envs, a0 + OBS_CHUNK)
                compare(case, t, "observation", obs[a0:a1].cpu().numpy(), ref.obs(a0, a1), lid(), e0=a0)
    assert (ref.flags & 2).any()  # (the last step, like every step, carries illegal actions)
