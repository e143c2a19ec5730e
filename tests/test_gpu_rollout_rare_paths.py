"""The paths through the rare branch of k_rollout5's step (step_duo5.hpp, dstep) against the C oracle, at the smallest shapes at which
each can go wrong (tests/rare_path_cases.py): rewards, flags (tiled and [step][env]), final packed states and episode returns by exact
equality.  Before its comparison every case counts, on the oracle, the cooking starts, open-gate dish pick-ups, deliveries,
shared-cell replays and restarts of its launch: each is above zero unless the case's id says it lacks it.  Two launches back to back
equal one launch of their steps."""
import numpy as np
import pytest

import rare_path_cases as RP
import rollout_cases as RC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import RolloutOutputs, gpu, no_sentinel  # noqa: E402, F401


def _env(gpu, c):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    env = VecOvercookedEnv(RP.table_of(c.table), c.n_envs, horizon=c.horizon, device=gpu, auto_reset=True, seed=c.seed,
                           env_offset=c.env_offset, layout_id=RP.layout_ids(c), **RP.start_kw(c))
    env.set_packed_state(RP.first_state(c, env.get_packed_state()))
    return env


def _launch(env, c, n_steps, t0=0):
    """One oc_rollout_random call of n_steps from global step t0 -> (rewards, flags untiled) or (None, None); the planner names the
    case's instance for it, and the launch writes every reward and flag and nothing around them."""
    tiled, outputs = c.out == "tiled", c.out != "no_outputs"
    plan = RC.plan_of(env.table, c.n_envs, n_steps, t0, c.horizon, tiled=tiled, outputs=outputs, start=RP.start_kw(c) or None,
                      seed=c.seed, env_offset=c.env_offset, epoch=env.reset_epoch)
    assert plan.startswith(c.expect), plan
    out = RolloutOutputs(n_steps, c.n_envs, env.device, tiled=tiled, outputs=outputs)
    env.rollout_random(n_steps, out.rew, out.fl, flags_tiled8=tiled)
    out.all_written(c)
    return (out.rew.cpu().numpy(), out.flags().cpu().numpy()) if outputs else (None, None)


def _differ(name, got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert len(bad) == 0, "%s: %d values differ, first at %s: got %s, oracle %s" % (
        name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _every_cause_is_hit(c):
    """On the oracle, before anything runs on the GPU: the launch holds every cause but those its id says it lacks."""
    got = RP.census(c)
    print(c.id, got)
    for cause in RP.CAUSES:
        assert (got[cause] > 0) == (cause not in c.lacks), "%s: %d env-steps with a %s" % (c.id, got[cause], cause)


@pytest.mark.parametrize("case", RP.CASES, ids=lambda c: c.id)
def test_rare_paths_against_oracle(case, gpu):
    _every_cause_is_hit(case)
    env = _env(gpu, case)
    run = RP.oracle_launch(case)
    _differ("first states", env.get_packed_state(), run.state)
    rew, fl = _launch(env, case, case.n_steps)
    (_, rew_o, fl_o, _), = run.chunks(case.n_steps)
    if case.out != "no_outputs":
        no_sentinel(case, rew_o, fl_o)
        _differ("flags", fl, fl_o)
        _differ("rewards", rew, rew_o)
    _differ("final states", env.get_packed_state(), run.state)
    _differ("episode returns", env.ep_returns.cpu().numpy(), run.ep_returns)


@pytest.mark.parametrize("case", RP.HANDOVER, ids=lambda c: c.id)
def test_two_launches_back_to_back_equal_one(case, gpu):
    """8 steps, then 16, against one launch of 24 and against the oracle: what a launch leaves in the packed state and the episode
    returns is all the next one needs."""
    got = RP.census(case, 24)
    assert all(got[cause] > 0 for cause in RP.CAUSES if cause != "replay"), got  # (a replay within 24 steps: not in every case)
    a, b = _env(gpu, case), _env(gpu, case)
    rew_a, fl_a = _launch(a, case, 24)
    first = _launch(b, case, 8)
    second = _launch(b, case, 16, t0=8)
    _differ("flags", np.concatenate([first[1], second[1]]), fl_a)
    _differ("rewards", np.concatenate([first[0], second[0]]), rew_a)
    _differ("final states", b.get_packed_state(), a.get_packed_state())
    _differ("episode returns", b.ep_returns.cpu().numpy(), a.ep_returns.cpu().numpy())
    run = RP.oracle_launch(case)
    (_, rew_o, fl_o, _), = run.chunks(24)
    _differ("flags against the oracle", fl_a, fl_o)
    _differ("rewards against the oracle", rew_a, rew_o)
    _differ("final states against the oracle", a.get_packed_state(), run.state)
    _differ("episode returns against the oracle", a.ep_returns.cpu().numpy(), run.ep_returns)
