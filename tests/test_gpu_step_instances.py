"""Every kernel instance of the caller-actions family (oc_step, oc_step_many, oc_step_server_*) against the C oracle alone, by name:
the cases of tests/step_cases.py (held to the planner and to the sources' instances by tests/test_host_step_instances.py), each
asked of oc_step_plan on this device, then run as VecOvercookedEnv calls — step (in place or out of place), step_many, or a
StepServer's play / sync / step — beside step_cases.OracleRun, step by step.

The tolerance is zero, and it is derived, not chosen: the transition, the restart draws and the layout re-draws are integer work;
the rewards are small integers (3, 3, 5, 20 x bonus) and so are their per-episode sums, all exact in float32.  So every array is
compared with np.array_equal.  Every output array, state_out included, is pre-filled with a value no result holds (0xEE; -7.0) and
has guard rows behind it that must come back untouched; out of place, the input state must be unchanged after the call."""
import numpy as np
import pytest

import step_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import gpu, guarded, guards_untouched, packed_counters  # noqa: E402, F401


def _new_env(case, gpu, epoch0=None):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    env = VecOvercookedEnv(SC.table_of(case.table), case.n_envs, device=gpu, **SC.env_kwargs(case))
    if epoch0 is not None:
        env._epoch = epoch0
    env.predicate_interact = case.predicate
    env.set_packed_state(SC.states_of(case).copy())
    return env


def _compare_env(case, k, env, ref, lid0):
    """What an env holds after step k against the oracle: state, episode returns, counters, layout ids."""
    lid = ref.layout_id
    if lid is not None:
        compare(case, k, "layout ids", env.layout_ids(), lid, lid0)
    compare(case, k, "state", env.get_packed_state(), ref.state, lid, env_axis=1)
    if case.returns:
        compare(case, k, "episode returns", env.ep_returns.cpu().numpy(), ref.ep_returns, lid)
    else:
        assert env.ep_returns is None
    if SC.with_counts(case):
        compare(case, k, "running event counters", packed_counters(env.event_counts), ref.counts, lid)
        compare(case, k, "published event counters", packed_counters(env.event_counts_done), ref.counts_done, lid)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_every_step_instance_against_the_oracle(case, gpu):
    step_case_against_the_oracle(case, gpu)


def step_case_against_the_oracle(case, gpu, epoch0=None):
    """epoch0: the epoch the case's calls start from (the env's own counter, set after its construction; the oracle's run likewise)."""
    table = SC.table_of(case.table)
    n, K = case.n_envs, case.n_steps
    env = _new_env(case, gpu, epoch0)
    ref = SC.OracleRun(case, epoch0)
    acts = torch.from_numpy(np.array(SC.actions_of(case))).to(gpu)
    masks_on = SC.with_masks(case)

    # 1. the plan of the call, on this device: the instance the case is there for
    entry = "step" if case.entry == "step_out_of_place" else case.entry
    plan = env.plan_step(entry, n_steps=K if entry == "step_many" else 1, state_out=case.entry == "step_out_of_place", events_out=masks_on)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)

    guards = []
    if case.entry in ("step", "step_out_of_place"):
        oop = case.entry == "step_out_of_place"
        ev, g_ev = guarded(n, (), torch.int64, -1, gpu) if masks_on else (None, None)
        out = None
        if oop:  # [n_planes][n][16], guard rows behind the last plane
            flat, g_out = guarded(table.n_planes * n, (16,), torch.uint8, 0xEE, gpu)
            out = flat.view(table.n_planes, n, 16)
            guards.append(("state_out", g_out, 0xEE))
        for k in range(K):
            env.rewards.fill_(-7.0)
            env.flags.fill_(0xEE)
            if ev is not None:
                ev.fill_(-1)
            lid0 = None if ref.layout_id is None else ref.layout_id.copy()
            if oop:
                out.fill_(0xEE)
                before = env.state.clone()
            r, f = env.step(acts[k], state_out=out, events_out=ev)
            rew_o, fl_o, masks_o = ref.step(k)
            compare(case, k, "flags", f.cpu().numpy(), fl_o, lid0)
            compare(case, k, "rewards", r.cpu().numpy(), rew_o, lid0)
            if ev is not None:
                compare(case, k, "event masks", ev.cpu().numpy().view(np.uint64), masks_o, lid0)
            if oop:
                assert torch.equal(env.state, before), "%s: step %d changed its input state" % (case.id, k)
                compare(case, k, "state_out", out.cpu().numpy(), ref.state, lid0, env_axis=1)
                env.state.copy_(out)
            _compare_env(case, k, env, ref, lid0)
        if ev is not None:
            guards.append(("event masks", g_ev, -1))
    elif case.entry == "step_many":
        rew, g_rew = guarded(K * n, (4,), torch.float32, -7.0, gpu)
        fl, g_fl = guarded(K * n, (), torch.uint8, 0xEE, gpu)
        ev, g_ev = guarded(K * n, (), torch.int64, -1, gpu) if masks_on else (None, None)
        lid0 = None if ref.layout_id is None else ref.layout_id.copy()
        env.step_many(acts, rew.view(K, n, 4), fl.view(K, n), events_out=None if ev is None else ev.view(K, n))
        rew_h, fl_h = rew.view(K, n, 4).cpu().numpy(), fl.view(K, n).cpu().numpy()
        ev_h = None if ev is None else ev.view(K, n).cpu().numpy().view(np.uint64)
        # ... and the same K steps as single step calls on a second env
        env2 = _new_env(case, gpu, epoch0)
        ev2 = torch.full((n,), -1, dtype=torch.int64, device=gpu) if masks_on else None
        for k in range(K):
            lid_k = None if ref.layout_id is None else ref.layout_id.copy()
            rew_o, fl_o, masks_o = ref.step(k)
            compare(case, k, "flags", fl_h[k], fl_o, lid_k)
            compare(case, k, "rewards", rew_h[k], rew_o, lid_k)
            if ev_h is not None:
                compare(case, k, "event masks", ev_h[k], masks_o, lid_k)
            r2, f2 = env2.step(acts[k], events_out=ev2)
            compare(case, k, "flags of single steps", f2.cpu().numpy(), fl_o, lid_k)
            compare(case, k, "rewards of single steps", r2.cpu().numpy(), rew_o, lid_k)
            if ev2 is not None:
                compare(case, k, "event masks of single steps", ev2.cpu().numpy().view(np.uint64), masks_o, lid_k)
            _compare_env(case, k, env2, ref, lid_k)
        _compare_env(case, K - 1, env, ref, lid0)
        guards += [("rewards", g_rew, -7.0), ("flags", g_fl, 0xEE)] + ([("event masks", g_ev, -1)] if ev is not None else [])
    else:  # the resident step: SERVER_SPLIT steps in one play, a sync (the kernel leaves), the others as single steps (a resume)
        A = SC.SERVER_SPLIT
        rew, g_rew = guarded(A * n, (4,), torch.float32, -7.0, gpu)
        fl, g_fl = guarded(A * n, (), torch.uint8, 0xEE, gpu)
        with env.step_server() as sv:
            sv.play(acts[:A].contiguous(), rew.view(A, n, 4), fl.view(A, n))
            rew_h, fl_h = rew.view(A, n, 4).cpu().numpy(), fl.view(A, n).cpu().numpy()
            for k in range(A):
                rew_o, fl_o, _ = ref.step(k)
                compare(case, k, "flags", fl_h[k], fl_o, ref.layout_id)
                compare(case, k, "rewards", rew_h[k], rew_o, ref.layout_id)
            sv.sync()
            assert sv.steps == A, (case.id, sv.steps)
            _compare_env(case, A - 1, env, ref, ref.layout_id)
            for k in range(A, K):
                env.rewards.fill_(-7.0)
                env.flags.fill_(0xEE)
                r, f = sv.step(acts[k])
                rew_o, fl_o, _ = ref.step(k)
                compare(case, k, "flags", f.cpu().numpy(), fl_o, ref.layout_id)
                compare(case, k, "rewards", r.cpu().numpy(), rew_o, ref.layout_id)
            sv.sync()
            assert sv.steps == K, (case.id, sv.steps)
            _compare_env(case, K - 1, env, ref, ref.layout_id)
        guards += [("rewards", g_rew, -7.0), ("flags", g_fl, 0xEE)]
    assert env.steps_done == K
    for what, g, v in guards:
        guards_untouched(case, what, g, v)
