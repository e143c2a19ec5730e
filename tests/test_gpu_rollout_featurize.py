"""oc_rollout_featurize against the C oracle alone: the cases of tests/featurize_rollout_cases.py (held to the planner and shown to
contain what they claim by tests/test_host_rollout_featurize.py), each asked of oc_rollout_featurize_plan on this device, then run as
ONE VecOvercookedEnv.rollout_featurize call beside the oracle stepped one step at a time (Oracle.step or Oracle.rollout_random of
one step, then oracle.featurize).  Every single-layout case runs twice on the same inputs: forced to k_rollout_featurize, and through
the step-by-step path.

The tolerance is zero, and it is derived, not chosen: the transition, the Philox draws, the restart draws and the features are
integer work; every feature is a small integer (a delta, a count, a flag, a cook time below 255) and the rewards are small integers,
all exact in float32.  Every output array is pre-filled with a value no result holds and has guard rows behind it that must come back
untouched."""
import numpy as np
import pytest

import featurize_rollout_cases as FC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import gpu, guarded, guards_untouched  # noqa: E402, F401

FILL = -7.0  # no feature, no reward


def case_against_the_oracle(case, gpu, epoch0=None):
    """epoch0: the epoch the case's call starts from (the env's own counter, set after its construction; the oracle's run likewise)."""
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    table = FC.table_of(case.table)
    n, K, total = case.n_envs, case.n_steps, FC.total_of(case.num_pots)
    env = VecOvercookedEnv(table, n, device=gpu, **FC.env_kwargs(case))
    env.one_kernel = case.one_kernel
    env.set_packed_state(FC.states_of(case).copy())
    env.t_global = case.t0
    if epoch0 is not None:
        env._epoch = epoch0
    ref = FC.oracle_trajectory(case, 1 if epoch0 is None else epoch0)
    FC.check_claims(case, ref)
    lid = FC.layout_ids(case)
    acts = FC.actions_of(case)

    # 1. the plan of the call, on this device: the path the case is there for
    plan = env.plan_rollout_featurize(K, case.num_pots, actions=acts is not None)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)

    # 2. one call
    single = case.call == "single_buffer"
    rows = 1 if single else K
    feats, g_feats = guarded(rows * n, (2, total), torch.float32, FILL, gpu)
    rew, g_rew = guarded(K * n, (4,), torch.float32, FILL, gpu)
    fl, g_fl = guarded(K * n, (), torch.uint8, 0xEE, gpu)
    rew, fl = rew.view(K, n, 4), fl.view(K, n)
    d_acts = None if acts is None else torch.from_numpy(np.array(acts)).to(gpu)
    feats_arg = feats if single else feats.view(K, n, 2, total)
    out = env.rollout_featurize(K, feats_arg, rew, fl, actions=d_acts, num_pots=case.num_pots, counter_goals=case.counter_goals)
    assert out[0] is feats_arg
    torch.cuda.synchronize()

    # 3. everything the call wrote
    rew_h, fl_h, feats_h = rew.cpu().numpy(), fl.cpu().numpy(), feats_arg.cpu().numpy()
    for k in range(K):
        compare(case, k, "rewards", rew_h[k], ref.rewards[k], lid)
        compare(case, k, "flags", fl_h[k], ref.flags[k], lid)
        if not single:
            compare(case, k, "features", feats_h[k], ref.features[k], lid)
    if single:  # one buffer, overwritten every step: the features of the last step
        compare(case, K - 1, "features", feats_h, ref.features[K - 1], lid)
    compare(case, K - 1, "state", env.get_packed_state(), ref.state, lid, env_axis=1)
    compare(case, K - 1, "episode returns", env.ep_returns.cpu().numpy(), ref.ep_returns, lid)
    assert env.t_global == case.t0 + (K if acts is None else 0), (case.id, env.t_global)
    for what, g, v in (("features", g_feats, FILL), ("rewards", g_rew, FILL), ("flags", g_fl, 0xEE)):
        guards_untouched(case, what, g, v)


@pytest.mark.parametrize("case", FC.CASES, ids=lambda c: c.id)
def test_every_rollout_featurize_case_against_the_oracle(case, gpu):
    case_against_the_oracle(case, gpu)


def test_the_default_plan_at_launch_size(gpu):
    """The unforced plan at the smallest batch the fill rule accepts names the kernel: a grid of whole eighths, placed through xcd_block."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = cus * 64
    case = FC.LAUNCH_SIZE._replace(n_envs=n)
    assert FC.plan_of_case(case).startswith(FC.ONE_KERNEL) and not FC.plan_of_case(case, n - 1).startswith(FC.ONE_KERNEL)
    assert not case.one_kernel
    case_against_the_oracle(case, gpu)


def test_far_counters(gpu):
    """Both paths at the far corner of the counter space: seed_hi in the key, g_lo wrapping inside the batch, the Philox block index
    wrapping inside the launch, epoch + k wrapping between two restarts."""
    far = FC.far_case()
    for case in (far, far._replace(id=far.id + "/steps", one_kernel=False, expect=FC.step_by_step("oc_rollout_random"))):
        case_against_the_oracle(case, gpu, FC.far_epoch0(case))


def test_sharded_rollout_featurize_equals_the_unsharded_env(gpu):
    from overcooked_ai_amd import ShardedVecOvercookedEnv, VecOvercookedEnv

    n, K, num_pots = 700, 12, 2
    kw = dict(horizon=8, auto_reset=True, seed=5, **FC.DRAWN)
    whole = VecOvercookedEnv("asymmetric_advantages", n, device=gpu, **kw)
    sh = ShardedVecOvercookedEnv("asymmetric_advantages", n, devices=[gpu, gpu], **kw)
    for one_kernel in (True, False):
        whole.one_kernel = one_kernel
        for s in sh.shards:
            s.env.one_kernel = one_kernel
        feats = torch.full((K, n, 2, FC.total_of(num_pots)), FILL, dtype=torch.float32, device=gpu)
        rew = torch.zeros((K, n, 4), dtype=torch.float32, device=gpu)
        fl = torch.zeros((K, n), dtype=torch.uint8, device=gpu)
        whole.rollout_featurize(K, feats, rew, fl, num_pots=num_pots, counter_goals="all")
        featss, (rews, fls) = sh.alloc_features(K, num_pots), sh.alloc_outputs(K)
        sh.rollout_featurize(K, featss, rews, fls, num_pots=num_pots, counter_goals="all")
        sh.synchronize()
        cat = lambda parts, axis: np.concatenate([p.cpu().numpy() for p in parts], axis=axis)  # noqa: E731
        assert np.array_equal(cat(featss, 1), feats.cpu().numpy()) and np.array_equal(cat(rews, 1), rew.cpu().numpy())
        assert np.array_equal(cat(fls, 1), fl.cpu().numpy()) and np.array_equal(sh.get_packed_state(), whole.get_packed_state())
        assert (fl.cpu().numpy() & 4).any() and float(feats.min()) > FILL
    last = sh.alloc_features(None, num_pots)
    assert last[0].shape == (sh.shards[0].stop - sh.shards[0].start, 2, FC.total_of(num_pots))


def test_a_padded_step_stride_on_both_paths(gpu):
    """feat_step_stride larger than a step's bytes (a multiple of 16): step k's rows land at k * stride, the padding behind each
    step's rows and the guard rows stay untouched.  The env class only passes 0 or a step's bytes, so this is the entry point itself,
    with the env's own arrays."""
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    base = next(c for c in FC.CASES if c.id == "asymmetric_counter_goals")
    pad_rows = 5  # (env, player) rows of padding behind a step's 2 n rows: 5 * 96 * 4 = 1920 bytes, a multiple of 16
    for case in (base, next(c for c in FC.CASES if c.id == base.id + "/steps")):
        n, K, total = case.n_envs, case.n_steps, FC.total_of(case.num_pots)
        env = VecOvercookedEnv(FC.table_of(case.table), n, device=gpu, **FC.env_kwargs(case))
        env.set_packed_state(FC.states_of(case).copy())
        ref = FC.oracle_trajectory(case)
        step_rows = 2 * n + pad_rows
        feats, g_feats = guarded(K * step_rows, (total,), torch.float32, FILL, gpu)
        rew = torch.full((K, n, 4), FILL, dtype=torch.float32, device=gpu)
        fl = torch.full((K, n), 0xEE, dtype=torch.uint8, device=gpu)
        blob, offs = env._plan(case.counter_goals)
        options = _lib.OPT_AUTO_RESET | (_lib.OPT_ONE_KERNEL if case.one_kernel else 0)
        rc = env._launch(env.lib.oc_rollout_featurize, env._bref, blob.data_ptr(), offs.data_ptr(), env._state_ptr, None, rew.data_ptr(),
                         fl.data_ptr(), env._ep_ptr, feats.data_ptr(), step_rows * total * 4, case.num_pots, case.horizon, options,
                         case.seed, case.env_offset, case.t0, K, env._start_spec())
        _lib.check(rc, "oc_rollout_featurize")
        torch.cuda.synchronize()
        got = feats.view(K, step_rows, total).cpu().numpy()
        for k in range(K):
            compare(case, k, "features", got[k, :2 * n].reshape(n, 2, total), ref.features[k], None)
            compare(case, k, "flags", fl[k].cpu().numpy(), ref.flags[k], None)
        assert (got[:, 2 * n:] == FILL).all(), "%s: the padding behind a step's rows was written" % case.id
        guards_untouched(case, "features", g_feats, FILL)
        compare(case, K - 1, "state", env.get_packed_state(), ref.state, None, env_axis=1)


def test_with_event_counters_the_one_step_calls_run_and_give_the_same_trajectory(gpu):
    """track_events: rollout_featurize loops over the one-step calls (the counters ride on their event sink), plan_rollout_featurize
    says so, and features, rewards, flags, states and the counters equal an untracked run's and rollout_random's."""
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    for case in (next(c for c in FC.CASES if c.id == "asymmetric_counter_goals"), next(c for c in FC.CASES if c.id == "tomato_actions")):
        n, K, total = case.n_envs, case.n_steps, FC.total_of(case.num_pots)
        ref = FC.oracle_trajectory(case)
        acts = FC.actions_of(case)
        d_acts = None if acts is None else torch.from_numpy(np.array(acts)).to(gpu)
        env = VecOvercookedEnv(FC.table_of(case.table), n, device=gpu, track_events=True, **FC.env_kwargs(case))
        env.one_kernel = True  # (asked for and not to be had: the counters need the one-step calls)
        env.set_packed_state(FC.states_of(case).copy())
        env.t_global = case.t0
        plan = env.plan_rollout_featurize(K, case.num_pots, actions=acts is not None)
        assert plan.startswith(FC.step_by_step("oc_step" if acts is not None else "oc_rollout_random")), plan
        feats = torch.full((K, n, 2, total), FILL, dtype=torch.float32, device=gpu)
        rew = torch.full((K, n, 4), FILL, dtype=torch.float32, device=gpu)
        fl = torch.full((K, n), 0xEE, dtype=torch.uint8, device=gpu)
        env.rollout_featurize(K, feats, rew, fl, actions=d_acts, num_pots=case.num_pots, counter_goals=case.counter_goals)
        torch.cuda.synchronize()
        compare(case, None, "features", feats.cpu().numpy(), ref.features, None, env_axis=1)
        compare(case, None, "rewards", rew.cpu().numpy(), ref.rewards, None, env_axis=1)
        compare(case, None, "flags", fl.cpu().numpy(), ref.flags, None, env_axis=1)
        compare(case, K - 1, "state", env.get_packed_state(), ref.state, None, env_axis=1)
        assert env.t_global == case.t0 + (K if acts is None else 0)
        # the counters: those of the same steps without the features
        plain = VecOvercookedEnv(FC.table_of(case.table), n, device=gpu, track_events=True, **FC.env_kwargs(case))
        plain.set_packed_state(FC.states_of(case).copy())
        plain.t_global = case.t0
        for k in range(K):
            if acts is None:
                plain.rollout_random(1)
            else:
                plain.step(d_acts[k])
        for finished in (False, True):
            a, b = plain.event_stats(finished), env.event_stats(finished)
            for name in a:
                assert torch.equal(a[name], b[name]), (case.id, name, finished)
        assert sum(int(v.sum()) for v in env.event_stats(True).values()) > 0
