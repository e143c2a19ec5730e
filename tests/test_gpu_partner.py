"""oc_partner_logits on the device: the cases of tests/partner_cases.py (held to the references on the CPU by
tests/test_host_partner.py), the reseating over episodes, step_sampled with a partner end to end on a fused and an unfused plan, a
sharded batch, the no-partner paths and a far-counter case.

What is compared, and how closely:
  * the seats equal the numpy restatement of the header's seating stream exactly;
  * every seated logit lies within its own a-priori forward error bound (partner_cases.mlp_bound: valid for any float32 summation
    order, with or without fma; nothing in it comes from the kernel) of the float64 reference on the env's own float32 feature rows —
    the largest error / bound ratio of a test is printed;
  * every other logit is bit-equal to the caller's fill (a distinct finite value per element), and the guard rows around the logits
    (which sit 8 bytes off a 16-byte boundary where the call alone is tested: the header asks 8) and around the seats are untouched;
  * end to end: the draws against sample_cases.sample_f64 / logp_f64 on the logits AS THE KERNEL LEFT THEM, with the band and the
    tolerance of tests/test_gpu_train_sample.py, and every output of the step against train_cases.OracleTrainStep at zero tolerance."""
import numpy as np
import pytest

import partner_cases as PC
import sample_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import DRAWN, compare, table_of  # noqa: E402
from gpu_support import GUARD, gpu, guarded, guards_untouched, packed_counters  # noqa: E402, F401

LOGIT_GUARD = -777.0  # no fill value and no logit of these networks (|logit| < 100: bounded weights, features within +-100)
SEAT_GUARD = 0xEE
WORST = {"ratio": 0.0}


def policy_of(c, device):
    from overcooked_ai_amd.partner import DensePolicy

    return DensePolicy(*PC.weights_of(c), device=device)


def env_of(c, device, policy, n=None, e0=0, **over):
    """The env of a case (or of its envs e0 .. e0 + n): drawn start states, a short horizon, featurize_state of the next states from the
    step call."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    kw = dict(horizon=7, use_phi=False, seed=c.seed, env_offset=c.env_offset + e0, obs="features", num_pots=c.num_pots, bc_policy=policy, **DRAWN)
    kw.update(over)
    env = VecOvercookedMultiAgent(table_of(c.table), c.n_envs if n is None else n, device=device, **kw)
    env.set_bc_factor(c.bc_factor)
    env.sample_step = c.step
    return env


def walk(env, c, e0=0, n_all=None, steps=PC.STEPS_BEFORE):
    """STEPS_BEFORE random steps (the same actions for env e0 + e of a shard as for that env of the whole batch): restarts included, so
    the feature rows differ and carry held objects, pot states and negative distances."""
    rng = np.random.default_rng([c.seed, 0xAC7])
    for _ in range(steps):
        a = rng.integers(0, 6, size=(c.n_envs if n_all is None else n_all, 2)).astype(np.uint8)
        env.step(torch.from_numpy(np.ascontiguousarray(a[e0:e0 + env.n_envs])).to(env.venv.device))
    return env.observations("features").cpu().numpy().copy()


def guarded_logits(fill, device, shift):
    """The caller's logits between guard rows, `shift` floats off the allocation's base: (logits [n, 2, 6], guard slices)"""
    n, g = len(fill), GUARD * 12
    whole = torch.full((shift + g + n * 12 + g,), LOGIT_GUARD, dtype=torch.float32, device=device)
    body = whole[shift + g:shift + g + n * 12].view(n, 2, 6)
    body.copy_(torch.from_numpy(fill))
    return body, (whole[:shift + g], whole[shift + g + n * 12:])


def guarded_seats(env):
    seat, g = guarded(env.n_envs, (), torch.uint8, SEAT_GUARD, env.venv.device, before=3)
    seat.fill_(255)
    env.seat = seat
    return g


def check_logits(c, what, got, fill, feats, seat, weights):
    """Seated rows within the bound of the float64 reference on feats[e, seat[e]], everything else bit-equal to the fill."""
    got, fill = np.asarray(got), np.asarray(fill)
    seated = np.nonzero(seat != PC.NO_SEAT)[0]
    p = seat[seated].astype(np.int64)
    untouched = np.ones(got.shape[:2], bool)
    untouched[seated, p] = False
    same = got.view(np.uint32)[untouched] == fill.view(np.uint32)[untouched]
    assert same.all(), "%s %s: %d logits outside the partner seats were written" % (c.id, what, (~same).sum())
    if len(seated) == 0:
        return 0.0
    x = feats[seated, p]
    ref, _ = PC.mlp_f64(x, weights)
    bound = PC.mlp_bound(x, weights)
    err = np.abs(got[seated, p].astype(np.float64) - ref)
    ratio = float((err / bound).max())
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("%s %s: %d seated rows, largest error %.3g, largest error / bound %.3g (largest so far %.3g)"
          % (c.id, what, len(seated), err.max(), ratio, WORST["ratio"]))
    assert np.isfinite(got[seated, p]).all() and (err <= bound).all(), (c.id, what, ratio)
    assert not (got[seated, p] == fill[seated, p]).all()
    return ratio


def run_call(c, gpu):
    """partner_logits alone on a fresh env of the case after the random walk."""
    policy = policy_of(c, gpu)
    env = env_of(c, gpu, policy)
    plan = env.plan_partner()
    assert plan.startswith("k_partner_logits grid=%d, " % ((c.n_envs + 255) // 256)) and "K %d -> 64 -> 64 -> 32" % PC.total_of(c.num_pots) in plan
    assert bool((env.seat == 255).all())
    feats = walk(env, c)
    assert len(np.unique(feats.reshape(-1, feats.shape[-1]), axis=0)) > min(c.n_envs, 3) - 1 and (c.n_envs < 33 or (feats < 0).any())
    seat_guards = guarded_seats(env)
    fill = PC.logits_fill(c.n_envs)
    logits, logit_guards = guarded_logits(fill, gpu, shift=2)
    assert logits.data_ptr() % 16 == 8
    step = env.sample_step
    got_seat = env.partner_logits(logits)
    assert env.sample_step == step and got_seat.data_ptr() == env.seat.data_ptr()
    seat = env.seat.cpu().numpy()
    want = PC.reseat(np.full(c.n_envs, 255, np.uint8), None, c.seed, c.env_offset, c.step, c.bc_factor)
    assert np.array_equal(seat, want), (c.id, np.nonzero(seat != want)[0][:5])
    if c.bc_factor == 0.0:
        assert (seat == 255).all()
    if c.bc_factor == 1.0:
        assert (seat != 255).all()
    check_logits(c, "call", logits.cpu().numpy(), fill, feats, seat, policy.weights())
    guards_untouched(c, "logits", logit_guards, LOGIT_GUARD)
    guards_untouched(c, "seats", seat_guards, SEAT_GUARD)
    assert np.array_equal(env.observations("features").cpu().numpy(), feats)  # (the call reads the features)
    return env, policy, feats, seat, logits


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_seats_and_logits_of_every_case(c, gpu):
    run_call(c, gpu)


def test_the_far_counter_case(gpu):
    c = PC.far_case()
    _, _, _, seat, _ = run_call(c, gpu)
    for drop in ("t_hi", "g_hi", "carry", "seed_hi", "tweak"):  # (what the device drew is none of the truncated streams)
        assert (seat != PC.seats(c.seed, c.env_offset, c.step, c.n_envs, c.bc_factor, drop=drop)).any(), drop


def test_a_done_mask_reseats_its_envs_and_no_others(gpu):
    """A second call with a done mask written by hand: a third of the envs (any non-zero byte counts), at another step."""
    c = next(c for c in PC.CASES if c.n_envs == 488 and c.bc_factor == 0.5 and c.num_pots == 2)
    env, policy, feats, first, logits = run_call(c, gpu)
    done = ((np.arange(c.n_envs) % 3 == 0) * (1 + np.arange(c.n_envs) % 250)).astype(np.uint8)
    env.done.copy_(torch.from_numpy(done).to(gpu))
    env.sample_step = c.step + 3
    fill = PC.logits_fill(c.n_envs)[::-1].copy()
    logits.copy_(torch.from_numpy(fill))
    env.partner_logits(logits)
    seat = env.seat.cpu().numpy()
    want = PC.reseat(first, done, c.seed, c.env_offset, c.step + 3, c.bc_factor)
    assert np.array_equal(seat, want) and np.array_equal(seat[done == 0], first[done == 0]) and (seat != first).any()
    check_logits(c, "second call", logits.cpu().numpy(), fill, feats, seat, policy.weights())


def test_seats_change_at_episode_ends_only_and_reset_reseats_everyone(gpu):
    """Horizon 5, 12 step_sampled calls, bc_factor 0.5: after every call the seats are the restatement driven by the done masks the
    env produced; then reset(), after which every env is redrawn at the current sample_step."""
    c = next(c for c in PC.CASES if c.n_envs == 488 and c.bc_factor == 0.5 and c.num_pots == 2)
    policy = policy_of(c, gpu)
    env = env_of(c, gpu, policy, horizon=5)
    rng = np.random.default_rng(7)
    seat, done, changes = np.full(c.n_envs, 255, np.uint8), None, 0
    for t in range(12):
        feats = env.observations("features").cpu().numpy().copy()
        fill = (rng.standard_normal((c.n_envs, 2, 6)) * 2).astype(np.float32)
        logits = torch.from_numpy(fill).to(gpu)
        want = PC.reseat(seat, done, c.seed, c.env_offset, c.step + t, c.bc_factor)
        assert env.sample_step == c.step + t
        _, _, d, infos = env.step_sampled(logits)
        got = infos["seat"].cpu().numpy()
        assert infos["seat"].data_ptr() == env.seat.data_ptr() and np.array_equal(got, want), t
        if done is not None:
            assert (got == seat)[done == 0].all(), t  # a seat changes only where the previous done was set
            changes += int((got != seat).sum())
        check_logits(c, "step %d" % t, logits.cpu().numpy(), fill, feats, got, policy.weights())
        seat, done = got, d.cpu().numpy().copy()
        assert done.all() == (t % 5 == 4)
    assert changes > 0
    env.reset()
    logits = torch.from_numpy(PC.logits_fill(c.n_envs)).to(gpu)
    env.partner_logits(logits)
    assert env.sample_step == c.step + 12
    assert np.array_equal(env.seat.cpu().numpy(), PC.seats(c.seed, c.env_offset, c.step + 12, c.n_envs, c.bc_factor))


def sampled_case(which):
    """One case of sample_cases for each kind of plan, with the feature observation a partner needs."""
    if which == "fused":
        return SC.by_id("feat_ragged_last_workgroup"), "k_train_step_feat<MAXP=1, SAMPLE=true>"
    return SC.by_id("unfused_event_sink")._replace(obs="features"), "k_sample_actions + k_train_step<UNIFORM=true, EV=true>"


@pytest.mark.parametrize("which", ("fused", "unfused"))
def test_step_sampled_with_a_partner_end_to_end(which, gpu):
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy

    case, expect = sampled_case(which)
    weights = PC.glorot(case.seed, PC.total_of(case.num_pots), 64, 64)
    policy = DensePolicy(*weights, device=gpu)
    env = VecOvercookedMultiAgent(table_of(case.table), case.n_envs, device=gpu, bc_policy=policy, **SC.env_kwargs(case))
    env.set_bc_factor(0.5)
    plan = env.plan_sampled()
    assert plan == SC.plan_of_case(case) and plan.startswith(expect), plan
    ref = SC.oracle_of(case)
    v = env.venv
    seat, done = np.full(case.n_envs, 255, np.uint8), None
    in_band = samples = 0
    for t in range(case.steps):
        fill, u = SC.logits_of(case, t), SC.uniforms_of(case, t)
        feats = env.observations("features").cpu().numpy().copy()
        d_logits = torch.from_numpy(fill).to(gpu)
        obs, shaped, d, infos = env.step_sampled(d_logits, greedy=case.greedy)
        logits = d_logits.cpu().numpy()  # as the kernel left them
        # ---- the partner
        want_seat = PC.reseat(seat, done, case.seed, case.env_offset, case.step0 + t, 0.5)
        got_seat = infos["seat"].cpu().numpy()
        assert np.array_equal(got_seat, want_seat), t
        check_logits(case, "step %d" % t, logits, fill, feats, got_seat, weights)  # (untouched: by bit pattern, NaN and -inf included)
        assert not (np.isnan(logits) & ~np.isnan(fill)).any()  # (the partner writes no NaN; a seat may overwrite one)
        # ---- the draws, from the logits as the kernel left them
        a, logp = infos["actions"].cpu().numpy(), infos["logp"].cpu().numpy()
        a64, _, band = SC.sample_f64(logits, u, case.greedy)
        differ, valid = a != a64, a != 255
        assert not (differ & ~band).any(), (case.id, t, np.nonzero(differ & ~band))
        err = np.abs(logp.astype(np.float64) - SC.logp_f64(logits, np.where(valid, a, 0)))[valid]
        assert err.max() <= SC.LOGP_TOL, (case.id, t, float(err.max()))
        assert np.isnan(logp[~valid]).all() and np.array_equal(~valid, np.isnan(logits).any(axis=-1))
        in_band += int(band.sum())
        samples += band.size
        # ---- the step, fed the actions the kernel wrote
        ref.step(a, case.factor)
        fields = [("state", v.get_packed_state(), ref.state), ("rewards", v.rewards, ref.rewards), ("flags", v.flags, ref.flags),
                  ("ep_returns", v.ep_returns, ref.ep_returns), ("infos[ep_returns]", infos["ep_returns"], ref.ep_out),
                  ("shaped", shaped, ref.shaped), ("done", d, ref.done), ("features", obs, SC.features_of(case, ref))]
        if case.use_phi:
            fields += [("phi_next", infos["phi_s_prime"], ref.phi_next), ("phi_cur", env.phi_cur, ref.phi_cur)]
        for field, got, want in fields:
            got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
            compare(case, t, field, got, want, None, env_axis=1 if field == "state" else 0)
        if case.events:
            compare(case, t, "event counters, running", packed_counters(v.event_counts), ref.counts, None)
            compare(case, t, "event counters, published", packed_counters(v.event_counts_done), ref.counts_done, None)
        seat, done = got_seat, d.cpu().numpy().copy()
    assert in_band <= SC.BAND_CAP * samples
    assert (seat != 255).any() and (seat == 255).any()


def test_a_sharded_batch_seats_and_computes_what_the_whole_batch_does(gpu):
    """488 envs as one batch, and as 200 + 288 envs with env offsets on slices of the same logits: the same seats and the same
    logits, bit for bit."""
    c = next(c for c in PC.CASES if c.n_envs == 488 and c.bc_factor == 0.5 and c.num_pots == 2)
    policy = policy_of(c, gpu)
    fill = PC.logits_fill(c.n_envs)
    got = []
    for e0, e1 in ((0, 488), (0, 200), (200, 488)):
        env = env_of(c, gpu, policy, n=e1 - e0, e0=e0)
        walk(env, c, e0=e0, n_all=c.n_envs)
        logits = torch.from_numpy(np.ascontiguousarray(fill[e0:e1])).to(gpu)
        env.partner_logits(logits)
        got.append((env.seat.cpu().numpy(), logits.cpu().numpy().view(np.uint32)))
    assert np.array_equal(got[0][0], np.concatenate([got[1][0], got[2][0]]))
    assert np.array_equal(got[0][1], np.concatenate([got[1][1], got[2][1]]))
    assert (got[0][0] != 255).any() and (got[0][1] != fill.view(np.uint32)).any()


def _np(x):
    return x.cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.array(x)


def _trace(env, case, steps=6):
    out = []
    for t in range(steps):
        fill = SC.logits_of(case, t)
        d_logits = torch.from_numpy(fill).to(env.venv.device)
        obs, shaped, d, infos = env.step_sampled(d_logits)
        assert np.array_equal(d_logits.cpu().numpy().view(np.uint32), fill.view(np.uint32)), t  # the logits come back bit-identical
        out.append([_np(x) for x in (obs, shaped, d, infos["actions"], infos["logp"], env.venv.rewards, env.venv.flags,
                                     env.venv.get_packed_state(), env.seat)])
    return out


def test_without_a_partner_nothing_changes(gpu):
    """bc_factor 0: the logits come back bit-identical and every result of step_sampled equals that of an env built without a
    policy on the same seed; bc_policy None: the plan is the step's own and infos carries no seat."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy

    case = SC.by_id("feat_ragged_last_workgroup")
    policy = DensePolicy(*PC.glorot(1, PC.total_of(case.num_pots), 64, 64), device=gpu)
    kw = SC.env_kwargs(case)
    plain = VecOvercookedMultiAgent(table_of(case.table), case.n_envs, device=gpu, **kw)
    assert plain.bc_policy is None and plain.plan_sampled() == SC.plan_of_case(case) and bool((plain.seat == 255).all())
    with pytest.raises(ValueError):
        plain.plan_partner()
    seated = VecOvercookedMultiAgent(table_of(case.table), case.n_envs, device=gpu, bc_policy=policy, **kw)
    assert seated.bc_factor == 0 and seated.plan_sampled() == plain.plan_sampled()
    a, b = _trace(plain, case), _trace(seated, case)
    for t, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            assert np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)), (t, i)
    assert bool((seated.seat == 255).all())
    infos = plain.step_sampled(torch.from_numpy(SC.logits_of(case, 6)).to(gpu))[3]
    assert "seat" not in infos
