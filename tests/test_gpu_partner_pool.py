"""oc_partner_pool_logits on the device: the cases of tests/pool_cases.py (held to the restatements on the CPU by
tests/test_host_partner_pool.py) on the env's own feature rows after tests/test_gpu_partner.py's random walk.

What is compared, and how closely:
  * seats and members equal the numpy restatement of the header's draw exactly;
  * every seated logit lies within partner_cases.mlp_bound (a-priori, valid for any float32 summation order) of the float64 reference
    with the weights of ITS member — the largest error / bound ratio of a test is printed;
  * for each member m the six floats are bit-equal to oc_partner_logits' with that one policy, the seats preset to
    where(member == m, seat, 255) and an all-zero done mask;
  * every other logit is bit-equal to the caller's fill; the logits sit 8 bytes off a 16-byte boundary; seats, members and the scratch
    (of exactly the planned size) lie between guard rows that come back untouched;
  * a second call, on fresh seat and member arrays and a scratch of other contents, gives the same bytes;
  * end to end: the draws against sample_cases on the logits as the kernels left them, the step against train_cases.OracleTrainStep
    at zero tolerance, as tests/test_gpu_partner.py does for the single policy."""
import ctypes
import re

import numpy as np
import pytest

import partner_cases as PC
import pool_cases as PP
import sample_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare, table_of  # noqa: E402
from gpu_support import gpu, guarded, guards_untouched, packed_counters  # noqa: E402, F401
from test_gpu_partner import LOGIT_GUARD, SEAT_GUARD, env_of, guarded_logits, guarded_seats, walk  # noqa: E402

SCRATCH_GUARD = 64  # bytes on either side of the scratch (its start stays 16-byte aligned)
WORST = {"ratio": 0.0}


def pool_of(c, device):
    """(PartnerPool, its policies, their host weights)"""
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool

    weights = PP.weights_of(c)
    policies = [DensePolicy(*w, device=device) for w in weights]
    return PartnerPool(policies, weights=c.weights), policies, weights


def guarded_members(env):
    member, g = guarded(env.n_envs, (), torch.uint8, SEAT_GUARD, env.venv.device, before=3)
    member.fill_(255)
    env.member = member
    return g


def guarded_scratch(env):
    n = env.pool_scratch.numel()
    whole = torch.full((SCRATCH_GUARD + n + SCRATCH_GUARD,), SEAT_GUARD, dtype=torch.uint8, device=env.venv.device)
    env.pool_scratch = whole[SCRATCH_GUARD:SCRATCH_GUARD + n]
    assert env.pool_scratch.data_ptr() % 16 == 0
    return whole[:SCRATCH_GUARD], whole[SCRATCH_GUARD + n:]


def check_logits(c, what, got, fill, feats, seat, member, weights):
    """Seated rows within the bound of the float64 reference of their member on feats[e, seat[e]], everything else bit-equal to the fill."""
    got, fill = np.asarray(got), np.asarray(fill)
    seated = np.nonzero(seat != PC.NO_SEAT)[0]
    p = seat[seated].astype(np.int64)
    untouched = np.ones(got.shape[:2], bool)
    untouched[seated, p] = False
    same = got.view(np.uint32)[untouched] == fill.view(np.uint32)[untouched]
    assert same.all(), "%s %s: %d logits outside the partner seats were written" % (c.id, what, (~same).sum())
    assert ((member == PP.NO_MEMBER) == (seat == PC.NO_SEAT)).all() and (member[seated] < len(weights)).all()
    worst = 0.0
    for m in np.unique(member[seated]):
        rows = seated[member[seated] == m]
        x = feats[rows, seat[rows]]
        ref, _ = PC.mlp_f64(x, weights[m])
        bound = PC.mlp_bound(x, weights[m])
        mine = got[rows, seat[rows]]
        err = np.abs(mine.astype(np.float64) - ref)
        assert np.isfinite(mine).all() and (err <= bound).all(), (c.id, what, int(m), float((err / bound).max()))
        assert not (mine == fill[rows, seat[rows]]).all()
        worst = max(worst, float((err / bound).max()))
    WORST["ratio"] = max(WORST["ratio"], worst)
    print("%s %s: %d seated rows of %d member(s), largest error / bound %.3g (largest so far %.3g)"
          % (c.id, what, len(seated), len(np.unique(member[seated])), worst, WORST["ratio"]))


def single_policy_logits(env, c, policy, seat, fill):
    """oc_partner_logits with one policy on the env's feature buffer: the seats preset, an all-zero done mask -> logits [n, 2, 6]"""
    from overcooked_ai_amd import _lib

    v = env.venv
    d_seat = torch.from_numpy(np.ascontiguousarray(seat)).to(v.device)
    done = torch.zeros((c.n_envs,), dtype=torch.uint8, device=v.device)
    logits = torch.from_numpy(fill).to(v.device)
    s = _lib.OcPartnerSeats(d_seat.data_ptr(), done.data_ptr(), float(c.bc_factor), v.seed, v.env_offset, c.step)
    rc = v._launch(v.lib.oc_partner_logits, v._bref, policy._ref, ctypes.byref(s), env._feat_buffer().data_ptr(), c.num_pots, logits.data_ptr())
    _lib.check(rc, "oc_partner_logits")
    assert np.array_equal(d_seat.cpu().numpy(), seat)
    return logits.cpu().numpy()


def pool_call(env, c, pool, fill, scratch_byte):
    """oc_partner_pool_logits through the C-ABI on fresh seat and member arrays (every env is reseated) and a scratch filled with
    `scratch_byte` -> (seat, member, logits)"""
    from overcooked_ai_amd import _lib

    v = env.venv
    seat = torch.full((c.n_envs,), 255, dtype=torch.uint8, device=v.device)
    member = torch.full((c.n_envs,), 255, dtype=torch.uint8, device=v.device)
    scratch = torch.full((env.pool_scratch.numel(),), scratch_byte, dtype=torch.uint8, device=v.device)
    logits = torch.from_numpy(fill).to(v.device)
    s = _lib.OcPartnerSeats(seat.data_ptr(), None, float(c.bc_factor), v.seed, v.env_offset, c.step)
    p = pool.struct_for(member)
    rc = v._launch(v.lib.oc_partner_pool_logits, v._bref, ctypes.byref(p), ctypes.byref(s), env._feat_buffer().data_ptr(), c.num_pots,
                   logits.data_ptr(), scratch.data_ptr())
    _lib.check(rc, "oc_partner_pool_logits")
    return seat.cpu().numpy(), member.cpu().numpy(), logits.cpu().numpy()


def run_call(c, gpu):
    """partner_logits alone on a fresh env of the case after the random walk, everything guarded."""
    pool, policies, weights = pool_of(c, gpu)
    env = env_of(c, gpu, pool)
    plan = env.plan_partner()
    blocks = (c.n_envs + 255) // 256
    assert plan.startswith("k_pool_seat grid=%d, " % blocks) and "k_pool_logits grid=%d (" % (blocks + c.n_members) in plan
    assert env.pool_scratch.numel() == int(re.search(r"scratch (\d+) B", plan).group(1)) == 1092 + 4 * c.n_members * blocks + 4 * c.n_envs
    assert bool((env.seat == 255).all()) and bool((env.member == 255).all())
    if "more_chunks_than_cus" in c.claims:  # (the case list counts on the MI355X's CUs for the path of more than two passes)
        assert torch.cuda.get_device_properties(gpu).multi_processor_count == PP.MI355X_CUS
    feats = walk(env, c)
    guards = {"seats": guarded_seats(env), "members": guarded_members(env), "scratch": guarded_scratch(env)}
    fill = PC.logits_fill(c.n_envs)
    logits, guards["logits"] = guarded_logits(fill, gpu, shift=2)
    assert logits.data_ptr() % 16 == 8
    step = env.sample_step
    got_seat = env.partner_logits(logits)
    assert env.sample_step == step and got_seat.data_ptr() == env.seat.data_ptr()
    seat, member = env.seat.cpu().numpy(), env.member.cpu().numpy()
    nobody = np.full(c.n_envs, 255, np.uint8)
    want_seat, want_member = PP.redraw(nobody, nobody, None, c.seed, c.env_offset, c.step, c.bc_factor, PP.thresholds_of(c))
    assert np.array_equal(seat, want_seat), (c.id, np.nonzero(seat != want_seat)[0][:5])
    assert np.array_equal(member, want_member), (c.id, np.nonzero(member != want_member)[0][:5])
    assert np.array_equal(seat, PC.seats(c.seed, c.env_offset, c.step, c.n_envs, c.bc_factor))  # the single-policy stream's
    got = logits.cpu().numpy()
    check_logits(c, "call", got, fill, feats, seat, member, weights)
    for what, g in guards.items():
        guards_untouched(c, what, g, LOGIT_GUARD if what == "logits" else SEAT_GUARD)
    assert np.array_equal(env.observations("features").cpu().numpy(), feats)  # (the call reads the features)
    return env, pool, policies, weights, feats, seat, member, logits, fill


ALL = PP.CASES + (PP.far_case(),)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.id)
def test_draws_logits_guards_and_the_repeat_of_every_case(c, gpu):
    env, pool, policies, weights, feats, seat, member, logits, fill = run_call(c, gpu)
    got = logits.cpu().numpy()
    # ---- member by member: oc_partner_logits with that one policy at that member's rows
    for m in range(c.n_members):
        mine = np.where(member == m, seat, 255).astype(np.uint8)
        single = single_policy_logits(env, c, policies[m], mine, fill)
        rows = np.nonzero(member == m)[0]
        assert np.array_equal(single[rows, seat[rows]].view(np.uint32), got[rows, seat[rows]].view(np.uint32)), (c.id, m)
        rest = np.ones(got.shape[:2], bool)
        rest[rows, seat[rows]] = False
        assert np.array_equal(single.view(np.uint32)[rest], fill.view(np.uint32)[rest]), (c.id, m)
    # ---- again, on fresh arrays and scratches of other contents
    for byte in (0x00, 0x55):
        s2, m2, l2 = pool_call(env, c, pool, fill, byte)
        assert np.array_equal(s2, seat) and np.array_equal(m2, member) and np.array_equal(l2.view(np.uint32), got.view(np.uint32)), (c.id, byte)
    if c.id.endswith("@far"):  # (what the device drew is none of the truncated streams)
        for drop in ("t_hi", "g_hi", "seed_hi", "tweak"):
            assert (member != PP.draws(c.seed, c.env_offset, c.step, c.n_envs, c.bc_factor, PP.thresholds_of(c), drop=drop)[1]).any(), drop


def test_one_member_is_oc_partner_logits_bit_for_bit(gpu):
    from overcooked_ai_amd.partner import DensePolicy

    c = next(c for c in PP.CASES if c.n_members == 1)
    env, pool, policies, weights, feats, seat, member, logits, fill = run_call(c, gpu)
    single = env_of(c, gpu, DensePolicy(*weights[0], device=gpu))
    assert np.array_equal(walk(single, c), feats)
    theirs = torch.from_numpy(fill).to(gpu)
    single.partner_logits(theirs)
    assert np.array_equal(single.seat.cpu().numpy(), seat) and set(np.unique(member)) == {0, 255}
    assert np.array_equal(theirs.cpu().numpy().view(np.uint32), logits.cpu().numpy().view(np.uint32))
    assert (seat != 255).any() and not hasattr(single, "member")


def test_a_done_mask_redraws_its_envs_and_no_others(gpu):
    """A second call with a done mask written by hand: a third of the envs (any non-zero byte counts), at another step."""
    c = next(c for c in PP.CASES if (c.n_envs, c.n_members, c.bc_factor, c.num_pots) == (488, 3, 0.5, 2))
    env, pool, policies, weights, feats, first_seat, first_member, logits, _ = run_call(c, gpu)
    done = ((np.arange(c.n_envs) % 3 == 0) * (1 + np.arange(c.n_envs) % 250)).astype(np.uint8)
    env.done.copy_(torch.from_numpy(done).to(gpu))
    env.sample_step = c.step + 3
    fill = PC.logits_fill(c.n_envs)[::-1].copy()
    logits.copy_(torch.from_numpy(fill))
    env.partner_logits(logits)
    seat, member = env.seat.cpu().numpy(), env.member.cpu().numpy()
    want_seat, want_member = PP.redraw(first_seat, first_member, done, c.seed, c.env_offset, c.step + 3, c.bc_factor, PP.thresholds_of(c))
    assert np.array_equal(seat, want_seat) and np.array_equal(member, want_member)
    assert np.array_equal(seat[done == 0], first_seat[done == 0]) and np.array_equal(member[done == 0], first_member[done == 0])
    assert (member != first_member).any() and ((member == 255) == (seat == 255)).all()
    check_logits(c, "second call", logits.cpu().numpy(), fill, feats, seat, member, weights)


def test_two_episodes_of_step_sampled_with_a_pool_end_to_end(gpu):
    """The fused case of tests/test_gpu_partner.py's end-to-end test (horizon 11, 25 steps: two episode ends) with a pool of three."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool

    case = SC.by_id("feat_ragged_last_workgroup")
    weights = [PC.glorot(case.seed + m, PC.total_of(case.num_pots), *PP.SHAPES[m]) for m in range(3)]
    pool = PartnerPool([DensePolicy(*w, device=gpu) for w in weights])
    thr = PP.uniform_thresholds(3)
    env = VecOvercookedMultiAgent(table_of(case.table), case.n_envs, device=gpu, bc_policy=pool, **SC.env_kwargs(case))
    env.set_bc_factor(0.5)
    plan = env.plan_sampled()
    assert plan == SC.plan_of_case(case) and plan.startswith("k_train_step_feat<MAXP=1, SAMPLE=true>"), plan
    ref = SC.oracle_of(case)
    v = env.venv
    seat, member, done = np.full(case.n_envs, 255, np.uint8), np.full(case.n_envs, 255, np.uint8), None
    in_band = samples = changes = ends = 0
    for t in range(case.steps):
        fill, u = SC.logits_of(case, t), SC.uniforms_of(case, t)
        feats = env.observations("features").cpu().numpy().copy()
        d_logits = torch.from_numpy(fill).to(gpu)
        obs, shaped, d, infos = env.step_sampled(d_logits, greedy=case.greedy)
        logits = d_logits.cpu().numpy()  # as the kernels left them
        # ---- the partners
        want_seat, want_member = PP.redraw(seat, member, done, case.seed, case.env_offset, case.step0 + t, 0.5, thr)
        got_seat, got_member = infos["seat"].cpu().numpy(), infos["member"].cpu().numpy()
        assert infos["member"].data_ptr() == env.member.data_ptr() and infos["seat"].data_ptr() == env.seat.data_ptr()
        assert np.array_equal(got_seat, want_seat) and np.array_equal(got_member, want_member), t
        if done is not None:
            assert (got_member == member)[done == 0].all() and (got_seat == seat)[done == 0].all(), t  # changes at episode ends only
            changes += int((got_member != member).sum())
            ends += int(done.any())
        check_logits(case, "step %d" % t, logits, fill, feats, got_seat, got_member, weights)
        assert not (np.isnan(logits) & ~np.isnan(fill)).any()
        # ---- the draws, from the logits as the kernels left them
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
        seat, member, done = got_seat, got_member, d.cpu().numpy().copy()
    assert in_band <= SC.BAND_CAP * samples and ends >= 2 and changes > 0
    assert set(np.unique(member)) == {0, 1, 2, 255}


def test_a_sharded_batch_draws_and_computes_what_the_whole_batch_does(gpu):
    """488 envs as one batch, and as 200 + 288 envs with env offsets on slices of the same logits: the same seats, members and
    logits, bit for bit."""
    c = next(c for c in PP.CASES if (c.n_envs, c.n_members, c.bc_factor, c.num_pots) == (488, 3, 0.5, 2))
    pool, _, _ = pool_of(c, gpu)
    fill = PC.logits_fill(c.n_envs)
    got = []
    for e0, e1 in ((0, 488), (0, 200), (200, 488)):
        env = env_of(c, gpu, pool, n=e1 - e0, e0=e0)
        walk(env, c, e0=e0, n_all=c.n_envs)
        logits = torch.from_numpy(np.ascontiguousarray(fill[e0:e1])).to(gpu)
        env.partner_logits(logits)
        got.append((env.seat.cpu().numpy(), env.member.cpu().numpy(), logits.cpu().numpy().view(np.uint32)))
    for k in range(3):
        assert np.array_equal(got[0][k], np.concatenate([got[1][k], got[2][k]])), k
    assert (got[0][0] != 255).any() and (got[0][2] != fill.view(np.uint32)).any() and len(np.unique(got[0][1])) == 4


def test_set_member_changes_that_members_rows_and_no_others(gpu):
    from overcooked_ai_amd.partner import DensePolicy

    c = next(c for c in PP.CASES if (c.n_envs, c.n_members, c.bc_factor, c.num_pots) == (488, 3, 1.0, 2))
    env, pool, policies, weights, feats, seat, member, logits, fill = run_call(c, gpu)
    before = logits.cpu().numpy()
    weights[1] = PC.glorot(77, PC.total_of(c.num_pots), 17, 64)
    pool.set_member(1, DensePolicy(*weights[1], device=gpu))
    env.done.zero_()  # nobody is reseated: the same seats and members under the new member 1
    logits.copy_(torch.from_numpy(fill))
    env.partner_logits(logits)
    after = logits.cpu().numpy()
    assert np.array_equal(env.seat.cpu().numpy(), seat) and np.array_equal(env.member.cpu().numpy(), member)
    check_logits(c, "after set_member", after, fill, feats, seat, member, weights)
    rows = np.nonzero(member == 1)[0]
    changed = (after.view(np.uint32) != before.view(np.uint32)).any(axis=-1)
    assert changed[rows, seat[rows]].all() and changed.sum() == len(rows) > 0
