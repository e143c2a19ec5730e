"""Every path of oc_multi_agent_step_sample against the references, by name: the cases of tests/sample_cases.py (held to the planner
and to the sources' instances by tests/test_host_train_sample.py), each asked of oc_multi_agent_step_sample_plan on this device, then
stepped as VecOvercookedMultiAgent.step_sampled.

What is compared, and how closely (each bound is derived in tests/sample_cases.py, none is chosen from a result):
  * the drawn actions equal the float64 reference's (sample_cases.sample_f64, the same u_p) except for samples inside the boundary
    band |u * S - c_i| <= 2^-18 * S, about five times the float32 error of a cumulative sum; at most BAND_CAP = 1e-3 of a case's
    samples may lie there.  Invalid rows (a NaN logit) are never in the band: action 255, exactly.  Argmax mode has no band: the
    actions are exactly the lowest-index maximum;
  * logp is within LOGP_TOL = 1e-5 of the float64 reference's log-probability of the action the kernel drew, NaN where that is 255;
  * every output of the step — rewards, flags, shaped, done, phi, episode returns, state, observation or features — equals
    train_cases.OracleTrainStep (and oracle.featurize / the lossless encoding) fed the actions the kernel wrote, at zero tolerance as
    in tests/test_gpu_train_instances.py; an invalid row shows OC_F_BAD_ACTION and leaves its env untouched (the reference does).
Every array the call must overwrite completely is filled with a value no result holds before each step; the drawn actions, their
log-probabilities, the observation and the features lie between guard rows, off the base of their allocation as far as the header's
alignment rules allow (actions 2-byte, logp 8-byte aligned)."""
import numpy as np
import pytest

import sample_cases as SC
import train_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import FLAG_FILL, GUARD, REW_FILL, gpu, guarded, guards_untouched, no_sentinel, packed_counters  # noqa: E402, F401

F64_FILL = -12345.0  # no training reward, potential or feature holds it
OBS_CHUNK = 16384    # envs per comparison of the observation


class Guarded:
    """The env's persistent outputs replaced by sentinel-filled arrays between guard rows; fill(): sentinels before a step."""

    def __init__(self, env, case, table, dt, device):
        from overcooked_ai_amd import _lib

        self.env, self.case, self.guards, self.obs_fill = env, case, [], None
        n = case.n_envs
        actions, g = guarded(n, (2,), torch.uint8, FLAG_FILL, device, before=3)
        self.guards.append(("drawn actions", g, FLAG_FILL))
        logp, g = guarded(n, (2,), torch.float32, REW_FILL, device, before=3)
        self.guards.append(("log-probabilities", g, REW_FILL))
        assert actions.data_ptr() % 4 == 2 and logp.data_ptr() % 16 == 8
        env._sampled = (actions, logp, _lib.OcActionSampler())
        if case.obs in ("u8", "f32"):
            self.obs_fill = FLAG_FILL if dt == torch.uint8 else REW_FILL
            row_bytes = 2 * table.width * table.height * 26 * torch.empty((), dtype=dt).element_size()
            before = next(r for r in range(GUARD, GUARD + 4) if r * row_bytes % 16 == 0)
            env._obs, g = guarded(n, (2, table.width, table.height, 26), dt, self.obs_fill, device, before=before)
            assert env._obs.data_ptr() % 16 == 0 and env._obs_buffer() is env._obs
            self.guards.append(("observation", g, self.obs_fill))
        if case.obs == "features":
            env._feat, g = guarded(n, (2, SC.total_of(case.num_pots)), torch.float32, F64_FILL, device, before=GUARD)
            assert env._feat.data_ptr() % 16 == 0 and env._feat_buffer() is env._feat
            self.guards.append(("features", g, F64_FILL))

    def fill(self):
        env, v = self.env, self.env.venv
        env._sampled[0].fill_(FLAG_FILL)
        env._sampled[1].fill_(REW_FILL)
        env.shaped.fill_(F64_FILL)
        env.done.fill_(FLAG_FILL)
        if self.case.use_phi:
            env.phi_next.fill_(F64_FILL)
        v.rewards.fill_(REW_FILL)
        v.flags.fill_(FLAG_FILL)
        if self.obs_fill is not None:
            env._obs.fill_(self.obs_fill)
        if self.case.obs == "features":
            env._feat.fill_(F64_FILL)

    def untouched(self):
        for what, g, fill in self.guards:
            guards_untouched(self.case, what, g, fill)


def run_case(case, gpu, two_calls=False, collect=False):
    """Steps the case, every output compared at every step.  two_calls: sample_actions() (oc_sample_actions), then step(), in the
    place of step_sampled(); collect: also returns every step's outputs (numpy), for a comparison of two runs."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    plan = SC.plan_of_case(case)
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    table = TC.table_of(case.table)
    dt = {"u8": torch.uint8, "f32": torch.float32}.get(case.obs)
    env = VecOvercookedMultiAgent(table, case.n_envs, device=gpu, obs_dtype=dt, **SC.env_kwargs(case))
    assert env.plan_sampled() == plan, (case.id, env.plan_sampled(), plan)
    assert env.sample_step == 0
    env.sample_step = case.step0
    out = Guarded(env, case, table, dt, gpu)
    ref = SC.oracle_of(case)
    v = env.venv
    lid = lambda: None if ref.layout_id is None else ref.layout_id  # noqa: E731
    compare(case, -1, "state", v.get_packed_state(), ref.state, lid(), env_axis=1)
    in_band = samples = 0
    worst_logp = 0.0
    trace = []
    for t in range(case.steps):
        logits, u = SC.logits_of(case, t), SC.uniforms_of(case, t)
        d_logits = torch.from_numpy(logits).to(gpu)
        out.fill()
        if two_calls:
            acts, lp = env.sample_actions(d_logits, greedy=case.greedy)
            obs, shaped, done, infos = env.step(acts)
        else:
            obs, shaped, done, infos = env.step_sampled(d_logits, greedy=case.greedy)
            acts, lp = infos["actions"], infos["logp"]
        assert env.sample_step == case.step0 + t + 1
        assert acts.data_ptr() == env._sampled[0].data_ptr() and lp.data_ptr() == env._sampled[1].data_ptr()
        assert acts.dtype == torch.uint8 and acts.shape == (case.n_envs, 2) and lp.dtype == torch.float32 and lp.shape == (case.n_envs, 2)
        a, logp = acts.cpu().numpy(), lp.cpu().numpy()
        # ---- the draws
        a64, _, band = SC.sample_f64(logits, u, case.greedy)
        differ = a != a64
        valid = a != 255
        want_logp = SC.logp_f64(logits, np.where(valid, a, 0))
        err = np.abs(logp.astype(np.float64) - want_logp)[valid]
        worst_logp = max(worst_logp, float(err.max()))
        in_band += int(band.sum())
        samples += band.size
        print("%s step %d: %d of %d samples in the band, %d of them drawn differently, %d outside it; max |logp - reference| %.3g"
              % (case.id, t, band.sum(), band.size, (differ & band).sum(), (differ & ~band).sum(), err.max()))
        if (differ & ~band).any():
            e, p = (int(i[0]) for i in np.nonzero(differ & ~band))
            pytest.fail("%s: step %d, env %d, player %d: action %d, reference %d, logits %s, u %r" % (case.id, t, e, p, a[e, p], a64[e, p], logits[e, p], u[e, p]))
        assert not case.greedy or not band.any()
        assert err.max() <= SC.LOGP_TOL, (case.id, t, float(err.max()))
        assert np.isnan(logp[~valid]).all() and np.array_equal(~valid, np.isnan(logits).any(axis=-1))
        # ---- the step, fed the actions the kernel wrote
        ref.step(a, case.factor)
        no_sentinel(case, ref.rewards, ref.flags)
        assert not (ref.done == FLAG_FILL).any() and not (ref.shaped == F64_FILL).any(), case.id
        assert np.array_equal((ref.flags & 2) != 0, (~valid).any(axis=1))  # an invalid row: OC_F_BAD_ACTION (and the env untouched)
        fields = [("state", v.get_packed_state(), ref.state), ("rewards", v.rewards, ref.rewards), ("flags", v.flags, ref.flags),
                  ("ep_returns", v.ep_returns, ref.ep_returns), ("infos[ep_returns]", infos["ep_returns"], ref.ep_out),
                  ("shaped", shaped, ref.shaped), ("done", done, ref.done)]
        if case.use_phi:
            fields += [("phi_next", infos["phi_s_prime"], ref.phi_next), ("phi_cur", env.phi_cur, ref.phi_cur)]
        if ref.layout_id is not None:
            fields.append(("layout_id", v.layout_ids(), ref.layout_id))
        if case.obs == "features":
            assert obs.data_ptr() == env._feat.data_ptr()
            want = SC.features_of(case, ref)
            assert not (want == F64_FILL).any()
            fields.append(("features", obs, want))
        got_all = {"actions": a.copy(), "logp": logp.copy()}
        for field, got, want in fields:
            got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
            compare(case, t, field, got, want, lid(), env_axis=1 if field == "state" else 0)
            got_all[field] = got.copy()
        if case.events:
            for field, got, want in (("event counters, running", v.event_counts, ref.counts), ("event counters, published", v.event_counts_done, ref.counts_done)):
                compare(case, t, field, packed_counters(got), want, lid())
        if case.obs in ("u8", "f32"):
            assert obs.dtype == dt and obs.shape == (case.n_envs, 2, table.width, table.height, 26) and obs.data_ptr() == env._obs.data_ptr()
            for a0 in range(0, case.n_envs, OBS_CHUNK):
                a1 = min(case.n_envs, a0 + OBS_CHUNK)
                want = ref.obs(a0, a1)
                assert not (np.asarray(want) == out.obs_fill).any(), "%s: an oracle observation cell equals the fill" % case.id
                compare(case, t, "observation", obs[a0:a1].cpu().numpy(), want, lid(), e0=a0)
        out.untouched()
        trace.append(got_all)
    print("%s: %d of %d samples in the band (cap %g); max |logp - reference| %.3g (bound %g)"
          % (case.id, in_band, samples, SC.BAND_CAP * samples, worst_logp, SC.LOGP_TOL))
    assert in_band <= SC.BAND_CAP * samples, (case.id, in_band, samples)
    assert case.n_envs < 127 or (ref.flags & 2).any()  # (the last step, like every step of these batches, carries invalid rows)
    return trace if collect else None


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.id)
def test_every_path_of_the_sampled_training_step_against_the_references(case, gpu):
    run_case(case, gpu)


def test_the_far_counter_case_against_the_references(gpu):
    run_case(SC.far_case(), gpu)


def test_the_fused_kernel_and_oc_sample_actions_then_step_agree_bit_for_bit(gpu):
    """A fused case run a second time as oc_sample_actions + step on the same inputs: the actions, their log-probabilities and every
    output of every step are bit-equal (both runs are also held to the references)."""
    case = SC.by_id("feat_two_pots_ragged_last_workgroup")
    a, b = run_case(case, gpu, collect=True), run_case(case, gpu, two_calls=True, collect=True)
    assert len(a) == len(b) == case.steps
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for field in x:
            p, q = (np.ascontiguousarray(z).view(np.uint8) for z in (x[field], y[field]))
            assert np.array_equal(p, q), (t, field)


def test_a_sharded_batch_draws_what_the_whole_batch_draws(gpu):
    """488 envs as one batch, and as 200 + 288 envs with env offsets 0 / 200 on slices of the same logits: the same actions and
    log-probabilities, bit for bit, at every step."""
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    case = SC.by_id("feat_ragged_last_workgroup")
    table, n, cut, base = TC.table_of(case.table), 488, 200, 1000
    kw = dict(SC.env_kwargs(case), layout_id=None)
    envs = [(0, n, VecOvercookedMultiAgent(table, n, device=gpu, **dict(kw, env_offset=base))),
            (0, cut, VecOvercookedMultiAgent(table, cut, device=gpu, **dict(kw, env_offset=base))),
            (cut, n, VecOvercookedMultiAgent(table, n - cut, device=gpu, **dict(kw, env_offset=base + cut)))]
    for t in range(5):
        logits = SC.logits_of(case._replace(n_envs=n), t)
        got = []
        for e0, e1, env in envs:
            infos = env.step_sampled(torch.from_numpy(np.ascontiguousarray(logits[e0:e1])).to(gpu))[3]
            got.append((infos["actions"].cpu().numpy(), infos["logp"].cpu().numpy().view(np.uint32)))
        assert np.array_equal(got[0][0], np.concatenate([got[1][0], got[2][0]])), t
        assert np.array_equal(got[0][1], np.concatenate([got[1][1], got[2][1]])), t
        assert (got[0][0] == 255).any() and (got[0][0] < 6).any()
