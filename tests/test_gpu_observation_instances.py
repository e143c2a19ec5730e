"""Every kernel instance of the observation path against the C oracle alone, by name: the cases of tests/obs_cases.py (held to the
planner and to the sources' instances by tests/test_host_observation_instances.py), each asked of oc_observation_plan on this
device, then run as a VecOvercookedEnv call — encode_lossless, rollout_encode (random policy or caller actions, trajectory or one
buffer), step_encode — beside obs_cases.OracleRun.  Nothing on the reference side is computed by the library: a mistake the single
kernel shares with the one-step kernels (enc_object_writes, the template, the item offsets) does not pass.

The tolerance is zero, and it is derived, not chosen: the transition, the Philox draws, the restart draws and the encoding are
integer work; an f32 observation holds integers of at most 255 and the rewards are small integers, both exact in float32.  So
every array is compared with np.array_equal.  Every output array is pre-filled with a value no result holds (0xEE; -7.0) and has
guard rows behind it that must come back untouched."""
import numpy as np
import pytest

import obs_cases as OC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import compare  # noqa: E402
from gpu_support import gpu, guarded, guards_untouched  # noqa: E402, F401

OBS_CHUNK_BYTES = 70 << 20  # the oracle's int32 image of one comparison of the observation: at most ~70 MB


def _compare_obs(case, k, obs, ref):
    """obs: tensor [n_envs, 2, W, H, 26] of the states `ref` is at, in env chunks of at most OBS_CHUNK_BYTES of reference"""
    per_env = obs[0].numel() * 4
    chunk = max(1, OBS_CHUNK_BYTES // per_env)
    for a in range(0, case.n_envs, chunk):
        b = min(case.n_envs, a + chunk)
        want = ref.obs(a, b)
        compare(case, k, "observation", obs[a:b].cpu().numpy(), want.astype(np.float32) if case.dtype == "f32" else want.astype(np.uint8),
                 ref.layout_id, e0=a)
        assert int(want.max()) <= 255


@pytest.mark.parametrize("case", OC.CASES, ids=lambda c: c.id)
def test_every_observation_instance_against_the_oracle(case, gpu):
    observation_case_against_the_oracle(case, gpu)


def observation_case_against_the_oracle(case, gpu, epoch0=None):
    """epoch0: the epoch the case's calls start from (the env's own counter, set after its construction; the oracle's run likewise)."""
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    table = OC.table_of(case.table)
    n, K, W, H = case.n_envs, case.n_steps, table.width, table.height
    tdt, fill = (torch.uint8, 0xEE) if case.dtype == "u8" else (torch.float32, -7.0)
    env = VecOvercookedEnv(table, n, device=gpu, **OC.env_kwargs(case))
    env.one_kernel = True
    env.set_packed_state(OC.states_of(case).copy())
    env.t_global = case.t0
    if epoch0 is not None:
        env._epoch = epoch0
    ref = OC.OracleRun(case, epoch0)
    lid = ref.layout_id
    acts = OC.actions_of(case)
    single = case.expect.startswith("k_rollout_encode<")

    # 1. the plan of the call, on this device: the instance the case is there for; the single kernel within the LDS the runtime reports
    plan = env.plan_observation(1 if case.call == "step_encode" else K, tdt, actions=acts is not None,
                                single_buffer=case.call == "rollout_single_buffer", step_encode=case.call == "step_encode")
    assert plan.startswith(case.expect), "%s is planned as\n  %s\nand is there for\n  %s" % (case.id, plan, case.expect)
    if single:
        assert plan.endswith(" B (queried)"), plan

    if case.call == "encode":
        out, guard = guarded(n, (2, W, H, 26), tdt, fill, gpu)
        assert env.encode_lossless(tdt, out=out) is out
        _compare_obs(case, 0, out, ref)
        guards_untouched(case, "observation", guard, fill)
        compare(case, 0, "state", env.get_packed_state(), ref.state, lid, env_axis=1)
        return

    rows = 1 if case.call in ("rollout_single_buffer", "step_encode") else K
    obs, g_obs = guarded(rows * n, (2, W, H, 26), tdt, fill, gpu)
    rew, g_rew = guarded(K * n, (4,), torch.float32, -7.0, gpu)
    fl, g_fl = guarded(K * n, (), torch.uint8, 0xEE, gpu)
    rew, fl = rew.view(K, n, 4), fl.view(K, n)
    d_acts = None if acts is None else torch.from_numpy(np.array(acts)).to(gpu)
    if case.call == "step_encode":
        for k in range(K):  # K calls of one step each, compared call by call
            obs.fill_(fill)
            r, f, o = env.step_encode(d_acts[k], tdt, out=obs)
            assert o is obs
            rew_o, fl_o = ref.step(k)
            compare(case, k, "rewards", r.cpu().numpy(), rew_o, lid)
            compare(case, k, "flags", f.cpu().numpy(), fl_o, lid)
            _compare_obs(case, k, obs, ref)
            compare(case, k, "state", env.get_packed_state(), ref.state, lid, env_axis=1)
            compare(case, k, "episode returns", env.ep_returns.cpu().numpy(), ref.ep_returns, lid)
    else:
        obs_arg = obs if rows == 1 else obs.view(K, n, 2, W, H, 26)
        env.rollout_encode(K, obs_arg, rew, fl, actions=d_acts, dtype=tdt)
        rew_h, fl_h = rew.cpu().numpy(), fl.cpu().numpy()
        for k in range(K):
            rew_o, fl_o = ref.step(k)
            compare(case, k, "rewards", rew_h[k], rew_o, lid)
            compare(case, k, "flags", fl_h[k], fl_o, lid)
            if rows == K:
                _compare_obs(case, k, obs_arg[k], ref)
        if rows == 1:  # one buffer, overwritten every step: the observation of the last step
            _compare_obs(case, K - 1, obs, ref)
        compare(case, K - 1, "state", env.get_packed_state(), ref.state, lid, env_axis=1)
        compare(case, K - 1, "episode returns", env.ep_returns.cpu().numpy(), ref.ep_returns, lid)
    assert env.t_global == case.t0 + (K if case.call in ("rollout", "rollout_single_buffer") else 0), (case.id, env.t_global)
    for what, g, v in (("observation", g_obs, fill), ("rewards", g_rew, -7.0), ("flags", g_fl, 0xEE)):
        guards_untouched(case, what, g, v)
