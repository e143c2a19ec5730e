"""Recorded random rollouts (oc_rollout_record / rollout_random(actions_out=, states_out=)) on the GPU: the recorded actions
are the Philox stream of oc_rollout_random, every recorded state is the state its step acts on (checked step by step against
the C oracle), recording changes none of the launch's other results, recorded states feed the observation kernels, and the
host converter reproduces the drop-in OvercookedEnv.get_rollouts."""
import numpy as np
import pytest

from helpers import CANONICAL_5

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from case_support import new_oracle as _oracle  # noqa: E402
from gpu_support import gpu, no_sentinel, record_buffers  # noqa: E402, F401

SEVEN = {"grid": "XPPPPPX\nO 1 2 O\nX     X\nXDPSPTX", "onion_time": 3, "tomato_time": 5, "onion_value": 7, "tomato_value": 4}


def _table(name):
    from overcooked_ai_amd.layouts import LayoutSpec, LayoutTable, spec_from_name

    if name == "mix5":
        return LayoutTable([spec_from_name(nm) for nm in CANONICAL_5], pad_to=(9, 5))
    if name == "seven_pots":
        return LayoutTable([LayoutSpec(SEVEN)])
    if name.endswith("_old"):  # old dynamics: a full pot starts cooking by itself
        return LayoutTable([spec_from_name(name[:-4], old_dynamics=True)])
    return LayoutTable([spec_from_name(name)])


def _env(gpu, name, n, horizon, seed=3, env_offset=0, t0=0, **kw):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    lid = (np.arange(n) % 5).astype(np.uint16) if name == "mix5" else None
    env = VecOvercookedEnv(_table(name), n, horizon=horizon, device=gpu, auto_reset=True, seed=seed, env_offset=env_offset,
                           layout_id=lid, **kw)
    env.t_global = t0
    return env, lid


def _buffers(env, K):
    """(actions, states, rewards, flags), all sentinels between guard rows, and the check of those rows (gpu_support.record_buffers)"""
    bufs, check = record_buffers(K, env.n_envs, env.n_planes, env.state.device)
    return (bufs["actions_out"], bufs["states_out"], bufs["rewards_out"], bufs["flags_out"]), check


def _record_and_check(gpu, name, n, K, horizon, t0=0, seed=3, env_offset=0, start=None, check_envs=None):
    """One recorded launch, then: actions = the Philox stream; states_out[0] = the state before the call; oracle.step of
    (states_out[k], actions_out[k]) = (states_out[k + 1] or the final state, rewards_out[k], flags_out[k]) byte for byte."""
    from oracle import oracle as O

    env, lid = _env(gpu, name, n, horizon, seed=seed, env_offset=env_offset, t0=t0, **(start or {}))
    before, epoch = env.get_packed_state().copy(), env.reset_epoch
    (acts, states, rew, fl), guards_untouched = _buffers(env, K)
    env.rollout_random(K, rew, fl, actions_out=acts, states_out=states)
    assert env.t_global == t0 + K
    guards_untouched(name)
    A, S, R, F = acts.cpu().numpy(), states.cpu().numpy(), rew.cpu().numpy(), fl.cpu().numpy()
    final = env.get_packed_state()
    for k in range(K):
        assert np.array_equal(A[k], O.random_actions(seed, env_offset, t0 + k, n)), "actions of step %d" % k
    assert np.array_equal(S[0], before), "states_out[0] is not the state before the call"
    sel = np.arange(n) if check_envs is None else np.asarray(check_envs)
    orc = _oracle(env.table.specs)
    lid_s = None if lid is None else np.ascontiguousarray(lid[sel])
    resets = 0
    for k in range(K):
        sp = None if start is None else O.start_spec(seed=seed, env_offset=env_offset, epoch=epoch + k, **start)
        if sp is not None and check_envs is not None:
            raise AssertionError("drawn starts are keyed by the global env: check all envs")
        nxt, r, f = orc.step(np.ascontiguousarray(S[k][:, sel]), A[k][sel], horizon=horizon, options=1, layout_id=lid_s, start=sp)
        after = S[k + 1][:, sel] if k + 1 < K else final[:, sel]
        no_sentinel(name, r, f)
        assert np.array_equal(nxt, after), "state after step %d" % k
        assert np.array_equal(r, R[k][sel]), "rewards of step %d" % k
        assert np.array_equal(f, F[k][sel]), "flags of step %d" % k
        resets += int(((f & 4) != 0).sum())
    return resets, R


@pytest.mark.parametrize("name,n", [("cramped_room", 4096), ("asymmetric_advantages", 4096), ("mix5", 5000),
                                    ("seven_pots", 1000), ("cramped_room", 1000)])
def test_actions_and_states_follow_the_oracle(gpu, name, n):
    resets, R = _record_and_check(gpu, name, n, K=90, horizon=40, t0=0)
    assert resets == 2 * n  # two horizons inside the launch
    assert R[..., 2:].sum() > 0


def test_off_grid_t0_and_old_dynamics(gpu):
    _record_and_check(gpu, "cramped_room_old", 2048, K=61, horizon=25, t0=5, seed=11)


def test_drawn_starts(gpu):
    _record_and_check(gpu, "asymmetric_advantages", 2048, K=70, horizon=30, t0=3, seed=5, env_offset=777,
                      start={"random_start_pos": True, "rnd_obj_prob_thresh": 0.4})


def test_actions_only_65536_envs(gpu):
    from oracle import oracle as O

    env, _ = _env(gpu, "cramped_room", 65536, 400, seed=9, t0=13)
    (acts, _, _, _), guards_untouched = _buffers(env, 19)
    env.rollout_random(19, actions_out=acts)
    guards_untouched("actions only")
    A = acts.cpu().numpy()
    for k in range(19):
        assert np.array_equal(A[k], O.random_actions(9, 0, 13 + k, 65536))


@pytest.mark.parametrize("name", ["cramped_room", "mix5", "cramped_room_old"])
def test_recording_changes_nothing(gpu, name):
    start = {"random_start_pos": True, "rnd_obj_prob_thresh": 0.2} if name == "mix5" else {}
    runs = []
    for record in (False, True):
        env, _ = _env(gpu, name, 3000, 50, seed=17, t0=6, **start)
        (acts, states, rew, fl), guards_untouched = _buffers(env, 130)
        if record:
            env.rollout_random(130, rew, fl, actions_out=acts, states_out=states)
        else:
            env.rollout_random(130, rew, fl)
        guards_untouched(name)
        # (two launches that could drop the same store: every reward and flag must have been written)
        assert not bool((rew == -7.0).any()) and not bool((fl == 0xEE).any()), (name, record)
        runs.append((rew.cpu().numpy(), fl.cpu().numpy(), env.ep_returns.cpu().numpy(), env.get_packed_state(), env.t_global,
                     env.reset_epoch))
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_recorded_states_encode_like_rollout_encode(gpu):
    K, n = 24, 1024
    env, _ = _env(gpu, "cramped_room", n, 10, seed=2)
    (acts, states, rew, fl), guards_untouched = _buffers(env, K)
    env.rollout_random(K, rew, fl, actions_out=acts, states_out=states)
    guards_untouched("recorded states")
    env2, _ = _env(gpu, "cramped_room", n, 10, seed=2)
    obs = torch.zeros((K, n, 2, env.width, env.height, 26), dtype=torch.uint8, device=gpu)
    env2.rollout_encode(K, obs)
    for k in range(K - 1):
        assert torch.equal(env.encode_lossless(state=states[k + 1]), obs[k]), k
    assert torch.equal(env.encode_lossless(), obs[K - 1])


class _Replay:
    """An agent pair that plays back one env's recorded actions."""

    def __init__(self, actions):
        from overcooked_ai_amd.actions import Action

        self.rows, self.i, self.A = actions, 0, Action.INDEX_TO_ACTION

    def joint_action(self, state):
        a = self.rows[self.i]
        self.i += 1
        return (self.A[int(a[0])], {}), (self.A[int(a[1])], {})


def test_converter_matches_dropin_get_rollouts(gpu):
    from overcooked_ai_amd.env import OvercookedEnv
    from overcooked_ai_amd.mdp import OvercookedGridworld
    from overcooked_ai_amd.state import canonical_state_dict
    from overcooked_ai_amd.trajectories import recorded_trajectories

    H, games, n = 30, 3, 64
    env, _ = _env(gpu, "cramped_room", n, H, seed=4)
    recs = []
    for K in (37, H * games - 37 + 5):  # two recordings joined along the step axis
        bufs, guards_untouched = _buffers(env, K)
        recs.append(bufs)
        env.rollout_random(K, recs[-1][2], recs[-1][3], actions_out=recs[-1][0], states_out=recs[-1][1])
        guards_untouched("converter")
    acts, states, rew, fl = (torch.cat([r[i] for r in recs]) for i in range(4))
    envs = [0, 7, 63]
    traj = recorded_trajectories(env, states, acts, rew, fl, envs=envs)
    assert len(traj["ep_lengths"]) == games * len(envs)
    A = acts.cpu().numpy()
    mdp = OvercookedGridworld.from_layout_name("cramped_room")
    for i, e in enumerate(envs):
        ref = OvercookedEnv.from_mdp(mdp, horizon=H).get_rollouts(_Replay(A[:, e]), games)
        for g in range(games):
            j = i * games + g
            assert [canonical_state_dict(s) for s in traj["ep_states"][j]] == [canonical_state_dict(s) for s in ref["ep_states"][g]]
            assert list(traj["ep_actions"][j]) == [tuple(a) for a in ref["ep_actions"][g]]
            assert list(traj["ep_rewards"][j]) == list(ref["ep_rewards"][g])
            assert list(traj["ep_dones"][j]) == list(ref["ep_dones"][g])
            assert traj["ep_returns"][j] == ref["ep_returns"][g] and traj["ep_lengths"][j] == ref["ep_lengths"][g] == H
            for a, b in zip(traj["ep_infos"][j], ref["ep_infos"][g]):
                assert list(a["sparse_r_by_agent"]) == list(b["sparse_r_by_agent"])
                assert list(a["shaped_r_by_agent"]) == list(b["shaped_r_by_agent"])
            last, ref_last = traj["ep_infos"][j][-1]["episode"], ref["ep_infos"][g][-1]["episode"]
            assert last["ep_sparse_r"] == ref_last["ep_sparse_r"] and last["ep_shaped_r"] == ref_last["ep_shaped_r"]
            assert last["ep_length"] == ref_last["ep_length"]
            assert traj["mdp_params"][j]["layout_name"] == mdp.mdp_params["layout_name"]


def test_large_launch_65536_x_400(gpu):
    check = np.arange(0, 65536, 16)  # 4 096 envs against the oracle
    resets, _ = _record_and_check(gpu, "cramped_room", 65536, K=400, horizon=150, seed=8, check_envs=check)
    assert resets == 2 * len(check)
