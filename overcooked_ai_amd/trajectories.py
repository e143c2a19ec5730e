"""Recorded rollouts -> the reference's trajectory dict (OvercookedEnv.get_rollouts, env.py:485-580).

`VecOvercookedEnv.rollout_random(..., actions_out=, states_out=)` records, for every step k of a launch, the packed state
the step acts on and the two action indices it draws; with the launch's rewards and flags that is every (s, a, r, done)
tuple of the batch.  With events_out the step's event mask and with layouts_out its layout id come along (the game_stats
of each episode, and episodes on layouts re-drawn at every restart).  `recorded_trajectories` cuts the complete episodes out of such a recording and lays them out under
DEFAULT_TRAJ_KEYS, the format BC datasets, offline RL and trajectory files use.
"""
import numpy as np
import torch

from .actions import Action
from .env import DEFAULT_TRAJ_KEYS
from .mdp import EVENT_TYPES, OvercookedGridworld, _num
from .state import unpack_states

OC_F_DONE = 0x01


def _host(t, dtype):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=dtype)


def _host_ids(t):
    """int16 / uint16 layout ids (torch or numpy) -> numpy uint16."""
    if isinstance(t, torch.Tensor):
        t = t.cpu()
        t = (t if t.dtype == torch.int16 else t.view(torch.int16)).numpy()
    return np.asarray(t).view(np.uint16)


def _game_stats(E, k, end, e, sparse, shaped, n_pl):
    """OvercookedEnv.game_stats (env.py:382-401) of the episode of env e on recorded steps k..end: each event stamped with the
    pre-step timestep, the cumulative rewards summed as the drop-in env sums them (same values, same types)."""
    gs = {name: [[] for _ in range(n_pl)] for name in EVENT_TYPES}
    for key in ("cumulative_sparse_rewards_by_agent", "cumulative_shaped_rewards_by_agent"):
        gs[key] = np.zeros(n_pl, dtype=np.int64)
    for j in range(k, end + 1):
        sp, sh = sparse[j - k], shaped[j - k]
        if any(sp):
            gs["cumulative_sparse_rewards_by_agent"] = gs["cumulative_sparse_rewards_by_agent"] + np.asarray(sp)
        if any(sh):
            gs["cumulative_shaped_rewards_by_agent"] = gs["cumulative_shaped_rewards_by_agent"] + np.asarray(sh)
        mask = int(E[j, e])
        while mask:  # bit 2 * event + agent
            low = mask & -mask
            b = low.bit_length() - 1
            gs[EVENT_TYPES[b >> 1]][b & 1].append(j - k)
            mask ^= low
    return gs


def recorded_trajectories(venv, states_out, actions_out, rewards_out, flags_out, envs=None, events_out=None, layouts_out=None):
    """The complete episodes of the selected envs (default: all) in get_rollouts' dict.

    states_out uint8 [K, n_planes, n_envs, 16], actions_out uint8 [K, n_envs, 2], rewards_out float32 [K, n_envs, 4],
    flags_out uint8 [K, n_envs]: one recorded launch, or several joined along axis 0 (consecutive calls of one env).  An
    episode runs from a recorded state with timestep 0 to the step flagged OC_F_DONE; steps before an env's first such
    state and after its last finished episode are left out.  Episodes are listed env by env, in step order.

    Per episode: ep_states (OvercookedState objects), ep_actions (tuples of Action.INDEX_TO_ACTION), ep_rewards (summed
    sparse reward), ep_dones, ep_infos (agent_infos, sparse_r_by_agent, shaped_r_by_agent, phi_s / phi_s_prime = None;
    the last step carries `episode` with the returns and the length), ep_returns, ep_lengths, mdp_params (the env's
    layout), env_params, metadatas.
    events_out int64 [K, n_envs] (the event masks of the same launches): `episode` also carries ep_game_stats, as the drop-in
    get_rollouts gives it; without it there is none.
    layouts_out int16 / uint16 [K, n_envs] (the recorded layout ids): each episode is unpacked on the layout recorded at its
    first step, and its mdp_params are that layout's (ValueError when the id changes inside an episode); without it the
    layout of an env is taken from venv as it is now."""
    S = _host(states_out, np.uint8)
    A = _host(actions_out, np.uint8)
    R = _host(rewards_out, np.float32)
    F = _host(flags_out, np.uint8)
    K = S.shape[0]
    E = None if events_out is None else _host(events_out, np.int64).view(np.uint64)
    Lid = None if layouts_out is None else _host_ids(layouts_out)
    if A.shape[0] != K or R.shape[0] != K or F.shape[0] != K or any(x is not None and x.shape[0] != K for x in (E, Lid)):
        raise ValueError("states_out, actions_out, rewards_out, flags_out (and events_out / layouts_out) must hold the same number of steps")
    venv._refresh_layout_ids()
    envs = range(venv.n_envs) if envs is None else [int(e) for e in envs]
    env_params = {"start_state_fn": None, "horizon": venv.horizon, "info_level": 0, "num_mdp": 1}
    mdps = {}
    out = {k: [] for k in DEFAULT_TRAJ_KEYS}
    for e in envs:
        spec = venv.spec_of(e) if Lid is None else None
        ts = S[:, 0, e, 6].astype(np.int64) | (S[:, 0, e, 7].astype(np.int64) << 8)  # header bytes 6..7: the timestep
        done = (F[:, e] & OC_F_DONE) != 0
        k = 0
        while k < K:
            if ts[k] != 0:
                k += 1
                continue
            ends = np.flatnonzero(done[k:])
            if len(ends) == 0:
                break  # the recording stops inside this episode
            end = k + int(ends[0])
            if Lid is not None:
                lid = int(Lid[k, e])
                if np.any(Lid[k:end + 1, e] != lid):
                    raise ValueError("env %d: the recorded layout id changes inside the episode of steps %d..%d" % (e, k, end))
                spec = venv.table.specs[lid]
            if id(spec) not in mdps:
                mdps[id(spec)] = OvercookedGridworld.from_spec(spec).mdp_params
            n_pl = spec.num_players
            states = unpack_states(spec, np.ascontiguousarray(S[k:end + 1, :, e, :].transpose(1, 0, 2)))
            actions = [tuple(Action.INDEX_TO_ACTION[int(a)] for a in A[j, e, :n_pl]) for j in range(k, end + 1)]
            sparse = [[_num(float(v)) for v in R[j, e, :n_pl]] for j in range(k, end + 1)]
            shaped = [[_num(float(v)) for v in R[j, e, 2:2 + n_pl]] for j in range(k, end + 1)]
            infos = [{"agent_infos": [{} for _ in range(n_pl)], "sparse_r_by_agent": sp, "shaped_r_by_agent": sh,
                      "phi_s": None, "phi_s_prime": None} for sp, sh in zip(sparse, shaped)]
            sparse_by_agent = np.sum(np.asarray(sparse, dtype=np.float64), axis=0)
            shaped_by_agent = np.sum(np.asarray(shaped, dtype=np.float64), axis=0)
            length = end + 1 - k
            infos[-1]["episode"] = dict(ep_sparse_r=_num(float(sparse_by_agent.sum())), ep_shaped_r=_num(float(shaped_by_agent.sum())),
                                        ep_sparse_r_by_agent=sparse_by_agent, ep_shaped_r_by_agent=shaped_by_agent,
                                        ep_length=length)
            if E is not None:
                infos[-1]["episode"]["ep_game_stats"] = _game_stats(E, k, end, e, sparse, shaped, n_pl)
            for key, col in zip(DEFAULT_TRAJ_KEYS[:5], (states, actions, [sum(sp) for sp in sparse],
                                                        [j == end for j in range(k, end + 1)], infos)):
                arr = np.empty((length,), dtype=object)
                for i, item in enumerate(col):
                    arr[i] = item
                out[key].append(arr)
            out["ep_returns"].append(_num(float(sparse_by_agent.sum())))
            out["ep_lengths"].append(length)
            out["mdp_params"].append(mdps[id(spec)])
            out["env_params"].append(dict(env_params))
            out["metadatas"].append({})
            k = end + 1
    # the container types of get_rollouts (env.py:574): object arrays of per-episode columns, plain arrays elsewhere
    res = {}
    for key, v in out.items():
        if key in DEFAULT_TRAJ_KEYS[:5]:
            arr = np.empty((len(v),), dtype=object)
            for i, col in enumerate(v):
                arr[i] = col
            res[key] = arr
        elif key == "metadatas":
            res[key] = {}
        else:
            res[key] = np.array(v) if key != "mdp_params" and key != "env_params" else np.array(v, dtype=object)
    return res
