"""The batched form of the reference's RLlib training environment (`OvercookedMultiAgent`,
human_aware_rl/rllib/rllib.py:112-438) on top of the accelerated path.

`VecOvercookedMultiAgent` is that environment for N envs resident in HBM: per batched step one
`oc_multi_agent_step` call (step -> phi(s') -> per-agent training reward sparse + factor * (phi(s') - phi(s) | shaped)
-> restart of finished envs -> observation), no host synchronisation.  By default every env has two learning ("ppo") agents.
With `bc_policy` (a `partner.DensePolicy`: the reference's behaviour-cloning network on featurize_state) an env is seated like
the reference's (rllib.py:262-281): at every episode start a `bc_factor` coin decides whether it has a "bc" partner and which
player that partner plays — drawn on the library's counter-based stream, not np.random — and `step_sampled` evaluates the
partners' network into the learner's logits array (`oc_partner_logits`, one launch in front of the step) before the actions are
drawn.  The partner's observation alone is available through `observations("bc")`.  With a `partner.PartnerPool` as `bc_policy`
every new partner is also one of the pool's up to 16 members, drawn with its seat (`member`, `infos["member"]`: uint8 [N], 255 = no
partner), and `partner_logits` evaluates each partner's own member (`oc_partner_pool_logits`); everything else is as with one policy.

With `obs="features"` the same call also returns featurize_state of the states the next step starts from (`obs="both"`: the
lossless encoding and the features), through `oc_multi_agent_step_featurize` — one kernel for single-layout batches.

`OvercookedMultiAgent` is the per-env, dict-keyed form RLlib-style training code holds (one `OvercookedEnv` underneath;
agent ids "ppo_0" / "bc_1" redrawn every reset from the bc schedule, observations by agent kind, the same reward
arithmetic) — the surface of the reference class without its RLlib base class or registry (those belong to the
out-of-scope RLlib stack).  Both are pinned by episodes recorded from the reference class
(tests/golden/multi_agent_*.npz).
"""
import numpy as np


def linear_anneal(start_value, t, t_end, end_value=0.0, t_start=0):
    """Value of a linear schedule at timestep t: from (t_start, start_value) to (t_end, end_value), constant afterwards;
    t_end == 0 switches annealing off.  Same floating-point expression as rllib.py:283-291 (weight of the start value
    first), so that annealed factors compare equal to the reference's."""
    if t_end == 0:
        return start_value
    keep = max(1 - float(t - t_start) / (t_end - t_start), 0)
    return keep * start_value + (1 - keep) * end_value


def schedule_value(points, t):
    """Piecewise-linear schedule through (timestep, value) points, flat after the last one (the bc_schedule of
    rllib.py:369-384): the value at timestep t."""
    lo, hi = points[0], points[1]
    for nxt in points[2:]:
        if t <= hi[0]:
            break
        lo, hi = hi, nxt
    return linear_anneal(lo[1], t, hi[0], hi[1], lo[0])


def _checked_schedule(points):
    """A bc schedule as the reference accepts it (rllib.py:187-211): >= 2 points, starting at timestep 0, increasing
    timesteps, values in [0, 1]; a closing point at infinity keeps the last value forever."""
    pts = [tuple(p) for p in points]
    ts, vs = [p[0] for p in pts], [p[1] for p in pts]
    assert len(pts) >= 2, "Need at least 2 points to linearly interpolate schedule"
    assert ts[0] == 0, "Schedule must start at timestep 0"
    assert all(t >= 0 for t in ts), "All timesteps in schedule must be non-negative"
    assert all(0 <= v <= 1 for v in vs), "All values in schedule must be between 0 and 1"
    assert sorted(ts) == ts, "Timesteps must be in increasing order in schedule"
    if ts[-1] < float("inf"):
        pts.append((float("inf"), vs[-1]))
    return pts


class OvercookedMultiAgent:
    """One two-agent training env with per-agent dict observations / rewards / dones, as RLlib-style code drives it
    (API of human_aware_rl/rllib/rllib.py:112-438).  Each reset seats a "ppo" learner and, with probability `bc_factor`
    (read off `bc_schedule`), a "bc" partner instead of a second learner, in random player order; agent ids are
    `<kind>_<player index>`.  ppo agents observe the lossless encoding of their player, bc agents featurize_state.
    reward_i = sparse + reward_shaping_factor * (phi(s') - phi(s)  if use_phi  else  shaped_i)."""

    supported_agents = ["ppo", "bc"]
    bc_schedule = self_play_bc_schedule = [(0, 0), (float("inf"), 0)]  # no bc partner at any time
    DEFAULT_CONFIG = {
        "mdp_params": {"layout_name": "cramped_room", "rew_shaping_params": {}},
        "env_params": {"horizon": 400},
        "multi_agent_params": {"reward_shaping_factor": 0.0, "reward_shaping_horizon": 0,
                               "bc_schedule": self_play_bc_schedule, "use_phi": True},
    }

    def __init__(self, base_env, reward_shaping_factor=0.0, reward_shaping_horizon=0, bc_schedule=None, use_phi=True):
        self.bc_schedule = _checked_schedule(bc_schedule or self.bc_schedule)
        self.base_env, self.use_phi = base_env, use_phi
        self._initial_reward_shaping_factor = self.reward_shaping_factor = reward_shaping_factor
        self.reward_shaping_horizon = reward_shaping_horizon
        self.anneal_bc_factor(0)
        self._agent_ids = set(self.reset())
        self._spaces_in_preferred_format = True

    # ---- observations
    def _features(self, kind, state):
        if kind == "ppo":
            return self.base_env.lossless_state_encoding_mdp(state)
        if kind == "bc":
            return self.base_env.featurize_state_mdp(state)
        raise ValueError("Unsupported agent type {0}".format(kind))

    def _observe(self, state):
        """{agent id: float32 observation of that agent's player}."""
        return {name: np.asarray(self._features(name.split("_")[0], state)[i], dtype=np.float32)
                for i, name in enumerate(self.curr_agents)}

    def _spaces(self, names):
        from .env import _mk_box, _mk_discrete

        n_act = 6
        probe = self.base_env.mdp.get_standard_start_state()
        box = {}
        for kind, hi, lo in (("ppo", float("inf"), 0.0), ("bc", 100.0, -100.0)):
            shape = np.asarray(self._features(kind, probe)[0]).shape
            box[kind] = _mk_box(np.full(shape, lo, np.float32), np.full(shape, hi, np.float32), np.float32)
        self.ppo_observation_space, self.bc_observation_space = box["ppo"], box["bc"]
        self.shared_action_space = _mk_discrete(n_act)
        self.action_space = {a: _mk_discrete(n_act) for a in names}
        self.observation_space = {a: box[a.split("_")[0]] for a in names}

    def _seat_agents(self):
        """One learner plus (bc_factor coin) a bc partner or a second learner, shuffled over the two player slots — the
        same two np.random draws, in the same order, as the reference (rllib.py:262-281)."""
        kinds = ["ppo", "bc" if np.random.uniform() < self.bc_factor else "ppo"]
        np.random.shuffle(kinds)
        names = ["%s_%d" % (k, i) for i, k in enumerate(kinds)]
        self._spaces(names)
        return names

    # ---- env API
    def reset(self, regen_mdp=True):
        self.base_env.reset(regen_mdp)
        self.curr_agents = self._seat_agents()
        return self._observe(self.base_env.state)

    def step(self, action_dict):
        from .actions import Action

        idx = [action_dict[a] for a in self.curr_agents]
        assert all(self.action_space[a].contains(action_dict[a]) for a in action_dict), "%r (%s) invalid" % (idx, type(idx))
        joint = [Action.INDEX_TO_ACTION[i] for i in idx]
        next_state, sparse, done, info = self.base_env.step(joint, display_phi=self.use_phi)
        if self.use_phi:
            dense = [info["phi_s_prime"] - info["phi_s"]] * 2
        else:
            dense = info["shaped_r_by_agent"]
        a0, a1 = self.curr_agents
        rewards = {a0: sparse + self.reward_shaping_factor * dense[0], a1: sparse + self.reward_shaping_factor * dense[1]}
        return self._observe(next_state), rewards, {a0: done, a1: done, "__all__": done}, {a0: info, a1: info}

    # ---- schedules
    def anneal_reward_shaping_factor(self, timesteps):
        self.set_reward_shaping_factor(linear_anneal(self._initial_reward_shaping_factor, timesteps,
                                                     self.reward_shaping_horizon))

    def anneal_bc_factor(self, timesteps):
        self.set_bc_factor(schedule_value(self.bc_schedule, timesteps))

    def set_reward_shaping_factor(self, factor):
        self.reward_shaping_factor = factor

    def set_bc_factor(self, factor):
        self.bc_factor = factor

    def seed(self, seed):
        """(the env itself draws nothing but the seating, from np.random)"""

    @classmethod
    def from_config(cls, env_config):
        """RLlib-style factory: {"mdp_params": kwargs of OvercookedGridworld.from_layout_name, "env_params": kwargs of
        OvercookedEnv.from_mdp, "multi_agent_params": kwargs of this class}.  The reference's alternative
        "mdp_params_schedule_fn" (a LayoutGenerator curriculum, rllib.py:415-424) is not supported here."""
        from .env import OvercookedEnv
        from .mdp import OvercookedGridworld

        assert env_config and "env_params" in env_config and "multi_agent_params" in env_config
        if "mdp_params" not in env_config:
            raise NotImplementedError("OvercookedMultiAgent.from_config: only fixed 'mdp_params' are supported "
                                      "('mdp_params_schedule_fn' needs the reference's LayoutGenerator curriculum)")
        params = dict(env_config["mdp_params"])
        mdp = OvercookedGridworld.from_layout_name(params.pop("layout_name"), **{k: v for k, v in params.items() if v not in ({}, None)})
        base_env = OvercookedEnv.from_mdp(mdp, info_level=0, **env_config["env_params"])
        return cls(base_env, **env_config["multi_agent_params"])


class VecOvercookedMultiAgent:
    """N two-agent training envs in HBM.  `step(actions)` takes uint8 [n_envs, 2] action indices (player order) and
    returns (obs, rewards, dones, infos) as device tensors; finished episodes restart inside the call, and `obs` of
    those envs is the first observation of the new episode (the usual vector-env convention).

    obs: "ppo" — the lossless encoding [n_envs, 2, W, H, 26], written by the step call; "bc" — the step call gets no observation
    array and step() returns observations("bc"), a second launch; "features" — featurize_state [n_envs, 2, 2*(num_pots*10+26)+4]
    float32 written by the step call itself (oc_multi_agent_step_featurize) into a persistent buffer, with `num_pots` and
    `counter_goals` as for VecOvercookedEnv.featurize; "both" — the pair (lossless, features) from the same call.  one_kernel:
    take the single-kernel path of "features" whatever the batch size (`plan()` says what runs)."""

    def __init__(self, layouts, n_envs, horizon=400, reward_shaping_factor=0.0, reward_shaping_horizon=0, use_phi=True,
                 gamma=0.99, obs="ppo", obs_dtype=None, device="cuda", random_start_pos=False, rnd_obj_prob_thresh=0.0,
                 num_pots=2, counter_goals="none", one_kernel=False, bc_policy=None, bc_schedule=None, **venv_kwargs):
        import re

        import torch

        from . import _lib
        from .partner import PartnerPool
        from .vec_env import VecOvercookedEnv

        self._torch, self._lib = torch, _lib
        # the partner (checked before anything is allocated): its network reads the feature buffer the step call writes
        self.bc_policy = bc_policy
        self.bc_schedule = _checked_schedule(bc_schedule or OvercookedMultiAgent.self_play_bc_schedule)
        if bc_policy is not None:
            if obs not in ("features", "both"):
                raise ValueError("a bc_policy needs obs=\"features\" or \"both\" (its input is the feature buffer), not %r" % (obs,))
            if bc_policy.in_dim != 2 * (int(num_pots) * 10 + 26) + 4:
                raise ValueError("bc_policy.in_dim = %d, but this env's feature length (num_pots = %d) is %d"
                                 % (bc_policy.in_dim, num_pots, 2 * (int(num_pots) * 10 + 26) + 4))
        venv_kwargs.pop("auto_reset", None)
        self.venv = VecOvercookedEnv(layouts, n_envs, horizon=horizon, device=device, auto_reset=False,
                                     random_start_pos=random_start_pos, rnd_obj_prob_thresh=rnd_obj_prob_thresh,
                                     **venv_kwargs)
        v = self.venv
        self.n_envs, self.horizon, self.use_phi, self.gamma = v.n_envs, v.horizon, bool(use_phi), float(gamma)
        self._initial_reward_shaping_factor = self.reward_shaping_factor = reward_shaping_factor
        self.reward_shaping_horizon = reward_shaping_horizon
        if obs not in ("ppo", "bc", "features", "both"):
            raise ValueError("Unsupported observation kind {0}".format(obs))
        self.obs_kind = obs
        self.num_pots, self.counter_goals, self.one_kernel = int(num_pots), counter_goals, bool(one_kernel)
        # start_state_fn = mdp.get_random_start_state_fn(random_start_pos, rnd_obj_prob_thresh) of the reference's
        # env_params (mdp.py:1307-1369): every episode, including the restarts inside step(), begins from a random state
        self.random_start_pos, self.rnd_obj_prob_thresh = bool(random_start_pos), float(rnd_obj_prob_thresh)
        self._random_starts = self.random_start_pos or self.rnd_obj_prob_thresh > 0.0
        self.obs_dtype = obs_dtype or torch.float32  # the reference casts observations to float32 (rllib.py:257)
        dev = v.device
        self.shaped = torch.zeros((self.n_envs, 2), dtype=torch.float64, device=dev)
        self.done = torch.zeros((self.n_envs,), dtype=torch.uint8, device=dev)
        self._last_done = self.done  # the tensor the last step wrote its done mask to (a TrajectoryBuffer row with `into`)
        self.phi_next = torch.zeros((self.n_envs,), dtype=torch.float64, device=dev)
        self.phi_cur = torch.zeros((self.n_envs,), dtype=torch.float64, device=dev)
        self.phi_start = torch.zeros((len(v.table),), dtype=torch.float64, device=dev)
        self.ep_returns = torch.zeros((self.n_envs, 4), dtype=torch.float32, device=dev)
        self._obs = None
        self._feat = None
        self._phi_args = None
        self.sample_step = 0  # step_sampled / sample_actions: the counter of the next draw (reset() leaves it alone)
        self._sampled = None
        # seat[e]: the player the bc partner of env e plays (0 / 1), 255 = no partner; drawn by partner_logits()
        self.seat = torch.full((self.n_envs,), 255, dtype=torch.uint8, device=dev)
        self._reseat_all = True  # construction and reset(): every env is seated anew at the next partner_logits()
        self._feat_current = False  # the feature buffer holds featurize_state of the current states
        self._seats = _lib.OcPartnerSeats()
        # a partner.PartnerPool: member[e] is the pool member the partner of env e is (255 = no partner), drawn with the seat; the
        # scratch of oc_partner_pool_logits is allocated once, at the size the plan states
        self._pool = None
        if isinstance(bc_policy, PartnerPool):
            self.member = torch.full((self.n_envs,), 255, dtype=torch.uint8, device=dev)
            self._pool = bc_policy.struct_for(self.member)
            nbytes = int(re.search(r"scratch (\d+) B", self.plan_partner()).group(1)) if self.n_envs else 0
            self.pool_scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.anneal_bc_factor(0)
        if self.use_phi:
            # phi of each layout's STANDARD start state (what a standard reset carries into phi_cur), from a probe batch of
            # one env per layout — the training batch itself may already hold drawn start states (epoch 0)
            L = len(v.table)
            probe = VecOvercookedEnv(v.table, L, horizon=horizon, device=dev, layout_id=np.arange(L) if L > 1 else None)
            self.phi_start.copy_(probe.potential(self.gamma))
            v.potential(self.gamma, out=self.phi_cur)

    def _obs_buffer(self):
        if self._obs is None or self._obs.dtype != self.obs_dtype:
            self._obs = self._torch.empty((self.n_envs, 2, self.venv.width, self.venv.height, 26),
                                          dtype=self.obs_dtype, device=self.venv.device)
        return self._obs

    def _feat_buffer(self):
        if self._feat is None:
            self._feat = self._torch.empty((self.n_envs, 2, 2 * (self.num_pots * 10 + 26) + 4), dtype=self._torch.float32,
                                           device=self.venv.device)
        return self._feat

    def observations(self, kind=None):
        """Both agents' observations of the current states: "ppo" -> [n_envs, 2, W, H, 26] (lossless encoding),
        "bc" -> [n_envs, 2, 96] (featurize_state), "features" -> [n_envs, 2, 2*(num_pots*10+26)+4] (featurize_state with this
        env's num_pots and counter_goals, in its persistent buffer), "both" -> the pair (lossless, features)."""
        kind = kind or self.obs_kind
        if kind == "ppo":
            return self.venv.encode_lossless(self.obs_dtype, out=self._obs_buffer())
        if kind == "bc":
            return self.venv.featurize()
        if kind == "features":
            return self.venv.featurize(self.num_pots, self.counter_goals, out=self._feat_buffer())
        if kind == "both":
            return self.observations("ppo"), self.observations("features")
        raise ValueError("Unsupported agent type {0}".format(kind))

    def reset(self):
        self._reseat_all, self._feat_current = True, False
        if self._random_starts:
            self.venv.reset(random_start_pos=self.random_start_pos, rnd_obj_prob_thresh=self.rnd_obj_prob_thresh)
            if self.use_phi:
                self.venv.potential(self.gamma, out=self.phi_cur)
            return self._observe()
        self.venv.reset()
        if self.use_phi:
            lid = self.venv.layout_id
            self.phi_cur.copy_(self.phi_start[lid.long() & 0xFFFF] if lid is not None else self.phi_start.expand(self.n_envs))
        return self._observe()

    def _observe(self):
        out = self.observations()
        self._feat_current = self._with_features
        return out

    def _call_args(self):
        """What step() hands to oc_multi_agent_step beside the arrays every call has: (observation buffer or None, obs_dtype
        code, OcStartSpec* or None — random starts: finished envs restart from drawn states in the same call —, OcEventSink* or
        None)."""
        v = self.venv
        obs = self._obs_buffer() if self.obs_kind in ("ppo", "both") else None
        code = {self._torch.uint8: self._lib.OBS_U8, self._torch.float32: self._lib.OBS_F32}[self.obs_dtype]
        return obs, code, v._start_spec(), v._event_sink() if v.event_counts is not None else None

    def plan(self):
        """The path and kernel instance the next step() runs, in oc_multi_agent_plan's words (up to and including '>' the
        instance's name): asked for this env's own batch and for the optional arrays step() itself would pass."""
        import ctypes

        v = self.venv
        obs, code, start, sink = self._call_args()
        out = ctypes.create_string_buffer(320)
        if self._with_features:  # (oc_multi_agent_step_featurize_plan's words)
            rc = v.lib.oc_multi_agent_step_featurize_plan(v._bref, self.horizon, int(obs is not None), code, 1, self.num_pots,
                                                          self._feat_options, int(self.use_phi), int(sink is not None), start, out,
                                                          len(out))
            self._lib.check(rc, "oc_multi_agent_step_featurize_plan")
            return out.value.decode()
        rc = v.lib.oc_multi_agent_plan(v._bref, self.horizon, int(obs is not None), code, int(self.use_phi), int(sink is not None),
                                       start, out, len(out))
        self._lib.check(rc, "oc_multi_agent_plan")
        return out.value.decode()

    @property
    def _with_features(self):
        return self.obs_kind in ("features", "both")

    @property
    def _feat_options(self):
        return self._lib.OPT_ONE_KERNEL if self.one_kernel else 0

    def step(self, actions):
        """One batched training step, enqueued by a single C call (oc_multi_agent_step; with obs = "features" or "both"
        oc_multi_agent_step_featurize, which also writes the feature buffer)."""
        v, torch = self.venv, self._torch
        if actions.dtype != torch.uint8 or actions.shape != (self.n_envs, 2) or not actions.is_contiguous() \
                or actions.device != v.state.device:
            raise ValueError("actions must be a contiguous uint8 [n_envs, 2] tensor on %s" % v.device)
        return self._step(actions.data_ptr(), None)

    def _step(self, actions_ptr, sampler, shaped=None, done=None, ep_returns=None):
        """step() with the caller's actions (sampler None), or step_sampled() with an OcActionSampler in their place.  shaped, done,
        ep_returns: the tensors that receive the training rewards, the done mask and the copy of the episode returns in place of the
        persistent buffers (step_sampled's `into`)."""
        v = self.venv
        shaped = self.shaped if shaped is None else shaped
        done = self.done if done is None else done
        ep_returns = self.ep_returns if ep_returns is None else ep_returns
        obs, code, start, sink = self._call_args()
        if self.use_phi:
            if self._phi_args is None:
                v.potential(self.gamma, out=self.phi_next)  # builds and caches the tables
                blob, offs = v._plan("none")
                self._phi_args = (blob.data_ptr(), offs.data_ptr(), v._phi_tables[self.gamma].data_ptr())
            plan, off, tables = self._phi_args
        else:
            plan = off = tables = None
        args = (v._bref, v._state_ptr, actions_ptr if sampler is None else sampler, v._rewards_ptr, v._flags_ptr, v._ep_ptr, ep_returns.data_ptr(), plan, off,
                tables, self.phi_next.data_ptr(), self.phi_cur.data_ptr(), self.phi_start.data_ptr(), float(self.reward_shaping_factor),
                shaped.data_ptr(), done.data_ptr(), obs.data_ptr() if obs is not None else None, code, self.horizon)
        feat = None
        if sampler is not None:
            fargs = (None, None, None)
            if self._with_features:
                feat = self._feat_buffer()
                fblob, foffs = v._plan(self.counter_goals)
                fargs = (fblob.data_ptr(), foffs.data_ptr(), feat.data_ptr())
            rc = v._launch(v.lib.oc_multi_agent_step_sample, *args, *fargs, self.num_pots, self._feat_options, start, sink)
            self._lib.check(rc, "oc_multi_agent_step_sample")
        elif self._with_features:
            feat = self._feat_buffer()
            fblob, foffs = v._plan(self.counter_goals)
            rc = v._launch(v.lib.oc_multi_agent_step_featurize, *args, fblob.data_ptr(), foffs.data_ptr(), feat.data_ptr(), self.num_pots,
                           self._feat_options, start, sink)
            self._lib.check(rc, "oc_multi_agent_step_featurize")
        else:
            rc = v._launch(v.lib.oc_multi_agent_step, *args, start, sink)
            self._lib.check(rc, "oc_multi_agent_step")
        v._advance(1)
        self._last_done = done
        self._feat_current = feat is not None
        infos = {"sparse_r_by_agent": v.rewards[:, 0:2], "shaped_r_by_agent": v.rewards[:, 2:4], "flags": v.flags,
                 "ep_returns": ep_returns}  # episode totals so far; final where done (the reset cleared the live ones)
        if self.use_phi:
            infos["phi_s_prime"] = self.phi_next
        if feat is not None:
            out = feat if obs is None else (obs, feat)
        else:
            out = obs if obs is not None else self.observations()
        return out, shaped, done, infos

    def _sampler(self, logits, greedy, into=None):
        """The OcActionSampler of the next draw (persistent, like its output buffers): this env's seed and env offset, the sample
        counter as the step.  into: the TrajectoryBuffer row whose actions and logp receive the draw in place of those buffers."""
        import ctypes

        v, torch = self.venv, self._torch
        if logits.dtype != torch.float32 or logits.shape != (self.n_envs, 2, 6) or not logits.is_contiguous() \
                or logits.device != v.state.device:
            raise ValueError("logits must be a contiguous float32 [n_envs, 2, 6] tensor on %s" % v.device)
        if self._sampled is None:
            self._sampled = (torch.zeros((self.n_envs, 2), dtype=torch.uint8, device=v.device),
                             torch.zeros((self.n_envs, 2), dtype=torch.float32, device=v.device), self._lib.OcActionSampler())
        actions, logp, s = self._sampled
        if into is not None:
            actions, logp = into.actions, into.logp
        s.d_logits, s.d_actions_out, s.d_logp_out = logits.data_ptr(), actions.data_ptr(), logp.data_ptr()
        s.seed, s.env_offset, s.step = v.seed, v.env_offset, self.sample_step
        s.mode = self._lib.SAMPLE_ARGMAX if greedy else self._lib.SAMPLE_CATEGORICAL
        self.sample_step += 1
        return actions, logp, ctypes.byref(s)

    def sample_actions(self, logits, greedy=False):
        """Both players' actions drawn from policy logits (float32 [n_envs, 2, 6]) on the library's counter-based stream, by
        oc_sample_actions alone: (actions uint8 [n_envs, 2], logp float32 [n_envs, 2]) in persistent buffers.  One draw of the
        env's sample counter, as in step_sampled(): `step(sample_actions(logits)[0])` is `step_sampled(logits)` in two calls."""
        v = self.venv
        actions, logp, s = self._sampler(logits, greedy)
        self._lib.check(v._launch(v.lib.oc_sample_actions, v._bref, s), "oc_sample_actions")
        return actions, logp

    def _checked_row(self, into):
        """step_sampled's `into`: a TrajectoryBuffer row of this env's batch size, on its device.  ep_returns and, with a PartnerPool,
        member are optional (a buffer with keep_returns has them)."""
        torch, dev = self._torch, self.venv.state.device
        n = self.n_envs
        wanted = (("rewards", torch.float64, (n, 2)), ("done", torch.uint8, (n,)), ("actions", torch.uint8, (n, 2)), ("logp", torch.float32, (n, 2)))
        if self.bc_policy is not None:
            wanted += (("seat", torch.uint8, (n,)),)
        if getattr(into, "ep_returns", None) is not None:
            wanted += (("ep_returns", torch.float32, (n, 4)),)
        if self._pool is not None and getattr(into, "member", None) is not None:
            wanted += (("member", torch.uint8, (n,)),)
        for name, dtype, shape in wanted:
            t = getattr(into, name, None)
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError("into.%s must be a contiguous %s %s tensor on %s" % (name, str(dtype).replace("torch.", ""), list(shape), dev))
        if into.rewards.data_ptr() % 16 or into.logp.data_ptr() % 8 or into.actions.data_ptr() % 2:
            raise ValueError("into: rewards must be 16-byte, logp 8-byte and actions 2-byte aligned")
        if getattr(into, "ep_returns", None) is not None and into.ep_returns.data_ptr() % 16:
            raise ValueError("into: ep_returns must be 16-byte aligned")
        return into

    def step_sampled(self, logits, greedy=False, into=None):
        """step() for a policy in the loop: `logits` is its output, contiguous float32 [n_envs, 2, 6] (player, action index) on the
        env's device; both players' actions are drawn from it (greedy: the lowest-index maximum) and stepped by a single C call
        (oc_multi_agent_step_sample; one launch wherever step() is one kernel).  Returns what step() returns, with the drawn
        actions (uint8 [n_envs, 2]) and their log-probabilities (float32 [n_envs, 2]) in infos["actions"] / infos["logp"],
        persistent buffers.  The draws are a function of (the env's seed, its env offset + env, sample_step): `sample_step`
        starts at 0, goes up by one per call, and reset() leaves it alone.  A row of logits with a NaN, a +inf or nothing but
        -inf draws action 255 with logp NaN: the env is flagged OC_F_BAD_ACTION and stays as it is.
        With a bc_policy, partner_logits(logits) runs first: the caller's `logits` tensor is OVERWRITTEN at the partner seats
        (logits[e, seat[e]] of every env with a partner) with the partner's own logits, the draw follows from those, and
        infos["seat"] is the seat tensor, so that a learner can drop the partner's samples.
        into: a row of a trajectory_buffer.TrajectoryBuffer (`buf.row(t, values)`).  The same C call then writes the training
        rewards, the done mask, the drawn actions and their log-probabilities into that row in place of the persistent buffers —
        which this call leaves untouched — and returns the row's views; with a bc_policy the seats of this step are copied into
        the row's seat (one copy), and with a PartnerPool their members into the row's member where it has one.  A row with
        ep_returns (a buffer with keep_returns) also receives the call's copy of the episode returns — infos["ep_returns"] is then
        the row's view — for `TrajectoryBuffer.outcomes()`.  The next call, with or without `into`, reseats by the done mask this call wrote.  Observations
        stay in their persistent buffers: the policy's next forward pass reads them there."""
        if into is not None:
            self._checked_row(into)
        if self.bc_policy is not None:
            self.partner_logits(logits)
            if into is not None:
                into.seat.copy_(self.seat)
                if self._pool is not None and getattr(into, "member", None) is not None:
                    into.member.copy_(self.member)
        actions, logp, s = self._sampler(logits, greedy, into)
        if into is None:
            out, shaped, done, infos = self._step(None, s)
        else:
            out, shaped, done, infos = self._step(None, s, into.rewards, into.done, getattr(into, "ep_returns", None))
        infos["actions"], infos["logp"] = actions, logp
        if self.bc_policy is not None:
            infos["seat"] = self.seat
            if self._pool is not None:
                infos["member"] = self.member
        return out, shaped, done, infos

    def partner_logits(self, logits):
        """The partners' part of step_sampled(), alone (oc_partner_logits, one launch): envs whose previous step was done — every
        env at the first call and after reset() — are seated anew from the current `bc_factor` on the seating stream of
        include/oc_amd.h at (the env's seed, its env offset + env, sample_step), and for every env with a partner the network's six
        logits on featurize_state of the CURRENT state of the partner's player overwrite `logits[e, seat[e]]`; nothing else of
        `logits` is written.  Does not advance `sample_step`.  Returns `seat` (uint8 [n_envs]: 0 / 1 the partner's player, 255 none).
        With a PartnerPool (oc_partner_pool_logits, four launches) a reseated env with a partner also draws its member into `member`,
        and the six logits are the network of that member; `pool_scratch` is the call's scratch, allocated once."""
        import ctypes

        v, torch = self.venv, self._torch
        if self.bc_policy is None:
            raise ValueError("partner_logits needs a bc_policy")
        if logits.dtype != torch.float32 or logits.shape != (self.n_envs, 2, 6) or not logits.is_contiguous() \
                or logits.device != v.state.device:
            raise ValueError("logits must be a contiguous float32 [n_envs, 2, 6] tensor on %s" % v.device)
        if not self._feat_current:  # (before the first step and after reset(): the step call itself keeps the buffer current)
            self.observations("features")
            self._feat_current = True
        s = self._seats
        s.d_seat, s.d_done = self.seat.data_ptr(), None if self._reseat_all else self._last_done.data_ptr()
        s.bc_factor, s.seed, s.env_offset, s.step = float(self.bc_factor), v.seed, v.env_offset, self.sample_step
        if self._pool is not None:  # (the stream is _launch's last argument: the scratch goes in front of it)
            self._pool.d_member = self.member.data_ptr()
            self._pool.thresholds = self.bc_policy.thresholds_ref()  # (the pool's current ones: PartnerPool.set_weights)
            rc = v._launch(v.lib.oc_partner_pool_logits, v._bref, ctypes.byref(self._pool), ctypes.byref(s), self._feat_buffer().data_ptr(),
                           self.num_pots, logits.data_ptr(), self.pool_scratch.data_ptr())
            self._lib.check(rc, "oc_partner_pool_logits")
        else:
            rc = v._launch(v.lib.oc_partner_logits, v._bref, self.bc_policy._ref, ctypes.byref(s), self._feat_buffer().data_ptr(),
                           self.num_pots, logits.data_ptr())
            self._lib.check(rc, "oc_partner_logits")
        self._reseat_all = False
        return self.seat

    def plan_partner(self):
        """What partner_logits() launches, in oc_partner_logits_plan's words."""
        import ctypes

        if self.bc_policy is None:
            raise ValueError("plan_partner needs a bc_policy")
        out = ctypes.create_string_buffer(512)
        if self._pool is not None:
            rc = self.venv.lib.oc_partner_pool_plan(self.venv._bref, ctypes.byref(self._pool), self.num_pots, out, len(out))
            self._lib.check(rc, "oc_partner_pool_plan")
        else:
            rc = self.venv.lib.oc_partner_logits_plan(self.venv._bref, self.bc_policy._ref, self.num_pots, out, len(out))
            self._lib.check(rc, "oc_partner_logits_plan")
        return out.value.decode()

    def anneal_bc_factor(self, timesteps):
        """bc_factor = the bc schedule at `timesteps` (rllib.py:369-384), as OvercookedMultiAgent.anneal_bc_factor"""
        self.set_bc_factor(schedule_value(self.bc_schedule, timesteps))

    def set_bc_factor(self, factor):
        self.bc_factor = factor

    def plan_sampled(self):
        """The path and kernel instance the next step_sampled() runs, in oc_multi_agent_step_sample_plan's words."""
        import ctypes

        v = self.venv
        obs, code, start, sink = self._call_args()
        out = ctypes.create_string_buffer(400)
        rc = v.lib.oc_multi_agent_step_sample_plan(v._bref, self.horizon, int(obs is not None), code, int(self._with_features),
                                                   self.num_pots, self._feat_options, int(self.use_phi), int(sink is not None), start,
                                                   out, len(out))
        self._lib.check(rc, "oc_multi_agent_step_sample_plan")
        return out.value.decode()

    def anneal_reward_shaping_factor(self, timesteps):
        self.reward_shaping_factor = linear_anneal(self._initial_reward_shaping_factor, timesteps,
                                                   self.reward_shaping_horizon)

    def set_reward_shaping_factor(self, factor):
        self.reward_shaping_factor = factor
