"""`TrajectoryBuffer`: the T steps of one PPO iteration on a `VecOvercookedMultiAgent`, time-major, written by the step itself.

    buf = TrajectoryBuffer(tenv, T)
    for t in range(T):
        logits, values = policy(obs)
        obs, _, _, infos = tenv.step_sampled(logits, into=buf.row(t, values))
    buf.last_values.copy_(policy(obs)[1])
    adv, targets, moments = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, targets, moments)
    for index in buf.minibatches(4096):
        loss, stats = ppo_loss.ppo_loss(*policy(buf.features.view(-1, F)[index.long()]), batch, index, clip_param=0.05, ...)

`row(t, values)` hands step t's slices to `step_sampled(into=...)`, whose C call then writes the training rewards, the done mask,
the drawn actions and their log-probabilities there in place of the env's persistent buffers: no copy per step, and the rows are the
step's own bytes.  `advantages` is `gae.gae` (oc_gae, one launch) over the whole buffer; `learner_batch` hands the buffer to
`ppo_loss.ppo_loss` as flat [S] views, S = T * N * 2, and `minibatches` cuts a device permutation of the samples into index tensors
(`permutation` hands it over whole, for `learner.PPOLearner.epoch`).  `learner_samples`, `learner_permutation` and
`learner_minibatches` do the same over the learner's samples alone and on the library's own random stream (`sample_index`): with a
behaviour-cloning partner a minibatch then holds only samples the loss counts.

Row t of every tensor meets the alignment the step and the sampler ask for whatever N is: rewards rows are 16 N bytes apart (16-byte
aligned), logp and values rows 8 N (8), actions rows 2 N (2), done and seat rows N (any address) — a fresh allocation starts on a
multiple of 256.  With keep_returns, ep_returns rows are 16 N bytes apart (16-byte aligned) and member rows N (any address);
`outcomes()` is `outcomes.outcome_table` (oc_outcome_table) over done, ep_returns, seat and member: the finished episodes by partner
member and seat.  `ReturnsBuffer` keeps those four alone (`outcomes.evaluate`)."""
import collections

# (ep_returns and member: trailing and defaulted, so that a five-field construction keeps working)
TrajectoryRow = collections.namedtuple("TrajectoryRow", "rewards done actions logp seat ep_returns member", defaults=(None, None))

ROW_BYTES = {"rewards": 16, "done": 1, "actions": 2, "logp": 8, "values": 8, "seat": 1}  # bytes per env of a row
ROW_ALIGN = {"rewards": 16, "done": 1, "actions": 2, "logp": 8, "values": 8, "seat": 1}  # what the C-ABI asks of a row's address


# the rows a buffer with keep_returns adds (tables of their own: tests/test_host_gae.py holds the two above to exactly their six rows)
RETURNS_ROW_BYTES = {"ep_returns": 16, "member": 1}
RETURNS_ROW_ALIGN = {"ep_returns": 16, "member": 1}


def row_offsets(name, T, n_envs):
    """Byte offsets of rows 0..T-1 of tensor `name` from its base."""
    nbytes = ROW_BYTES[name] if name in ROW_BYTES else RETURNS_ROW_BYTES[name]
    return [t * n_envs * nbytes for t in range(T)]


def _outcomes_of(buf, per_env):
    from .outcomes import outcome_table

    if buf.ep_returns is None:
        raise ValueError("outcomes() needs a buffer with keep_returns")
    pool = getattr(buf.tenv, "_pool", None)
    return outcome_table(buf.done, buf.ep_returns, seat=buf.seat, member=buf.member,
                         n_members=buf.tenv.bc_policy.n_members if pool is not None else None, per_env=per_env)


class ReturnsBuffer:
    """What `outcomes.evaluate` collects through: done uint8 [T, N], ep_returns float32 [T, N, 4] and, with a bc_policy, seat (and with
    a `PartnerPool` member) uint8 [T, N], time-major, and nothing else.  `row(t)` is a `TrajectoryRow` for `step_sampled(into=...)`
    whose rewards, actions and logp are ONE [N, 2] row shared by every t: the step call has to write them somewhere, and an
    evaluation does not read them."""

    def __init__(self, tenv, T):
        import torch

        T = int(T)
        if T < 1:
            raise ValueError("ReturnsBuffer: T must be at least 1, not %d" % T)
        self.tenv, self.T, self.n_envs = tenv, T, tenv.n_envs
        N, dev = tenv.n_envs, tenv.venv.device
        self.done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.ep_returns = torch.zeros((T, N, 4), dtype=torch.float32, device=dev)
        self.seat = torch.full((T, N), 255, dtype=torch.uint8, device=dev) if tenv.bc_policy is not None else None
        self.member = torch.full((T, N), 255, dtype=torch.uint8, device=dev) if getattr(tenv, "_pool", None) is not None else None
        self._shared = (torch.zeros((N, 2), dtype=torch.float64, device=dev), torch.zeros((N, 2), dtype=torch.uint8, device=dev),
                        torch.zeros((N, 2), dtype=torch.float32, device=dev))

    def row(self, t):
        if not 0 <= t < self.T:
            raise ValueError("ReturnsBuffer.row: t = %d outside 0..%d" % (t, self.T - 1))
        rewards, actions, logp = self._shared
        return TrajectoryRow(rewards, self.done[t], actions, logp, self.seat[t] if self.seat is not None else None, self.ep_returns[t],
                             self.member[t] if self.member is not None else None)

    def outcomes(self, per_env=False):
        """outcomes.outcome_table over the whole buffer, as `TrajectoryBuffer.outcomes`."""
        return _outcomes_of(self, per_env)


class TrajectoryBuffer:
    """Time-major tensors on the env's device: rewards float64 [T, N, 2], done uint8 [T, N], actions uint8 [T, N, 2], logp float32
    [T, N, 2], values float32 [T, N, 2], last_values float32 [N, 2] and, when the env has a bc_policy, seat uint8 [T, N] (else
    None).  keep_obs: also obs [T, N, 2, W, H, 26] (the env's obs_dtype) and / or features float32 [T, N, 2, F], whichever the
    env's observation kind has, copied by row() from the env's persistent observation buffers — the observation step t starts
    from, which the policy has just read there.  keep_logits: also logits float32 [T, N, 2, 6], the learner's logits that row()
    is given (the exact KL of the loss needs them).  keep_returns: also ep_returns float32 [T, N, 4] — the episode totals the step
    call copies out (sparse p0, sparse p1, shaped p0, shaped p1), final where done is set — and, for an env with a
    `partner.PartnerPool`, member uint8 [T, N]: what `outcomes()` reduces."""

    def __init__(self, tenv, T, keep_obs=False, keep_logits=False, keep_returns=False):
        import torch

        T = int(T)
        if T < 1:
            raise ValueError("TrajectoryBuffer: T must be at least 1, not %d" % T)
        self.tenv, self.T, self.n_envs = tenv, T, tenv.n_envs
        N, dev = tenv.n_envs, tenv.venv.device
        self.rewards = torch.zeros((T, N, 2), dtype=torch.float64, device=dev)
        self.done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros((T, N, 2), dtype=torch.uint8, device=dev)
        self.logp = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.values = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.last_values = torch.zeros((N, 2), dtype=torch.float32, device=dev)
        self.seat = torch.full((T, N), 255, dtype=torch.uint8, device=dev) if tenv.bc_policy is not None else None
        self.logits = torch.zeros((T, N, 2, 6), dtype=torch.float32, device=dev) if keep_logits else None
        self.obs = self.features = None
        if keep_obs:
            if tenv.obs_kind == "bc":
                raise ValueError("TrajectoryBuffer: keep_obs needs an env whose step writes its observation (obs \"ppo\", \"features\" or \"both\")")
            if tenv.obs_kind in ("ppo", "both"):
                self.obs = torch.zeros((T,) + tuple(tenv._obs_buffer().shape), dtype=tenv.obs_dtype, device=dev)
            if tenv.obs_kind in ("features", "both"):
                self.features = torch.zeros((T,) + tuple(tenv._feat_buffer().shape), dtype=torch.float32, device=dev)
        self.ep_returns = self.member = None
        if keep_returns:
            self.ep_returns = torch.zeros((T, N, 4), dtype=torch.float32, device=dev)
            if getattr(tenv, "_pool", None) is not None:
                self.member = torch.full((T, N), 255, dtype=torch.uint8, device=dev)
        self._rows = [TrajectoryRow(self.rewards[t], self.done[t], self.actions[t], self.logp[t],
                                    self.seat[t] if self.seat is not None else None,
                                    self.ep_returns[t] if self.ep_returns is not None else None,
                                    self.member[t] if self.member is not None else None) for t in range(T)]

    def row(self, t, values, logits=None):
        """The destinations of step t, for `step_sampled(into=...)`; `values` (float32 [N, 2], the policy's value estimates of the
        observation step t starts from) is stored in values[t].  With keep_obs the env's current observation is copied too, with
        keep_logits `logits` (floating-point [N, 2, 6], what step_sampled is about to draw from) is stored in logits[t]."""
        torch = self.tenv._torch
        if not 0 <= t < self.T:
            raise ValueError("TrajectoryBuffer.row: t = %d outside 0..%d" % (t, self.T - 1))
        if not isinstance(values, torch.Tensor) or tuple(values.shape) != (self.n_envs, 2) or values.device != self.values.device \
                or not values.dtype.is_floating_point:
            raise ValueError("TrajectoryBuffer.row: values must be a floating-point [n_envs, 2] tensor on %s" % self.values.device)
        if (logits is not None) != (self.logits is not None):
            raise ValueError("TrajectoryBuffer.row: logits are stored by a buffer with keep_logits, and only by one")
        if logits is not None:
            if not isinstance(logits, torch.Tensor) or tuple(logits.shape) != (self.n_envs, 2, 6) or logits.device != self.values.device \
                    or not logits.dtype.is_floating_point:
                raise ValueError("TrajectoryBuffer.row: logits must be a floating-point [n_envs, 2, 6] tensor on %s" % self.values.device)
            self.logits[t].copy_(logits)
        self.values[t].copy_(values)
        if self.obs is not None:
            self.obs[t].copy_(self.tenv._obs_buffer())
        if self.features is not None:
            self.features[t].copy_(self.tenv._feat_buffer())
        return self._rows[t]

    def advantages(self, gamma, lam, moments=True, out=None):
        """gae.gae over the whole buffer: (advantages, targets) float32 [T, N, 2] and, with moments, the float64 [3] tensor
        (count, sum A, sum A^2) over the learner samples."""
        from .gae import gae

        return gae(self.rewards, self.values, self.done, gamma, lam, last_values=self.last_values, seat=self.seat, moments=moments,
                   out=out)

    def outcomes(self, per_env=False):
        """outcomes.outcome_table over the whole buffer (oc_outcome_table, two launches): the finished episodes by partner member and
        seat, as an `outcomes.Outcomes`; per_env: also its env table.  Needs keep_returns.  Nothing here waits for the device."""
        return _outcomes_of(self, per_env)

    def learner_batch(self, advantages, targets, moments=None):
        """The buffer as `ppo_loss.ppo_loss` reads it: flat [S] views (S = T * N * 2, sample (t * N + e) * 2 + p) of the actions, logp
        and the given advantages and targets (float32 [T, N, 2], `advantages()`'s), seat [S / 2] and the old logits [S, 6] where the
        buffer has them, and `moments` (float64 [3], `advantages()`'s; None: the advantages are used as they are)."""
        from .gae import _checked
        from .ppo_loss import LearnerBatch

        torch = self.tenv._torch
        shape, dev = (self.T, self.n_envs, 2), self.values.device
        _checked("advantages", advantages, torch.float32, shape, dev, torch)
        _checked("targets", targets, torch.float32, shape, dev, torch)
        if moments is not None:
            _checked("moments", moments, torch.float64, (3,), dev, torch)
        S = self.T * self.n_envs * 2
        return LearnerBatch(self.actions.view(S), self.logp.view(S), advantages.view(S), targets.view(S),
                            self.seat.view(S // 2) if self.seat is not None else None,
                            self.logits.view(S, 6) if self.logits is not None else None, moments)

    def permutation(self, generator=None):
        """One permutation of the samples 0 .. S - 1 as an int32 [S] tensor on the buffer's device — what `minibatches` cuts, whole:
        `learner.PPOLearner.epoch` takes it and a minibatch size in ONE call (generator: as for `minibatches`)."""
        torch = self.tenv._torch
        S = self.T * self.n_envs * 2
        if S >= 2 ** 31:
            raise ValueError("TrajectoryBuffer.permutation: %d samples do not fit an int32 index" % S)
        return torch.randperm(S, dtype=torch.int32, device=self.values.device, generator=generator)

    def minibatches(self, size, generator=None):
        """Index tensors (int32 [size], the last one shorter) that cut one permutation of the samples 0 .. S - 1, drawn on the
        buffer's device (generator: a torch.Generator of that device; None: the device's default one)."""
        torch = self.tenv._torch
        size = int(size)
        if size < 1:
            raise ValueError("TrajectoryBuffer.minibatches: size must be at least 1, not %d" % size)
        S = self.T * self.n_envs * 2
        if S >= 2 ** 31:
            raise ValueError("TrajectoryBuffer.minibatches: %d samples do not fit an int32 index" % S)
        perm = torch.randperm(S, dtype=torch.int32, device=self.values.device, generator=generator)
        for lo in range(0, S, size):
            yield perm[lo:lo + size]

    def learner_samples(self):
        """The samples of the buffer that the PPO loss uses — not the partner's (by `seat`), not an invalid row's (by `actions`) —
        as a `sample_index.LearnerSamples`, in ascending order on the device: oc_sample_select, three launches, once per iteration.
        Nothing here waits for the device; reading the result's `.n` does, once."""
        from .sample_index import select

        S = self.T * self.n_envs * 2
        if S >= 2 ** 31:
            raise ValueError("TrajectoryBuffer.learner_samples: %d samples do not fit an int32 index" % S)
        return select(self.seat.view(S // 2) if self.seat is not None else None, self.actions.view(S), S)

    def learner_permutation(self, samples, epoch, seed=None):
        """One permutation of the learner's samples (`learner_samples()`'s) as an int32 [samples.n] tensor on the buffer's device,
        for `learner.PPOLearner.epoch`: every entry is a sample the loss counts, so a minibatch of M rows holds M learner samples.
        The permutation is include/oc_amd.h's function of (seed, epoch) — seed: the env's seed by default; epoch: any counter that
        differs from pass to pass, such as iteration * num_sgd_iter + pass — and of nothing else: no torch generator is read."""
        from .sample_index import permute

        return permute(samples, samples.n, self.tenv.venv.seed if seed is None else seed, epoch)

    def learner_minibatches(self, size, samples, epoch, seed=None):
        """Index tensors (int32 [size], the last one shorter) that cut `learner_permutation(samples, epoch, seed)`."""
        size = int(size)
        if size < 1:
            raise ValueError("TrajectoryBuffer.learner_minibatches: size must be at least 1, not %d" % size)
        perm = self.learner_permutation(samples, epoch, seed)
        for lo in range(0, int(perm.shape[0]), size):
            yield perm[lo:lo + size]
