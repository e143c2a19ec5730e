"""Episode outcomes of a collected batch by partner member and seat, on the device: `outcome_table` (oc_outcome_table, two launches),
`evaluate` and `plan`.

    buf = TrajectoryBuffer(tenv, T, keep_returns=True)
    ...                                               # T calls of tenv.step_sampled(logits, into=buf.row(t, values))
    out = buf.outcomes()                              # nothing waits for the device
    out.mean, out.episodes                            # the mean sparse return of the finished episodes (waits, once)
    pool.set_weights(rank_weights(out.by_member()["mean"].mean(axis=1)))

Time-major tensors as `step_sampled(into=...)` leaves them: done uint8 [T, N], ep_returns float32 [T, N, 4] (sparse p0, sparse p1,
shaped p0, shaped p1 of the episode so far — final where done, and read only there), seat and member uint8 [T, N].  The groups, the
columns and the order of summation are stated in include/oc_amd.h (OcOutcomeBatch); tests/outcome_cases.py restates them in numpy."""
import ctypes
import re

import numpy as np

from .gae import _checked, _stream

COLUMNS = ("episodes", "sum_R", "sum_R2", "min_R", "max_R", "sum_shaped_p0", "sum_shaped_p1", "sum_sparse_p0")
ENV_COLUMNS = ("episodes", "sum_R", "sum_R2", "sum_shaped")


def plan(n_envs, n_steps, seat=False, member=False, n_members=1, per_env=False):
    """What outcome_table() launches for N envs and T steps, in oc_outcome_plan's words (no device needed)."""
    from . import _lib

    out = ctypes.create_string_buffer(512)
    rc = _lib.load().oc_outcome_plan(int(n_envs), int(n_steps), int(bool(seat)), int(bool(member)), int(n_members), int(bool(per_env)), out,
                                     len(out))
    _lib.check(rc, "oc_outcome_plan")
    return out.value.decode()


def scratch_bytes(n_envs, n_steps, seat=False, member=False, n_members=1):
    """The bytes of oc_outcome_table's d_scratch, as the plan states them."""
    return int(re.search(r"scratch (\d+) B", plan(n_envs, n_steps, seat, member, n_members)).group(1))


def n_groups(seat=False, n_members=1):
    """G: 1 without seats, else 1 + 2 K."""
    return 1 + 2 * int(n_members) if seat else 1


class Outcomes:
    """What `outcome_table` leaves on the device: `table` float64 [G + 1, 8] (COLUMNS; row 0 "no partner", row 1 + 2 m + s "member m
    plays seat s", row G the unattributed count) and `env_table` float64 [N, 4] (ENV_COLUMNS) or None.  Reading any of `episodes`,
    `mean`, `std`, `min`, `max`, `unattributed`, `by_member()` or `host` is the ONE host synchronisation: the first read waits for
    the reduction and copies the table; later reads use that copy."""

    def __init__(self, table, env_table, n_members, with_seat):
        self.table, self.env_table, self.n_members, self.with_seat = table, env_table, int(n_members), bool(with_seat)
        self._host = None

    @property
    def host(self):
        """The table as a numpy float64 [G + 1, 8] array."""
        if self._host is None:
            self._host = self.table.cpu().numpy()
        return self._host

    @property
    def episodes(self):
        """The number of attributed finished episodes, all groups."""
        return int(self.host[:-1, 0].sum())

    @property
    def unattributed(self):
        return int(self.host[-1, 0])

    @property
    def mean(self):
        """The mean sparse return R of the attributed finished episodes (NaN: none)."""
        n = self.host[:-1, 0].sum()
        return float(self.host[:-1, 1].sum() / n) if n else float("nan")

    @property
    def std(self):
        """The (population) standard deviation of R over the attributed finished episodes (NaN: none)."""
        n = self.host[:-1, 0].sum()
        if not n:
            return float("nan")
        m = self.host[:-1, 1].sum() / n
        return float(np.sqrt(max(self.host[:-1, 2].sum() / n - m * m, 0.0)))

    @property
    def min(self):
        return float(self.host[:-1, 3].min())

    @property
    def max(self):
        return float(self.host[:-1, 4].max())

    def by_member(self):
        """{"episodes", "mean", "std", "min", "max"}: float64 [K, 2] arrays, [m, s] = member m playing seat s (mean and std NaN,
        min +inf and max -inf where there was no episode).  Needs a table made with seats."""
        if not self.with_seat:
            raise ValueError("Outcomes.by_member: the table was made without seats")
        t = self.host[1:-1].reshape(self.n_members, 2, 8)
        n = t[..., 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = t[..., 1] / n
            std = np.sqrt(np.maximum(t[..., 2] / n - mean * mean, 0.0))
        return {"episodes": n.copy(), "mean": mean, "std": std, "min": t[..., 3].copy(), "max": t[..., 4].copy()}


def outcome_table(done, ep_returns, seat=None, member=None, n_members=None, per_env=False):
    """The `Outcomes` of done uint8 [T, N] and ep_returns float32 [T, N, 4], contiguous tensors on one CUDA device; seat uint8 [T, N]
    (None: no partner anywhere); member uint8 [T, N] (None with seats: one partner policy); n_members: K, 1..16 (default 1; required
    with member); per_env: also the env table.  Nothing here waits for the device.  Raises ValueError for a tensor of another dtype,
    shape, device or layout, a member array without seats and K outside 1..16."""
    import torch

    from . import _lib

    if not isinstance(done, torch.Tensor) or done.dim() != 2:
        raise ValueError("done must be a contiguous uint8 [T, N] tensor")
    T, N = int(done.shape[0]), int(done.shape[1])
    dev = done.device
    _checked("done", done, torch.uint8, (T, N), dev, torch)
    _checked("ep_returns", ep_returns, torch.float32, (T, N, 4), dev, torch)
    if member is not None and seat is None:
        raise ValueError("outcome_table: member needs seat")
    if seat is not None:
        _checked("seat", seat, torch.uint8, (T, N), dev, torch)
    if member is not None:
        _checked("member", member, torch.uint8, (T, N), dev, torch)
        if n_members is None:
            raise ValueError("outcome_table: member needs n_members")
    K = 1 if n_members is None else int(n_members)
    if not 1 <= K <= _lib.MAX_POOL or (member is None and K != 1):
        raise ValueError("outcome_table: n_members must be in 1..%d, and 1 without member, not %d" % (_lib.MAX_POOL, K))
    if T < 1 or T * N >= 2 ** 31:
        raise ValueError("outcome_table: T must be at least 1 and T * N below 2^31, not %d and %d" % (T, T * N))
    if dev.type != "cuda":
        raise ValueError("outcome_table works on device tensors, not on %s (there is no CPU fallback)" % dev)
    if N and ep_returns.data_ptr() % 16:
        raise ValueError("outcome_table: ep_returns must be 16-byte aligned")
    G = n_groups(seat is not None, K)
    table = torch.empty((G + 1, 8), dtype=torch.float64, device=dev)
    env_table = torch.empty((N, 4), dtype=torch.float64, device=dev) if per_env else None
    scratch = torch.empty((max(1, scratch_bytes(N, T, seat is not None, member is not None, K) // 8),), dtype=torch.float64, device=dev)
    # (an empty tensor has no address to hand over: of no env the arrays are never read, but which of them are given says which
    # groups the table has, so they point at the scratch)
    ptr = lambda t: None if t is None else t.data_ptr() if t.numel() else scratch.data_ptr()  # noqa: E731
    q = _lib.OcOutcomeBatch(ptr(done), ptr(ep_returns), ptr(seat), ptr(member), ptr(table), ptr(env_table) if N else None, ptr(scratch), N, T, K)
    with torch.cuda.device(dev):
        rc = _lib.load().oc_outcome_table(ctypes.byref(q), _stream(dev))
    _lib.check(rc, "oc_outcome_table")
    return Outcomes(table, env_table, K, seat is not None)


def evaluate(tenv, act, episodes=1, greedy=False):
    """The `Outcomes` of `episodes` whole episodes of every env of a `VecOvercookedMultiAgent`: the env is reset and stepped
    episodes * horizon times with `act(obs) -> logits float32 [N, 2, 6]` (`step_sampled`; greedy: the lowest-index maximum), collected
    through a buffer that keeps the done mask, the episode returns, the seats and the members only.  With
    `bc_policy=PartnerPool(...)` and `bc_factor = 1` this is one row of a cross-play table per call: `.by_member()`."""
    from .trajectory_buffer import ReturnsBuffer

    episodes = int(episodes)
    if episodes < 1:
        raise ValueError("evaluate: episodes must be at least 1, not %d" % episodes)
    buf = ReturnsBuffer(tenv, episodes * tenv.horizon)
    obs = tenv.reset()
    for t in range(buf.T):
        obs = tenv.step_sampled(act(obs), greedy=greedy, into=buf.row(t))[0]
    return buf.outcomes()
