"""The behaviour-cloning partner's model on the device: `DensePolicy`, the weights `oc_partner_logits` evaluates.

The reference's BC model (human_aware_rl/imitation/behavior_cloning_tf2.py) is a small dense network on featurize_state:
in_dim -> h1 -> h2 -> 6 logits with ReLU after the two hidden layers (96 -> 64 -> 64 -> 6 by default).  `DensePolicy` takes its six
arrays in the Keras Dense layout (kernels [in, out], biases [out]; `model.get_weights()` of such a model, in order), validates
them, uploads them once as contiguous float32 and holds the `OcDensePolicy` the C-ABI takes.  `VecOvercookedMultiAgent(...,
bc_policy=policy)` seats it.  `PartnerPool` is up to 16 of them, one drawn per episode on the device (`oc_partner_pool_logits`):
`bc_policy=PartnerPool([...])`."""
import ctypes

import numpy as np

N_ACTIONS = 6
MAX_HIDDEN = 64  # include/oc_amd.h: 1 <= h1, h2 <= 64


class DensePolicy:
    """w1 [in_dim, h1], b1 [h1], w2 [h1, h2], b2 [h2], w3 [h2, 6], b3 [6]: numpy arrays or torch tensors of a floating dtype (kept
    as float32).  Raises ValueError for anything else.  `in_dim`, `h1`, `h2`; `struct` is the OcDensePolicy (pointers into tensors
    this object keeps alive); `weights()` returns the float32 numpy copies, in the constructor's order."""

    def __init__(self, w1, b1, w2, b2, w3, b3, device="cuda"):
        import torch

        from . import _lib

        names = ("w1", "b1", "w2", "b2", "w3", "b3")
        host = []
        for name, a in zip(names, (w1, b1, w2, b2, w3, b3)):
            if isinstance(a, torch.Tensor):
                a = a.detach().cpu().numpy()
            a = np.asarray(a)
            if a.dtype.kind != "f":
                raise ValueError("DensePolicy: %s must be a floating-point array, not %s" % (name, a.dtype))
            if a.ndim != (2 if name[0] == "w" else 1):
                raise ValueError("DensePolicy: %s must have %d dimension(s), not shape %r" % (name, 2 if name[0] == "w" else 1, a.shape))
            if not np.isfinite(a).all():
                raise ValueError("DensePolicy: %s holds a NaN or an infinity" % name)
            host.append(np.ascontiguousarray(a, dtype=np.float32))
        w1, b1, w2, b2, w3, b3 = host
        self.in_dim, self.h1, self.h2 = int(w1.shape[0]), int(w1.shape[1]), int(w2.shape[1])
        if self.in_dim < 1:
            raise ValueError("DensePolicy: w1 has no input rows")
        for h, name in ((self.h1, "h1"), (self.h2, "h2")):
            if not 1 <= h <= MAX_HIDDEN:
                raise ValueError("DensePolicy: %s = %d, must be in 1..%d" % (name, h, MAX_HIDDEN))
        for name, a, want in (("b1", b1, (self.h1,)), ("w2", w2, (self.h1, self.h2)), ("b2", b2, (self.h2,)),
                              ("w3", w3, (self.h2, N_ACTIONS)), ("b3", b3, (N_ACTIONS,))):
            if a.shape != want:
                raise ValueError("DensePolicy: %s has shape %r, expected %r" % (name, a.shape, want))
        self._host = host
        self.device = torch.device(device)
        self._dev = [torch.from_numpy(a).to(self.device) for a in host]  # uploaded once
        self.struct = _lib.OcDensePolicy(*[t.data_ptr() for t in self._dev], self.in_dim, self.h1, self.h2)
        self._ref = ctypes.byref(self.struct)

    def weights(self):
        return tuple(self._host)

    def tensors(self):
        """The six device tensors (float32), in the constructor's order."""
        return tuple(self._dev)


def thresholds_of(weights):
    """The OcPartnerPool thresholds of non-negative member weights: thresholds[m] = ceil(2^32 * (w_0 + ... + w_m) / sum(w)) for
    m < len(weights) - 1, in exact rational arithmetic, capped at 2^32 - 1.  Member m is drawn with probability (thresholds[m] -
    thresholds[m - 1]) / 2^32 (0 before the first, 2^32 after the last): its share rounded to a multiple of 2^-32, and exactly 0 for
    a weight of 0, whose two thresholds are equal — except for a LAST member of weight 0, which the cap leaves 2^-32."""
    from fractions import Fraction

    w = [Fraction(x) for x in weights]
    if any(x < 0 for x in w) or sum(w) <= 0:
        raise ValueError("PartnerPool: weights must be non-negative with a positive sum")
    total, run, out = sum(w), Fraction(0), []
    for x in w[:-1]:
        run += x
        out.append(min(-((-run * 2**32) // total), 2**32 - 1))
    return [int(t) for t in out]


class PartnerPool:
    """1 to 16 `DensePolicy` on one device with one `in_dim` (h1 and h2 may differ): the members of `oc_partner_pool_logits`.
    `VecOvercookedMultiAgent(..., bc_policy=pool)` draws one of them for every new partner, uniformly, or by `weights`
    (non-negative numbers, one per member: see `thresholds_of` for their rounding).  `set_member(i, policy)` swaps a member in place
    — a league that ages — for every env built on this pool, from its next call on; `set_weights(weights)` changes the draw the
    same way (`rank_weights`: towards the members the learner does worst with).  `n_members`, `in_dim`, `policies`, `thresholds`
    (None: uniform)."""

    def __init__(self, policies, weights=None):
        from . import _lib

        policies = list(policies)
        if not 1 <= len(policies) <= _lib.MAX_POOL:
            raise ValueError("PartnerPool: %d members, must be 1..%d" % (len(policies), _lib.MAX_POOL))
        self.n_members, self.in_dim, self.device = len(policies), policies[0].in_dim, policies[0].device
        self.policies = [None] * self.n_members
        self._members = (_lib.OcDensePolicy * self.n_members)()
        for i, p in enumerate(policies):
            self.set_member(i, p)
        self.thresholds = self._thresholds = None
        self._threshold_store = (ctypes.c_uint32 * max(1, self.n_members - 1))()  # (one array for the pool's life: set_weights rewrites it)
        self.set_weights(weights)

    def set_weights(self, weights):
        """New draw weights (non-negative numbers, one per member; None: uniform again) for every env built on this pool, from its
        next call on, as `set_member` does for a member: envs already seated keep their partner until their episode ends.  Works on
        a pool built uniform as well.  `thresholds` follows (`thresholds_of`)."""
        if weights is None:
            self.thresholds = self._thresholds = None
            return
        weights = list(weights)
        if len(weights) != self.n_members:
            raise ValueError("PartnerPool: %d weights for %d members" % (len(weights), self.n_members))
        thresholds = thresholds_of(weights)
        self._threshold_store[:len(thresholds)] = thresholds
        self.thresholds, self._thresholds = thresholds, self._threshold_store

    def thresholds_ref(self):
        """The OcPartnerPool.thresholds pointer of the current weights (None: uniform)."""
        return ctypes.cast(self._thresholds, ctypes.POINTER(ctypes.c_uint32)) if self._thresholds is not None else None

    def set_member(self, i, policy):
        if not isinstance(policy, DensePolicy):
            raise ValueError("PartnerPool: member %d is not a DensePolicy" % i)
        if not 0 <= i < self.n_members:
            raise ValueError("PartnerPool: no member %d among %d" % (i, self.n_members))
        if policy.in_dim != self.in_dim or policy.device != self.device:
            raise ValueError("PartnerPool: member %d has in_dim %d on %s, the pool %d on %s"
                             % (i, policy.in_dim, policy.device, self.in_dim, self.device))
        self.policies[i] = policy  # (kept alive: the array below points into its tensors)
        self._members[i] = policy.struct

    def struct_for(self, member):
        """The OcPartnerPool of an env whose member array is the uint8 tensor `member` (the pool's arrays are shared)."""
        from . import _lib

        return _lib.OcPartnerPool(self._members, self.n_members, self.thresholds_ref(), member.data_ptr())


def rank_weights(mean_returns, beta=1.0):
    """Prioritised partner sampling (the rank-based prioritisation of the maximum-entropy-population work): weights proportional to
    rank^beta, where the member with the WORST mean return has the highest rank K' (the number of distinct means, a member without
    an episode counting as worse than any) and the best has rank 1; members with equal means share a rank.  mean_returns: K
    numbers, NaN or None for a member without an episode (`Outcomes.by_member()["mean"]` of one seat, or averaged over both).
    Returns K floats summing to 1, for `PartnerPool.set_weights`.  Plain Python on K numbers; beta = 0 is uniform."""
    import math

    means = [None if m is None or math.isnan(float(m)) else float(m) for m in mean_returns]
    if not means:
        raise ValueError("rank_weights: no members")
    beta = float(beta)
    if beta < 0:
        raise ValueError("rank_weights: beta must not be negative, not %r" % beta)
    levels = sorted({m for m in means if m is not None}, reverse=True)  # best first: rank 1
    rank = {m: i + 1 for i, m in enumerate(levels)}
    worst = len(levels) + (1 if any(m is None for m in means) else 0)
    raw = [float((worst if m is None else rank[m]) ** beta) for m in means]
    total = sum(raw)
    return [x / total for x in raw]
