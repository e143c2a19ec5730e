"""Behaviour cloning on the device: `bc_loss` (oc_bc_loss: sparse categorical cross-entropy from logits with optional class weights,
its gradients and its accuracy in one launch) and `BCLearner` (oc_bc_update: forward, loss, backward and optimiser step of a run of
minibatches in ONE C call; with fused=True oc_bc_epoch_fused: the same run in ONE kernel of one workgroup, for minibatches of at most
128 rows, bit for bit the same result) — the reference's BC objective (human_aware_rl/imitation/behavior_cloning_tf2.py) on the partner's network.

    feats, actions = ...                                          # rollout_featurize's feats_out[:-1] with actions[1:], or human data
    policy = ActorCritic(env.feature_length).to(device)
    learner = BCLearner(policy, lr=1e-3, class_weights=None)
    for _ in range(epochs):
        perm = torch.randperm(n_train, device=device, dtype=torch.int32)
        stats, info = learner.epoch(feats, actions, perm, 64)     # [K, 8] and [K, 4] on the device; fused=True: one kernel
    held_out = learner.evaluate(feats, actions, validation_index) # BcStats: .loss, .accuracy
    env = VecOvercookedMultiAgent(..., bc_policy=policy.dense_policy())

or, with autograd and a network of one's own,

    loss, stats = bc_loss(logits, actions, index)
    loss.backward()

The arithmetic is stated in include/oc_amd.h (OcBcLoss, OcBcUpdate): a row whose index names no sample or whose action is above 5 is
left out; the loss is the sum of c * ce over the kept rows divided by their count (Keras's class_weight convention); a minibatch
without a kept row is skipped (`info[..., 3]` is 1).  Nothing here synchronises with the host."""
import collections
import ctypes
import re

import torch

from . import _lib
from .gae import _checked, _stream
from .learner import _ChainLearner, _ptr, _scratch_rows
from .policy import ActorCritic, _forward

BcStats = collections.namedtuple("BcStats", "tensor count loss accuracy mean_weight inv_count")
N_ACTIONS = 6

_PARTIAL = None


def plan_bc_loss(n_minibatch, index=False, class_weights=False, gradients=True, loss_out=False):
    """What bc_loss() launches for M minibatch rows, in oc_bc_loss_plan's words (no device needed)."""
    out = ctypes.create_string_buffer(320)
    rc = _lib.load().oc_bc_loss_plan(int(n_minibatch), int(bool(index)), int(bool(class_weights)), int(bool(gradients)), int(bool(loss_out)),
                                     out, len(out))
    _lib.check(rc, "oc_bc_loss_plan")
    return out.value.decode()


def plan_bc_update(n_index, minibatch, in_dim=96, h1=64, h2=64, class_weights=False):
    """What BCLearner.epoch() launches for an index of n_index entries cut into minibatches of `minibatch`, in oc_bc_update_plan's
    words: K, the kernels of one minibatch and the sizes of the scratch (no device needed)."""
    out = ctypes.create_string_buffer(2048)
    rc = _lib.load().oc_bc_update_plan(int(n_index), int(minibatch), int(in_dim), int(h1), int(h2), int(bool(class_weights)), out, len(out))
    _lib.check(rc, "oc_bc_update_plan")
    return out.value.decode()


def plan_bc_epoch_fused(n_index, minibatch, in_dim=96, h1=64, h2=64, class_weights=False):
    """What BCLearner.epoch(..., fused=True) launches, in oc_bc_epoch_fused_plan's words: the kernel instance, the minibatches, the
    launches and the LDS (no device needed).  ValueError with the library's message for a shape the fused kernel does not serve (a
    minibatch above 128 rows, an in_dim other than 56, 76 or 96)."""
    out = ctypes.create_string_buffer(1024)
    L = _lib.load()
    rc = L.oc_bc_epoch_fused_plan(int(n_index), int(minibatch), int(in_dim), int(h1), int(h2), int(bool(class_weights)), out, len(out))
    if rc != 0:
        raise ValueError(L.oc_last_error().decode(errors="replace"))
    return out.value.decode()


def partial_samples():
    """P, the minibatch rows per row of partial sums, read from oc_bc_loss_plan's words (no device needed)."""
    global _PARTIAL
    if _PARTIAL is None:
        _PARTIAL = int(re.search(r"(\d+) samples per partial", plan_bc_loss(1)).group(1))
    return _PARTIAL


def scratch_rows(n_index, minibatch, in_dim, h1, h2):
    """(rows of a minibatch, rows of the loss partials, rows of the policy partials, floats of a policy partial), read from the
    plan's words."""
    return _scratch_rows(plan_bc_update(n_index, minibatch, in_dim, h1, h2), 4)


def _weights(class_weights):
    """None, or the six class weights as a float32 [6] host tensor; ValueError for anything that is not six finite numbers >= 0."""
    if class_weights is None:
        return None
    try:
        w = torch.as_tensor(class_weights).detach().to("cpu", torch.float32).contiguous()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("class_weights must be six finite numbers >= 0 or None, not %r" % (class_weights,))
    if tuple(w.shape) != (N_ACTIONS,) or not bool(torch.isfinite(w).all()) or not bool((w >= 0).all()):
        raise ValueError("class_weights must be six finite numbers >= 0 or None, not %r" % (class_weights,))
    return w


def _checked_actions(actions, dev):
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.uint8 or not actions.is_contiguous() or actions.device != dev:
        raise ValueError("actions must be a contiguous uint8 tensor on %s" % dev)
    return int(actions.numel())


def _call(fn, dev, *args):
    L = _lib.load()
    with torch.cuda.device(dev):
        rc = getattr(L, fn)(*args, _stream(dev))
    _lib.check(rc, fn)


def _head(logits, actions, index, first, weights, gradients):
    """One oc_bc_loss call on checked tensors: (grad_logits or None, stats)."""
    M, dev = int(logits.shape[0]), logits.device
    grad_logits = torch.empty((M, N_ACTIONS), dtype=torch.float32, device=dev) if gradients else None
    grad_values = torch.empty((M,), dtype=torch.float32, device=dev) if gradients else None
    P = partial_samples()
    partials = torch.empty((max((M + P - 1) // P, 1), 4), dtype=torch.float64, device=dev)
    stats = torch.empty((8,), dtype=torch.float64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    q = _lib.OcBcLoss(ptr(actions), ptr(weights), int(actions.numel()), ptr(logits), ptr(index), int(first), M, ptr(grad_logits), ptr(grad_values),
                      None, ptr(partials), ptr(stats))
    _call("oc_bc_loss", dev, ctypes.byref(q))
    return grad_logits, stats


class _BcLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, actions, index, first, weights, box):
        grad_logits, stats = _head(logits, actions, index, first, weights, True)
        ctx.save_for_backward(grad_logits, stats)
        box.append(stats)
        return stats[1].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        grad_logits, stats = ctx.saved_tensors
        scale = (grad_out.to(torch.float64) * stats[7]).to(torch.float32)  # a device scalar: grad_out / count
        return grad_logits * scale, None, None, None, None, None


def _stats(t):
    return BcStats(t, t[0], t[1], t[2], t[3], t[7])


def bc_loss(logits, actions, index=None, first=0, class_weights=None):
    """(loss, stats) of the policy's logits float32 [M, 6] on the demonstrated actions, a contiguous uint8 tensor of S elements, that
    index int32 [M] names (None: samples first .. first + M - 1).  loss: a 0-dim float32 tensor, the sum over the kept rows of
    class_weights[a] * cross-entropy divided by their count, whose backward() hands the logits the gradients the same launch computed.
    stats: BcStats — the float64 [8] tensor on the device and 0-dim views of it (count, loss, accuracy, mean_weight, inv_count).
    class_weights: six finite numbers >= 0, or None.  Raises ValueError for a tensor of another dtype, shape, device or layout and for
    a tensor on the host (there is no CPU fallback)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != N_ACTIONS:
        raise ValueError("logits must be a contiguous float32 [M, 6] tensor")
    M, dev = int(logits.shape[0]), logits.device
    _checked("logits", logits, torch.float32, (M, N_ACTIONS), dev, torch)
    S = _checked_actions(actions, dev)
    if index is not None:
        _checked("index", index, torch.int32, (M,), dev, torch)
        if S >= 2 ** 31:
            raise ValueError("an index names samples below 2^31, there are %d" % S)
        first = 0
    else:
        first = int(first)
        if first < 0 or first + M > S:
            raise ValueError("samples %d .. %d lie outside the actions' 0 .. %d" % (first, first + M - 1, S - 1))
    weights = _weights(class_weights)
    if dev.type != "cuda":
        raise ValueError("bc_loss works on device tensors, not on %s (there is no CPU fallback)" % dev)
    if weights is not None:
        weights = weights.to(dev)
    box = []
    loss = _BcLossFunction.apply(logits, actions, index, first, weights, box)
    return loss, _stats(box[0])


class BCLearner(_ChainLearner):
    """The whole update of a behaviour-cloning minibatch — policy forward, weighted cross-entropy, backward to the weights, clipped
    Adam step — as stream-ordered kernels behind ONE C call (oc_bc_update), for one minibatch (`update`) or a whole pass over a
    permutation (`epoch`), and `evaluate`, the loss and accuracy of held-out samples.  The optimiser's hyperparameters are Adam's
    (`self.adam`, whose state_dict holds the moments).  The value head gets zero gradients.  No autograd: the parameters' `.grad`s are
    not touched."""

    _plan, _WIDTH, _UPDATE, _ENTRY = staticmethod(plan_bc_update), 4, _lib.OcBcUpdate, "oc_bc_update"

    def __init__(self, policy, lr=1e-3, class_weights=None, max_grad_norm=None, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(policy, ActorCritic):
            raise ValueError("BCLearner: policy must be an ActorCritic")
        super().__init__(policy, lr, betas, eps, max_grad_norm)
        self.class_weights = _weights(class_weights)
        self._weights_on = None  # the class weights on the parameters' device

    def _device_weights(self, dev):
        if self.class_weights is None:
            return None
        if self._weights_on is None or self._weights_on.device != dev:
            self._weights_on = self.class_weights.to(dev)
        return self._weights_on

    def _check_batch(self, features, actions, index, dev):
        pol = self.policy
        self._check_features(features, dev)
        S = _checked_actions(actions, dev)
        if S != features.numel() // pol.in_dim:
            raise ValueError("actions must have one element per feature row: %d, not %d" % (features.numel() // pol.in_dim, S))
        if index is not None:
            self._check_index(index, dev)
            if S >= 2 ** 31:
                raise ValueError("an index names samples and feature rows below 2^31")
        return S

    def _run(self, features, actions, index, minibatch, fused=False):
        minibatch = int(minibatch)
        if fused and minibatch >= 1:  # the shapes oc_bc_epoch_fused serves, in the library's words, ahead of everything that needs a device
            rows = int(index.shape[0]) if isinstance(index, torch.Tensor) and index.dim() == 1 else 0
            plan_bc_epoch_fused(rows, minibatch, self.policy.in_dim, self.policy.h1, self.policy.h2)
        params, dev = self.adam._device_params()
        if index is None:
            raise ValueError("index must be a contiguous int32 [n] tensor")
        S = self._check_batch(features, actions, index, dev)
        self._check_minibatch(minibatch)
        self.adam._state(dev)
        weights = self._device_weights(dev)
        key = (int(index.shape[0]), minibatch, _ptr(features), S, _ptr(index), _ptr(actions), _ptr(weights))
        loss = lambda: _lib.OcBcLoss(_ptr(actions), _ptr(weights), S, None, None, 0, 0, None, None, None, None, None)  # noqa: E731
        if fused:
            return self._run_fused(key, loss, features, index, minibatch, params, dev, S)
        return self._chain(key, loss, features, S, index, minibatch, params, dev)

    def _run_fused(self, key, loss, features, index, minibatch, params, dev, S):
        """oc_bc_epoch_fused on checked tensors: no scratch (self._scratch is not touched), the optimiser's moments and clock"""
        n = int(index.shape[0])
        polc, q, ad, e = self._cached(("fused",) + key, params, loss, lambda: _lib.OcBcEpochFused(_ptr(features), S, _ptr(index), n, minibatch, None, None))
        stats, info = self._outputs(n, minibatch, dev, e, ad)
        L = _lib.load()
        with torch.cuda.device(dev):
            rc = L.oc_bc_epoch_fused(ctypes.byref(polc), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(e), _stream(dev))
        if rc == -1:  # (OC_EINVAL: a shape or an array the library does not serve)
            raise ValueError(L.oc_last_error().decode(errors="replace"))
        _lib.check(rc, "oc_bc_epoch_fused")
        return stats, info

    def update(self, features, actions, index, fused=False):
        """One minibatch: the rows of `features` (any contiguous float32 [..., in_dim] tensor) and the elements of `actions` (a
        contiguous uint8 tensor, one element per feature row) that index int32 [M] names.  (stats float64 [1, 8] — bc_loss's
        BcStats.tensor —, info float64 [1, 4] — Adam's), on the device.  fused: see epoch()."""
        rows = int(index.shape[0]) if isinstance(index, torch.Tensor) and index.dim() == 1 else 1  # (_run refuses what is no index)
        return self._run(features, actions, index, max(rows, 1), fused)

    def epoch(self, features, actions, permutation, minibatch, fused=False):
        """One pass: the index int32 [n] cut into K = ceil(n / minibatch) minibatches, the last one shorter, each updated from the
        weights the one before left — ONE C call.  (stats [K, 8], info [K, 4]) on the device.
        fused=True: the pass runs in ONE kernel of one workgroup (oc_bc_epoch_fused) instead of six launches per minibatch; the
        results are the same bit for bit, no scratch is used, and the optimiser's state is shared, so fused and staged calls may
        alternate.  It serves minibatches of 1..128 rows and in_dim 56, 76 or 96 and raises ValueError, with the library's message,
        for anything else."""
        return self._run(features, actions, permutation, minibatch, fused)

    def evaluate(self, features, actions, index=None):
        """The loss and accuracy of the samples index int32 [M] names (None: all of them) under the current weights: the forward
        pass and the head without gradient stores.  BcStats on the device; no weight, moment or `.grad` is touched."""
        params, dev = self.adam._device_params()
        self._check_batch(features, actions, index, dev)
        params, n_rows, first = self.policy._checked_call(features, index, 0)
        with torch.no_grad():
            logits, _ = _forward([p.detach() for p in params], (self.policy.in_dim, self.policy.h1, self.policy.h2), features, index, first, n_rows)
        _, stats = _head(logits, actions, index, 0, self._device_weights(dev), False)
        return _stats(stats)
