"""The learner's actor-critic on the device: `ActorCritic`, a torch module whose forward is oc_policy_forward (one launch) and
whose backward is oc_policy_backward (two), and `plan`.

    policy = ActorCritic(env.feature_length).to(device)           # in_dim -> 64 -> 64 -> 6 logits + a value, a shared trunk
    opt = torch.optim.Adam(policy.parameters(), 1e-3)
    logits, values = policy.act(env.features)                      # collecting: [N, 2, 6] and [N, 2], no graph
    for index in buf.minibatches(4096):
        loss, stats = ppo_loss(*policy(buf.features, index), batch, index, clip_param=0.05, ...)
        opt.zero_grad(); loss.backward(); opt.step()

The arithmetic is stated in include/oc_amd.h (OcActorCritic): the partner's fmaf chains with a value head, and for the backward pass
a fixed order of summation without atomics.  The C calls read the parameters' current storage at every call, so an optimiser's
in-place step is seen by the next call; nothing is cached."""
import ctypes
import functools
import re

import numpy as np
import torch

from . import _lib
from .gae import _checked, _stream
from .partner import MAX_HIDDEN, N_ACTIONS

NAMES = ("w1", "b1", "w2", "b2", "wp", "bp", "wv", "bv")
FEATURE_LENGTHS = tuple(2 * (pots * 10 + 26) + 4 for pots in range(5))


def shapes(in_dim, h1, h2):
    """The eight parameter shapes, in NAMES' order (the Keras layout: kernels [in, out])."""
    return ((in_dim, h1), (h1,), (h1, h2), (h2,), (h2, N_ACTIONS), (N_ACTIONS,), (h2,), (1,))


def plan(n_rows, index=False, in_dim=96, h1=64, h2=64, backward=False):
    """What a forward (backward=True: backward) call on n_rows rows launches, in oc_policy_plan's words (no device needed)."""
    out = ctypes.create_string_buffer(512)
    rc = _lib.load().oc_policy_plan(int(n_rows), int(bool(index)), int(in_dim), int(h1), int(h2), int(bool(backward)), out, len(out))
    _lib.check(rc, "oc_policy_plan")
    return out.value.decode()


@functools.lru_cache(maxsize=64)
def partials_shape(n_rows, in_dim, h1, h2):
    """(rows, floats) of the partial-gradient scratch of a backward call, read from the plan's words (and remembered: a training
    loop asks for the same few shapes again and again)."""
    m = re.search(r"(\d+) partial\(s\) of (\d+) floats", plan(n_rows, False, in_dim, h1, h2, backward=True))
    return int(m.group(1)), int(m.group(2))


def _call(fn, dev, *args):
    L = _lib.load()
    if torch.cuda.current_device() != (dev.index if dev.index is not None else torch.cuda.current_device()):
        with torch.cuda.device(dev):
            rc = getattr(L, fn)(*args, _stream(dev))
    else:
        rc = getattr(L, fn)(*args, _stream(dev))
    _lib.check(rc, fn)


def _structs(params, dims, features, index, first, n_rows):
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    pol = _lib.OcActorCritic(*[ptr(p) for p in params], *dims)
    rows = _lib.OcPolicyRows(ptr(features), features.numel() // dims[0], ptr(index), int(first), int(n_rows))
    return pol, rows


def _forward(params, dims, features, index, first, n_rows, out=None):
    dev = features.device
    if out is None:
        out = (torch.empty((n_rows, N_ACTIONS), dtype=torch.float32, device=dev), torch.empty((n_rows,), dtype=torch.float32, device=dev))
    pol, rows = _structs(params, dims, features, index, first, n_rows)
    _call("oc_policy_forward", dev, ctypes.byref(pol), ctypes.byref(rows), out[0].data_ptr(), out[1].data_ptr())
    return out


class _Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, index, first, n_rows, dims, *params):
        ctx.save_for_backward(features, *params)
        ctx.call = (index, first, n_rows, dims)
        logits, values = _forward([p.detach() for p in params], dims, features, index, first, n_rows)
        return logits, values

    @staticmethod
    def backward(ctx, grad_logits, grad_values):
        features, *params = ctx.saved_tensors
        index, first, n_rows, dims = ctx.call
        dev = features.device
        grad_logits = torch.zeros((n_rows, N_ACTIONS), dtype=torch.float32, device=dev) if grad_logits is None else grad_logits.contiguous()
        grad_values = torch.zeros((n_rows,), dtype=torch.float32, device=dev) if grad_values is None else grad_values.contiguous()
        grads = [torch.empty_like(p) for p in params]
        count, size = partials_shape(n_rows, *dims)
        partials = torch.empty((max(count, 1), size), dtype=torch.float32, device=dev)
        pol, rows = _structs(params, dims, features, index, first, n_rows)
        g = _lib.OcPolicyGrads(*[t.data_ptr() for t in grads])
        _call("oc_policy_backward", dev, ctypes.byref(pol), ctypes.byref(rows), grad_logits.data_ptr(), grad_values.data_ptr(), ctypes.byref(g),
              partials.data_ptr())
        return (None, None, None, None, None, *grads)


class ActorCritic(torch.nn.Module):
    """in_dim -> h1 -> h2 -> (6 logits, 1 value): eight float32 parameters w1, b1, w2, b2, wp, bp, wv, bv in the Keras layout.
    in_dim is a featurize_state length (56, 76, 96, 116 or 136), 1 <= h1, h2 <= 64.  Glorot-uniform kernels and zero biases from
    `seed`.  `.to(device)` moves it; every call needs the parameters on a GPU (there is no CPU fallback)."""

    def __init__(self, in_dim, h1=64, h2=64, seed=0):
        super().__init__()
        in_dim, h1, h2 = int(in_dim), int(h1), int(h2)
        if in_dim not in FEATURE_LENGTHS:
            raise ValueError("ActorCritic: in_dim = %d is no featurize_state length %r" % (in_dim, FEATURE_LENGTHS))
        for h, name in ((h1, "h1"), (h2, "h2")):
            if not 1 <= h <= MAX_HIDDEN:
                raise ValueError("ActorCritic: %s = %d, must be in 1..%d" % (name, h, MAX_HIDDEN))
        self.in_dim, self.h1, self.h2 = in_dim, h1, h2
        rng = np.random.default_rng([int(seed), in_dim, h1, h2])
        for name, shape in zip(NAMES, shapes(in_dim, h1, h2)):
            if name[0] == "w":
                fan_in, fan_out = (shape[0], shape[1]) if len(shape) == 2 else (shape[0], 1)
                lim = np.sqrt(6.0 / (fan_in + fan_out))
                a = rng.uniform(-lim, lim, shape).astype(np.float32)
            else:
                a = np.zeros(shape, np.float32)
            setattr(self, name, torch.nn.Parameter(torch.from_numpy(a)))

    @classmethod
    def from_weights(cls, w1, b1, w2, b2, wp, bp, wv, bv, device="cuda"):
        """From eight arrays or tensors of a floating dtype (kept as float32) in the Keras layout, moved to `device`."""
        host = []
        for name, a in zip(NAMES, (w1, b1, w2, b2, wp, bp, wv, bv)):
            if isinstance(a, torch.Tensor):
                a = a.detach().cpu().numpy()
            a = np.asarray(a)
            if a.dtype.kind != "f":
                raise ValueError("ActorCritic: %s must be a floating-point array, not %s" % (name, a.dtype))
            host.append(np.ascontiguousarray(a, dtype=np.float32))
        if host[0].ndim != 2 or host[2].ndim != 2:
            raise ValueError("ActorCritic: w1 and w2 must have 2 dimensions, not shapes %r and %r" % (host[0].shape, host[2].shape))
        self = cls(host[0].shape[0], host[0].shape[1], host[2].shape[1])
        for name, a, want in zip(NAMES, host, shapes(self.in_dim, self.h1, self.h2)):
            if a.shape != want:
                raise ValueError("ActorCritic: %s has shape %r, expected %r" % (name, a.shape, want))
            getattr(self, name).data = torch.from_numpy(a.copy())
        return self.to(device)

    def _params(self):
        return [getattr(self, n) for n in NAMES]

    def _checked_call(self, features, index, first):
        """(features, index, first, n_rows) of a call, or ValueError"""
        params = self._params()
        dev = params[0].device
        for name, p, shape in zip(NAMES, params, shapes(self.in_dim, self.h1, self.h2)):
            _checked("ActorCritic." + name, p.data, torch.float32, shape, dev, torch)
        if not isinstance(features, torch.Tensor) or features.dim() < 2 or features.shape[-1] != self.in_dim or features.dtype != torch.float32 \
                or not features.is_contiguous():
            raise ValueError("features must be a contiguous float32 [..., %d] tensor" % self.in_dim)
        if features.device != dev:
            raise ValueError("features are on %s, the parameters on %s" % (features.device, dev))
        if features.requires_grad:
            raise ValueError("features must not require a gradient: the backward pass returns the parameters' only")
        if features.data_ptr() % 16:
            raise ValueError("features must be 16-byte aligned")
        total = features.numel() // self.in_dim
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.dim() != 1:
                raise ValueError("index must be a contiguous int32 [M] tensor")
            _checked("index", index, torch.int32, (int(index.shape[0]),), dev, torch)
            if total >= 2 ** 31:
                raise ValueError("an index names feature rows below 2^31, there are %d" % total)
            first, n_rows = 0, int(index.shape[0])
        else:
            first = int(first)
            if first < 0 or first > total:
                raise ValueError("first = %d lies outside the features' 0 .. %d rows" % (first, total))
            n_rows = total - first
        if dev.type != "cuda":
            raise ValueError("ActorCritic works on device tensors, not on %s (there is no CPU fallback)" % dev)
        return params, n_rows, first

    def forward(self, features, index=None, first=0):
        """(logits float32 [M, 6], values float32 [M]) of the feature rows index int32 [M] names (out-of-range entries: zeros and
        no gradient), or without an index of rows first .. of `features`, any contiguous float32 tensor whose last dimension is
        in_dim (TrajectoryBuffer.features, the env's [N, 2, F] buffer).  Differentiable with respect to the eight parameters, not
        the features.  Raises ValueError for a tensor of another dtype, shape, device or layout and for host tensors."""
        params, n_rows, first = self._checked_call(features, index, first)
        dims = (self.in_dim, self.h1, self.h2)
        if not torch.is_grad_enabled() or not any(p.requires_grad for p in params):
            return _forward([p.detach() for p in params], dims, features, index, first, n_rows)
        return _Function.apply(features, index, first, n_rows, dims, *params)

    def act(self, features, out=None):
        """(logits [N, 2, 6], values [N, 2]) of the env's features [N, 2, in_dim] under no_grad, one launch: what step_sampled and
        TrajectoryBuffer.row take.  out: the pair of tensors to write."""
        if not isinstance(features, torch.Tensor) or features.dim() != 3 or features.shape[1] != 2:
            raise ValueError("features must be a contiguous float32 [N, 2, %d] tensor" % self.in_dim)
        N, dev = int(features.shape[0]), features.device
        if out is not None:
            _checked("out[0]", out[0], torch.float32, (N, 2, N_ACTIONS), dev, torch)
            _checked("out[1]", out[1], torch.float32, (N, 2), dev, torch)
            if out[0].data_ptr() % 8:
                raise ValueError("out[0] must be 8-byte aligned")
        params, n_rows, _ = self._checked_call(features, None, 0)
        if out is None:
            out = (torch.empty((N, 2, N_ACTIONS), dtype=torch.float32, device=dev), torch.empty((N, 2), dtype=torch.float32, device=dev))
        with torch.no_grad():
            _forward([p.detach() for p in params], (self.in_dim, self.h1, self.h2), features, None, 0, n_rows, out)
        return out

    def dense_policy(self):
        """A partner.DensePolicy snapshot of the trunk and the logit head (a copy: later optimiser steps do not reach it): a frozen
        self-play partner, or the start of behaviour cloning."""
        from .partner import DensePolicy

        w = [getattr(self, n).detach() for n in NAMES[:6]]
        return DensePolicy(*w, device=w[0].device)

    def plan(self, n_rows, index=False, backward=False):
        return plan(n_rows, index, self.in_dim, self.h1, self.h2, backward)
