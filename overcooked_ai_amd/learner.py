"""The PPO learner's update on the device: `Adam` (oc_adam_step: gradient clipping by global norm and Adam in ONE launch) and
`PPOLearner` (oc_ppo_update: forward, loss, backward and optimiser step of a run of minibatches in ONE C call).

    policy = ActorCritic(env.feature_length).to(device)
    learner = PPOLearner(policy, lr=1e-3, clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=0.1, max_grad_norm=0.1)
    adv, targets, moments = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, targets, moments)
    for _ in range(num_sgd_iter):
        stats, info = learner.epoch(buf.features, batch, buf.permutation(), 2000)     # [K, 8] and [K, 4] on the device

or, with autograd and a loss of one's own,

    opt = Adam(policy, lr=1e-3, max_grad_norm=0.1)
    opt.zero_grad(); loss.backward(); opt.step()                                      # instead of clip_grad_norm_ + torch.optim.Adam

The arithmetic is stated in include/oc_amd.h (OcAdam, OcPpoUpdate): the norm's order of summation is fixed, a step whose norm is not
finite or whose minibatch has no learner sample is skipped (nothing is written, `info[..., 3]` is 1 and the clock's fourth number
counts it).  Nothing here synchronises with the host."""
import ctypes
import re

import torch

from . import _lib
from .gae import _checked, _stream
from .policy import NAMES, ActorCritic, shapes
from .ppo_loss import LearnerBatch

CLOCK0 = (0.0, 1.0, 1.0, 0.0)  # steps, beta1^steps, beta2^steps, skipped


def plan_adam(in_dim=96, h1=64, h2=64):
    """What Adam.step() launches, in oc_adam_plan's words (no device needed)."""
    out = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().oc_adam_plan(int(in_dim), int(h1), int(h2), out, len(out)), "oc_adam_plan")
    return out.value.decode()


def plan_update(n_index, minibatch, in_dim=96, h1=64, h2=64, seat=False, moments=False, old_logits=False):
    """What PPOLearner.epoch() launches for an index of n_index entries cut into minibatches of `minibatch`, in oc_ppo_update_plan's
    words: K, the kernels of one minibatch and the sizes of the scratch (no device needed)."""
    out = ctypes.create_string_buffer(2048)
    rc = _lib.load().oc_ppo_update_plan(int(n_index), int(minibatch), int(in_dim), int(h1), int(h2), int(bool(seat)), int(bool(moments)),
                                        int(bool(old_logits)), out, len(out))
    _lib.check(rc, "oc_ppo_update_plan")
    return out.value.decode()


def scratch_rows(n_index, minibatch, in_dim, h1, h2):
    """(rows of a minibatch, rows of the loss partials, rows of the policy partials, floats of a policy partial), read from the
    plan's words."""
    return _scratch_rows(plan_update(n_index, minibatch, in_dim, h1, h2), 6)


def _scratch_rows(text, width):
    """scratch_rows() of an update plan's words whose loss partials are `width` f64 wide."""
    m = re.search(r"scratch: logits (\d+) x 6 f32.*loss partials (\d+) x %d f64, policy partials (\d+) x (\d+) f32" % width, text)
    return tuple(int(x) for x in m.groups())


def _hyper(lr, betas, eps, max_grad_norm):
    import math

    lr, b1, b2, eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
    if not (math.isfinite(lr) and lr >= 0):
        raise ValueError("lr must be finite and >= 0, not %r" % lr)
    if not (0 <= b1 < 1 and 0 <= b2 < 1):
        raise ValueError("betas must be in [0, 1), not %r" % ((b1, b2),))
    if not eps > 0:
        raise ValueError("eps must be positive, not %r" % eps)
    if max_grad_norm is not None:
        max_grad_norm = float(max_grad_norm)
        if not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive or None, not %r" % max_grad_norm)
    return lr, b1, b2, eps, max_grad_norm


class Adam:
    """Adam on the eight parameters of an ActorCritic, with gradient clipping by global norm when max_grad_norm is given: step() is
    ONE launch (oc_adam_step).  The moments (float32, the parameters' shapes), the clock (float64 [4]: steps, beta1^steps,
    beta2^steps, skipped) and `info` (float64 [4]: the norm before clipping, the clip factor, the gradient scale, 1 if the step was
    skipped) live on the parameters' device and are allocated at the first step (or by load_state_dict)."""

    def __init__(self, policy, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        if not isinstance(policy, ActorCritic):
            raise ValueError("Adam: policy must be an ActorCritic")
        self.policy = policy
        self.lr, self.beta1, self.beta2, self.eps, self.max_grad_norm = _hyper(lr, betas, eps, max_grad_norm)
        self.m = self.v = self.clock = self.info = None
        self._call = None

    def _state(self, dev):
        if self.m is None or self.m[0].device != dev:
            dims = (self.policy.in_dim, self.policy.h1, self.policy.h2)
            self.m = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes(*dims)]
            self.v = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes(*dims)]
            self.clock = torch.tensor(CLOCK0, dtype=torch.float64, device=dev)
            self.info = torch.zeros(4, dtype=torch.float64, device=dev)
            self._call = None

    def _struct(self, grad_scale=None, info=None):
        ptrs = ctypes.c_void_p * 8
        return _lib.OcAdam(ptrs(*[t.data_ptr() for t in self.m]), ptrs(*[t.data_ptr() for t in self.v]), self.clock.data_ptr(),
                           grad_scale, self.info.data_ptr() if info is None else info, self.lr, self.beta1, self.beta2, self.eps,
                           self.max_grad_norm if self.max_grad_norm is not None else 0.0)

    def _device_params(self):
        params = self.policy._params()
        dev = params[0].device
        if dev.type != "cuda":
            raise ValueError("Adam works on device tensors, not on %s (there is no CPU fallback)" % dev)
        for name, p, shape in zip(NAMES, params, shapes(self.policy.in_dim, self.policy.h1, self.policy.h2)):
            _checked("ActorCritic." + name, p.data, torch.float32, shape, dev, torch)
        return params, dev

    def step(self):
        """One clipped Adam step from the eight `.grad`s (ValueError where one is missing or of another dtype, shape or layout)."""
        params, dev = self._device_params()
        self._state(dev)
        for name, p in zip(NAMES, params):
            if p.grad is None:
                raise ValueError("Adam.step: %s has no gradient" % name)
            _checked(name + ".grad", p.grad, torch.float32, tuple(p.shape), dev, torch)
        key = tuple(p.data_ptr() for p in params) + tuple(p.grad.data_ptr() for p in params)
        if self._call is None or self._call[0] != key:  # (the structs are rebuilt only when a tensor has moved)
            pol = _lib.OcActorCritic(*key[:8], self.policy.in_dim, self.policy.h1, self.policy.h2)
            self._call = (key, pol, _lib.OcPolicyGrads(*key[8:]), self._struct())
        _, pol, grads, ad = self._call
        ad.lr, ad.max_grad_norm = self.lr, self.max_grad_norm if self.max_grad_norm is not None else 0.0  # (a schedule may have set them)
        with torch.cuda.device(dev):
            rc = _lib.load().oc_adam_step(ctypes.byref(pol), ctypes.byref(grads), ctypes.byref(ad), _stream(dev))
        _lib.check(rc, "oc_adam_step")

    def zero_grad(self, set_to_none=False):
        """Zero the eight gradients in place (set_to_none: drop them instead; the next backward allocates new ones)."""
        for p in self.policy._params():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def state_dict(self):
        """The moments and the clock (clones; zeros and the initial clock before the first step) and the hyperparameters."""
        dims = (self.policy.in_dim, self.policy.h1, self.policy.h2)
        m = [t.clone() for t in self.m] if self.m is not None else [torch.zeros(s) for s in shapes(*dims)]
        v = [t.clone() for t in self.v] if self.v is not None else [torch.zeros(s) for s in shapes(*dims)]
        clock = self.clock.clone() if self.clock is not None else torch.tensor(CLOCK0, dtype=torch.float64)
        return {"m": dict(zip(NAMES, m)), "v": dict(zip(NAMES, v)), "clock": clock, "lr": self.lr, "betas": (self.beta1, self.beta2),
                "eps": self.eps, "max_grad_norm": self.max_grad_norm}

    def load_state_dict(self, state):
        """Take the moments, the clock and the hyperparameters of a state_dict(), onto the parameters' device."""
        dev = self.policy._params()[0].device
        dims = (self.policy.in_dim, self.policy.h1, self.policy.h2)
        for which in ("m", "v"):
            for name, shape in zip(NAMES, shapes(*dims)):
                t = state[which][name]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32:
                    raise ValueError("Adam.load_state_dict: %s[%s] must be a float32 %s tensor" % (which, name, list(shape)))
        if not isinstance(state["clock"], torch.Tensor) or tuple(state["clock"].shape) != (4,) or state["clock"].dtype != torch.float64:
            raise ValueError("Adam.load_state_dict: clock must be a float64 [4] tensor")
        self.lr, self.beta1, self.beta2, self.eps, self.max_grad_norm = _hyper(state["lr"], state["betas"], state["eps"], state["max_grad_norm"])
        self.m = [state["m"][n].detach().to(dev, copy=True).contiguous() for n in NAMES]
        self.v = [state["v"][n].detach().to(dev, copy=True).contiguous() for n in NAMES]
        self.clock = state["clock"].detach().to(dev, copy=True)
        self.info = torch.zeros(4, dtype=torch.float64, device=dev)
        self._call = None


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _ChainLearner:
    """What the learners of the update chain (csrc/update_chain.hpp) share: the optimiser, the scratch of a minibatch, the cache of a
    call's ctypes structs (rebuilt only when an address changes) and the call itself.  A learner supplies its batch checks, the head of
    its cache key, its loss struct and
        _plan     its plan call, (n_index, minibatch, in_dim, h1, h2) -> text
        _WIDTH    the f64 of a row of its loss partials
        _UPDATE   its update struct
        _ENTRY    its entry point's name"""

    def __init__(self, policy, lr, betas, eps, max_grad_norm):
        self.adam = Adam(policy, lr, betas, eps, max_grad_norm)
        self.policy = policy
        self._scratch = {}   # (rows of a minibatch) -> the tensors of one minibatch
        self._calls = {}     # the addresses and sizes of a call -> its ctypes structs

    def scratch(self, rows):
        """The scratch of minibatches of up to `rows` rows, as a dict of tensors: logits, values, grad_logits, grad_values, the loss
        and policy partials and `grads`, the eight RAW gradient arrays (a sum over the minibatch, not divided by its count)."""
        return self._scratch[rows]

    def _check_features(self, features, dev):
        pol = self.policy
        if not isinstance(features, torch.Tensor) or features.dim() < 2 or features.shape[-1] != pol.in_dim or features.dtype != torch.float32 \
                or not features.is_contiguous() or features.device != dev:
            raise ValueError("features must be a contiguous float32 [..., %d] tensor on %s" % (pol.in_dim, dev))
        if features.data_ptr() % 16:
            raise ValueError("features must be 16-byte aligned")

    @staticmethod
    def _check_index(index, dev):
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index must be a contiguous int32 [n] tensor")
        _checked("index", index, torch.int32, (int(index.shape[0]),), dev, torch)

    @staticmethod
    def _check_minibatch(minibatch):
        if minibatch < 1:
            raise ValueError("minibatch must be at least 1, not %d" % minibatch)

    def _cached(self, key_head, params, loss, update):
        """The policy, loss, optimiser and update structs of the call `key_head` names on these parameters, moments and clock
        (load_state_dict brings new moments and a new clock); loss() and update() build the second and the fourth.  Up to 64 are kept."""
        key = key_head + tuple(_ptr(p) for p in params) + tuple(_ptr(t) for t in self.adam.m) + (_ptr(self.adam.clock),)
        call = self._calls.get(key)
        if call is None:
            pol = self.policy
            call = (_lib.OcActorCritic(*[_ptr(p) for p in params], pol.in_dim, pol.h1, pol.h2), loss(), self.adam._struct(), update())
            if len(self._calls) >= 64:
                self._calls.clear()
            self._calls[key] = call
        return call

    def _outputs(self, n, minibatch, dev, u, ad):
        """New stats [K, 8] and info [K, 4], bound to the update struct `u`; the optimiser's struct with today's lr and max_grad_norm."""
        K = (n + minibatch - 1) // minibatch
        stats = torch.empty((K, 8), dtype=torch.float64, device=dev)
        info = torch.empty((K, 4), dtype=torch.float64, device=dev)
        u.d_stats, u.d_info = stats.data_ptr(), info.data_ptr()
        ad.lr, ad.max_grad_norm = self.adam.lr, self.adam.max_grad_norm if self.adam.max_grad_norm is not None else 0.0
        return stats, info

    def _chain(self, key_head, loss, features, n_feature_rows, index, minibatch, params, dev):
        """The entry point on checked tensors.  key_head: what names the call beside parameters, moments and clock; loss: () -> the
        loss struct of a call that is not in the cache."""
        n = int(index.shape[0])

        def update():
            dims = (self.policy.in_dim, self.policy.h1, self.policy.h2)
            rows, loss_rows, pol_rows, size = _scratch_rows(self._plan(n, minibatch, *dims), self._WIDTH)
            s = self._scratch.get(rows)
            if s is None or s["logits"].device != dev:
                f32 = dict(dtype=torch.float32, device=dev)
                s = dict(logits=torch.empty((max(rows, 1), 6), **f32), values=torch.empty((max(rows, 1),), **f32),
                         grad_logits=torch.empty((max(rows, 1), 6), **f32), grad_values=torch.empty((max(rows, 1),), **f32),
                         loss_partials=torch.empty((loss_rows, self._WIDTH), dtype=torch.float64, device=dev),
                         policy_partials=torch.empty((pol_rows, size), **f32), grads=[torch.empty(sh, **f32) for sh in shapes(*dims)])
                self._scratch[rows] = s
            return self._UPDATE(_ptr(features), n_feature_rows, _ptr(index), n, minibatch, _ptr(s["logits"]), _ptr(s["values"]),
                                _ptr(s["grad_logits"]), _ptr(s["grad_values"]), _ptr(s["loss_partials"]), _ptr(s["policy_partials"]),
                                _lib.OcPolicyGrads(*[_ptr(t) for t in s["grads"]]), None, None)

        polc, q, ad, u = self._cached(key_head, params, loss, update)
        stats, info = self._outputs(n, minibatch, dev, u, ad)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), self._ENTRY)(ctypes.byref(polc), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(u), _stream(dev))
        _lib.check(rc, self._ENTRY)
        return stats, info


class PPOLearner(_ChainLearner):
    """The whole update of a PPO minibatch — policy forward, clipped-surrogate loss, backward to the weights, clipped Adam step — as
    stream-ordered kernels behind ONE C call (oc_ppo_update), for one minibatch (`update`) or a whole pass over a permutation
    (`epoch`).  The loss's hyperparameters are ppo_loss()'s, the optimiser's are Adam's (`self.adam`, whose state_dict holds the
    moments).  No autograd: the parameters' `.grad`s are not touched."""

    _plan, _WIDTH, _UPDATE, _ENTRY = staticmethod(plan_update), 6, _lib.OcPpoUpdate, "oc_ppo_update"

    def __init__(self, policy, lr, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff=0.0, max_grad_norm=None,
                 betas=(0.9, 0.999), eps=1e-8):
        import math

        super().__init__(policy, lr, betas, eps, max_grad_norm)
        self.hyper = tuple(float(x) for x in (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff))
        if not all(math.isfinite(x) and x > 0 for x in self.hyper[:2]):
            raise ValueError("clip_param and vf_clip_param must be finite and positive, not %r and %r" % self.hyper[:2])
        if not all(x >= 0 for x in self.hyper[2:]):
            raise ValueError("vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0, not %r, %r and %r" % self.hyper[2:])

    def _check_batch(self, features, batch, index, dev):
        self._check_features(features, dev)
        if not isinstance(batch, LearnerBatch):
            raise ValueError("batch must be a LearnerBatch (TrajectoryBuffer.learner_batch)")
        if not isinstance(batch.actions, torch.Tensor) or batch.actions.dim() != 1:
            raise ValueError("batch.actions must be a contiguous uint8 [S] tensor")
        S = int(batch.actions.shape[0])
        _checked("batch.actions", batch.actions, torch.uint8, (S,), dev, torch)
        _checked("batch.logp_old", batch.logp_old, torch.float32, (S,), dev, torch)
        _checked("batch.advantages", batch.advantages, torch.float32, (S,), dev, torch)
        _checked("batch.targets", batch.targets, torch.float32, (S,), dev, torch)
        if batch.seat is not None:
            if S % 2:
                raise ValueError("batch.seat needs an even number of samples, not %d" % S)
            _checked("batch.seat", batch.seat, torch.uint8, (S // 2,), dev, torch)
        if batch.logits_old is not None:
            _checked("batch.logits_old", batch.logits_old, torch.float32, (S, 6), dev, torch)
        if batch.moments is not None:
            _checked("batch.moments", batch.moments, torch.float64, (3,), dev, torch)
        if self.hyper[4] > 0 and batch.logits_old is None:
            raise ValueError("kl_coeff > 0 needs the batch's old logits (TrajectoryBuffer(keep_logits=True))")
        self._check_index(index, dev)
        if S >= 2 ** 31 or features.numel() // self.policy.in_dim >= 2 ** 31:
            raise ValueError("an index names samples and feature rows below 2^31")
        return S

    def _run(self, features, batch, index, minibatch):
        params, dev = self.adam._device_params()
        S = self._check_batch(features, batch, index, dev)
        minibatch = int(minibatch)
        self._check_minibatch(minibatch)
        self.adam._state(dev)
        key = (int(index.shape[0]), minibatch, _ptr(features), features.numel(), _ptr(index), S) + tuple(_ptr(t) for t in batch)
        loss = lambda: _lib.OcPpoLoss(_ptr(batch.actions), _ptr(batch.logp_old), _ptr(batch.advantages), _ptr(batch.targets), _ptr(batch.seat),  # noqa: E731
                                      _ptr(batch.logits_old), _ptr(batch.moments), S, None, None, None, 0, 0, None, None, None, None, None, *self.hyper)
        return self._chain(key, loss, features, features.numel() // self.policy.in_dim, index, minibatch, params, dev)

    def update(self, features, batch, index):
        """One minibatch: the rows of `features` (any contiguous float32 [..., in_dim] tensor) and the samples of `batch` (a
        LearnerBatch) that index int32 [M] names.  (stats float64 [1, 8] — ppo_loss's PpoStats.tensor —, info float64 [1, 4] —
        Adam's), on the device."""
        rows = int(index.shape[0]) if isinstance(index, torch.Tensor) and index.dim() == 1 else 1  # (_run refuses what is no index)
        return self._run(features, batch, index, max(rows, 1))

    def epoch(self, features, batch, permutation, minibatch):
        """One pass: the index int32 [n] (TrajectoryBuffer.permutation) cut into K = ceil(n / minibatch) minibatches, the last one
        shorter, each updated from the weights the one before left — ONE C call.  (stats [K, 8], info [K, 4]) on the device."""
        return self._run(features, batch, permutation, minibatch)
