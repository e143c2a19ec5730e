"""The PPO loss head on the device: `ppo_loss` (oc_ppo_loss, one launch) and `plan_ppo_loss`.

    adv, targets, moments = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, targets, moments)
    for index in buf.minibatches(4096):
        logits, values = policy(buf.features.view(-1, F)[index.long()])
        loss, stats = ppo_loss(logits, values, batch, index, clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=0.1)
        loss.backward()

The clipped-surrogate loss of the minibatch rows that are learner samples (not the partner's, not an invalid row's), its mean terms
and — saved for backward — its gradients with respect to logits and values.  The arithmetic is stated in include/oc_amd.h
(OcPpoLoss).  Nothing here synchronises with the host: the count the mean divides by stays on the device."""
import collections
import ctypes

from .gae import _checked, _stream

LearnerBatch = collections.namedtuple("LearnerBatch", "actions logp_old advantages targets seat logits_old moments")
PpoStats = collections.namedtuple("PpoStats", "tensor count total policy_loss vf_loss entropy kl clip_frac inv_count terms")

_PARTIAL = None


def partial_samples():
    """P, the minibatch rows per row of partial sums, read from oc_ppo_loss_plan's words (no device needed)."""
    global _PARTIAL
    if _PARTIAL is None:
        import re

        _PARTIAL = int(re.search(r"(\d+) samples per partial", plan_ppo_loss(1)).group(1))
    return _PARTIAL


def _call(q, dev):
    import torch

    from . import _lib

    L = _lib.load()
    if torch.cuda.current_device() != (dev.index if dev.index is not None else torch.cuda.current_device()):
        with torch.cuda.device(dev):
            rc = L.oc_ppo_loss(ctypes.byref(q), _stream(dev))
    else:
        rc = L.oc_ppo_loss(ctypes.byref(q), _stream(dev))
    _lib.check(rc, "oc_ppo_loss")


def _forward(logits, values, batch, index, first, hyper, terms):
    """One oc_ppo_loss call on checked tensors: (grad_logits, grad_values, stats, terms or None)."""
    import torch

    from . import _lib

    M, dev = int(logits.shape[0]), logits.device
    S = int(batch.actions.shape[0])
    grad_logits = torch.empty((M, 6), dtype=torch.float32, device=dev)
    grad_values = torch.empty((M,), dtype=torch.float32, device=dev)
    P = partial_samples()
    partials = torch.empty(((M + P - 1) // P, 6), dtype=torch.float64, device=dev)
    stats = torch.empty((8,), dtype=torch.float64, device=dev)
    terms_out = torch.empty((M, 4), dtype=torch.float32, device=dev) if terms else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    q = _lib.OcPpoLoss(ptr(batch.actions), ptr(batch.logp_old), ptr(batch.advantages), ptr(batch.targets), ptr(batch.seat),
                       ptr(batch.logits_old), ptr(batch.moments), S, ptr(logits), ptr(values), ptr(index), int(first), M,
                       ptr(grad_logits), ptr(grad_values), ptr(partials), ptr(stats), ptr(terms_out), *hyper)
    _call(q, dev)
    return grad_logits, grad_values, stats, terms_out


def _function():
    import torch

    class PpoLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, values, batch, index, first, hyper, terms, box):
            grad_logits, grad_values, stats, terms_out = _forward(logits, values, batch, index, first, hyper, terms)
            ctx.save_for_backward(grad_logits, grad_values, stats)
            box.extend((stats, terms_out))
            return stats[1].to(torch.float32)

        @staticmethod
        def backward(ctx, grad_out):
            grad_logits, grad_values, stats = ctx.saved_tensors
            scale = (grad_out.to(torch.float64) * stats[7]).to(torch.float32)  # a device scalar: grad_out / count
            return grad_logits * scale, grad_values * scale, None, None, None, None, None, None

    return PpoLossFunction


_FUNCTION = None


def ppo_loss(logits, values, batch, index=None, first=0, *, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff=0.0,
             terms=False):
    """(loss, stats) of the policy's logits float32 [M, 6] and values float32 [M] on the samples of `batch`
    (TrajectoryBuffer.learner_batch: flat [S] tensors, optionally seat, old logits and oc_gae's moments) that index int32 [M] names
    (None: samples first .. first + M - 1).  loss: a 0-dim float32 tensor, the mean over the minibatch's learner samples of
    -surr + vf_loss_coeff * vfc - entropy_coeff * H + kl_coeff * kl, whose backward() hands the logits and values the gradients the
    same launch computed.  stats: PpoStats — the float64 [8] tensor and 0-dim views of it (count, total, policy_loss, vf_loss,
    entropy, kl, clip_frac, inv_count); terms=True adds the float32 [M, 4] per-sample terms (surr, vfc, H, kl).  Raises ValueError
    for a tensor of another dtype, shape, device or layout, for a tensor on the host (there is no CPU fallback) and for the
    hyperparameters oc_ppo_loss refuses."""
    import math

    import torch

    global _FUNCTION
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != 6:
        raise ValueError("logits must be a contiguous float32 [M, 6] tensor")
    if not isinstance(batch, LearnerBatch):
        raise ValueError("batch must be a LearnerBatch (TrajectoryBuffer.learner_batch)")
    M, dev = int(logits.shape[0]), logits.device
    _checked("logits", logits, torch.float32, (M, 6), dev, torch)
    _checked("values", values, torch.float32, (M,), dev, torch)
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
    if index is not None:
        _checked("index", index, torch.int32, (M,), dev, torch)
        if S >= 2 ** 31:
            raise ValueError("an index names samples below 2^31, the batch has %d" % S)
    else:
        first = int(first)
        if first < 0 or first + M > S:
            raise ValueError("samples %d .. %d lie outside the batch's 0 .. %d" % (first, first + M - 1, S - 1))
    hyper = tuple(float(x) for x in (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff))
    if not all(math.isfinite(x) and x > 0 for x in hyper[:2]):
        raise ValueError("clip_param and vf_clip_param must be finite and positive, not %r and %r" % hyper[:2])
    if not all(x >= 0 for x in hyper[2:]):
        raise ValueError("vf_loss_coeff, entropy_coeff and kl_coeff must be >= 0, not %r, %r and %r" % hyper[2:])
    if hyper[4] > 0 and batch.logits_old is None:
        raise ValueError("kl_coeff > 0 needs the batch's old logits (TrajectoryBuffer(keep_logits=True))")
    if dev.type != "cuda":
        raise ValueError("ppo_loss works on device tensors, not on %s (there is no CPU fallback)" % dev)
    if _FUNCTION is None:
        _FUNCTION = _function()
    box = []
    loss = _FUNCTION.apply(logits, values, batch, index, 0 if index is not None else first, hyper, bool(terms), box)
    stats, terms_out = box
    return loss, PpoStats(stats, *(stats[i] for i in range(8)), terms_out)


def plan_ppo_loss(n_minibatch, index=False, seat=False, moments=False, old_logits=False, terms=False):
    """What ppo_loss() launches for M minibatch rows, in oc_ppo_loss_plan's words (no device needed)."""
    from . import _lib

    out = ctypes.create_string_buffer(320)
    rc = _lib.load().oc_ppo_loss_plan(int(n_minibatch), int(bool(index)), int(bool(seat)), int(bool(moments)), int(bool(old_logits)),
                                      int(bool(terms)), out, len(out))
    _lib.check(rc, "oc_ppo_loss_plan")
    return out.value.decode()
