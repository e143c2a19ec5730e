"""Advantages and value targets of a collected batch on the device: `gae` (oc_gae, one launch) and `plan_gae`.

Time-major tensors as T calls of `VecOvercookedMultiAgent.step_sampled(..., into=buf.row(t, values))` leave them
(`trajectory_buffer.TrajectoryBuffer`): rewards float64 [T, N, 2], values float32 [T, N, 2], done uint8 [T, N] and, with a
behaviour-cloning partner, seat uint8 [T, N].  The arithmetic — per-agent GAE(gamma, lambda) in float32, a done step cutting the
chain, the partner's samples zeroed and left out — is stated in include/oc_amd.h (OcGaeBatch)."""
import ctypes

PARTIAL_ENVS = 256  # envs per row of the moments' partial sums (include/oc_amd.h: d_partials)


def _checked(name, t, dtype, shape, device, torch):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() \
            or t.device != device:
        raise ValueError("%s must be a contiguous %s %s tensor on %s" % (name, str(dtype).replace("torch.", ""), list(shape), device))
    return t


def _stream(device):
    import torch

    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if device.type != "cuda":
        return None
    index = device.index if device.index is not None else torch.cuda.current_device()
    return raw(index) if raw is not None else torch.cuda.current_stream(device).cuda_stream


def gae(rewards, values, done, gamma, lam, last_values=None, seat=None, moments=False, out=None):
    """(advantages, targets) float32 [T, N, 2] of rewards float64 [T, N, 2], values float32 [T, N, 2] and done uint8 [T, N], all
    contiguous tensors on one device; last_values float32 [N, 2]: the value estimates behind the last step (None: zeros); seat
    uint8 [T, N]: the partner's player during every step (None: no partner anywhere); out: the pair of output tensors to write.
    moments=True appends a float64 [3] tensor (count, sum A, sum A^2 over the learner samples), summed without atomics.  Raises
    ValueError for a tensor of another dtype, shape, device or layout and for gamma or lam outside [0, 1]."""
    import torch

    from . import _lib

    if not isinstance(rewards, torch.Tensor) or rewards.dim() != 3 or rewards.shape[2] != 2:
        raise ValueError("rewards must be a contiguous float64 [T, N, 2] tensor")
    T, N = int(rewards.shape[0]), int(rewards.shape[1])
    dev = rewards.device
    _checked("rewards", rewards, torch.float64, (T, N, 2), dev, torch)
    _checked("values", values, torch.float32, (T, N, 2), dev, torch)
    _checked("done", done, torch.uint8, (T, N), dev, torch)
    if last_values is not None:
        _checked("last_values", last_values, torch.float32, (N, 2), dev, torch)
    if seat is not None:
        _checked("seat", seat, torch.uint8, (T, N), dev, torch)
    gamma, lam = float(gamma), float(lam)
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError("gamma and lam must be in [0, 1], not %r and %r" % (gamma, lam))
    if out is None:
        adv, tgt = torch.empty((T, N, 2), dtype=torch.float32, device=dev), torch.empty((T, N, 2), dtype=torch.float32, device=dev)
    else:
        adv, tgt = out
        _checked("out[0]", adv, torch.float32, (T, N, 2), dev, torch)
        _checked("out[1]", tgt, torch.float32, (T, N, 2), dev, torch)
    if dev.type != "cuda":
        raise ValueError("gae works on device tensors, not on %s (there is no CPU fallback)" % dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    mom = partials = None
    if moments:
        partials = torch.empty(((N + PARTIAL_ENVS - 1) // PARTIAL_ENVS, 3), dtype=torch.float64, device=dev)
        mom = torch.empty((3,), dtype=torch.float64, device=dev)
    g = _lib.OcGaeBatch(ptr(rewards), ptr(values), ptr(last_values), ptr(done), ptr(seat), ptr(adv), ptr(tgt), ptr(partials), ptr(mom),
                        T, gamma, lam)
    b = _lib.OcBatch(n_envs=N)
    L = _lib.load()
    if dev.type == "cuda" and torch.cuda.current_device() != (dev.index if dev.index is not None else torch.cuda.current_device()):
        with torch.cuda.device(dev):
            rc = L.oc_gae(ctypes.byref(b), ctypes.byref(g), _stream(dev))
    else:
        rc = L.oc_gae(ctypes.byref(b), ctypes.byref(g), _stream(dev))
    _lib.check(rc, "oc_gae")
    return (adv, tgt, mom) if moments else (adv, tgt)


def plan_gae(n_envs, n_steps, seat=False, moments=False):
    """What gae() launches for N envs and T steps, in oc_gae_plan's words (no device needed)."""
    from . import _lib

    out = ctypes.create_string_buffer(320)
    b = _lib.OcBatch(n_envs=int(n_envs))
    rc = _lib.load().oc_gae_plan(ctypes.byref(b), int(n_steps), int(bool(seat)), int(bool(moments)), out, len(out))
    _lib.check(rc, "oc_gae_plan")
    return out.value.decode()
