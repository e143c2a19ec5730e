"""The learner's sample index on the device: `select` (oc_sample_select), `permute` (oc_sample_permute) and `plan`.

    samples = select(buf.seat.view(-1), buf.actions.view(-1), S)       # once per iteration
    for epoch in range(num_sgd_iter):
        index = permute(samples, samples.n, seed, epoch)               # int32 [L]: the learner's samples, shuffled
        learner.epoch(buf.features, batch, index, 2000)

`select` compacts the samples the PPO loss uses — not the partner's, not an invalid row's — in ascending order; `permute` shuffles
them by a bijection that is a stated function of (seed, epoch): include/oc_amd.h ("The learner's sample index") has the arithmetic,
tests/sample_index_cases.py restates it in numpy.  `TrajectoryBuffer.learner_samples`, `.learner_permutation` and
`.learner_minibatches` are these calls on a buffer's own tensors."""
import ctypes
import re

from .gae import _checked, _stream

_BLOCK = None


def block_samples():
    """P, the samples per block of the selection's counts, read from oc_sample_index_plan's words (no device needed)."""
    global _BLOCK
    if _BLOCK is None:
        _BLOCK = int(re.search(r"P = (\d+) samples per block", plan(0)).group(1))
    return _BLOCK


def scratch_bytes(n_samples, seat=False):
    """The bytes of oc_sample_select's d_block_offsets for S samples: a u32 per block of P samples, at least one, as the plan
    states it (P is read from the plan once; `seat` does not change the size)."""
    P = block_samples()
    return 4 * max(1, (int(n_samples) + P - 1) // P)


def _call(fn, dev, *args):
    import torch

    from . import _lib

    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), fn)(*args, _stream(dev))
    _lib.check(rc, fn)


class LearnerSamples:
    """What `select` leaves on the device: `ids` int32 [S] — the selected samples in ascending order, then -1 — and `count`
    int64 [1], their number L.  `n` is L on the host: reading it is the ONE host synchronisation of the index (the first read
    waits for the selection and copies eight bytes; later reads return the same number).  A caller who must not wait passes
    n = S to `permute` instead and gets an index whose entries from L on are -1, which the loss and the policy's passes leave out."""

    def __init__(self, ids, count):
        self.ids, self.count, self._n = ids, count, None

    @property
    def n(self):
        if self._n is None:
            self._n = int(self.count.item())
        return self._n


def select(seat, actions, n_samples):
    """The learner's samples of a batch of S = n_samples samples, as LearnerSamples.  seat: uint8 [S / 2] (the partner's player
    of every (step, env)) or None; actions: uint8 [S] or None; both contiguous on one CUDA device (None, None: every sample, on
    the current device).  Raises ValueError for a tensor of another dtype, shape, device or layout, for S outside 0 .. 2^31 - 1
    and for an odd S with seats."""
    import torch

    S = int(n_samples)
    if not 0 <= S < 2 ** 31:
        raise ValueError("select: n_samples must be in 0 .. 2^31 - 1, not %d" % S)
    given = [t for t in (seat, actions) if t is not None]
    if not all(isinstance(t, torch.Tensor) for t in given):
        raise ValueError("select: seat and actions must be tensors or None")
    dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    if seat is not None:
        if S % 2:
            raise ValueError("select: seats need an even number of samples, not %d" % S)
        _checked("seat", seat, torch.uint8, (S // 2,), dev, torch)
    if actions is not None:
        _checked("actions", actions, torch.uint8, (S,), dev, torch)
    if dev.type != "cuda":
        raise ValueError("select works on device tensors, not on %s (there is no CPU fallback)" % dev)
    ids = torch.empty((max(S, 1),), dtype=torch.int32, device=dev)  # (an empty tensor has no address to hand over)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    scratch = torch.empty((scratch_bytes(S) // 4,), dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _call("oc_sample_select", dev, S, ptr(seat) if S else None, ptr(actions) if S else None, ptr(ids), ptr(count), ptr(scratch))
    return LearnerSamples(ids[:S], count)


def permute(samples, n, seed, epoch, out=None, device=None):
    """int32 [n]: entry i is samples.ids[pi(i)] for i < L and -1 from L on, pi the header's bijection of 0 .. L - 1 under (seed,
    epoch), both taken modulo 2^64.  samples: a LearnerSamples (n = samples.n: the whole shuffled index; n = S: the same without
    reading L, with a -1 tail), or None: the plain permutation of 0 .. n - 1 (L = n), for a learner whose every sample counts
    (`BCLearner.epoch`), on `device` (default: the current CUDA device).  out: the int32 [n] tensor to write."""
    import torch

    n = int(n)
    if not 0 <= n < 2 ** 31:
        raise ValueError("permute: n must be in 0 .. 2^31 - 1, not %d" % n)
    if samples is None:
        dev = torch.device(device) if device is not None else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise ValueError("permute works on a CUDA device, not on %s (there is no CPU fallback)" % dev)
        ids, count = None, torch.full((1,), n, dtype=torch.int64, device=dev)
    else:
        if not isinstance(samples, LearnerSamples):
            raise ValueError("permute: samples must be a LearnerSamples (select) or None")
        ids, count, dev = samples.ids, samples.count, samples.ids.device
        if n > int(ids.shape[0]):
            raise ValueError("permute: n = %d is more than the %d samples selected from" % (n, int(ids.shape[0])))
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=dev)
    else:
        _checked("out", out, torch.int32, (n,), dev, torch)
    mask = 2 ** 64 - 1
    if n == 0:  # (nothing to launch, and an empty tensor has no address to hand over)
        return out
    _call("oc_sample_permute", dev, ids.data_ptr() if ids is not None else None, count.data_ptr(), n, int(seed) & mask, int(epoch) & mask,
          out.data_ptr())
    return out


def plan(n_samples, seat=False, actions=False, ids=True, n_out=0, n_learner=0):
    """What select() and permute() launch, in oc_sample_index_plan's words (no device needed)."""
    from . import _lib

    out = ctypes.create_string_buffer(1024)
    rc = _lib.load().oc_sample_index_plan(int(n_samples), int(bool(seat)), int(bool(actions)), int(bool(ids)), int(n_out), int(n_learner),
                                          out, len(out))
    _lib.check(rc, "oc_sample_index_plan")
    return out.value.decode()
