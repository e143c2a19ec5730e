"""The behaviour-cloning partner's model on the device: `DensePolicy`, the weights `oc_partner_logits` evaluates.

The reference's BC model (human_aware_rl/imitation/behavior_cloning_tf2.py) is a small dense network on featurize_state:
in_dim -> h1 -> h2 -> 6 logits with ReLU after the two hidden layers (96 -> 64 -> 64 -> 6 by default).  `DensePolicy` takes its six
arrays in the Keras Dense layout (kernels [in, out], biases [out]; `model.get_weights()` of such a model, in order), validates
them, uploads them once as contiguous float32 and holds the `OcDensePolicy` the C-ABI takes.  `VecOvercookedMultiAgent(...,
bc_policy=policy)` seats it."""
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
