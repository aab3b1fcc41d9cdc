"""A tensor whose values are computed on first use.

``Detect.lazy_nms`` (models/yolo.py) returns its prediction ``z`` (bs, A, no) and raw head ``x[i]`` as ``LazyTensor``s: they
report the shape, dtype and device of the eager tensors, but nothing is computed until an aten op touches them.
``utils.general.non_max_suppression_obb`` recognises a lazy prediction that was never touched and runs its fused entry on the
conv outputs instead (include/obb_hip.h: obb_non_max_suppression_obb_head), so in ``detect.py`` / ``val.py`` neither ``z`` nor
``x`` is ever written.

Any other use materialises the tensor ONCE (the ``materialize`` callable the producer handed over builds the real tensor);
every op from then on runs on that real tensor.  In-place ops write the real tensor and return the wrapper, so the object the
caller holds stays the one it operates on (``Model._descale_pred``'s ``p[..., :4] /= scale``, TTA's ``torch.cat``).
"""
import torch
from torch.utils._pytree import tree_map

__all__ = ["LazyTensor"]


class LazyTensor(torch.Tensor):
    """Wrapper subclass: metadata of the eager tensor, values from ``materialize()`` on first use.

    ``payload`` is whatever the producer wants to keep with the tensor (the conv outputs for the fused NMS); it is dropped
    when the tensor materialises."""

    @staticmethod
    def __new__(cls, shape, dtype, device, materialize, payload=None):
        r = torch.Tensor._make_wrapper_subclass(cls, tuple(shape), dtype=dtype, device=device, requires_grad=False)
        r._lazy_fn = materialize
        r._lazy_real = None
        r._lazy_payload = payload
        return r

    __torch_function__ = torch._C._disabled_torch_function_impl

    def is_materialized(self):
        return self._lazy_real is not None

    @property
    def payload(self):
        """The producer's record, or None once the tensor has materialised."""
        return self._lazy_payload

    def materialize(self):
        """The real tensor (computed on the first call)."""
        if self._lazy_real is None:
            real = self._lazy_fn()
            if real.shape != self.shape or real.dtype != self.dtype or real.device != self.device:
                raise RuntimeError(f"LazyTensor: the materialiser returned {tuple(real.shape)} {real.dtype} {real.device}, "
                                   f"expected {tuple(self.shape)} {self.dtype} {self.device}")
            self._lazy_real, self._lazy_fn, self._lazy_payload = real, None, None
        return self._lazy_real

    def __repr__(self):
        if self._lazy_real is None:
            return f"LazyTensor(shape={tuple(self.shape)}, dtype={self.dtype}, device={self.device}, not materialised)"
        return f"LazyTensor({self._lazy_real!r})"

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        wrappers = {}

        def unwrap(t):
            if isinstance(t, LazyTensor):
                real = t.materialize()
                wrappers[id(real)] = t
                return real
            return t

        out = func(*tree_map(unwrap, args), **tree_map(unwrap, kwargs or {}))
        # an op that returns one of its inputs (in-place, out=) hands back the wrapper the caller holds
        return tree_map(lambda t: wrappers.get(id(t), t) if isinstance(t, torch.Tensor) else t, out)
