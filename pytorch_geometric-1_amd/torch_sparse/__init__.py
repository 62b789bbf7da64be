"""torch_sparse 0.4.4-compatible front door over the MI355X engine.

    spspmm(indexA, valueA, indexB, valueB, m, k, n) -> (index [2, nnz] int64, value [nnz])

The sparse x sparse product C = A B of two COO matrices, A [m, k] and B [k, n]:
the result is coalesced (distinct entries in row-major order); inputs may be
unsorted and may repeat an entry, which counts as its sum; an entry whose
products cancel is kept, as cusparse's symbolic structure keeps it upstream.
float32 values on a ROCm device (mi355_mp.ops.spgemm -> mp_spgemm_count /
mp_spgemm_fill_f32, csrc/mp_spgemm.hip) -- there is no CPU path.  The backward
of upstream's SpSpMM is not built: values that require grad raise.
"""
import torch

from mi355_mp import ops as _ops
from mi355_mp import _lib

__version__ = "0.4.4"

__all__ = ["spspmm"]


def spspmm(indexA, valueA, indexB, valueB, m, k, n):
    for v in (valueA, valueB):
        if torch.is_tensor(v) and v.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("torch_sparse.spspmm: the backward of the sparse product is not implemented; "
                                      "pass values that do not require grad (detach them)")
    _lib.require_device(indexA, valueA, indexB, valueB)
    if valueA.dtype != torch.float32 or valueB.dtype != torch.float32:
        raise TypeError("torch_sparse.spspmm: values must be float32 (got %s, %s)" % (valueA.dtype, valueB.dtype))
    return _ops.spgemm(indexA, valueA, indexB, valueB, m, k, n)
