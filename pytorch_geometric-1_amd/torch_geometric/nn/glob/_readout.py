"""What Set2Set and GlobalAttention share: the choice between the fused
attention readout (mi355_mp.ops.attention_readout, csrc/mp_glob.hip) and the
upstream recipe on the native softmax and scatter_ ops."""
import torch
from mi355_mp import ops as _ops

from ...utils import softmax
from ...utils.scatter import scatter_


def fused_layout(x, batch, size):
    """The BatchLayout (starts for `size` graphs) the fused call takes, or None
    when the recipe has to run: x not float32, or a batch that is not sorted.
    Cached on the batch tensor, a size beyond its graphs included."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.shape[1] < 1:
        return None
    layout = _ops.cached_batch_layout_for(batch, x.shape[0], size, x.device)
    if layout.unsorted or layout.n_graphs != size:
        return None
    return layout


def last_graph_plus_one(batch, n):
    """batch[-1] + 1, upstream's default size: from the cached layout (it counts
    graphs from the last entry) when the batch is one the engine lays out, so
    only the first call on a batch tensor reads from the device."""
    if n > 0 and batch.is_cuda and batch.dtype == torch.int64 and batch.dim() == 1 and batch.shape[0] == n:
        return _ops.cached_batch_layout(batch, n).n_graphs
    return int(batch[-1].item()) + 1


def recipe(x, e, batch, size):
    """softmax(e, batch) then scatter_add(a * x, batch), as upstream writes it."""
    a = softmax(e, batch, size)
    return scatter_("add", a * x, batch, dim=0, dim_size=size)
