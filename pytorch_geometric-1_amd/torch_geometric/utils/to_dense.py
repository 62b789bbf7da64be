"""torch_geometric.utils.to_dense_batch / to_dense_adj (PyG 1.4.3).

A sorted batch vector of float32 rows on the GPU is filled by the native kernels
over its cached BatchLayout (csrc/mp_dense.hip).  Anything else takes the recipe
in plain torch ops, which also serves host tensors, as utils.degree does."""
import torch
from mi355_mp import ops as _ops


def _layout(batch, n, device):
    """The cached BatchLayout of a sorted device batch vector (None = one graph), else None."""
    if device.type != "cuda":
        return None
    if batch is not None and (not batch.is_cuda or batch.dtype != torch.int64 or batch.dim() != 1
                              or batch.shape[0] != n):
        return None
    layout = _ops.cached_batch_layout(batch, n, device)
    return None if layout.unsorted else layout


def _positions(batch):
    """(B, N_max, pos): the graphs, the largest one, and every node's rank among
    the nodes of its graph in node order (any batch order)."""
    n, dev = batch.numel(), batch.device
    B = int(batch.max()) + 1 if n else 0
    counts = torch.zeros(B, dtype=torch.long, device=dev).scatter_add_(0, batch, torch.ones_like(batch))
    starts = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    order = torch.sort(batch, stable=True)[1]
    pos = torch.empty_like(order)
    pos[order] = torch.arange(n, device=dev) - starts[batch[order]]
    return B, (int(counts.max()) if B else 0), pos


def to_dense_batch(x, batch=None, fill_value=0):
    """(out [B, N_max, *], mask [B, N_max] bool): the rows of x grouped by graph,
    each graph padded with fill_value to the largest one."""
    n = x.size(0)
    layout = _layout(batch, n, x.device) if x.dtype == torch.float32 and x.dim() >= 2 and x[0:1].numel() >= 1 \
        else None
    if layout is not None and layout.n_graphs > 0:
        out, mask = _ops.to_dense_batch(x.reshape(n, -1), layout, fill_value)
        return out.view(layout.n_graphs, layout.max_n, *x.shape[1:]), mask
    if batch is None:
        batch = x.new_zeros(n, dtype=torch.long)
    B, Nmax, pos = _positions(batch)
    idx = batch * Nmax + pos
    out = x.new_full((B * Nmax,) + tuple(x.shape[1:]), fill_value)
    out[idx] = x
    mask = torch.zeros(B * Nmax, dtype=torch.bool, device=x.device)
    mask[idx] = True
    return out.view((B, Nmax) + tuple(x.shape[1:])), mask.view(B, Nmax)


def to_dense_adj(edge_index, batch=None, edge_attr=None):
    """[B, N_max, N_max] with 1 per edge, or [B, N_max, N_max, *] holding edge_attr.
    Of several edges between one pair the last in edge order wins (upstream
    leaves that case undefined)."""
    dev = edge_index.device
    if batch is None:
        n = int(edge_index.max()) + 1 if edge_index.numel() else 0
    else:
        n = batch.size(0)
    fusable = edge_attr is None or (edge_attr.dtype == torch.float32 and edge_attr.is_cuda
                                    and edge_attr[0:1].numel() >= 1 and not edge_attr.requires_grad)
    layout = _layout(batch, n, dev) if fusable and edge_index.dtype == torch.int64 else None
    if layout is not None and layout.n_graphs > 0:
        attr = None if edge_attr is None else edge_attr.reshape(edge_attr.size(0), -1)
        out = _ops.to_dense_adj(edge_index, layout, batch, attr)
        return out if edge_attr is None else out.view(out.shape[:3] + tuple(edge_attr.shape[1:]))
    if batch is None:
        batch = edge_index.new_zeros(n)
    B, Nmax, pos = _positions(batch)
    g = batch[edge_index[0]]
    cell = (g * Nmax + pos[edge_index[0]]) * Nmax + pos[edge_index[1]]
    if edge_attr is None:
        out = torch.zeros(B * Nmax * Nmax, dtype=torch.float, device=dev)
        out[cell] = 1
        return out.view(B, Nmax, Nmax)
    out = edge_attr.new_zeros((B * Nmax * Nmax,) + tuple(edge_attr.shape[1:]))
    # the last edge of a cell: the largest edge index that lands in it
    E = cell.numel()
    last = torch.full((B * Nmax * Nmax,), -1, dtype=torch.long, device=dev)
    last = last.scatter_reduce(0, cell, torch.arange(E, device=dev), "amax", include_self=True)
    keep = last[cell] == torch.arange(E, device=dev)
    out = out.index_put((cell[keep],), edge_attr[keep])
    return out.view((B, Nmax, Nmax) + tuple(edge_attr.shape[1:]))
