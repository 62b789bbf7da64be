"""pool_edge / pool_batch / pool_pos (PyG 1.4.3 nn.pool.pool [U]) on the native
engine (csrc/mp_cluster.hip).  `cluster` is a consecutive cluster vector (the
first output of consecutive_cluster)."""
import torch

from mi355_mp import _lib, ops


def _selection(cluster):
    """A selection around an already consecutive cluster vector: M = max + 1 is
    reduced on the device."""
    _lib.require_device(cluster)
    counts = torch.zeros(4, dtype=torch.int64, device=cluster.device)
    if cluster.numel():
        counts[0] = cluster.max() + 1
    return ops.ClusterSelection(cluster.contiguous(), None, None, None, counts, cluster.numel())


def pool_edge(cluster, edge_index, edge_attr=None):
    """cluster[edge_index] without its loops, coalesced: the distinct (row, col)
    pairs in ascending row * M + col order, float32 edge_attr (any trailing shape;
    other dtypes raise TypeError) summed over the duplicates in ascending
    original edge position.  An edge end outside [0, N) raises IndexError.  One
    host read."""
    _lib.require_device(cluster, edge_index, edge_attr)
    sel = _selection(cluster)
    ep = ops.pool_edges(edge_index, sel)
    if edge_attr is not None:
        edge_attr = ops.pool_edge_attr_sum(edge_attr, ep, sel)
    kept = ops.cluster_read_counts(sel)[1]
    return ep.out[:, :kept].contiguous(), None if edge_attr is None else edge_attr[:kept]


def pool_batch(perm, batch):
    return batch[perm]


def pool_pos(cluster, pos):
    """scatter_mean(pos, cluster): the float32 sum in ascending node order over
    the member count.  One host read."""
    _lib.require_device(cluster, pos)
    sel = ops.cluster_build(cluster)
    squeeze = pos.dim() == 1
    out = ops.cluster_reduce(sel, None, "mean", pos=pos.view(-1, 1) if squeeze else pos)[2]
    out = out[:ops.cluster_read_counts(sel)[0]]
    return out.view(-1) if squeeze else out
