"""max_pool / max_pool_x (PyG 1.4.3 nn.pool.max_pool [U]) on the native engine
(csrc/mp_cluster.hip):

    cluster, perm = consecutive_cluster(cluster)
    x     = scatter_('max', data.x, cluster)          (out < -10000 := 0)
    pos   = scatter_mean(data.pos, cluster)
    batch = data.batch[perm]
    edge_index, edge_attr = pool_edge(cluster, data.edge_index, data.edge_attr)

Upstream chains a unique, an atomic scatter_max and its argmax pass, a
scatter_mean, a scatter_ whose winner among duplicates is unspecified, a
boolean-mask self-loop removal and torch_sparse's coalesce (an unstable sort, a
second unique and an atomic scatter_add): 25 to 30 launches and three or four
host reads.  Here one stable sort of the nodes by cluster key gives the cluster
ids, the cluster CSR and perm; one pass over that CSR gives x, pos and batch; one
stable sort of the relabelled edge keys gives the coalesced edges.  Where
upstream's order is open, ours is fixed: the lowest node index wins a tie of the
max, perm is the largest node index of a cluster, duplicates of an edge add
their attributes in ascending original edge position.  There is no CPU path.
"""
from mi355_mp import _lib, ops

from ...data import Batch


def _pool(cluster, data, transform, reduce):
    _lib.require_device(cluster, data.x, data.pos, data.batch, data.edge_index, data.edge_attr)
    sel = ops.cluster_build(cluster)
    x, pos = data.x, data.pos
    x2 = x.view(-1, 1) if x.dim() == 1 else x
    pos2 = None if pos is None else (pos.view(-1, 1) if pos.dim() == 1 else pos)
    x_out, _, pos_out, batch_out = ops.cluster_reduce(sel, x2, reduce, pos=pos2, batch=data.batch)
    ep = ops.pool_edges(data.edge_index, sel)
    attr = data.edge_attr
    if attr is not None:
        attr = ops.pool_edge_attr_sum(attr, ep, sel)
    M, kept, _ = ops.cluster_read_counts(sel)
    x_out = x_out[:M]
    if pos_out is not None:
        pos_out = pos_out[:M].view(-1) if pos.dim() == 1 else pos_out[:M]
    if batch_out is not None:
        batch_out = batch_out[:M]
        ops.note_num_graphs(batch_out, ops.known_num_graphs(data.batch))
    out = Batch(batch=batch_out, x=x_out.view(-1) if x.dim() == 1 else x_out,
                edge_index=ep.out[:, :kept].contiguous(), edge_attr=None if attr is None else attr[:kept],
                pos=pos_out)
    if transform is not None:
        out = transform(out)
    return out


def _pool_x(cluster, x, batch, size, reduce):
    _lib.require_device(cluster, x, batch)
    x2 = x.view(-1, 1) if x.dim() == 1 else x
    if size is not None:
        if x2.shape[0] == 0:
            # upstream sizes the output by batch.max() + 1: undefined without a node
            raise RuntimeError("max_pool_x / avg_pool_x with size: no nodes (batch.max() of an empty batch)")
        rows = ops.num_graphs(batch, x2.shape[0]) * int(size)
        return ops.segment_reduce(x2, cluster, rows, reduce, pyg_mask=reduce == "max")[0], None
    sel = ops.cluster_build(cluster)
    x_out, _, _, batch_out = ops.cluster_reduce(sel, x2, reduce, batch=batch)
    M = ops.cluster_read_counts(sel)[0]
    if batch_out is not None:
        batch_out = batch_out[:M]
        ops.note_num_graphs(batch_out, ops.known_num_graphs(batch))
    return x_out[:M], batch_out


def max_pool(cluster, data, transform=None):
    r"""Pools and coarsens the graph `data` by the clustering `cluster` (any int64
    vector, e.g. voxel_grid's): the node features are the maximum of every
    cluster, the positions their mean, and the coarsened edges the distinct
    cluster pairs with summed attributes.  Returns a Batch; `transform` is
    applied to it when given.

    Host synchronisation: one device-to-host read, of (clusters, output edges,
    bad edge ends) together, after every kernel of the stage has been enqueued.
    An edge end outside [0, N) raises IndexError.
    """
    return _pool(cluster, data, transform, "max")


def max_pool_x(cluster, x, batch, size=None):
    r"""Max-pools the node features `x` by `cluster`; returns (x_out, batch_out).

    With `size`: x_out = scatter_('max', x, cluster, dim_size=(batch.max() + 1) *
    size) with the cluster ids as they are (rows that receive nothing are 0, an id
    outside the range raises IndexError) and batch_out None -- the engine's
    segment reduction; no host read of its own beyond that reduction's index
    check and the batch layout, both cached per tensor.  Without `size`: the
    clusters are relabelled (consecutive_cluster) and batch_out = batch[perm];
    one host read.
    """
    return _pool_x(cluster, x, batch, size, "max")
