"""CPU restatement of the cluster-pooling semantics (PyG 1.4.3 nn.pool voxel_grid /
consecutive_cluster / max_pool / avg_pool / pool_edge over torch_cluster 1.5 and
torch_sparse 0.6.1 [U]) -- TEST INFRASTRUCTURE ONLY.  Plain torch on the CPU; the
max and the mean come from oracle/scatter_ref.py (torch_scatter's serial loop and
its edge-order scatter_add).  Where upstream leaves an order open, the project's
rule is stated: perm = the largest node index of a cluster, the lowest node index
wins a tie of the max, duplicates of an edge add in ascending original position.
"""
import numbers

import torch

from oracle import scatter_ref as S


def repeat(src, length):
    if src is None:
        return None
    if torch.is_tensor(src):
        src = src.reshape(-1).tolist()
    if isinstance(src, numbers.Number):
        return [src] * length
    src = list(src)
    if len(src) > length:
        return src[:length]
    return src + [src[-1]] * (length - len(src))


def voxel_grid(pos, batch, size, start=None, end=None):
    """int64 key [N]; float32 arithmetic, true division, truncation."""
    pos = pos.unsqueeze(-1) if pos.dim() == 1 else pos
    D = pos.size(1)
    size, start, end = repeat(size, D), repeat(start, D), repeat(end, D)
    pos = torch.cat([pos, batch.unsqueeze(-1).to(pos.dtype)], dim=-1)
    size = torch.tensor(size + [1], dtype=pos.dtype)
    start = pos.min(dim=0)[0] if start is None else torch.tensor(start + [0], dtype=pos.dtype)
    end = pos.max(dim=0)[0] if end is None else torch.tensor(end + [int(batch.max())], dtype=pos.dtype)
    c = ((pos - start) / size).long()
    m = ((end - start) / size).long() + 1
    mult = torch.ones(D + 1, dtype=torch.int64)
    for d in range(1, D + 1):
        mult[d] = mult[d - 1] * m[d - 1]
    return (c * mult).sum(1)


def consecutive_cluster(src):
    """(inv, perm): inv = unique's inverse, perm[c] = the last index of cluster c."""
    uniq, inv = torch.unique(src, sorted=True, return_inverse=True)
    # upstream: perm = inv.new_empty(M).scatter_(0, inv, arange(N)); the CPU loop leaves the last write
    perm = torch.zeros(uniq.numel(), dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(src.numel()), "amax",
                                                                        include_self=False)
    return inv, perm


def scatter_max(x, inv, M, mask=True):
    """(out, arg): torch_scatter's max (first member wins a tie, arg = N for none), then
    utils.scatter_'s out < -10000 := 0."""
    out, arg = S.scatter_max(x, inv, M)
    if mask:
        out = out.masked_fill(out < -10000, 0.0)
    return out, arg


def scatter_mean(src, inv, M):
    return S.scatter_mean(src, inv, M)


def pool_edge(inv, edge_index, edge_attr, M):
    """(edge_index_out, edge_attr_out, edge_slot): relabel, drop loops, coalesce; the
    duplicates add in ascending original edge position (index_add_ on the CPU is serial)."""
    E = edge_index.size(1)
    n = inv.numel()
    if E and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
        raise IndexError("pool_edge: edge end outside [0, %d)" % n)
    ei = inv[edge_index.reshape(-1)].view(2, E)
    keep = ei[0] != ei[1]
    slot = torch.full((E,), -1, dtype=torch.int64)
    ei = ei[:, keep]
    attr = None if edge_attr is None else edge_attr[keep]
    if ei.numel() > 0:
        uniq, idx = torch.unique(ei[0] * M + ei[1], sorted=True, return_inverse=True)
        slot[keep] = idx
        ei = torch.stack([uniq // M, uniq % M])
        if attr is not None:
            attr = torch.zeros((uniq.numel(),) + tuple(attr.shape[1:]), dtype=attr.dtype).index_add_(0, idx, attr)
    return ei, attr, slot


def pool(cluster, x, pos, batch, edge_index, edge_attr, reduce="max"):
    """Everything max_pool / avg_pool return, plus inv, perm, arg and edge_slot."""
    inv, perm = consecutive_cluster(cluster)
    M = perm.numel()
    x2 = x.view(-1, 1) if x.dim() == 1 else x
    if reduce == "max":
        x_out, arg = scatter_max(x2, inv, M)
    else:
        x_out, arg = scatter_mean(x2, inv, M), None
    ei, attr, slot = pool_edge(inv, edge_index, edge_attr, M)
    return {"inv": inv, "perm": perm, "x": x_out.view(-1) if x.dim() == 1 else x_out, "arg": arg,
            "pos": None if pos is None else scatter_mean(pos, inv, M),
            "batch": None if batch is None else batch[perm], "edge_index": ei, "edge_attr": attr, "edge_slot": slot}


def pool_x_sized(cluster, x, batch, size, reduce="max"):
    """max_pool_x / avg_pool_x with size: the cluster ids as they are."""
    rows = (int(batch.max()) + 1) * size
    if int(cluster.min()) < 0 or int(cluster.max()) >= rows:
        raise IndexError("max_pool_x: cluster id outside [0, %d)" % rows)
    if reduce == "max":
        return scatter_max(x, cluster, rows)[0]
    return scatter_mean(x, cluster, rows)


def pool_f64(x, pos, edge_attr, inv, arg, edge_slot, M, n_edges_out, reduce="max"):
    """Differentiable float64 form given the forward's inv / arg / edge_slot: x_out
    (max: x[arg] where a member won and the value is not masked, else 0; mean: sum /
    count), pos_out and the coalesced edge_attr."""
    n = inv.numel()
    cnt = torch.zeros(M, dtype=torch.float64).index_add_(0, inv, torch.ones(n, dtype=torch.float64)).view(-1, 1)
    if x is None:
        x_out = None
    elif reduce == "max":
        won = arg < n
        v = torch.gather(x, 0, arg.clamp(max=max(n - 1, 0)))
        x_out = torch.where(won & ~(v < -10000), v, torch.zeros_like(v))
    else:
        x_out = torch.zeros((M, x.shape[1]), dtype=torch.float64).index_add(0, inv, x) / cnt
    pos_out = None if pos is None else torch.zeros((M, pos.shape[1]), dtype=torch.float64).index_add(0, inv, pos) / cnt
    attr_out = None
    if edge_attr is not None:
        keep = edge_slot >= 0
        attr_out = torch.zeros((n_edges_out,) + tuple(edge_attr.shape[1:]), dtype=torch.float64).index_add(
            0, edge_slot[keep], edge_attr[keep])
    return x_out, pos_out, attr_out
