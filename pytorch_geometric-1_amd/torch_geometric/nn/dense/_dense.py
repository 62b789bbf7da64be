"""What DenseSAGEConv and dense_diff_pool share: the choice between the fused
native calls (mi355_mp.ops.dense_mean_agg / dense_diff_pool, csrc/mp_dense.hip)
and the upstream recipes in torch device ops."""
import torch
from mi355_mp import ops as _ops

EPS = 1e-15


# Graphs up to this many nodes take the fused mean aggregation: it wins at N = 100
# and loses to the recipe's matrix-core bmm at N = 1000; 128 is the
# largest graph of dense_diff_pool's one-workgroup form, the other measured win.
AGG_FUSED_MAX_N = 128


def fused(adj, *tensors):
    """True when a fused call can serve these inputs: float32 tensors on the GPU
    and an adjacency that needs no gradient (data adjacency).  The fused backward
    never reads adj, so it cannot give it a gradient: a pooled adjacency that
    requires one (the second level of a stack, N = the cluster count) takes the
    recipe."""
    if adj.requires_grad:
        return False
    return all(t.is_cuda and t.dtype == torch.float32 for t in (adj,) + tensors)


def pool_fused(x, adj, s):
    """dense_diff_pool's pick: the fused call where it runs as one workgroup per
    graph (mp_diff_pool_path = 0).  Its row-tile form is slower than the recipe
    where it was measured, so that range runs the recipe;
    mi355_mp.ops.dense_diff_pool still runs it on request (a sixth of the memory)."""
    return fused(adj, x, s) and _ops.diff_pool_path(x.shape[1], s.shape[2], x.shape[2]) == 0


def agg_fused(x, adj):
    """DenseSAGEConv's pick for its mean aggregation."""
    return fused(adj, x) and x.shape[1] <= AGG_FUSED_MAX_N


def diff_pool_recipe(x, adj, s, mask=None):
    """dense_diff_pool as upstream writes it; x, adj, s are 3-D."""
    batch_size, num_nodes, _ = x.size()
    s = torch.softmax(s, dim=-1)
    if mask is not None:
        mask = mask.view(batch_size, num_nodes, 1).to(x.dtype)
        x, s = x * mask, s * mask
    out = torch.matmul(s.transpose(1, 2), x)
    out_adj = torch.matmul(torch.matmul(s.transpose(1, 2), adj), s)
    link_loss = adj - torch.matmul(s, s.transpose(1, 2))
    link_loss = torch.norm(link_loss, p=2)
    link_loss = link_loss / adj.numel()
    ent_loss = (-s * torch.log(s + EPS)).sum(dim=-1).mean()
    return out, out_adj, link_loss, ent_loss


def mean_agg_recipe(x, adj, add_loop=True):
    """DenseSAGEConv's aggregation as upstream writes it: adj is cloned to set its diagonal."""
    if add_loop:
        adj = adj.clone()
        idx = torch.arange(adj.size(1), dtype=torch.long, device=adj.device)
        adj[:, idx, idx] = 1
    out = torch.matmul(adj, x)
    return out / adj.sum(dim=-1, keepdim=True).clamp(min=1)


def mean_agg(x, adj, add_loop=True):
    if agg_fused(x, adj):
        return _ops.dense_mean_agg(x, adj, add_loop)
    return mean_agg_recipe(x, adj, add_loop)
