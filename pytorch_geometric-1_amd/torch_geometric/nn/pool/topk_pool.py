"""TopKPooling (PyG 1.4.3 nn.pool.topk_pool [U]; callers: the reference's ConvexPruning.py:301-338
and examples/enzymes_topk_pool.py) on the native engine (csrc/mp_pool.hip):

    z      = (attn * weight).sum(-1)
    score  = nonlinearity(z / ||weight||_2)          min_score is None
           = utils.softmax(z, batch)                 min_score set
    perm   = topk(score, ratio, batch, min_score)
    x_out  = x[perm] * score[perm].view(-1, 1)  (* multiplier when it is not 1)
    edge_index_out, edge_attr_out = filter_adj(edge_index, edge_attr, perm, num_nodes=N)

Upstream chains torch ops (a dense [G, max_nodes] copy of the scores, a full
sort, one arange per graph, four boolean-mask gathers); here the score, the
per-graph select, the gate and the edge compaction are one deterministic kernel
each.  Graph g of n_g nodes keeps ceil(fl32(ratio * fl32(n_g))) of them (one
float32 multiply, as upstream: ratio 0.3 of 50 nodes keeps 16).  Where upstream's
sort leaves the order of equal scores open, here the lower node index ranks
first (torch.sort(descending=True, stable=True) within each graph; -0.0 equals
+0.0, NaN ranks above +inf).  `batch` must be non-decreasing (upstream assumes
it silently; debug mode raises when it is not).  There is no CPU path.
"""
import torch
from torch.nn import Parameter

from mi355_mp import _lib, ops

from ...debug import is_debug_enabled
from ...utils.num_nodes import maybe_num_nodes
from ...utils.softmax import softmax
from ..inits import uniform


def _layout(batch, n, device):
    layout = ops.batch_layout(batch, n, device)
    if layout.unsorted and is_debug_enabled():
        raise ValueError("topk: `batch` must be non-decreasing and non-negative (%d descents)" % layout.unsorted)
    return layout


def _select(score, ratio, batch, min_score, tol, layout):
    if min_score is None:
        if layout.n == 0:
            # upstream takes num_nodes.max() of the per-graph node counts: no graph, nothing to reduce
            raise RuntimeError("topk: no nodes (the largest graph of an empty batch is undefined)")
        return ops.topk_select(score, ratio, layout)
    return ops.select_min_score(score, float(min_score), batch, layout, tol)


def topk(x, ratio, batch, min_score=None, tol=1e-7):
    """perm: per graph of `batch`, the ceil(ratio * n_g) nodes of largest score x
    [N] in descending order (equal scores: lower index first), graph after
    graph; with min_score, the nodes with x > min(max_g(x) - tol, min_score) in
    ascending order.  Two host reads (the batch layout, then K)."""
    if min_score is None:
        ops.check_ratio(ratio)
    _lib.require_device(x, batch)
    x = x.detach().reshape(-1).float()
    layout = _layout(batch, x.shape[0], x.device)
    sel = _select(x, ratio, batch, min_score, tol, layout)
    K, _ = ops.pool_read_counts(sel, x.shape[0])
    return sel.perm[:K]


def filter_adj(edge_index, edge_attr, perm, num_nodes=None):
    """The edges between kept nodes, in original order, relabelled by position in
    perm; edge_attr (any trailing shape) gathered along.  An edge end outside
    [0, num_nodes) raises IndexError."""
    _lib.require_device(edge_index, edge_attr, perm)
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    sel = ops.PoolSelection(perm, None, ops.pool_inverse(perm, num_nodes),
                            torch.zeros(4, dtype=torch.int64, device=perm.device))
    out, pos = ops.pool_filter_adj(edge_index, sel, num_nodes)
    _, kept = ops.pool_read_counts(sel, num_nodes)
    if edge_attr is not None:
        edge_attr = ops.pool_edge_attr(edge_attr, pos[:kept])
    return out[:, :kept].contiguous(), edge_attr


class TopKPooling(torch.nn.Module):
    r"""TopKPooling(in_channels, ratio=0.5, min_score=None, multiplier=1, nonlinearity=torch.tanh)

    forward(x, edge_index, edge_attr=None, batch=None, attn=None)
        -> (x_out, edge_index_out, edge_attr_out, batch_out, perm, score[perm])

    Host synchronisation: a forward makes at most two device-to-host reads --
    the batch layout (number of graphs, largest graph and sortedness in one
    read; none when batch is None) and the pair (K kept nodes, kept edges) read
    together after the select and the edge compaction have been enqueued.  The
    min_score path composes the engine's softmax / segment-max / gather ops,
    whose index checks read once per batch tensor and are then cached.
    """

    def __init__(self, in_channels, ratio=0.5, min_score=None, multiplier=1, nonlinearity=torch.tanh):
        super(TopKPooling, self).__init__()
        if min_score is None:
            ops.check_ratio(ratio)
        self.in_channels = in_channels
        self.ratio = ratio
        self.min_score = min_score
        self.multiplier = multiplier
        self.nonlinearity = nonlinearity
        self.weight = Parameter(torch.Tensor(1, in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        uniform(self.in_channels, self.weight)

    def forward(self, x, edge_index, edge_attr=None, batch=None, attn=None):
        _lib.require_device(x, edge_index, edge_attr, batch, attn, self.weight)
        n = x.size(0)
        attn = x if attn is None else attn
        attn = attn.unsqueeze(-1) if attn.dim() == 1 else attn
        layout = _layout(batch, n, x.device)
        if self.min_score is None:
            native = self.nonlinearity is torch.tanh
            score = ops.pool_score(attn, self.weight, tanh=native)
            if not native:
                score = self.nonlinearity(score)
        else:
            z = ops.pool_score(attn, self.weight, tanh=False, raw=True)
            index = batch if batch is not None else torch.zeros(n, dtype=torch.int64, device=x.device)
            score = softmax(z, index, layout.n_graphs)
        sel = _select(score, self.ratio, batch, self.min_score, 1e-7, layout)
        out, pos = ops.pool_filter_adj(edge_index, sel, n)
        K, kept = ops.pool_read_counts(sel, n)
        perm = sel.perm[:K]
        x_out, score_out, batch_out = ops.pool_gate(x, score, perm, sel.inv, batch, self.multiplier)
        if edge_attr is not None:
            edge_attr = ops.pool_edge_attr(edge_attr, pos[:kept])
        return x_out, out[:, :kept].contiguous(), edge_attr, batch_out, perm, score_out

    def __repr__(self):
        return "{}({}, {}={}, multiplier={})".format(
            self.__class__.__name__, self.in_channels, "ratio" if self.min_score is None else "min_score",
            self.ratio if self.min_score is None else self.min_score, self.multiplier)
