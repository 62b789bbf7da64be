"""DNAConv: the dynamic neighborhood aggregation of Fey (Just Jump: Dynamic
Neighborhood Aggregation in Graph Neural Networks, 2019), PyG 1.4.3
nn.conv.dna_conv [U]:

    x'_i = sum_{j in N(i) + i} n_ij Attention(x_i[T-1] Theta_Q, x_j Theta_K, x_j Theta_V)

x [N, T, C] holds every node's T earlier layer outputs; one query (the node's
latest output) attends over the T entries of each in-neighbour's history with
multi-head scaled dot-product attention under the restricted softmax (margin
0), and the messages are summed with the GCN normalisation n_ij.  Linear (a
grouped, block-diagonal linear map), restricted_softmax, Attention and
MultiHead keep upstream's names and parameter layout, so state dicts load.

MI355X engine: upstream gathers x_j as [E, T, C] and projects keys and values
per edge.  The projections depend on the node only, so Q [N, C] and K, V
[N, T, C] are computed once per node (the grouped Linears: plain GEMMs), and a
fused HIP pass per destination row runs the one-query attention over its
in-neighbours' keys and values (mi355_mp.ops.dna_propagate: csrc/mp_dna.hip),
forward and backward, deterministic; no [E, T, C] array exists.  The fused path
is taken for device fp32 contiguous x, node_dim 0, message / update / aggregate
not overridden, a norm that needs no gradient, a shape inside mp_dna_ok and
dropout inactive or 0 < p < 1 in training (the keep mask is then a hash of a
seed drawn from torch's generator: another draw than F.dropout's, the same
law, as for GATConv); everything else on the device (a learnable edge_weight,
float64, T above ops.dna_max_layers(heads, channels)) runs upstream's message on
the generic MessagePassing path.  CPU tensors raise RuntimeError, as for every
other layer: the normalisation and the aggregation have no CPU path.

The normalised edge list is cached on the caller's edge_index tensor (its
structure half, _structure.remaining_loops_structure), so with cached=False the
layer still meets the same tensor on every call and graph_for returns the CSRs
and schedules it built the first time; cached=True also keeps norm.
"""
import math

import torch
import torch.nn.functional as F
from torch.nn import Parameter

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import uniform, kaiming_uniform
from .gcn_conv import GCNConv
from .message_passing import MessagePassing


class Linear(torch.nn.Module):
    """Block-diagonal linear map: output group g is src[..., g * in/G:(g + 1) *
    in/G] @ weight[g]; weight [G, in/G, out/G], bias [out]."""

    def __init__(self, in_channels, out_channels, groups=1, bias=True):
        super(Linear, self).__init__()
        assert in_channels % groups == 0 and out_channels % groups == 0
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.groups = groups
        self.weight = Parameter(torch.Tensor(groups, in_channels // groups, out_channels // groups))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        kaiming_uniform(self.weight, fan=self.weight.size(1), a=math.sqrt(5))
        uniform(self.weight.size(1), self.bias)

    def forward(self, src):
        if self.groups > 1:
            size = list(src.size())[:-1]
            src = src.view(-1, self.groups, self.in_channels // self.groups)
            src = src.transpose(0, 1).contiguous()
            out = torch.matmul(src, self.weight)
            out = out.transpose(1, 0).contiguous()
            out = out.view(*(size + [self.out_channels]))
        else:
            out = torch.matmul(src, self.weight.squeeze(0))
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self):  # pragma: no cover
        return "{}({}, {}, groups={}, bias={})".format(self.__class__.__name__, self.in_channels, self.out_channels,
                                                       self.groups, self.bias is not None)


def restricted_softmax(src, dim=-1, margin=0):
    src_max = torch.clamp(src.max(dim=dim, keepdim=True)[0], min=0)
    out = (src - src_max).exp()
    out = out / (out.sum(dim=dim, keepdim=True) + (margin - src_max).exp())
    return out


class Attention(torch.nn.Module):
    def __init__(self, dropout=0):
        super(Attention, self).__init__()
        self.dropout = dropout

    def forward(self, query, key, value):
        # query [*, query_entries, dim_k], key [*, key_entries, dim_k], value [*, key_entries, dim_v]
        assert query.dim() == key.dim() == value.dim() >= 2
        assert query.size(-1) == key.size(-1)
        assert key.size(-2) == value.size(-2)
        score = torch.matmul(query, key.transpose(-2, -1))
        score = score / math.sqrt(key.size(-1))
        score = restricted_softmax(score, dim=-1)
        score = F.dropout(score, p=self.dropout, training=self.training)
        return torch.matmul(score, value)

    def __repr__(self):  # pragma: no cover
        return "{}(dropout={})".format(self.__class__.__name__, self.dropout)


class MultiHead(Attention):
    def __init__(self, in_channels, out_channels, heads=1, groups=1, dropout=0, bias=True):
        super(MultiHead, self).__init__(dropout)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.groups = groups
        self.bias = bias
        assert in_channels % heads == 0 and out_channels % heads == 0
        assert in_channels % groups == 0 and out_channels % groups == 0
        assert max(groups, self.heads) % min(groups, self.heads) == 0
        self.lin_q = Linear(in_channels, out_channels, groups, bias)
        self.lin_k = Linear(in_channels, out_channels, groups, bias)
        self.lin_v = Linear(in_channels, out_channels, groups, bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_q.reset_parameters()
        self.lin_k.reset_parameters()
        self.lin_v.reset_parameters()

    def forward(self, query, key, value):
        assert query.dim() == key.dim() == value.dim() >= 2
        assert query.size(-1) == key.size(-1) == value.size(-1)
        assert key.size(-2) == value.size(-2)
        query = self.lin_q(query)
        key = self.lin_k(key)
        value = self.lin_v(value)
        size = list(query.size())[:-2]
        d = self.out_channels // self.heads
        query = query.view(*(size + [query.size(-2), self.heads, d])).transpose(-2, -3)
        key = key.view(*(size + [key.size(-2), self.heads, d])).transpose(-2, -3)
        value = value.view(*(size + [value.size(-2), self.heads, d])).transpose(-2, -3)
        out = super(MultiHead, self).forward(query, key, value)
        out = out.transpose(-3, -2).contiguous()
        return out.view(*(size + [query.size(-2), self.out_channels]))

    def __repr__(self):  # pragma: no cover
        return "{}({}, {}, heads={}, groups={}, dropout={}, bias={})".format(
            self.__class__.__name__, self.in_channels, self.out_channels, self.heads, self.groups, self.dropout,
            self.bias)


class DNAConv(MessagePassing):
    r"""Args:
        channels (int), heads (int, default 1), groups (int, default 1), dropout
        (float, default 0: of the attention coefficients), cached (bool, default
        False: keep the normalised edge_index / norm of the first call), bias
        (bool, default True).
    """

    def __init__(self, channels, heads=1, groups=1, dropout=0, cached=False, bias=True, **kwargs):
        super(DNAConv, self).__init__(aggr="add", **kwargs)
        self.bias = bias
        self.cached = cached
        self.cached_result = None
        self.cached_num_edges = None
        self.multi_head = MultiHead(channels, channels, heads, groups, dropout, bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.multi_head.reset_parameters()
        self.cached_result = None
        self.cached_num_edges = None

    def fused_layer(self):
        """Whether the fused path's conditions on the layer itself hold: node_dim
        0 and message / update / aggregate not overridden."""
        cls = type(self)
        return (self.node_dim == 0 and self.aggr == "add" and cls.message is DNAConv.message
                and cls.update is MessagePassing.update and cls.aggregate is MessagePassing.aggregate)

    def _fused_ok(self, x, edge_index, norm):
        if not self.fused_layer():
            return False
        mh = self.multi_head
        for p in mh.parameters():
            if not (p.is_cuda and p.dtype == torch.float32):
                return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.is_contiguous() and x.shape[2] == mh.in_channels and x.shape[1] >= 1):
            return False
        if not (edge_index.is_cuda and torch.is_tensor(norm) and norm.is_cuda and norm.dtype == torch.float32
                and norm.dim() == 1 and not norm.requires_grad):
            return False
        p = float(mh.dropout)
        if mh.training and p != 0.0 and not 0.0 < p < 1.0:    # p = 1 (all dropped) stays with F.dropout
            return False
        return _ops.dna_ok(x.shape[1], mh.heads, mh.out_channels)

    def forward(self, x, edge_index, edge_weight=None):
        """x [N, T, channels]: the T earlier layer outputs of every node."""
        if x.dim() != 3:
            raise ValueError("Feature shape must be [num_nodes, num_layers, channels].")
        if self.cached and self.cached_result is not None:
            if edge_index.size(1) != self.cached_num_edges:
                raise RuntimeError(
                    "Cached {} number of edges, but found {}. Please disable the caching behavior "
                    "of this layer by removing the `cached=True` argument in its constructor."
                    .format(self.cached_num_edges, edge_index.size(1)))
        if not self.cached or self.cached_result is None:
            self.cached_num_edges = edge_index.size(1)
            edge_index, norm = GCNConv.norm(edge_index, x.size(self.node_dim), edge_weight, dtype=x.dtype)
            self.cached_result = edge_index, norm
        edge_index, norm = self.cached_result
        if not self._fused_ok(x, edge_index, norm):
            return self.propagate(edge_index, x=x, norm=norm)
        mh = self.multi_head
        n = x.shape[0]
        q = mh.lin_q(x[:, -1])
        k = mh.lin_k(x)
        v = mh.lin_v(x)
        p = float(mh.dropout) if mh.training else 0.0
        # tasks of at least 64 units: the kernels then split long rows over tasks on a graph of any size
        graph = graph_for(edge_index, n, n, self.flow, _ops.dna_target_tasks(n, edge_index.size(1)))
        return _ops.dna_propagate(graph, q, k, v, norm, mh.heads, p=p)

    def message(self, x_i, x_j, norm):
        x_i = x_i[:, -1:]                                   # [E, 1, channels]
        out = self.multi_head(x_i, x_j, x_j)                # [E, 1, channels]
        return norm.view(-1, 1) * out.squeeze(1)

    def __repr__(self):
        return "{}({}, heads={}, groups={})".format(self.__class__.__name__, self.multi_head.in_channels,
                                                    self.multi_head.heads, self.multi_head.groups)
