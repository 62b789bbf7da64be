"""RGCNConv: the relational graph convolution of Schlichtkrull et al. (Modeling
Relational Data with Graph Convolutional Networks, ESWC 2018) with the basis
decomposition, PyG 1.4.3 nn.conv.rgcn_conv [U]:

    x'_i = sum_r sum_{j in N_r(i)} n_ij x_j W_r + x_i root + b,   W_r = sum_b att[r, b] basis[b]

``x = None`` is the featureless first layer: x is the identity (one node per
input channel, in_channels = num_nodes), the message of edge (j -> i) is row j
of W_r and root is added as it is.

MI355X engine: the per-edge weight matrices index_select(W, edge_type)
([E, Cin, Cout]) and the featureless [R * N, Cout] table are never built.  With
a_e = n_e att[type_e, :] and V = basis viewed as [B * Cin, Cout],

    sum_e n_e x_j W_{type_e} = (sum_e a_e (x) x_j) V

one segmented HIP pass plus one node-level GEMM (mi355_mp.ops.rgcn_propagate:
csrc/mp_rgcn.hip), forward and backward, deterministic.  The fused path is taken
for device fp32 tensors, node_dim 0, message / update / aggregate not
overridden, x one tensor or None, an edge_norm that needs no gradient and a
shape inside mp_rgcn_ok; everything else runs upstream's message / update on
the generic MessagePassing path.
"""
import torch

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import uniform
from .message_passing import MessagePassing


class RGCNConv(MessagePassing):
    r"""Args:
        in_channels (int), out_channels (int), num_relations (int), num_bases
        (int), root_weight (bool, default True), bias (bool, default True).
    """

    def __init__(self, in_channels, out_channels, num_relations, num_bases, root_weight=True, bias=True, **kwargs):
        super(RGCNConv, self).__init__(aggr="add", **kwargs)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.num_relations, self.num_bases = int(num_relations), int(num_bases)
        self.basis = torch.nn.Parameter(torch.empty(self.num_bases, self.in_channels, self.out_channels))
        self.att = torch.nn.Parameter(torch.empty(self.num_relations, self.num_bases))
        if root_weight:
            self.root = torch.nn.Parameter(torch.empty(self.in_channels, self.out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        size = self.num_bases * self.in_channels
        uniform(size, self.basis)
        uniform(size, self.att)
        uniform(size, self.root)
        uniform(size, self.bias)

    def fused_layer(self):
        """Whether the fused path's conditions on the layer itself hold: node_dim
        0 and message / update / aggregate not overridden."""
        cls = type(self)
        return (self.node_dim == 0 and self.aggr == "add" and cls.message is RGCNConv.message
                and cls.update is RGCNConv.update and cls.aggregate is MessagePassing.aggregate)

    def _fused_ok(self, x, edge_index, edge_type, edge_norm, size):
        if not self.fused_layer():
            return False
        for p in (self.basis, self.att, self.root, self.bias):
            if p is not None and not (p.is_cuda and p.dtype == torch.float32):
                return False
        if x is None:
            n = self.in_channels
        elif torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 \
                and x.shape[1] == self.in_channels:
            n = x.shape[0]
        else:                                              # a bipartite (x_src, x_dst) pair, another dtype
            return False
        if size is not None and tuple(size) != (n, n):
            return False
        if not (edge_index.is_cuda and torch.is_tensor(edge_type) and edge_type.is_cuda
                and edge_type.dtype == torch.int64 and edge_type.dim() == 1):
            return False
        if edge_norm is not None and not (edge_norm.is_cuda and edge_norm.dtype == torch.float32
                                          and edge_norm.dim() == 1 and not edge_norm.requires_grad):
            return False
        # the featureless kernels see rows of B * Cout floats only (Cin is the node count there)
        return _ops.rgcn_ok(self.num_relations, self.num_bases, self.out_channels if x is None else self.in_channels,
                            self.out_channels)

    def forward(self, x, edge_index, edge_type, edge_norm=None, size=None, form=None):
        """x [N, in_channels] or None (featureless: N = in_channels), edge_type
        int64 [E] in [0, num_relations), edge_norm [E] or None; form: None, or
        "bins" / "gather" to force one kernel form of the fused path."""
        if not self._fused_ok(x, edge_index, edge_type, edge_norm, size):
            if form is not None:
                raise ValueError("RGCNConv: form=%r needs the fused path (see the module docstring)" % (form,))
            if x is None and size is None:                 # every node owns a row of the output
                size = (self.in_channels, self.in_channels)
            return self.propagate(edge_index, size=size, x=x, edge_type=edge_type, edge_norm=edge_norm)
        n = self.in_channels if x is None else x.shape[0]
        return _ops.rgcn_propagate(graph_for(edge_index, n, n, self.flow), x, edge_type, edge_norm, self.att,
                                   self.basis, root=self.root, bias=self.bias, form=form)

    def message(self, x_j, edge_index_j, edge_type, edge_norm):
        w = torch.matmul(self.att, self.basis.view(self.num_bases, -1))
        if x_j is None:                                    # an embedding lookup by (relation, source node)
            w = w.view(-1, self.out_channels)
            index = edge_type * self.in_channels + edge_index_j
            out = torch.index_select(w, 0, index)
        else:
            w = w.view(self.num_relations, self.in_channels, self.out_channels)
            w = torch.index_select(w, 0, edge_type)
            out = torch.bmm(x_j.unsqueeze(1), w).squeeze(-2)
        return out if edge_norm is None else out * edge_norm.view(-1, 1)

    def update(self, aggr_out, x):
        out = aggr_out
        if self.root is not None:
            out = out + self.root if x is None else out + torch.matmul(x, self.root)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self):
        return "{}({}, {}, num_relations={})".format(self.__class__.__name__, self.in_channels, self.out_channels,
                                                     self.num_relations)
