"""PointConv (PyG 1.4.3 nn.conv.point_conv [U]; upstream example
examples/pointnet++.py in the reference tree): the PointNet++ set abstraction

    x'_i = gamma( max_{j in N(i) u {i}} h( [x_j | pos_j - pos_i] ) )

The per-edge matrix [x_j | pos_j - pos_i] is written by one HIP kernel
(mi355_mp.ops.point_edge_features: the three gathers, the subtraction and the
cat of the generic path in one pass); h (local_nn) stays torch, the max is the
engine's segmented max with first-index argmax and gamma (global_nn) follows.
A subclass that overrides message() runs through the generic MessagePassing
path instead.
"""
import torch

from mi355_mp import ops as _ops

from ..inits import reset
from ...utils import remove_self_loops, add_self_loops
from .message_passing import MessagePassing


class PointConv(MessagePassing):
    def __init__(self, local_nn=None, global_nn=None, **kwargs):
        super(PointConv, self).__init__(aggr="max", **kwargs)
        self.local_nn = local_nn
        self.global_nn = global_nn
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.local_nn)
        reset(self.global_nn)

    def forward(self, x, pos, edge_index):
        """x: None, [N, F] or (x_src, x_dst); pos: [N, D] (self-loops are removed,
        then added) or (pos_src, pos_dst) (the edges are taken as they are)."""
        if torch.is_tensor(pos):
            edge_index, _ = remove_self_loops(edge_index)
            edge_index, _ = add_self_loops(edge_index, num_nodes=pos.size(0))
        if type(self).message is not PointConv.message or self.node_dim != 0:
            return self.propagate(edge_index, x=x, pos=pos)
        i, j = self._ij()
        pos_src, pos_dst = (pos[j], pos[i]) if isinstance(pos, (tuple, list)) else (pos, pos)
        x_src = x[j] if isinstance(x, (tuple, list)) else x
        if x_src is not None and x_src.dim() == 1:
            x_src = x_src.unsqueeze(-1)
        index = edge_index[i]
        msg = _ops.point_edge_features(x_src, pos_src, pos_dst, edge_index[j], index)
        if self.local_nn is not None:
            msg = self.local_nn(msg)
        out = self.aggregate(msg, index, pos_dst.size(0))
        return self.update(out)

    def message(self, x_j, pos_i, pos_j):
        msg = pos_j - pos_i
        if x_j is not None:
            msg = torch.cat([x_j, msg], dim=1)
        if self.local_nn is not None:
            msg = self.local_nn(msg)
        return msg

    def update(self, aggr_out):
        if self.global_nn is not None:
            aggr_out = self.global_nn(aggr_out)
        return aggr_out

    def __repr__(self):
        return "{}(local_nn={}, global_nn={})".format(self.__class__.__name__, self.local_nn, self.global_nn)
