"""AGNNConv (PyG 1.4.3 nn.conv.agnn_conv [U]; caller
/root/reference/ConvexPruning.py:236-237, `AGNNConv(requires_grad=True)`).

    x'_i = sum_{j in N(i) u {i}} P_ij x_j,
    P_ij = softmax_j( beta * cos(x_i, x_j) )

forward: self loops removed then added, then the attention and the weighted sum.

MI355X engine: the row that gives the score, x_j through cos(x_i, x_j), is the row
that is the message, so one fused HIP pass per destination row gathers each x_j
once, takes the dot product and the online softmax from it and adds it into the
output from the same registers (mi355_mp.ops.agnn_propagate: csrc/mp_agnn.hip),
forward and backward, deterministic; no [E, F] array exists, and beta is read on
the device.  The fused path is taken for device fp32 2-D x with at least one
node (a non-contiguous view is copied once, so a view and its contiguous clone
give the same bits), node_dim 0, message / update / aggregate not overridden and F
inside ops.agnn_ok; it serves both flows, the learned beta and the beta buffer.
The looped edge list is cached on the caller's edge_index (_structure.gat_loops),
so graph_for meets the same tensor on every call.  Everything else (float64, a
subclass's own message, F above the limit) runs the message below on the generic
MessagePassing path: native row gathers of x_j / x_norm_i / x_norm_j, the per-edge
score, utils.softmax on the native segment max / sum (+1e-16), and the native
segmented sum of x_j * alpha.
"""
import torch
import torch.nn.functional as F
from torch.nn import Parameter

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ...utils import remove_self_loops, add_self_loops, softmax
from .message_passing import MessagePassing
from ._structure import gat_loops


class AGNNConv(MessagePassing):
    def __init__(self, requires_grad=True, **kwargs):
        super(AGNNConv, self).__init__(aggr="add", **kwargs)
        self.requires_grad = requires_grad
        if requires_grad:
            self.beta = Parameter(torch.Tensor(1))
        else:
            self.register_buffer("beta", torch.ones(1))
        self.reset_parameters()

    def reset_parameters(self):
        if self.requires_grad:
            self.beta.data.fill_(1)

    def _beta(self):
        return self.beta if self.requires_grad else self._buffers["beta"]

    def _fused_ok(self, x, edge_index):
        cls = type(self)
        if not (self.node_dim == 0 and self.aggr == "add" and cls.message is AGNNConv.message
                and cls.update is MessagePassing.update and cls.aggregate is MessagePassing.aggregate):
            return False
        beta = self._beta()
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and x.size(0) > 0 and x.size(1) > 0):
            return False
        if not (edge_index.is_cuda and beta.dtype == torch.float32 and beta.device == x.device):
            return False
        return _ops.agnn_ok(x.size(1))

    def forward(self, x, edge_index):
        """"""
        if self._fused_ok(x, edge_index):
            n = x.size(0)
            edge_index = gat_loops(edge_index, n)
            # tasks of at least agnn_split_chunk() units: the kernels then split long rows on a graph of any size
            graph = graph_for(edge_index, n, n, self.flow, _ops.agnn_target_tasks(n, edge_index.size(1)))
            # one contiguous x whatever the view: the kernels' lane mapping (vec4 or scalar) follows the rows'
            # alignment, so a view would be summed in another order than its own copy
            return _ops.agnn_propagate(graph, x.contiguous(), self._beta())
        edge_index, _ = remove_self_loops(edge_index)
        edge_index, _ = add_self_loops(edge_index, num_nodes=x.size(self.node_dim))
        x_norm = F.normalize(x, p=2, dim=-1)
        return self.propagate(edge_index, x=x, x_norm=x_norm, num_nodes=x.size(self.node_dim))

    def message(self, edge_index_i, x_j, x_norm_i, x_norm_j, num_nodes):
        beta = self._beta()
        alpha = beta * (x_norm_i * x_norm_j).sum(dim=-1)
        alpha = softmax(alpha, edge_index_i, num_nodes)
        return x_j * alpha.view(-1, 1)

    def __repr__(self):
        return "{}()".format(self.__class__.__name__)
