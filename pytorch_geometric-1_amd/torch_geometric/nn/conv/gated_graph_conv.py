"""GatedGraphConv: the gated graph network of Li et al. (Gated Graph Sequence
Neural Networks), PyG's nn.conv.gated_graph_conv [U]: L recurrent steps

    m_i = AGGR_{j in N(i)} e_ji * (h_j W_l),   h_i <- GRUCell(m_i, h_i),   h^(0) = x padded with zeros to C

MI355X engine: sum and mean aggregation are linear, so W_l folds into the cell's
input weight, (A h)(W_l W_ih^T), and a step is the engine's fused aggregation of
h itself plus one MFMA kernel for the whole cell (both gate GEMMs and the gate
chain: mi355_mp.ops.gru_cell, csrc/mp_gru.hip).  torch computes W_l W_ih^T inside
the autograd graph, so weight and rnn.weight_ih get their gradients through it.
The fused path is taken for aggr "add" / "mean", C inside mp_gru_ok, fp32 device
tensors and a 1-D or 2-D x; everything else runs upstream's recipe in torch ops
(max does not commute with W_l).  The edge weights get no gradient on the fused
path: an edge_weight that requires one takes the recipe.
"""
import torch
from torch.nn import Parameter

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import uniform
from .message_passing import MessagePassing


class GatedGraphConv(MessagePassing):
    r"""Args:
        out_channels (int): C, num_layers (int): L, aggr (string, default
        "add"): "add", "mean" or "max", bias (bool, default True): of the GRU cell.
    """

    def __init__(self, out_channels, num_layers, aggr="add", bias=True, **kwargs):
        super(GatedGraphConv, self).__init__(aggr=aggr, **kwargs)
        self.out_channels, self.num_layers = int(out_channels), int(num_layers)
        self.weight = Parameter(torch.Tensor(self.num_layers, self.out_channels, self.out_channels))
        self.rnn = torch.nn.GRUCell(self.out_channels, self.out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        uniform(self.out_channels, self.weight)
        self.rnn.reset_parameters()

    def _state(self, x, width):
        h = x if x.dim() == 2 else x.unsqueeze(-1)
        if h.size(1) > self.out_channels:
            raise ValueError("The number of input channels is not allowed to be larger than the number of output "
                             "channels")
        return torch.nn.functional.pad(h, (0, width - h.size(1))) if h.size(1) < width else h

    def fused(self, x, edge_weight=None):
        """Whether the fused path's conditions hold for this input."""
        if self.aggr not in ("add", "mean") or x.dim() not in (1, 2):
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in (x, self.weight)):
            return False
        if edge_weight is not None and (edge_weight.requires_grad or not edge_weight.is_cuda):
            return False
        return _ops.gru_ok(self.out_channels)

    def forward(self, x, edge_index, edge_weight=None, form=None):
        """x [N, <= out_channels] (or [N]), edge_weight [E] or None; form: None, or
        "fused" / "unfused" to force a path ("fused" raises where it cannot run)."""
        if form not in (None, "fused", "unfused"):
            raise ValueError("GatedGraphConv: unknown form %r" % (form,))
        fused = self.fused(x, edge_weight)
        if form == "fused" and not fused:
            raise ValueError("GatedGraphConv: form='fused' needs aggr 'add' / 'mean', out_channels inside gru_ok, "
                             "fp32 device tensors, a 1-D or 2-D x and no gradient for edge_weight (see "
                             "GatedGraphConv.fused)")
        if not fused or form == "unfused":
            return self.recipe(x, edge_index, edge_weight)
        C = self.out_channels
        P = _ops.gru_width(C)
        h = self._state(x, P)
        n = h.size(0)
        graph = graph_for(edge_index, n, n, self.flow)
        wh = self.rnn.weight_hh.t()
        b_ih, b_hh = (self.rnn.bias_ih, self.rnn.bias_hh) if self.rnn.bias else (None, None)
        for layer in range(self.num_layers):
            a = _ops.fused_propagate(graph, h, edge_index, edge_weight=edge_weight, reduce=self.aggr)
            h = _ops.gru_cell(a, h, torch.mm(self.weight[layer], self.rnn.weight_ih.t()), wh, b_ih, b_hh)
        return h[:, :C] if P != C else h

    def recipe(self, x, edge_index, edge_weight=None):
        """Upstream's forward in torch ops: index_add_ for "add" / "mean" (any device), propagate for "max"."""
        h = self._state(x, self.out_channels)
        i, j = self._ij()
        for layer in range(self.num_layers):
            m = torch.matmul(h, self.weight[layer])
            if self.aggr == "max":
                m = self.propagate(edge_index, x=m, edge_weight=edge_weight)
            else:
                msg = self.message(m[edge_index[j]], edge_weight)
                m = torch.zeros_like(m).index_add_(0, edge_index[i], msg)
                if self.aggr == "mean":
                    deg = torch.bincount(edge_index[i], minlength=h.size(0)).clamp(min=1)
                    m = m / deg.to(m.dtype).view(-1, 1)
            h = self.rnn(m, h)
        return h

    def message(self, x_j, edge_weight):
        return x_j if edge_weight is None else edge_weight.view(-1, 1) * x_j

    def _fused_message(self, kwargs):
        if type(self).message is GatedGraphConv.message:
            return "x", kwargs.get("edge_weight", None)
        return None

    def __repr__(self):
        return "{}({}, num_layers={})".format(self.__class__.__name__, self.out_channels, self.num_layers)
