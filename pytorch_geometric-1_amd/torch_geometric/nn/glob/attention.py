import torch

from ..inits import reset
from ._readout import fused_layout, last_graph_plus_one, recipe
from mi355_mp import ops as _ops


class GlobalAttention(torch.nn.Module):
    r"""Global soft attention of `"Gated Graph Sequence Neural Networks"
    <https://arxiv.org/abs/1511.05493>`_ (PyG 1.4.3 nn.glob.GlobalAttention):

        r_g = sum_{i in g} softmax_graph(gate_nn(x_i)) * nn(x_i)

    Args:
        gate_nn (torch.nn.Module): maps [-1, in_channels] to [-1, 1].
        nn (torch.nn.Module, optional): maps [-1, in_channels] to
            [-1, out_channels] before the sum. (default: None)
    """

    def __init__(self, gate_nn, nn=None):
        super(GlobalAttention, self).__init__()
        self.gate_nn = gate_nn
        self.nn = nn
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.gate_nn)
        reset(self.nn)

    def forward(self, x, batch, size=None):
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        if size is None:
            size = 1 if batch is None else last_graph_plus_one(batch, x.shape[0])
        gate = self.gate_nn(x).view(-1, 1)
        x = self.nn(x) if self.nn is not None else x
        assert gate.dim() == x.dim() and gate.size(0) == x.size(0)
        layout = fused_layout(x, batch, size) if gate.dtype == torch.float32 else None
        if layout is not None:
            return _ops.attention_readout(x, layout, score=gate.view(-1))
        if batch is None:
            batch = x.new_zeros(x.shape[0], dtype=torch.long)
        return recipe(x, gate, batch, size)

    def __repr__(self):
        return "{}(gate_nn={}, nn={})".format(self.__class__.__name__, self.gate_nn, self.nn)
