import torch
import torch.nn.functional as F
from torch.nn import Parameter

from ..inits import uniform
from . import _dense


class DenseSAGEConv(torch.nn.Module):
    r"""The dense-batch GraphSAGE operator (PyG 1.4.3 nn.dense.DenseSAGEConv):

        out = mean_{j in N(i) + i} x_j  @  W + b

    on x [B, N, F] and adj [B, N, N], with the mean's degree clamped at 1.  The
    aggregation is one fused pass over adj (no clone for the self loops, the
    degree from the same pass) when the inputs are float32 on the GPU, adj needs
    no gradient and the graphs have at most 128 nodes (nn/dense/_dense.py
    agg_fused); otherwise the upstream recipe in torch ops.

    Args:
        in_channels (int), out_channels (int)
        normalize (bool): L2-normalise the output rows. (default: False)
        bias (bool): learn an additive bias. (default: True)
    """

    def __init__(self, in_channels, out_channels, normalize=False, bias=True):
        super(DenseSAGEConv, self).__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.normalize = normalize
        self.weight = Parameter(torch.Tensor(self.in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        uniform(self.in_channels, self.weight)
        uniform(self.in_channels, self.bias)

    def forward(self, x, adj, mask=None, add_loop=True):
        """x [B, N, F] (or [N, F]), adj [B, N, N] (or [N, N]), mask [B, N] of the
        valid nodes of each graph, add_loop: count every node as its own neighbour."""
        x = x.unsqueeze(0) if x.dim() == 2 else x
        adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        B, N, _ = x.size()
        if adj.size(0) != B:
            adj = adj.expand(B, N, N)
        out = _dense.mean_agg(x, adj, add_loop)
        out = torch.matmul(out, self.weight)
        if self.bias is not None:
            out = out + self.bias
        if self.normalize:
            out = F.normalize(out, p=2, dim=-1)
        if mask is not None:
            out = out * mask.view(B, N, 1).to(x.dtype)
        return out

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)
