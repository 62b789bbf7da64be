"""ARMAConv: the auto-regressive moving average graph filter of Bianchi et al.
(Graph Neural Networks with Convolutional ARMA Filters), PyG 1.4.3
nn.conv.arma_conv [U]: K parallel stacks of T recurrent steps

    H_{t+1}[k] = act(L H_t[k] W_t[k] + dropout(x) V_t[k] + b_t[k]),   H_0[k] = x
    out = mean_k H_T[k],   L = D^-1/2 A D^-1/2 (no self loops, summed at edge_index[0])

MI355X engine: the hidden state lives stack-minor as [N, K*C], so one gathered
row carries all K stacks, and each step is one fused launch (gather, skip,
bias, activation, the next step's per-stack transform or the final mean;
mi355_mp.ops.arma_propagate: csrc/mp_arma.hip).  The fused path is taken for
act None / ReLU, a (K, C) inside mp_arma_ok, fp32 device tensors and a 2-D x;
everything else runs upstream's recipe in torch ops.  The edge weights get no
gradient on the fused path: an edge_weight that requires one takes the recipe.
"""
import torch
import torch.nn.functional as F

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import glorot, zeros


def _is_relu(act):
    return act in (F.relu, torch.relu, torch.nn.functional.relu)


class ARMAConv(torch.nn.Module):
    r"""Args:
        in_channels (int), out_channels (int), num_stacks (int, default 1): K,
        num_layers (int, default 1): T, shared_weights (bool, default False):
        the steps share their parameters (the first transform aside), act
        (callable or None, default F.relu), dropout (float, default 0): on the
        skip connection, bias (bool, default True).
    """

    def __init__(self, in_channels, out_channels, num_stacks=1, num_layers=1, shared_weights=False, act=F.relu,
                 dropout=0, bias=True):
        super(ARMAConv, self).__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.num_stacks, self.num_layers = int(num_stacks), int(num_layers)
        self.shared_weights = bool(shared_weights)
        self.act = act
        self.dropout = dropout
        K, T, F_in, F_out = self.num_stacks, self.num_layers, self.in_channels, self.out_channels
        w = torch.nn.Parameter
        self.ws = torch.nn.ParameterList([w(torch.empty(K, F_in, F_out))])
        for _ in range(min(1, T - 1) if self.shared_weights else T - 1):
            self.ws.append(w(torch.empty(K, F_out, F_out)))
        n_skip = 1 if self.shared_weights else T
        self.vs = torch.nn.ParameterList([w(torch.empty(K, F_in, F_out)) for _ in range(n_skip)])
        if bias:
            self.bias = torch.nn.ParameterList([w(torch.empty(K, 1, F_out)) for _ in range(n_skip)])
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for p in self.ws:
            glorot(p)
        for p in self.vs:
            glorot(p)
        if self.bias is not None:
            for p in self.bias:
                zeros(p)

    def fused(self, x, edge_weight=None):
        """Whether the fused path's conditions hold for this input."""
        if not (self.act is None or _is_relu(self.act)):
            return False
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in (x, self.ws[0])):
            return False
        if edge_weight is not None and (edge_weight.requires_grad or not edge_weight.is_cuda):
            return False
        return _ops.arma_ok(self.num_stacks, self.out_channels)

    def forward(self, x, edge_index, edge_weight=None, form=None):
        """x [N, in_channels], edge_weight [E] or None (ones); form: None, or
        "fused" / "unfused" to force a path ("fused" raises where it cannot run)."""
        if form not in (None, "fused", "unfused"):
            raise ValueError("ARMAConv: unknown form %r" % (form,))
        fused = self.fused(x, edge_weight)
        if form == "fused" and not fused:
            raise ValueError("ARMAConv: form='fused' needs act None / ReLU, a shape inside arma_ok, fp32 device "
                             "tensors, a 2-D x and no gradient for edge_weight (see ARMAConv.fused)")
        if not fused or form == "unfused":
            return self.recipe(x, edge_index, edge_weight)
        n = x.shape[0]
        graph = graph_for(edge_index, n, n, "target_to_source")     # row = edge_index[0] is the destination
        return _ops.arma_propagate(graph, x, list(self.ws), list(self.vs),
                                   None if self.bias is None else list(self.bias), self.num_stacks,
                                   self.out_channels, self.num_layers, self.shared_weights, self.act is not None,
                                   self.dropout, self.training, edge_weight=edge_weight)

    def recipe(self, x, edge_index, edge_weight=None):
        """Upstream's forward in torch ops."""
        if edge_weight is None:
            edge_weight = x.new_ones((edge_index.size(1),))
        edge_weight = edge_weight.view(-1)
        row, col = edge_index
        n = x.size(0)
        deg = torch.zeros(n, dtype=edge_weight.dtype, device=edge_weight.device).index_add_(0, row, edge_weight)
        dinv = deg.pow(-0.5)
        dinv[dinv == float("inf")] = 0
        lap = (dinv[row] * edge_weight * dinv[col]).view(1, -1, 1)
        x = x.unsqueeze(0)
        out = x
        for t in range(self.num_layers):
            w = self.ws[min(t, 1) if self.shared_weights else t]
            out = torch.matmul(out, w)
            msg = out[:, col] * lap
            out = torch.zeros_like(out).index_add_(1, row, msg)
            skip = F.dropout(x, p=self.dropout, training=self.training)
            out = out + torch.matmul(skip, self.vs[0 if self.shared_weights else t])
            if self.bias is not None:
                out = out + self.bias[0 if self.shared_weights else t]
            if self.act is not None:
                out = self.act(out)
        return out.mean(dim=0)

    def __repr__(self):
        return "{}({}, {}, num_stacks={}, num_layers={})".format(self.__class__.__name__, self.in_channels,
                                                                  self.out_channels, self.num_stacks,
                                                                  self.num_layers)
