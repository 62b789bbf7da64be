"""NNConv: the edge-conditioned convolution of Gilmer et al. (Neural Message
Passing for Quantum Chemistry, ICML 2017) and Simonovsky & Komodakis (CVPR
2017), PyG 1.4.3 nn.conv.nn_conv [U]:

    x'_i = AGGR_{j in N(i)} x_j . reshape(nn(e_ij), [Cin, Cout])  + x_i root + b

MI355X engine: when ``nn`` ends in a torch.nn.Linear (the head) the per-edge
weight matrices are never built.  With h_e the head's input, ht_e = [h_e, 1]
and L[(h, c), o] = head.weight[c * Cout + o, h] (row block h = H: head.bias),

    sum_e x_j W_e = (sum_e ht_e (x) x_j) L

one segmented HIP pass plus one node-level GEMM (mi355_mp.ops.nnconv_propagate:
csrc/mp_nnconv.hip); the trunk nn[:-1] runs in torch and receives its gradient
through d h.  The fused path is taken for aggr "add" / "mean", a head with
out_features == Cin * Cout and no hooks, a shape inside mp_nnconv_ok and device
tensors; everything else (aggr "max", any other nn, a hooked head) runs
upstream's message / update on the generic MessagePassing path.
"""
import torch

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import reset, uniform
from .message_passing import MessagePassing


def _as_columns(t):
    """A per-node or per-edge vector as a one-column matrix."""
    return t.unsqueeze(-1) if t.dim() == 1 else t


def _hooked(module):
    """True when any forward, forward-pre or backward hook sits on the module:
    folding it into the kernels would skip them."""
    names = ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks",
             "_forward_hooks_with_kwargs", "_forward_pre_hooks_with_kwargs")
    return any(len(getattr(module, n, None) or ()) > 0 for n in names)


class NNConv(MessagePassing):
    r"""Args:
        in_channels (int), out_channels (int), nn (torch.nn.Module): maps edge
        features [E, D] to [E, in_channels * out_channels], aggr ("add" / "mean"
        / "max", default "add"), root_weight (bool, default True), bias (bool,
        default True).
    """

    def __init__(self, in_channels, out_channels, nn, aggr="add", root_weight=True, bias=True, **kwargs):
        super(NNConv, self).__init__(aggr=aggr, **kwargs)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.nn = nn
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
        reset(self.nn)
        uniform(self.in_channels, self.root)
        uniform(self.in_channels, self.bias)

    def fused_head(self):
        """(trunk, head) when the fused path's conditions on the layer hold --
        aggr add / mean, nn a Linear or a Sequential ending in one, that Linear
        producing Cin * Cout values, no hooks on it, node_dim 0 and message /
        update / aggregate not overridden -- else None.  trunk is the tuple
        of the modules before the head, called in order (None when there are
        none: a bare Linear)."""
        if self.aggr not in ("add", "mean") or self.node_dim != 0:
            return None
        cls = type(self)
        if (cls.message is not NNConv.message or cls.update is not NNConv.update
                or cls.aggregate is not MessagePassing.aggregate):
            return None
        nn = self.nn
        if type(nn) is torch.nn.Linear:
            trunk, head = None, nn
        elif type(nn) is torch.nn.Sequential and len(nn) > 0 and type(nn[-1]) is torch.nn.Linear:
            if _hooked(nn):                                # a hook on the container sees nn's output
                return None
            mods = tuple(nn.children())
            trunk, head = (mods[:-1] or None), mods[-1]
        else:
            return None
        if head.out_features != self.in_channels * self.out_channels or _hooked(head):
            return None
        return trunk, head

    def _fused_ok(self, x, edge_attr):
        fused = self.fused_head()
        if fused is None:
            return None
        head = fused[1]
        if not (x.is_cuda and edge_attr.is_cuda and head.weight.is_cuda and x.dtype == torch.float32
                and edge_attr.dtype == torch.float32 and head.weight.dtype == torch.float32):
            return None
        if not _ops.nnconv_ok(head.in_features, self.in_channels, self.out_channels):
            return None
        return fused

    def forward(self, x, edge_index, edge_attr, form=None):
        """x [N, in_channels] (or [N]), edge_attr [E, D] (or [E]); form: None, or
        "bins" / "gather" to force one kernel form of the fused path."""
        x, pseudo = _as_columns(x), _as_columns(edge_attr)
        fused = self._fused_ok(x, pseudo)
        if fused is None:
            if form is not None:
                raise ValueError("NNConv: form=%r needs the fused path (see NNConv.fused_head)" % (form,))
            return self.propagate(edge_index, x=x, pseudo=pseudo)
        trunk, head = fused
        # one layout for the kernels and the GEMMs (x root, x L'): the GEMM library picks its kernel by the
        # operand layout, so a strided or transposed view of x would round differently from its contiguous copy
        x = x.contiguous()
        h = pseudo
        for module in trunk or ():
            h = module(h)
        n = x.shape[0]
        out = _ops.nnconv_propagate(graph_for(edge_index, n, n, self.flow), x, h, head.weight, head.bias, self.aggr,
                                    form=form, bias=self.bias)
        return out if self.root is None else torch.addmm(out, x, self.root)

    def message(self, x_j, pseudo):
        weight = self.nn(pseudo).view(-1, self.in_channels, self.out_channels)
        return torch.matmul(x_j.unsqueeze(1), weight).squeeze(1)

    def update(self, aggr_out, x):
        if self.root is not None:
            aggr_out = aggr_out + torch.mm(x, self.root)
        if self.bias is not None:
            aggr_out = aggr_out + self.bias
        return aggr_out

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)
