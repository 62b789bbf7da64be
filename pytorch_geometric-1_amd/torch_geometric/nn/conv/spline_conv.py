"""SplineConv: the spline-based convolution of SplineCNN (Fey et al., CVPR 2018).

    x'_i = AGGR_{j in N(i)} sum_s basis_s(u_ij) * x_j Theta[wi_s(u_ij)]  + x_i Theta_root + b

with open or closed B-spline bases of degree 1..3 over ``dim`` pseudo-coordinate
dimensions u_ij in [0, 1] (per edge: S = (degree + 1)^dim basis values and
kernel indices into the K = prod(kernel_size) weight matrices).

MI355X engine: the per-edge basis, weighting and scatter run as ONE segmented
HIP pass over the cached destination CSR plus one dense GEMM
(mi355_mp.ops.spline_propagate): neither x_j, the basis, the kernel indices nor
the messages are ever materialised, and the backward reuses the same two
kernels over the transposed CSR.  aggr is "mean" or "add"; "max", shapes
outside the fused path's limits (mp_spline_ok in include/mi355_mp.h) and
gradients with respect to the pseudo-coordinates raise NotImplementedError.
"""
import math

import torch

import torch_geometric
from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ...utils.repeat import repeat
from .message_passing import MessagePassing


def _as_columns(t):
    """A per-node or per-edge vector as a one-column matrix."""
    return t[:, None] if t.dim() == 1 else t


class SplineConv(MessagePassing):
    r"""Args:
        in_channels (int), out_channels (int), dim (int): pseudo-coordinate
        dimensionality, kernel_size (int or [int]), is_open_spline (bool or
        [bool], default True), degree (int, default 1), aggr ("add" / "mean" /
        "max", default "mean"), root_weight (bool, default True), bias (bool,
        default True).
    """

    def __init__(self, in_channels, out_channels, dim, kernel_size, is_open_spline=True, degree=1, aggr="mean",
                 root_weight=True, bias=True, **kwargs):
        super().__init__(aggr=aggr, **kwargs)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.dim, self.degree = int(dim), int(degree)
        sizes = [int(k) for k in repeat(kernel_size, self.dim)]
        opens = [bool(o) for o in repeat(is_open_spline, self.dim)]
        if min(sizes) < 1:
            raise ValueError("SplineConv: kernel_size entries must be positive (got %s)" % (sizes,))
        self.register_buffer("kernel_size", torch.tensor(sizes, dtype=torch.long))
        self.register_buffer("is_open_spline", torch.tensor(opens, dtype=torch.uint8))
        self._sync_geometry()
        n_kernels = math.prod(sizes)
        self.weight = torch.nn.Parameter(torch.empty(n_kernels, self.in_channels, self.out_channels))
        self.root = torch.nn.Parameter(torch.empty(self.in_channels, self.out_channels)) if root_weight else None
        self.bias = torch.nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def _sync_geometry(self):
        """Host copies of the two buffers: the kernels take them as launch
        arguments, and reading the buffers back on every forward would be a
        device sync.  The buffers stay authoritative: the copies are refreshed
        whenever a state dict is loaded."""
        self._kernel_size = [int(k) for k in self.kernel_size.tolist()]
        self._is_open_spline = [int(o) for o in self.is_open_spline.tolist()]

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._sync_geometry()

    def reset_parameters(self):
        # weight and root: uniform in +-1/sqrt(in_channels * K); bias: zeros
        bound = 1.0 / math.sqrt(self.in_channels * self.weight.shape[0])
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.root is not None:
                self.root.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def _debug_checks(self, x, pseudo):
        if x.shape[1] != self.in_channels:
            raise RuntimeError("SplineConv(%d, %d): x carries %d node features"
                               % (self.in_channels, self.out_channels, x.shape[1]))
        if pseudo.shape[1] != self.dim:
            raise RuntimeError("SplineConv(dim=%d): pseudo has dimensionality %d" % (self.dim, pseudo.shape[1]))
        if pseudo.numel():
            lo, hi = float(pseudo.min()), float(pseudo.max())
            if lo < 0.0 or hi > 1.0:
                raise RuntimeError("SplineConv: pseudo-coordinates span [%g, %g], outside [0, 1]" % (lo, hi))

    def forward(self, x, edge_index, pseudo, form=None):
        """x [N, in_channels] (or [N]), pseudo [E, dim] (or [E]) in [0, 1];
        form: None, or "bins" / "gather" to force one kernel form."""
        x, pseudo = _as_columns(x), _as_columns(pseudo)
        if torch_geometric.is_debug_enabled():
            self._debug_checks(x, pseudo)
        n = x.shape[0]
        out = _ops.spline_propagate(graph_for(edge_index, n, n, self.flow), x, self.weight, pseudo,
                                    self._kernel_size, self._is_open_spline, self.degree, self.aggr, form=form,
                                    bias=self.bias)
        return out if self.root is None else torch.addmm(out, x, self.root)

    def __repr__(self):
        return f"{type(self).__name__}({self.in_channels}, {self.out_channels}, dim={self.dim})"
