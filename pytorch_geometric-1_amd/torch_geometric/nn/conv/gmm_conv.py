"""GMMConv: the Gaussian mixture model convolution of Monti et al. (Geometric
deep learning on graphs and manifolds using mixture model CNNs, CVPR 2017),
PyG 1.4.3 nn.conv.gmm_conv [U]:

    x'_i = AGGR_{j in N(i)} sum_k w_k(e_ij) . (x_j g)_k  + x_i root + b
    w_k(e) = exp(sum_d -0.5 (e_d - mu_kd)^2 / (1e-15 + sigma_kd^2))

MI355X engine: with shared Gaussians the K weights of an edge are a closed-form
function of its D pseudo-coordinates, so they are evaluated inside the
segmented HIP pass and neither the gathered [E, K, Cout] operand nor an [E, K]
coefficient array is built.  With G'[(k, c), m] = g[c, k * Cout + m],

    sum_e sum_k w_k(e) (x_j g)_k = (sum_e w(e) (x) x_j) G'

one segmented pass plus one node-level GEMM (mi355_mp.ops.gmm_propagate:
csrc/mp_gmm.hip), and mu / sigma / pseudo receive their gradients from one
deterministic two-stage reduction.  The fused path is taken for shared
Gaussians, aggr "add" / "mean", a shape inside mp_gmm_ok and fp32 device
tensors; everything else (separate_gaussians=True, aggr "max", a subclass that
overrides message / update / aggregate) runs upstream's message on the generic
MessagePassing path.
"""
import torch

from mi355_mp import ops as _ops
from mi355_mp.graph import graph_for

from ..inits import glorot, zeros
from .message_passing import MessagePassing

EPS = 1e-15


def _as_columns(t):
    """A per-node or per-edge vector as a one-column matrix."""
    return t.unsqueeze(-1) if t.dim() == 1 else t


class GMMConv(MessagePassing):
    r"""Args:
        in_channels (int), out_channels (int), dim (int): pseudo-coordinate
        dimensionality, kernel_size (int): number of Gaussians K,
        separate_gaussians (bool, default False): one set of Gaussians per
        (input, output) channel pair, aggr ("add" / "mean" / "max", default
        "mean"), root_weight (bool, default True), bias (bool, default True).
    """

    def __init__(self, in_channels, out_channels, dim, kernel_size, separate_gaussians=False, aggr="mean",
                 root_weight=True, bias=True, **kwargs):
        super(GMMConv, self).__init__(aggr=aggr, **kwargs)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.dim, self.kernel_size = int(dim), int(kernel_size)
        self.separate_gaussians = bool(separate_gaussians)
        Cin, M, K, D = self.in_channels, self.out_channels, self.kernel_size, self.dim
        self.g = torch.nn.Parameter(torch.empty(Cin, M * K))
        if not self.separate_gaussians:
            self.mu = torch.nn.Parameter(torch.empty(K, D))
            self.sigma = torch.nn.Parameter(torch.empty(K, D))
        else:
            self.mu = torch.nn.Parameter(torch.empty(Cin, M, K, D))
            self.sigma = torch.nn.Parameter(torch.empty(Cin, M, K, D))
        if root_weight:
            self.root = torch.nn.Parameter(torch.empty(Cin, M))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(M))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.g)
        glorot(self.mu)
        glorot(self.sigma)
        glorot(self.root)
        zeros(self.bias)

    def fused(self):
        """Whether the fused path's conditions on the layer hold: shared
        Gaussians, aggr add / mean, node_dim 0 and message / update / aggregate
        not overridden."""
        if self.separate_gaussians or self.aggr not in ("add", "mean") or self.node_dim != 0:
            return False
        cls = type(self)
        return (cls.message is GMMConv.message and cls.update is GMMConv.update
                and cls.aggregate is MessagePassing.aggregate)

    def _fused_ok(self, x, pseudo):
        if not self.fused():
            return False
        tensors = (x, pseudo, self.g, self.mu, self.sigma)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return False
        if pseudo.dim() != 2 or pseudo.shape[1] != self.dim or x.dim() != 2 or x.shape[1] != self.in_channels:
            return False
        return _ops.gmm_ok(self.kernel_size, self.dim, self.in_channels, self.out_channels)

    def forward(self, x, edge_index, pseudo, form=None):
        """x [N, in_channels] (or [N]), pseudo [E, dim] (or [E]); form: None, or
        "bins" / "gather" to force one kernel form of the fused path."""
        x, pseudo = _as_columns(x), _as_columns(pseudo)
        if not self._fused_ok(x, pseudo):
            if form is not None:
                raise ValueError("GMMConv: form=%r needs the fused path (see GMMConv.fused)" % (form,))
            if not self.separate_gaussians:
                out = self.propagate(edge_index, x=torch.matmul(x, self.g), pseudo=pseudo)
            else:
                out = self.propagate(edge_index, x=x, pseudo=pseudo)
            if self.root is not None:
                out = out + torch.matmul(x, self.root)
            if self.bias is not None:
                out = out + self.bias
            return out
        # one layout for the kernels and the GEMMs (x root, x g): the GEMM library picks its kernel by the
        # operand layout, so a strided or transposed view of x would round differently from its contiguous copy
        x = x.contiguous()
        n = x.shape[0]
        out = _ops.gmm_propagate(graph_for(edge_index, n, n, self.flow), x, pseudo, self.mu, self.sigma, self.g,
                                 self.aggr, form=form, bias=self.bias)
        return out if self.root is None else torch.addmm(out, x, self.root)

    def message(self, x_j, pseudo):
        F, M = self.in_channels, self.out_channels
        (E, D), K = pseudo.size(), self.kernel_size
        if not self.separate_gaussians:
            gaussian = -0.5 * (pseudo.view(E, 1, D) - self.mu.view(1, K, D)).pow(2)
            gaussian = gaussian / (EPS + self.sigma.view(1, K, D).pow(2))
            gaussian = torch.exp(gaussian.sum(dim=-1))                      # [E, K]
            return (x_j.view(E, K, M) * gaussian.view(E, K, 1)).sum(dim=-2)
        gaussian = -0.5 * (pseudo.view(E, 1, 1, 1, D) - self.mu.view(1, F, M, K, D)).pow(2)
        gaussian = gaussian / (EPS + self.sigma.view(1, F, M, K, D).pow(2))
        gaussian = torch.exp(gaussian.sum(dim=-1))                          # [E, F, M, K]
        gaussian = (gaussian * self.g.view(1, F, M, K)).sum(dim=-1)         # [E, F, M]
        return (x_j.view(E, F, 1) * gaussian).sum(dim=-2)                   # [E, M]

    def update(self, aggr_out):
        return aggr_out

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)
