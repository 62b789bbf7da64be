"""SplineConv on the GPU: the standalone basis, both fused aggregation kernels,
the layer's forward and backward in both forms, bit-exact and determinism
cases, the documented refusals and the example, all against the float64
restatement tests/_spline_ref.py.

Every float comparison uses the project's bound |err| <= 1e-5 * sum |terms|
(sum |terms| = the same computation on absolute values).  A serial fp32 sum
over the 700-slot row emulated on the CPU stays at 1.9e-7 * sum |terms|, so
the restatement's own rounding is far inside the bound.
"""
import importlib.util
import math
import os

import pytest
import torch

from tests import _spline_ref as R
from tests._fuzz_cases import pseudo as _pseudo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 257
BOUND = 1e-5
KS, OPEN = [5, 3, 4], [1, 0, 1]


def _graph_edges():
    """N = 257 nodes, ~3000 edges: random edges with duplicates, node 5 with 700
    in-edges, nodes 200.. with no in-edge, nodes 230.. isolated."""
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 230, (2300,), generator=g)
    dst = torch.randint(0, 200, (2300,), generator=g)
    ei = torch.stack([src, dst])
    dup = ei[:, :40]                                                  # repeated (j, i) pairs
    hub = torch.stack([torch.randint(0, 230, (700,), generator=g), torch.full((700,), 5, dtype=torch.int64)])
    ei = torch.cat([ei, dup, hub], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()


@pytest.fixture(scope="module")
def edges():
    ei = _graph_edges()
    assert int(torch.bincount(ei[1], minlength=N)[5]) >= 700 and int(torch.bincount(ei[1], minlength=N)[200:].sum()) == 0
    return ei


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    ei = edges.to(DEV)
    return Graph(ei, N, N)


_assert_bound = R.assert_bound


# 1. basis -------------------------------------------------------------------

@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_basis_matches_the_restatement(D, M):
    from mi355_mp import ops
    ks, op = KS[:D], OPEN[:D]
    u = _pseudo(3000, D, ks, 10 * D + M)
    b, wi = ops.spline_basis(u.to(DEV), ks, op, M)
    rb, rwi = R.basis(u, ks, op, M)
    assert b.shape == rb.shape and wi.dtype == torch.int64
    assert torch.equal(wi.cpu(), rwi)
    assert float((b.cpu().double() - rb).abs().max()) <= 1e-6


# 2. both kernels directly ---------------------------------------------------

_GEOMS = {2: ([2], [1], 1), 25: ([5, 5], [1, 0], 2), 125: ([5, 5, 5], [1, 1, 0], 1)}


@pytest.mark.parametrize("K", [2, 25, 125])
@pytest.mark.parametrize("F", [1, 5, 33, 64, 130])
def test_kernels_against_float64(edges, graph, F, K):
    ks, op, M = _GEOMS[K]
    _check_kernels(edges, graph, ks, op, M, F, K)


# the instantiations the grid above does not launch: degree 3 at D = 3 (the widest
# bins / gather kernels), and kernel sizes <= degree at D > 1 (bins repeat within
# a slot: the serial read-modify-write path)
#
# and the block shapes of the bins kernel that K alone selects (waves = min(4,
# 65536 / (256 K))): three waves (K in 65..85), one wave (K in 129..256), and
# K = 256, whose 65536 bytes of dynamic LDS are the launch limit; F = 130 there
# has two feature tiles and a third with a two-lane tail
@pytest.mark.parametrize("ks,op,M,F", [([5, 5, 5], [1, 1, 0], 3, 1), ([3, 2], [0, 0], 2, 5),
                                       ([4, 3, 2], [0, 0, 0], 2, 33), ([3, 3, 3], [0, 0, 0], 3, 5),
                                       ([9, 8], [1, 0], 2, 5), ([4, 4, 5], [0, 1, 0], 1, 33),
                                       ([16, 16], [1, 1], 3, 5), ([256], [1], 1, 1), ([256], [0], 3, 64),
                                       ([8, 8, 4], [1, 0, 1], 2, 130), ([13, 10], [0, 0], 1, 1)])
def test_kernels_other_instantiations(edges, graph, ks, op, M, F):
    _check_kernels(edges, graph, ks, op, M, F, math.prod(ks))


def _check_kernels(edges, graph, ks, op, M, F, K):
    from mi355_mp import ops
    D = len(ks)
    E = edges.shape[1]
    u = _pseudo(E, D, ks, K + F)
    rb, rwi = R.basis(u, ks, op, M)
    geom = ops._spline_geom(ks, op, M, D, F)
    assert geom[2] == K
    g = torch.Generator().manual_seed(F * 1000 + K)
    x = torch.randn(N, F, generator=g)
    xk = torch.randn(N, K * F, generator=g)
    bias = torch.randn(F, generator=g)
    scale = torch.rand(N, generator=g) + 0.5
    ud, csr = u.to(DEV), graph.dst
    dst, src = edges[1], edges[0]
    for sc in (None, scale):
        scd = None if sc is None else sc.to(DEV)
        A = ops.spline_bins(csr, ud, geom, M, x.to(DEV), scd)
        assert A.shape == (N, K * F)
        _assert_bound(A, R.bins(dst, src, N, rb, rwi, K, x, sc), R.bins(dst, src, N, rb, rwi, K, x.abs(), sc),
                      "bins F=%d K=%d scale=%s" % (F, K, sc is not None))
        assert float(A[200:].abs().max()) == 0.0                       # rows without slots are zero
        for bs in (None, bias):
            bd = None if bs is None else bs.to(DEV)
            o = ops.spline_gather(csr, ud, geom, M, xk.to(DEV), F, scd, bd)
            _assert_bound(o, R.gather(dst, src, N, rb, rwi, K, xk, F, sc, bs),
                          R.gather(dst, src, N, rb, rwi, K, xk.abs(), F, sc, None if bs is None else bs.abs()),
                          "gather F=%d K=%d scale=%s bias=%s" % (F, K, sc is not None, bs is not None))


def test_bins_leaves_row_padding_untouched(edges, graph):
    """ldo > K*F: the K*F entries of each row are written, the padding is not."""
    from mi355_mp import _lib, ops
    ks, op, M = _GEOMS[25]
    F, K, E = 5, 25, edges.shape[1]
    u = _pseudo(E, 2, ks, 7).to(DEV)
    geom = ops._spline_geom(ks, op, M, 2, F)
    x = torch.randn(N, F, device=DEV)
    out = torch.full((N, K * F + 3), 7.0, device=DEV)
    _lib.check(_lib.load().mp_spline_aggregate_bins_f32(
        graph.dst.struct("other"), u.data_ptr(), E, 2, geom[0], geom[1], M, x.data_ptr(), F, F, None, out.data_ptr(),
        out.stride(0), _lib.stream_ptr(x.device)), "mp_spline_aggregate_bins_f32")
    assert torch.equal(out[:, :K * F], ops.spline_bins(graph.dst, u, geom, M, x))
    assert float((out[:, K * F:] - 7.0).abs().max()) == 0.0


# 3 / 4. the layer: forward and gradients -----------------------------------------

def _layer_case(edges, f_in, f_out, D, M, aggr, flow, seed, root=True, bias=True):
    from torch_geometric.nn import SplineConv
    torch.manual_seed(seed)
    ks, op = KS[:D], OPEN[:D]
    conv = SplineConv(f_in, f_out, dim=D, kernel_size=ks, is_open_spline=[bool(o) for o in op], degree=M, aggr=aggr,
                      flow=flow, root_weight=root, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.normal_()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, f_in, generator=g)
    u = _pseudo(edges.shape[1], D, ks, seed)
    return conv, x, u, ks, op


def _ref_layer(conv, x, ei, u, ks, op, M, aggr, flow, absolute=False):
    p = [t.detach().cpu().double().requires_grad_(True) if t is not None else None
         for t in (conv.weight, conv.root, conv.bias)]
    xr = x.detach().double().requires_grad_(True)
    out = R.spline_conv(xr, ei, u, p[0], p[1], p[2], ks, op, M, aggr, flow, absolute=absolute)
    return out, xr, p


@pytest.mark.parametrize("form", ["bins", "gather", None])
@pytest.mark.parametrize("aggr", ["mean", "add"])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_layer_forward(edges, form, aggr, flow):
    f_in, f_out, D, M = 6, 10, 2, 1
    conv, x, u, ks, op = _layer_case(edges, f_in, f_out, D, M, aggr, flow, 3)
    conv = conv.to(DEV)
    out = conv(x.to(DEV), edges.to(DEV), u.to(DEV), form=form)
    ref, _, _ = _ref_layer(conv, x, edges, u, ks, op, M, aggr, flow)
    scale, _, _ = _ref_layer(conv, x, edges, u, ks, op, M, aggr, flow, absolute=True)
    assert out.shape == (N, f_out)
    _assert_bound(out, ref, scale, "layer %s %s %s" % (form, aggr, flow))


def test_layer_takes_1d_inputs_and_picks_the_form(edges):
    """x [N] and pseudo [E] are unsqueezed (ConvexPruning's SplineNet shape:
    dim=1, kernel_size=2); the automatic form is the one ops.spline_form names."""
    from mi355_mp import ops
    from torch_geometric.nn import SplineConv
    torch.manual_seed(0)
    conv = SplineConv(1, 8, dim=1, kernel_size=2).to(DEV)
    g = torch.Generator().manual_seed(0)
    x, u = torch.randn(N, generator=g), torch.rand(edges.shape[1], generator=g)
    out = conv(x.to(DEV), edges.to(DEV), u.to(DEV))
    ref, _, _ = _ref_layer(conv, x, edges, u, [2], [1], 1, "mean", "source_to_target")
    scale, _, _ = _ref_layer(conv, x, edges, u, [2], [1], 1, "mean", "source_to_target", absolute=True)
    _assert_bound(out, ref, scale, "1-D inputs")
    # the automatic form is bitwise the forced form that ops.spline_form names: both outcomes
    for conv, f_in, D in ((SplineConv(100, 3, dim=1, kernel_size=2), 100, 1),
                          (SplineConv(64, 8, dim=3, kernel_size=5), 64, 3)):
        conv = conv.to(DEV)
        xw = torch.randn(N, f_in, device=DEV)
        uw = torch.rand(edges.shape[1], D, device=DEV)
        form = ops.spline_form(2 ** D, f_in, conv.out_channels, conv.weight.shape[0])
        assert form == ("bins" if D == 1 else "gather")
        assert torch.equal(conv(xw, edges.to(DEV), uw), conv(xw, edges.to(DEV), uw, form=form))


@pytest.mark.parametrize("form", ["bins", "gather"])
@pytest.mark.parametrize("shape", [(6, 10, 2, 1, "mean"), (3, 70, 1, 2, "add"), (70, 2, 3, 1, "mean"),
                                   (5, 4, 2, 3, "add")])
def test_layer_gradients(edges, form, shape):
    """d x, d weight, d root, d bias against the restatement's float64 autograd;
    the shapes take both grad_x routes (gather over the transposed CSR when
    S * Fin < Fout, else bins) and both grad_W routes."""
    f_in, f_out, D, M, aggr = shape
    conv, x, u, ks, op = _layer_case(edges, f_in, f_out, D, M, aggr, "source_to_target", 11)
    conv = conv.to(DEV)
    g = torch.Generator().manual_seed(5)
    gout = torch.randn(N, f_out, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, edges.to(DEV), u.to(DEV), form=form)
    (out * gout.to(DEV)).sum().backward()
    ref, xr, p = _ref_layer(conv, x, edges, u, ks, op, M, aggr, "source_to_target")
    (ref * gout.double()).sum().backward()
    for name, got, want in (("x", xd.grad, xr.grad), ("weight", conv.weight.grad, p[0].grad),
                            ("root", conv.root.grad, p[1].grad), ("bias", conv.bias.grad, p[2].grad)):
        _assert_bound(got, want, _abs_grad_scale(name, conv, x, edges, u, ks, op, M, aggr, gout),
                      "grad %s %s %s" % (name, form, shape))


def _abs_grad_scale(name, conv, x, ei, u, ks, op, M, aggr, gout):
    """sum |terms| of one gradient: the float64 autograd of the restatement on
    absolute inputs with |grad_out| (all terms >= 0, so the gradient of the
    absolute computation is the sum of the terms' magnitudes)."""
    return R.abs_grad_scale(conv.weight, conv.root, conv.bias, x, ei, u, ks, op, M, aggr, gout)[name]


# 5. bit-exact ---------------------------------------------------------------

def _exact_inputs(edges, f_in):
    g = torch.Generator().manual_seed(9)
    E = edges.shape[1]
    u = torch.randint(0, 9, (E, 2), generator=g).float() / 8           # multiples of 1/8, 0 and 1 included
    x = torch.randint(-4, 5, (N, f_in), generator=g).float()
    return u, x


def test_bins_bit_exact_on_dyadic_inputs(edges, graph):
    """Degree 1, pseudo on multiples of 1/8, ks - degree*open = 4: every basis
    value, product and partial sum is exact in fp32, so the kernel equals the
    float64 restatement bit for bit."""
    from mi355_mp import ops
    ks, op, M, F = [5, 5], [1, 1], 1, 7
    u, x = _exact_inputs(edges, F)
    geom = ops._spline_geom(ks, op, M, 2, F)
    A = ops.spline_bins(graph.dst, u.to(DEV), geom, M, x.to(DEV))
    rb, rwi = R.basis(u, ks, op, M)
    ref = R.bins(edges[1], edges[0], N, rb, rwi, 25, x)
    assert torch.equal(A.cpu().double(), ref)


def test_bins_bit_exact_at_the_lds_limit(edges, graph):
    """The same at K = 256 ([16, 16], the one-wave block with 65536 bytes of
    dynamic LDS): open splines, so v = u * 15 is a multiple of 1/8 below 16,
    exact in fp32, as are the degree-1 basis values (multiples of 1/8), their
    products (of 1/64) with |x| <= 4 and every partial sum of a row's 700
    slots; the bins reach index 255.  A bin-addressing error shows without a
    tolerance."""
    from mi355_mp import ops
    ks, op, M, F = [16, 16], [1, 1], 1, 7
    u, x = _exact_inputs(edges, F)
    geom = ops._spline_geom(ks, op, M, 2, F)
    assert geom[2] == 256
    A = ops.spline_bins(graph.dst, u.to(DEV), geom, M, x.to(DEV))
    rb, rwi = R.basis(u, ks, op, M)
    assert int(rwi.max()) == 255 and int(rwi.min()) == 0
    ref = R.bins(edges[1], edges[0], N, rb, rwi, 256, x)
    assert torch.equal(A.cpu().double(), ref)


def test_layer_forward_bit_exact_with_integer_weights(edges):
    from torch_geometric.nn import SplineConv
    f_in, f_out = 7, 6
    u, x = _exact_inputs(edges, f_in)
    conv = SplineConv(f_in, f_out, dim=2, kernel_size=5, aggr="add")
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-4, 5, conv.weight.shape, generator=g).float())
        conv.root.copy_(torch.randint(-4, 5, conv.root.shape, generator=g).float())
        conv.bias.copy_(torch.randint(-4, 5, conv.bias.shape, generator=g).float())
    conv = conv.to(DEV)
    ref = R.spline_conv(x, edges, u, conv.weight.detach().cpu(), conv.root.detach().cpu(), conv.bias.detach().cpu(),
                        [5, 5], [1, 1], 1, "add")
    for form in ("bins", "gather"):
        out = conv(x.to(DEV), edges.to(DEV), u.to(DEV), form=form)
        assert torch.equal(out.detach().cpu().double(), ref), form


# 6. determinism ---------------------------------------------------------------

def test_two_runs_bitwise_equal_and_forms_agree(edges):
    conv, x, u, ks, op = _layer_case(edges, 33, 20, 2, 2, "mean", "source_to_target", 21)
    conv = conv.to(DEV)
    ei, ud = edges.to(DEV), u.to(DEV)
    outs, grads = {}, {}
    for form in ("bins", "gather"):
        runs = []
        for _ in range(2):
            conv.zero_grad()
            xd = x.to(DEV).requires_grad_(True)
            o = conv(xd, ei, ud, form=form)
            o.square().sum().backward()
            runs.append((o.detach().clone(), xd.grad.clone(), conv.weight.grad.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b), form
        outs[form] = runs[0][0]
    ref, _, _ = _ref_layer(conv, x, edges, u, ks, op, 2, "mean", "source_to_target")
    scale, _, _ = _ref_layer(conv, x, edges, u, ks, op, 2, "mean", "source_to_target", absolute=True)
    for form in ("bins", "gather"):
        _assert_bound(outs[form], ref, scale, "forms: %s against float64" % form)
    _assert_bound(outs["bins"], outs["gather"].cpu().double(), scale, "forms: bins against gather")


# 7. refusals ------------------------------------------------------------------

def test_documented_refusals(edges):
    import torch_geometric
    from torch_geometric.nn import SplineConv
    conv = SplineConv(2, 3, dim=2, kernel_size=5).to(DEV)
    x = torch.randn(N, 2, device=DEV)
    ei = edges.to(DEV)
    u = torch.rand(edges.shape[1], 2, device=DEV)
    bad_u = u.clone()
    bad_u[3, 1] = 1.5
    with torch_geometric.debug():
        conv(x, ei, u)
        with pytest.raises(RuntimeError, match=r"\[0, 1\]"):
            conv(x, ei, bad_u)
        with pytest.raises(RuntimeError, match="node features"):
            conv(torch.randn(N, 3, device=DEV), ei, u)
        with pytest.raises(RuntimeError, match="dimensionality"):
            conv(x, ei, u[:, :1])
    conv(x, ei, bad_u)                                                 # outside debug mode: wraps, no fault
    bad_ei = ei.clone()
    bad_ei[0, 10] = N
    with pytest.raises(IndexError):
        conv(x, bad_ei, u)
    with pytest.raises(NotImplementedError, match="max"):
        SplineConv(2, 3, dim=2, kernel_size=5, aggr="max").to(DEV)(x, ei, u)
    with pytest.raises(NotImplementedError, match="pseudo"):
        conv(x, ei, u.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="K <= 256"):
        SplineConv(2, 3, dim=3, kernel_size=7).to(DEV)(x, ei, torch.rand(edges.shape[1], 3, device=DEV))


# 8. the example ---------------------------------------------------------------

def test_example_mnist_spline():
    spec = importlib.util.spec_from_file_location("example_mnist_spline",
                                                  os.path.join(ROOT, "examples", "mnist_spline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    losses = mod.main(["--epochs", "3", "--graphs", "256"])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
