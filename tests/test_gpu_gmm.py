"""GMMConv on the GPU: the three kernels, the layer's forward and backward in
both forms, the generic path, underflowed weights, bit-exact and determinism
cases, the absence of the gathered [E, K, Cout] operand and the example, all
against the float64 restatement tests/_gmm_ref.py.

Every float comparison uses the project's bound |err| <= 1e-5 * sum |terms|
(sum |terms| = the same computation on absolute values).  The graph is the
257-node one of tests/test_gpu_nnconv.py: ~3000 edges with duplicates, one row
with 700 in-edges, rows 200.. without in-edges and isolated nodes.  Inputs of
every bound check: pseudo and mu uniform in [0, 1), |sigma| uniform in [0.5,
1.5) with a random sign, so |q| <= 2 D and an fp32 evaluation of a weight stays
within 1e-6 relative of float64 -- a tenth of the bound.
"""
import importlib.util
import math
import os

import pytest
import torch

from tests import _gmm_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 257


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
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg[5]) >= 700 and int(deg[200:].sum()) == 0
    return ei


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    return Graph(edges.to(DEV), N, N)


def _table(K, D, g):
    """mu uniform in [0, 1), |sigma| uniform in [0.5, 1.5) with a random sign."""
    mu = torch.rand(K, D, generator=g)
    sigma = (torch.rand(K, D, generator=g) + 0.5) * (torch.randint(0, 2, (K, D), generator=g).float() * 2 - 1)
    return mu, sigma


def _nan(*shape):
    """An output to hand to a kernel: an entry it leaves unwritten fails every comparison."""
    return torch.full(shape, float("nan"), device=DEV)


# 1. the three kernels ---------------------------------------------------------

def check_aggregates(edges, csr, n, C, K, D, first_empty_row):
    """bins (Cin = C) and gather (F = C), pseudo with ldp = D + 3, with and
    without row_scale and bias, into NaN-filled outputs; a second call bitwise equal."""
    from mi355_mp import ops
    assert ops.gmm_ok(K, D, C, C)
    E = edges.shape[1]
    dst, src = edges[1], edges[0]
    g = torch.Generator().manual_seed(C * 10000 + K * 10 + D)
    pw = torch.rand(E, D + 3, generator=g)
    p = pw[:, :D]
    mu, sigma = _table(K, D, g)
    x = torch.randn(n, C, generator=g)
    y = torch.randn(n, K * C, generator=g)
    bias = torch.randn(C, generator=g)
    scale = torch.rand(n, generator=g) + 0.5
    pd = pw.to(DEV)[:, :D]
    assert pd.stride(0) == D + 3
    mud, sgd = mu.to(DEV), sigma.to(DEV)
    z_ref, z_abs = R.bins(dst, src, n, p, mu, sigma, x), R.bins(dst, src, n, p, mu, sigma, x, absolute=True)
    o_ref = R.gather(dst, src, n, p, mu, sigma, y, C)
    o_abs = R.gather(dst, src, n, p, mu, sigma, y, C, absolute=True)
    tag = "C=%d K=%d D=%d" % (C, K, D)
    for sc in (None, scale):
        scd = None if sc is None else sc.to(DEV)
        mul = 1.0 if sc is None else sc.double().view(-1, 1)
        Z = ops.gmm_bins(csr, pd, mud, sgd, x.to(DEV), scd, out=_nan(n, K * C))
        assert Z.shape == (n, K * C)
        R.assert_bound(Z, z_ref * mul, z_abs * mul, "bins %s scale=%s" % (tag, sc is not None))
        assert float(Z[first_empty_row:].abs().max()) == 0.0           # rows without slots are zero
        assert torch.equal(ops.gmm_bins(csr, pd, mud, sgd, x.to(DEV), scd), Z)
        for bs in (None, bias):
            bd = None if bs is None else bs.to(DEV)
            add, add_abs = (0.0, 0.0) if bs is None else (bs.double(), bs.double().abs())
            o = ops.gmm_gather(csr, pd, mud, sgd, y.to(DEV), C, scd, bd, out=_nan(n, C))
            R.assert_bound(o, o_ref * mul + add, o_abs * mul + add_abs,
                           "gather %s scale=%s bias=%s" % (tag, sc is not None, bs is not None))
            if bs is None:
                assert float(o[first_empty_row:].abs().max()) == 0.0
            assert torch.equal(ops.gmm_gather(csr, pd, mud, sgd, y.to(DEV), C, scd, bd), o)


def check_param_grad(edges, n, C, K, D, sizes=None):
    """param_grad (Cin = C) on the first n_edges edges for each size, dpseudo
    requested and not, into NaN-filled outputs; two runs bitwise equal."""
    from mi355_mp import ops
    g = torch.Generator().manual_seed(C * 10000 + K * 10 + D + 500000)
    E = edges.shape[1]
    pw = torch.rand(E, D + 3, generator=g)
    mu, sigma = _table(K, D, g)
    x = torch.randn(n, C, generator=g)
    dz = torch.randn(n, K * C, generator=g)
    chunk = ops.gmm_grad_chunk(E, K, D)
    assert chunk >= 1024 and (sizes is not None or chunk + 1 <= E)
    mud, sgd, xd, dzd = mu.to(DEV), sigma.to(DEV), x.to(DEV), dz.to(DEV)
    for ne in (sizes or (1, chunk, chunk + 1, E)):
        assert ops.gmm_grad_chunk(ne, K, D) == chunk
        dst, src = edges[1, :ne], edges[0, :ne]
        p = pw[:ne, :D]
        pd = pw.to(DEV)[:ne, :D]
        want = R.param_grad(dst, src, p, mu, sigma, dz, x)
        scale = R.param_grad(dst, src, p, mu, sigma, dz, x, absolute=True)
        tag = "C=%d K=%d D=%d n_edges=%d" % (C, K, D, ne)
        for want_p in (True, False):
            outs = []
            for _ in range(2):
                dpb = _nan(ne, D + 2) if want_p else None              # lddp = D + 2
                dmu, dsigma, dp = ops.gmm_param_grad(dst.to(DEV), src.to(DEV), pd, mud, sgd, dzd, xd,
                                                     dmu=_nan(K, D), dsigma=_nan(K, D),
                                                     dpseudo=None if dpb is None else dpb[:, :D])
                outs.append((dmu, dsigma, dp, dpb))
            dmu, dsigma, dp, dpb = outs[0]
            R.assert_bound(dmu, want[0], scale[0], "dmu %s dpseudo=%s" % (tag, want_p))
            R.assert_bound(dsigma, want[1], scale[1], "dsigma %s dpseudo=%s" % (tag, want_p))
            assert torch.equal(dmu, outs[1][0]) and torch.equal(dsigma, outs[1][1])
            if want_p:
                R.assert_bound(dp, want[2], scale[2], "dpseudo %s" % tag)
                assert torch.equal(dp, outs[1][2])
                assert bool(torch.isnan(dpb[:, D:]).all())              # the padding is untouched
            else:
                assert dp is None
        # dpseudo requested or not: the same dmu / dsigma bit for bit
        a = ops.gmm_param_grad(dst.to(DEV), src.to(DEV), pd, mud, sgd, dzd, xd, want_pseudo=True)
        assert torch.equal(a[0], dmu) and torch.equal(a[1], dsigma) and a[2].shape == (ne, D)


@pytest.mark.parametrize("K", [1, 3, 25])
@pytest.mark.parametrize("C", [1, 5, 33, 64, 70])
def test_kernels_against_float64(edges, graph, C, K):
    """bins (Cin = C: the flat mapping below 32 columns, the column mapping from
    32 on, two column tiles at 70, two k tiles at K = 25), gather (F = C: the
    grouped and the one-row-per-wave mappings) and param_grad (Cin = C), for D =
    1, 2, 3."""
    for D in (1, 2, 3):
        check_aggregates(edges, graph.dst, N, C, K, D, 200)
        check_param_grad(edges, N, C, K, D)


def test_kernels_at_the_table_limit(edges, graph):
    """K * D = 1024: the whole 8 KiB table, k strided over the lanes in param_grad."""
    check_aggregates(edges, graph.dst, N, 5, 128, 8, 200)
    check_param_grad(edges, N, 5, 128, 8)


@pytest.mark.parametrize("C", [5, 33])
def test_padded_outputs_come_back_untouched(edges, graph, C):
    """ldo above the row: the row's entries are written, the padding is not
    (both bins mappings, and gather)."""
    from mi355_mp import ops
    K, D, E = 25, 2, edges.shape[1]
    Q = K * C
    g = torch.Generator().manual_seed(C)
    mu, sigma = (t.to(DEV) for t in _table(K, D, g))
    p = torch.rand(E, D, device=DEV)
    x = torch.randn(N, C, device=DEV)
    y = torch.randn(N, Q, device=DEV)
    out = torch.full((N, Q + 3), 7.0, device=DEV)
    ops.gmm_bins(graph.dst, p, mu, sigma, x, out=out)
    assert torch.equal(out[:, :Q], ops.gmm_bins(graph.dst, p, mu, sigma, x))
    assert float((out[:, Q:] - 7.0).abs().max()) == 0.0
    out = torch.full((N, C + 3), 7.0, device=DEV)
    ops.gmm_gather(graph.dst, p, mu, sigma, y, C, out=out)
    assert torch.equal(out[:, :C], ops.gmm_gather(graph.dst, p, mu, sigma, y, C))
    assert float((out[:, C:] - 7.0).abs().max()) == 0.0


# 2. the layer ------------------------------------------------------------------

def _layer(c_in, c_out, K, D, aggr, flow, seed, cls=None, **kw):
    """A layer with mu, sigma drawn like the kernel tests' and a non-zero bias."""
    from torch_geometric.nn import GMMConv
    torch.manual_seed(seed)
    conv = (cls or GMMConv)(c_in, c_out, D, K, aggr=aggr, flow=flow, **kw)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        conv.mu.copy_(torch.rand(conv.mu.shape, generator=g))
        sign = torch.randint(0, 2, conv.sigma.shape, generator=g).float() * 2 - 1
        conv.sigma.copy_((torch.rand(conv.sigma.shape, generator=g) + 0.5) * sign)
        if conv.bias is not None:
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g))
    return conv


def _inputs(edges, c_in, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, c_in, generator=g), torch.rand(edges.shape[1], D, generator=g)


def _reference(conv, x, ei, p, absolute=False, gout=None, p_grad=False):
    """The restatement on float64 copies of the layer's parameters; with gout its
    autograd too.  absolute: sum |terms| -- x, g, root, bias and gout by their
    magnitude; the sums of |terms| of d mu, d sigma, d pseudo come from the
    closed forms (R.param_grad on |dZ|, |x|).  Returns (out, {name: grad})."""
    cvt = (lambda t: t.detach().cpu().double().abs()) if absolute else (lambda t: t.detach().cpu().double())
    leaves = {n: t.detach().cpu().double() for n, t in conv.named_parameters()}
    for n in ("g", "root", "bias"):
        if n in leaves:
            leaves[n] = cvt(leaves[n])
    leaves["x"] = cvt(x.view(-1, 1) if x.dim() == 1 else x)
    p = p.detach().cpu().double()
    leaves["pseudo"] = p.view(-1, 1) if p.dim() == 1 else p
    leaves = {n: t.clone().requires_grad_(True) for n, t in leaves.items()}
    K = conv.kernel_size
    out = R.gmm_conv(leaves["x"], ei, leaves["pseudo"], leaves["g"], leaves["mu"], leaves["sigma"], K,
                     leaves.get("root"), leaves.get("bias"), conv.aggr, conv.flow)
    grads = None
    if gout is not None:
        go = gout.double().abs() if absolute else gout.double()
        (out * go).sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        if absolute and not conv.separate_gaussians:
            i, j = (1, 0) if conv.flow == "source_to_target" else (0, 1)
            dst, src = ei[i], ei[j]
            if conv.aggr == "mean":
                go = go / torch.bincount(dst, minlength=go.shape[0]).clamp(min=1).double().view(-1, 1)
            c_in, c_out = conv.in_channels, conv.out_channels
            dz = go @ R.mix_matrix(leaves["g"].detach(), K, c_in, c_out).t()
            grads["mu"], grads["sigma"], grads["pseudo"] = R.param_grad(
                dst, src, leaves["pseudo"].detach(), leaves["mu"].detach(), leaves["sigma"].detach(), dz,
                leaves["x"].detach(), absolute=True)
        if not p_grad:
            del grads["pseudo"]
    return out.detach(), grads


def _forward_check(conv, x, ei, p, form, what):
    conv = conv.to(DEV)
    out = conv(x.to(DEV), ei.to(DEV), p.to(DEV), form=form)
    assert out.shape == (x.shape[0], conv.out_channels)
    R.assert_bound(out, _reference(conv, x, ei, p)[0], _reference(conv, x, ei, p, absolute=True)[0], what)
    return out


def check_layer(conv, x, ei, p, form, what, p_grad=False, seed=5):
    """Forward and every gradient (x, every parameter; p_grad: pseudo) of one
    layer call on any graph against the restatement.  Returns (out, {name:
    grad}) of the device run."""
    conv = conv.to(DEV)
    n = x.shape[0]
    gout = torch.randn(n, conv.out_channels, generator=torch.Generator().manual_seed(seed))
    xd = x.to(DEV).requires_grad_(True)
    pd = p.to(DEV).requires_grad_(p_grad)
    out = conv(xd, ei.to(DEV), pd, form=form)
    assert tuple(out.shape) == (n, conv.out_channels), what
    (out * gout.to(DEV)).sum().backward()
    ref, want = _reference(conv, x, ei, p, gout=gout, p_grad=p_grad)
    ref_abs, scale = _reference(conv, x, ei, p, absolute=True, gout=gout, p_grad=p_grad)
    R.assert_bound(out, ref, ref_abs, "forward " + what)
    got = {name: t.grad for name, t in conv.named_parameters()}
    got["x"] = xd.grad
    if p_grad:
        got["pseudo"] = pd.grad
    else:
        assert pd.grad is None
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(got):
        assert got[name] is not None, name
        assert tuple(got[name].shape) == tuple(want[name].shape), name
        R.assert_bound(got[name], want[name], scale[name], "grad %s %s" % (name, what))
    return out, got


@pytest.mark.parametrize("form", ["bins", "gather", None])
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_layer_forward(edges, form, aggr, flow):
    conv = _layer(6, 10, 25, 2, aggr, flow, 3)
    x, p = _inputs(edges, 6, 2, 3)
    _forward_check(conv, x, edges, p, form, "layer %s %s %s" % (form, aggr, flow))


@pytest.mark.parametrize("form", ["bins", "gather"])
@pytest.mark.parametrize("root,bias", [(False, False), (True, False), (False, True)])
def test_layer_forward_without_root_or_bias(edges, form, root, bias):
    conv = _layer(33, 4, 7, 3, "mean", "source_to_target", 5, root_weight=root, bias=bias)
    x, p = _inputs(edges, 33, 3, 5)
    _forward_check(conv, x, edges, p, form, "layer %s root=%s bias=%s" % (form, root, bias))


def test_layer_1d_inputs_and_the_chosen_form(edges):
    """x [N] and pseudo [E] are taken as one column; the automatic form is
    bitwise the one gmm_form names."""
    from mi355_mp import ops
    conv = _layer(1, 32, 25, 1, "mean", "source_to_target", 7)
    g = torch.Generator().manual_seed(7)
    x, p = torch.randn(N, generator=g), torch.rand(edges.shape[1], generator=g)
    _forward_check(conv, x, edges, p, None, "1-D inputs")
    E = edges.shape[1]
    for c_in, c_out, K, want in ((1, 32, 25, "bins"), (70, 2, 4, "gather")):
        assert ops.gmm_form(K, 2, c_in, c_out, E, N) == want
        conv = _layer(c_in, c_out, K, 2, "add", "source_to_target", 8).to(DEV)
        xd, pd = torch.randn(N, c_in, device=DEV), torch.rand(E, 2, device=DEV)
        assert torch.equal(conv(xd, edges.to(DEV), pd), conv(xd, edges.to(DEV), pd, form=want))


@pytest.mark.parametrize("form", ["bins", "gather"])
@pytest.mark.parametrize("p_grad", [False, True])
@pytest.mark.parametrize("shape", [(6, 10, 5, 2, "mean"), (70, 2, 4, 3, "add"), (1, 32, 25, 2, "mean"),
                                   (33, 33, 3, 1, "add")])
def test_layer_gradients(edges, form, shape, p_grad):
    """d x, d g, d mu, d sigma, d root, d bias, and d pseudo when it requires
    grad, against the restatement's float64 autograd."""
    c_in, c_out, K, D, aggr = shape
    conv = _layer(c_in, c_out, K, D, aggr, "source_to_target", 11)
    x, p = _inputs(edges, c_in, D, 11)
    _, got = check_layer(conv, x, edges, p, form, "%s %s" % (form, shape), p_grad=p_grad)
    assert sorted(got) == sorted(["bias", "g", "mu", "root", "sigma", "x"] + ["pseudo"] * p_grad)


@pytest.mark.parametrize("case", ["separate", "max", "subclass"])
def test_generic_path_matches_the_restatement(edges, case):
    """separate_gaussians=True, aggr='max' and a subclass overriding message run
    upstream's message on the generic path: same result, no fused call."""
    from mi355_mp import ops
    from torch_geometric.nn import GMMConv

    class Same(GMMConv):
        def message(self, x_j, pseudo):
            return GMMConv.message(self, x_j, pseudo)

    c_in, c_out, K, D = 5, 3, 4, 2
    kw = dict(separate_gaussians=True) if case == "separate" else {}
    conv = _layer(c_in, c_out, K, D, "max" if case == "max" else "mean", "source_to_target", 13,
                  cls=Same if case == "subclass" else None, **kw)
    assert not conv.fused()
    x, p = _inputs(edges, c_in, D, 13)
    conv = conv.to(DEV)
    calls = []
    real = ops.gmm_propagate
    ops.gmm_propagate = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        out = conv(x.to(DEV), edges.to(DEV), p.to(DEV))
        with pytest.raises(ValueError, match="fused path"):
            conv(x.to(DEV), edges.to(DEV), p.to(DEV), form="bins")
    finally:
        ops.gmm_propagate = real
    assert calls == []
    ref = _reference(conv, x, edges, p)[0]
    if case == "max":
        conv.aggr = "add"                                              # max: one message of the row's sum
    scale = _reference(conv, x, edges, p, absolute=True)[0]
    R.assert_bound(out, ref, scale, "generic path: %s" % case)
    # the fused layer does call it
    fused = _layer(c_in, c_out, K, D, "mean", "source_to_target", 13).to(DEV)
    ops.gmm_propagate = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        fused(x.to(DEV), edges.to(DEV), p.to(DEV))
    finally:
        ops.gmm_propagate = real
    assert calls == [1]


@pytest.mark.parametrize("form", ["bins", "gather"])
def test_underflowed_weights_give_finite_gradients(edges, form):
    """A sigma of 1e-4 on kernel 1, whose mu lies a unit away from every pseudo:
    all its weights underflow to 0.  Forward and every gradient stay finite and
    that kernel's d mu / d sigma rows are exactly 0 (upstream's autograd: NaN)."""
    c_in, c_out, K, D = 6, 10, 5, 2
    conv = _layer(c_in, c_out, K, D, "mean", "source_to_target", 19)
    with torch.no_grad():
        conv.sigma[1] = 1e-4
        conv.mu[1] = 2.0
    x, p = _inputs(edges, c_in, D, 19)
    w = torch.exp((-0.5 * (p.view(-1, 1, D) - conv.mu.detach().view(1, K, D)).pow(2)
                   / (1e-15 + conv.sigma.detach().view(1, K, D).pow(2))).sum(-1))
    assert bool((w[:, 1] == 0).all()) and bool((w[:, 0] > 0).all())
    conv = conv.to(DEV)
    xd, pd = x.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    out = conv(xd, edges.to(DEV), pd, form=form)
    gout = torch.randn(N, c_out, generator=torch.Generator().manual_seed(5))
    (out * gout.to(DEV)).sum().backward()
    R.assert_bound(out, _reference(conv, x, edges, p)[0], _reference(conv, x, edges, p, absolute=True)[0],
                   "forward with an underflowed kernel, %s" % form)
    for name, t in list(conv.named_parameters()) + [("x", xd), ("pseudo", pd)]:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()), name
    assert float(conv.mu.grad[1].abs().max()) == 0.0 and float(conv.sigma.grad[1].abs().max()) == 0.0
    assert float(conv.mu.grad[0].abs().max()) > 0.0 and float(conv.sigma.grad[0].abs().max()) > 0.0


# 3. bit-exact, determinism -------------------------------------------------------

def test_forward_bit_exact_on_small_integers(edges):
    """Every pseudo row and every mu row equal to one point: all w = exp(0) = 1.
    Integer x, g, root, bias in [-4, 4]: each product and every partial sum of
    the 700-slot row (at most 700 * 4 * 7 * 16 < 2^24) is exact in fp32 in any
    order, so both forms equal the restatement and each other bit for bit."""
    from torch_geometric.nn import GMMConv
    c_in, c_out, K, D = 7, 6, 4, 2
    g = torch.Generator().manual_seed(9)
    E = edges.shape[1]
    p0 = torch.tensor([0.375, 0.8125])
    p = p0.repeat(E, 1)
    x = torch.randint(-4, 5, (N, c_in), generator=g).float()
    conv = GMMConv(c_in, c_out, D, K, aggr="add")
    with torch.no_grad():
        for name, t in conv.named_parameters():
            if name in ("g", "root", "bias"):
                t.copy_(torch.randint(-4, 5, t.shape, generator=g).float())
        conv.mu.copy_(p0.repeat(K, 1))
        conv.sigma.copy_(torch.rand(K, D, generator=g) + 0.5)
    ref = _reference(conv, x, edges, p)[0]
    conv = conv.to(DEV)
    outs = [conv(x.to(DEV), edges.to(DEV), p.to(DEV), form=form) for form in ("bins", "gather")]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].detach().cpu().double(), ref)


def test_two_runs_bitwise_equal_and_forms_agree(edges):
    conv = _layer(33, 20, 9, 2, "mean", "source_to_target", 21).to(DEV)
    x, p = _inputs(edges, 33, 2, 21)
    ei = edges.to(DEV)
    outs = {}
    for form in ("bins", "gather"):
        runs = []
        for _ in range(2):
            conv.zero_grad()
            xd = x.to(DEV).requires_grad_(True)
            pd = p.to(DEV).requires_grad_(True)
            o = conv(xd, ei, pd, form=form)
            o.square().sum().backward()
            runs.append([o.detach().clone(), xd.grad.clone(), pd.grad.clone()]
                        + [t.grad.clone() for t in conv.parameters()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), form
        outs[form] = runs[0][0]
    scale = _reference(conv, x, edges, p, absolute=True)[0]
    R.assert_bound(outs["bins"], outs["gather"].cpu().double(), scale, "forms: bins against gather")


def test_frozen_gaussians_skip_the_param_grad_launch(edges):
    """With mu and sigma frozen and pseudo needing no gradient the backward does
    not launch the parameter-gradient kernels; any one of the three brings it back."""
    from mi355_mp import ops
    conv = _layer(6, 10, 5, 2, "mean", "source_to_target", 17).to(DEV)
    x, p = _inputs(edges, 6, 2, 17)
    calls = []
    real = ops.gmm_param_grad
    ops.gmm_param_grad = lambda *a, **k: calls.append(bool(k.get("want_pseudo"))) or real(*a, **k)
    try:
        conv.mu.requires_grad_(False)
        conv.sigma.requires_grad_(False)
        xd = x.to(DEV).requires_grad_(True)
        conv(xd, edges.to(DEV), p.to(DEV)).square().sum().backward()
        assert calls == [] and xd.grad is not None and conv.g.grad is not None and conv.mu.grad is None
        pd = p.to(DEV).requires_grad_(True)
        conv(x.to(DEV), edges.to(DEV), pd).square().sum().backward()
        assert calls == [True] and pd.grad is not None and conv.mu.grad is None and conv.sigma.grad is None
        conv.sigma.requires_grad_(True)
        conv(x.to(DEV), edges.to(DEV), p.to(DEV)).square().sum().backward()
        assert calls == [True, False] and conv.sigma.grad is not None and conv.mu.grad is None
    finally:
        ops.gmm_param_grad = real


# 4. no gathered operand ------------------------------------------------------------

@pytest.mark.parametrize("form", ["bins", "gather"])
def test_no_gathered_operand(edges, form):
    """E = 3000, K = 25, Cin = Cout = 64: the gathered [E, K, Cout] fp32 operand of
    the upstream recipe alone is 19 MB, far above everything the fused path
    holds (Z and dZ: 1.6 MB each); forward + backward must peak below it."""
    c_in = c_out = 64
    K = 25
    conv = _layer(c_in, c_out, K, 2, "mean", "source_to_target", 31).to(DEV)
    x, p = _inputs(edges, c_in, 2, 31)
    xd, ei, pd = x.to(DEV).requires_grad_(True), edges.to(DEV), p.to(DEV)
    conv(xd, ei, pd, form=form).sum().backward()                      # builds and caches both CSRs
    conv.zero_grad()
    xd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    conv(xd, ei, pd, form=form).square().sum().backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    gathered = edges.shape[1] * K * c_out * 4
    print("%s: peak growth %d bytes, the gathered operand %d bytes" % (form, growth, gathered))
    assert growth < gathered


# 5. the example ------------------------------------------------------------------

def test_example_mnist_gmm_conv():
    spec = importlib.util.spec_from_file_location("example_mnist_gmm_conv",
                                                  os.path.join(ROOT, "examples", "mnist_gmm_conv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    losses = mod.main(["--epochs", "2", "--graphs", "256"])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
