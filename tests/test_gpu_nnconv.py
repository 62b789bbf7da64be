"""NNConv on the GPU: the three kernels, the layer's forward and backward in
both forms, the generic path, bit-exact and determinism cases, the absence of
the per-edge weight array and the example, all against the float64
restatement tests/_nnconv_ref.py.

Every float comparison uses the project's bound |err| <= 1e-5 * sum |terms|
(sum |terms| = the same computation on absolute values).  The graph is the
257-node one of tests/test_gpu_spline.py: ~3000 edges with duplicates, one row
with 700 in-edges (its serial fp32 sum of 700 * (H + 1) terms: the largest
ratio any kernel case here reaches is 3e-7 * sum |terms|), rows 200.. without
in-edges and isolated nodes.
"""
import importlib.util
import math
import os

import pytest
import torch

from tests import _nnconv_ref as R

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


# 1. the three kernels ---------------------------------------------------------

def _nan(*shape):
    """An output to hand to a kernel: an entry it leaves unwritten fails every comparison."""
    return torch.full(shape, float("nan"), device=DEV)


def check_aggregates(edges, csr, n, C, H, first_empty_row):
    """bins (Cin = C) and gather (F = C) on the graph `edges` ([2, E] on the CPU;
    csr: its destination CSR on the device, n nodes, rows first_empty_row.. without
    in-edges), h with ldh = H + 3, with and without row_scale and bias, into
    NaN-filled outputs."""
    from mi355_mp import ops
    assert ops.nnconv_ok(H, C, C)
    E = edges.shape[1]
    dst, src = edges[1], edges[0]
    g = torch.Generator().manual_seed(C * 1000 + H)
    hw = torch.randn(E, H + 3, generator=g)
    h = hw[:, :H]
    x = torch.randn(n, C, generator=g)
    y = torch.randn(n, (H + 1) * C, generator=g)
    bias = torch.randn(C, generator=g)
    scale = torch.rand(n, generator=g) + 0.5
    hd = hw.to(DEV)[:, :H]
    assert hd.stride(0) == H + 3
    z_ref, z_abs = R.bins(dst, src, n, h, x), R.bins(dst, src, n, h.abs(), x.abs())
    o_ref, o_abs = R.gather(dst, src, n, h, y, C), R.gather(dst, src, n, h.abs(), y.abs(), C)
    for sc in (None, scale):
        scd = None if sc is None else sc.to(DEV)
        mul = 1.0 if sc is None else sc.double().view(-1, 1)
        Z = ops.nnconv_bins(csr, hd, x.to(DEV), scd, out=_nan(n, (H + 1) * C))
        assert Z.shape == (n, (H + 1) * C)
        R.assert_bound(Z, z_ref * mul, z_abs * mul, "bins C=%d H=%d scale=%s" % (C, H, sc is not None))
        assert float(Z[first_empty_row:].abs().max()) == 0.0           # rows without slots are zero
        assert torch.equal(ops.nnconv_bins(csr, hd, x.to(DEV), scd), Z)
        for bs in (None, bias):
            bd = None if bs is None else bs.to(DEV)
            add, add_abs = (0.0, 0.0) if bs is None else (bs.double(), bs.double().abs())
            o = ops.nnconv_gather(csr, hd, y.to(DEV), C, scd, bd, out=_nan(n, C))
            R.assert_bound(o, o_ref * mul + add, o_abs * mul + add_abs,
                           "gather F=%d H=%d scale=%s bias=%s" % (C, H, sc is not None, bs is not None))
            if bs is None:
                assert float(o[first_empty_row:].abs().max()) == 0.0
            assert torch.equal(ops.nnconv_gather(csr, hd, y.to(DEV), C, scd, bd), o)


def check_edge_grad(edges, n, C, H):
    """edge_grad (Cin = C) on the graph `edges`, into a NaN-filled output."""
    from mi355_mp import ops
    E = edges.shape[1]
    dst, src = edges[1], edges[0]
    g = torch.Generator().manual_seed(C * 1000 + H + 500000)
    x = torch.randn(n, C, generator=g)
    dz = torch.randn(n, (H + 1) * C, generator=g)
    dh = ops.nnconv_edge_grad(edges[1].to(DEV), edges[0].to(DEV), dz.to(DEV), x.to(DEV), H, out=_nan(E, H))
    assert dh.shape == (E, H)
    R.assert_bound(dh, R.edge_grad(dst, src, dz, x, H), R.edge_grad(dst, src, dz.abs(), x.abs(), H),
                   "edge_grad C=%d H=%d" % (C, H))
    assert torch.equal(ops.nnconv_edge_grad(edges[1].to(DEV), edges[0].to(DEV), dz.to(DEV), x.to(DEV), H), dh)


@pytest.mark.parametrize("H", [1, 25, 128])
@pytest.mark.parametrize("C", [1, 5, 33, 64, 70])
def test_kernels_against_float64(edges, graph, C, H):
    """bins (Cin = C: the flat mapping below 32 columns, the column mapping from
    32 on, two column tiles at 70), gather (F = C) and edge_grad (Cin = C), h
    with ldh = H + 3, with and without row_scale and bias."""
    check_aggregates(edges, graph.dst, N, C, H, 200)
    check_edge_grad(edges, N, C, H)


@pytest.mark.parametrize("C", [5, 33])
def test_padded_outputs_come_back_untouched(edges, graph, C):
    """ldo above the row: the row's entries are written, the padding is not
    (both bins mappings, and gather)."""
    from mi355_mp import ops
    H, E = 25, edges.shape[1]
    Q = (H + 1) * C
    h = torch.randn(E, H, device=DEV)
    x = torch.randn(N, C, device=DEV)
    y = torch.randn(N, Q, device=DEV)
    out = torch.full((N, Q + 3), 7.0, device=DEV)
    ops.nnconv_bins(graph.dst, h, x, out=out)
    assert torch.equal(out[:, :Q], ops.nnconv_bins(graph.dst, h, x))
    assert float((out[:, Q:] - 7.0).abs().max()) == 0.0
    out = torch.full((N, C + 3), 7.0, device=DEV)
    ops.nnconv_gather(graph.dst, h, y, C, out=out)
    assert torch.equal(out[:, :C], ops.nnconv_gather(graph.dst, h, y, C))
    assert float((out[:, C:] - 7.0).abs().max()) == 0.0


# 2. the layer ------------------------------------------------------------------

def _layer(c_in, c_out, H, aggr, flow, seed, root=True, bias=True, head_bias=True, nn=None, D=2):
    from torch_geometric.nn import NNConv
    torch.manual_seed(seed)
    if nn is None:
        nn = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(),
                                 torch.nn.Linear(H, c_in * c_out, bias=head_bias))
    conv = NNConv(c_in, c_out, nn, aggr=aggr, flow=flow, root_weight=root, bias=bias)
    return conv


def _inputs(edges, c_in, seed, D=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, c_in, generator=g), torch.rand(edges.shape[1], D, generator=g)


def _split(conv):
    """(trunk, head) of the layer's nn, whatever path the layer takes."""
    nn = conv.nn
    if isinstance(nn, torch.nn.Linear):
        return None, nn
    mods = [m for m in nn if not isinstance(m, torch.nn.Identity)]
    return torch.nn.Sequential(*mods[:-1]), mods[-1]


def _reference(conv, x, ei, ea, absolute=False, gout=None, ea_grad=False):
    """The restatement on float64 copies of the layer's parameters; with gout
    its autograd too.  absolute: sum |terms| -- every leaf by its magnitude, the
    trunk's ReLU as the fixed mask of the signed computation.  Returns (out,
    {name: grad}) with the layer's parameter names and 'x'; ea_grad (a bare
    Linear nn, whose h is edge_attr itself): and 'edge_attr'."""
    trunk, head = _split(conv)
    cvt = (lambda t: t.detach().cpu().double().abs()) if absolute else (lambda t: t.detach().cpu().double())
    leaves = {n: cvt(p).requires_grad_(True) for n, p in conv.named_parameters()}
    leaves["x"] = cvt(x).requires_grad_(True)
    prefix = "nn." if trunk is None else "nn.%d." % (len(list(conv.nn)) - 1 - sum(
        isinstance(m, torch.nn.Identity) for m in conv.nn))
    ea = ea.detach().cpu().double()
    ea = ea.view(-1, 1) if ea.dim() == 1 else ea
    if trunk is None:
        h = ea.abs() if absolute else ea
        if ea_grad:
            h = leaves["edge_attr"] = h.clone().requires_grad_(True)
    else:
        assert not ea_grad
        assert len(trunk) == 2 and isinstance(trunk[1], torch.nn.ReLU)
        w1, b1 = trunk[0].weight.detach().cpu().double(), trunk[0].bias.detach().cpu().double()
        mask = ((ea @ w1.t() + b1) > 0).double()
        h = ((ea.abs() if absolute else ea) @ leaves["nn.0.weight"].t() + leaves["nn.0.bias"]) * mask
    out = R.nn_conv(leaves["x"], ei, h, leaves[prefix + "weight"], leaves.get(prefix + "bias"), conv.in_channels,
                    conv.out_channels, leaves.get("root"), leaves.get("bias"), conv.aggr, conv.flow)
    grads = None
    if gout is not None:
        (out * (gout.double().abs() if absolute else gout.double())).sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return out.detach(), grads


def check_layer(conv, x, ei, ea, form, what, ea_grad=False, seed=5):
    """Forward and every gradient (x, every parameter; ea_grad: edge_attr, a leaf
    the edge-gradient kernel writes) of one layer call on any graph against the
    restatement.  Returns (out, {name: grad}) of the device run."""
    conv = conv.to(DEV)
    n = x.shape[0]
    gout = torch.randn(n, conv.out_channels, generator=torch.Generator().manual_seed(seed))
    xd = x.to(DEV).requires_grad_(True)
    ead = ea.to(DEV).requires_grad_(ea_grad)
    out = conv(xd, ei.to(DEV), ead, form=form)
    assert tuple(out.shape) == (n, conv.out_channels), what
    (out * gout.to(DEV)).sum().backward()
    ref, want = _reference(conv, x, ei, ea, gout=gout, ea_grad=ea_grad)
    ref_abs, scale = _reference(conv, x, ei, ea, absolute=True, gout=gout, ea_grad=ea_grad)
    R.assert_bound(out, ref, ref_abs, "forward " + what)
    got = {name: p.grad for name, p in conv.named_parameters()}
    got["x"] = xd.grad
    if ea_grad:
        got["edge_attr"] = ead.grad
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
    conv = _layer(6, 10, 25, aggr, flow, 3)
    x, ea = _inputs(edges, 6, 3)
    out = conv.to(DEV)(x.to(DEV), edges.to(DEV), ea.to(DEV), form=form)
    assert out.shape == (N, 10)
    R.assert_bound(out, _reference(conv, x, edges, ea)[0], _reference(conv, x, edges, ea, absolute=True)[0],
                   "layer %s %s %s" % (form, aggr, flow))


@pytest.mark.parametrize("form", ["bins", "gather"])
@pytest.mark.parametrize("root,bias,head_bias", [(False, False, True), (True, False, False), (False, True, False)])
def test_layer_forward_without_root_bias_or_head_bias(edges, form, root, bias, head_bias):
    conv = _layer(33, 4, 7, "mean", "source_to_target", 5, root=root, bias=bias, head_bias=head_bias)
    x, ea = _inputs(edges, 33, 5)
    out = conv.to(DEV)(x.to(DEV), edges.to(DEV), ea.to(DEV), form=form)
    R.assert_bound(out, _reference(conv, x, edges, ea)[0], _reference(conv, x, edges, ea, absolute=True)[0],
                   "layer %s root=%s bias=%s head_bias=%s" % (form, root, bias, head_bias))


def test_layer_bare_linear_1d_inputs_and_the_chosen_form(edges):
    """nn a bare Linear (h is edge_attr itself); x [N] and edge_attr [E] are
    taken as one column; the automatic form is bitwise the one nnconv_form names."""
    from mi355_mp import ops
    conv = _layer(1, 32, 1, "add", "source_to_target", 7, nn=torch.nn.Linear(1, 32))
    g = torch.Generator().manual_seed(7)
    x, ea = torch.randn(N, generator=g), torch.rand(edges.shape[1], generator=g)
    conv = conv.to(DEV)
    out = conv(x.to(DEV), edges.to(DEV), ea.to(DEV))
    assert out.shape == (N, 32)
    R.assert_bound(out, _reference(conv, x, edges, ea)[0], _reference(conv, x, edges, ea, absolute=True)[0],
                   "bare Linear, 1-D inputs")
    E = edges.shape[1]
    for c_in, c_out, H, want in ((1, 32, 25, "bins"), (70, 2, 4, "gather")):
        assert ops.nnconv_form(H, c_in, c_out, E, N) == want
        conv = _layer(c_in, c_out, H, "add", "source_to_target", 8).to(DEV)
        xd, ead = torch.randn(N, c_in, device=DEV), torch.rand(E, 2, device=DEV)
        assert torch.equal(conv(xd, edges.to(DEV), ead), conv(xd, edges.to(DEV), ead, form=want))


@pytest.mark.parametrize("case", ["max", "identity_tail", "hooked_head"])
def test_generic_path_matches_the_restatement(edges, case):
    """aggr='max', an nn whose last module is not a Linear and a hooked head run
    upstream's message / update on the generic path: same result, no fused call."""
    from mi355_mp import ops
    c_in, c_out, H = 5, 3, 6
    nn = None
    if case == "identity_tail":
        nn = torch.nn.Sequential(torch.nn.Linear(2, H), torch.nn.ReLU(), torch.nn.Linear(H, c_in * c_out),
                                 torch.nn.Identity())
    conv = _layer(c_in, c_out, H, "max" if case == "max" else "add", "source_to_target", 13, nn=nn)
    seen = []
    if case == "hooked_head":
        conv.nn[2].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    assert conv.fused_head() is None
    x, ea = _inputs(edges, c_in, 13)
    conv = conv.to(DEV)
    real = ops.nnconv_propagate
    ops.nnconv_propagate = None                                       # the generic path never touches it
    try:
        out = conv(x.to(DEV), edges.to(DEV), ea.to(DEV))
    finally:
        ops.nnconv_propagate = real
    if case == "hooked_head":
        assert seen == [(edges.shape[1], c_in * c_out)]
    ref = _reference(conv, x, edges, ea)[0]
    conv.aggr = "add"
    scale = _reference(conv, x, edges, ea, absolute=True)[0]          # max: one message of the row's sum
    R.assert_bound(out, ref, scale, "generic path: %s" % case)


@pytest.mark.parametrize("form", ["bins", "gather"])
@pytest.mark.parametrize("shape", [(6, 10, 5, "mean"), (70, 2, 4, "add"), (1, 32, 25, "add"), (33, 33, 3, "mean")])
def test_layer_gradients(edges, form, shape):
    """d x, d root, d bias, the trunk's parameters (through d h) and d
    head.weight / d head.bias against the restatement's float64 autograd."""
    c_in, c_out, H, aggr = shape
    conv = _layer(c_in, c_out, H, aggr, "source_to_target", 11).to(DEV)
    x, ea = _inputs(edges, c_in, 11)
    gout = torch.randn(N, c_out, generator=torch.Generator().manual_seed(5))
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, edges.to(DEV), ea.to(DEV), form=form)
    (out * gout.to(DEV)).sum().backward()
    _, want = _reference(conv, x, edges, ea, gout=gout)
    _, scale = _reference(conv, x, edges, ea, absolute=True, gout=gout)
    got = {n: p.grad for n, p in conv.named_parameters()}
    got["x"] = xd.grad
    assert sorted(got) == sorted(want) == ["bias", "nn.0.bias", "nn.0.weight", "nn.2.bias", "nn.2.weight", "root", "x"]
    for name in sorted(got):
        assert got[name] is not None, name
        R.assert_bound(got[name], want[name], scale[name], "grad %s %s %s" % (name, form, shape))


def test_edge_attr_without_grad_skips_the_edge_grad_launch(edges):
    """A bare-Linear nn reads edge_attr as h: it needs no gradient, so the
    backward does not launch the edge-grad kernel; one that requires grad gets it."""
    from mi355_mp import ops
    conv = _layer(6, 10, 2, "add", "source_to_target", 17, nn=torch.nn.Linear(2, 60)).to(DEV)
    x, ea = _inputs(edges, 6, 17)
    calls = []
    real = ops.nnconv_edge_grad
    ops.nnconv_edge_grad = lambda *a: calls.append(1) or real(*a)
    try:
        xd = x.to(DEV).requires_grad_(True)
        conv(xd, edges.to(DEV), ea.to(DEV)).square().sum().backward()
        assert calls == [] and xd.grad is not None and conv.nn.weight.grad is not None
        ead = ea.to(DEV).requires_grad_(True)
        gout = torch.randn(N, 10, generator=torch.Generator().manual_seed(2))
        (conv(x.to(DEV), edges.to(DEV), ead) * gout.to(DEV)).sum().backward()
        assert calls == [1]
    finally:
        ops.nnconv_edge_grad = real
    ear = ea.double().requires_grad_(True)
    eaa = ea.double().requires_grad_(True)
    p = {n: t.detach().cpu().double() for n, t in conv.named_parameters()}
    (R.nn_conv(x, edges, ear, p["nn.weight"], p["nn.bias"], 6, 10, p["root"], p["bias"]) * gout.double()).sum().backward()
    (R.nn_conv(x, edges, eaa, p["nn.weight"], p["nn.bias"], 6, 10, p["root"], p["bias"], absolute=True)
     * gout.double().abs()).sum().backward()
    R.assert_bound(ead.grad, ear.grad, eaa.grad, "grad edge_attr")


# 3. bit-exact, determinism -------------------------------------------------------

def test_forward_bit_exact_on_small_integers(edges):
    """Integer h in [-3, 3], x and every weight in [-4, 4]: each product and
    every partial sum of the 700-slot row (at most 700 * 5 * 7 * 48 < 2^24) is
    exact in fp32 in any order, so both forms equal the restatement bit for bit."""
    from torch_geometric.nn import NNConv
    c_in, c_out, H = 7, 6, 4
    g = torch.Generator().manual_seed(9)
    E = edges.shape[1]
    ea = torch.randint(-3, 4, (E, H), generator=g).float()
    x = torch.randint(-4, 5, (N, c_in), generator=g).float()
    conv = NNConv(c_in, c_out, torch.nn.Linear(H, c_in * c_out))
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randint(-4, 5, p.shape, generator=g).float())
    ref = _reference(conv, x, edges, ea)[0]
    conv = conv.to(DEV)
    outs = [conv(x.to(DEV), edges.to(DEV), ea.to(DEV), form=form) for form in ("bins", "gather")]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].detach().cpu().double(), ref)


def test_two_runs_bitwise_equal_and_forms_agree(edges):
    conv = _layer(33, 20, 9, "mean", "source_to_target", 21).to(DEV)
    x, ea = _inputs(edges, 33, 21)
    ei, ead = edges.to(DEV), ea.to(DEV)
    outs = {}
    for form in ("bins", "gather"):
        runs = []
        for _ in range(2):
            conv.zero_grad()
            xd = x.to(DEV).requires_grad_(True)
            o = conv(xd, ei, ead, form=form)
            o.square().sum().backward()
            runs.append([o.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), form
        outs[form] = runs[0][0]
    scale = _reference(conv, x, edges, ea, absolute=True)[0]
    R.assert_bound(outs["bins"], outs["gather"].cpu().double(), scale, "forms: bins against gather")


# 4. no per-edge weight array -------------------------------------------------------

@pytest.mark.parametrize("form", ["bins", "gather"])
def test_no_per_edge_weight_array(edges, form):
    """E = 3000, Cin = Cout = 64, H = 25: one [E, Cin * Cout] fp32 array is 49 MB,
    far above everything the fused path holds (Z and dZ: 1.7 MB each); forward +
    backward must peak below it."""
    c_in = c_out = 64
    conv = _layer(c_in, c_out, 25, "add", "source_to_target", 31).to(DEV)
    x, ea = _inputs(edges, c_in, 31)
    xd, ei, ead = x.to(DEV).requires_grad_(True), edges.to(DEV), ea.to(DEV)
    conv(xd, ei, ead, form=form).sum().backward()                     # builds and caches both CSRs
    conv.zero_grad()
    xd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    conv(xd, ei, ead, form=form).square().sum().backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    per_edge = edges.shape[1] * c_in * c_out * 4
    print("%s: peak growth %d bytes, one per-edge weight array %d bytes" % (form, growth, per_edge))
    assert growth < per_edge


# 5. the example ------------------------------------------------------------------

def test_example_mnist_nn_conv():
    spec = importlib.util.spec_from_file_location("example_mnist_nn_conv",
                                                  os.path.join(ROOT, "examples", "mnist_nn_conv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    losses = mod.main(["--epochs", "2", "--graphs", "256"])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
