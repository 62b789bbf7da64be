"""RGCNConv on the GPU: the three kernels under both stride settings, the layer's
forward and every gradient (featured in both forms, featureless, both flows),
the generic path, bit-exact and determinism cases, the absence of the per-edge
weight array and of the [R * N, Cout] table, and the example, all against the
float64 restatement tests/_rgcn_ref.py.

Every float comparison uses the project's bound |err| <= 1e-5 * sum |terms|
(sum |terms| = the same computation on absolute values).  One fixed graph: 300
nodes, about 4000 edges in random order with duplicate edges, self loops, node
5 with 700 in-edges (its serial fp32 sum of up to 700 * B terms), nodes 250..
without in-edges and nodes 280.. isolated.  Its relations, for R >= 7: relation
1 has no edge, relation 2 one edge, relation 3 exactly 2 * chunk edges and
relation 4 chunk + 1 (chunk = the att gradient's exported chunk size; the edge
count grows with it), the rest spread with skewed frequencies.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import _rgcn_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 300


def _graph_edges(chunk):
    g = torch.Generator().manual_seed(1)
    n_random = max(3200, 3 * chunk + 2 + 1200)
    ei = torch.stack([torch.randint(0, 280, (n_random,), generator=g), torch.randint(0, 250, (n_random,), generator=g)])
    dup = ei[:, :40]                                                  # repeated (j, i) pairs
    loops = torch.randint(0, 250, (20,), generator=g).repeat(2, 1)    # self loops
    hub = torch.stack([torch.randint(0, 280, (700,), generator=g), torch.full((700,), 5, dtype=torch.int64)])
    ei = torch.cat([ei, dup, loops, hub], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()


def _edge_types(E, n_rel, chunk):
    """int64 [E] in [0, n_rel); n_rel >= 7: the relation sizes of the module docstring."""
    if n_rel == 1:
        return torch.zeros(E, dtype=torch.int64)
    g = torch.Generator().manual_seed(n_rel)
    others = torch.tensor([0] + list(range(5, n_rel)))
    freq = 1.0 / torch.arange(1, others.numel() + 1, dtype=torch.float64)
    et = others[torch.multinomial(freq / freq.sum(), E, replacement=True, generator=g)]
    pos = torch.randperm(E, generator=g)
    et[pos[:1]] = 2
    et[pos[1:1 + 2 * chunk]] = 3
    et[pos[1 + 2 * chunk:2 + 3 * chunk]] = 4
    return et


@pytest.fixture(scope="module")
def chunk():
    from mi355_mp import ops
    return ops.rgcn_att_chunk()


@pytest.fixture(scope="module")
def edges(chunk):
    ei = _graph_edges(chunk)
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg[5]) >= 600 and int(deg[250:].sum()) == 0 and int((ei[0] == ei[1]).sum()) >= 20
    assert int(torch.bincount(ei[0], minlength=N)[280:].sum()) == 0  # isolated nodes
    assert torch.unique(ei[0] * N + ei[1]).numel() < ei.shape[1]      # duplicate edges
    return ei


@pytest.fixture(scope="module")
def types(edges, chunk):
    out = {n_rel: _edge_types(edges.shape[1], n_rel, chunk) for n_rel in (1, 7, 46)}
    for n_rel in (7, 46):
        count = torch.bincount(out[n_rel], minlength=n_rel)
        assert count[1:5].tolist() == [0, 1, 2 * chunk, chunk + 1] and int(count.min()) == 0
    return out


@pytest.fixture(scope="module")
def norm(edges):
    return torch.rand(edges.shape[1], generator=torch.Generator().manual_seed(3)) + 0.5


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    return Graph(edges.to(DEV), N, N)


# 1. the three kernels ---------------------------------------------------------

def _nan(*shape):
    """An output to hand to a kernel: an entry it leaves unwritten fails every comparison."""
    return torch.full(shape, float("nan"), device=DEV)


def check_kernels(edges, csr, n, types, norm, C, B, first_empty_row):
    """bins, gather (F = C) and att_grad (both roles) on the graph `edges` ([2, E]
    on the CPU; csr: its destination CSR on the device, n nodes, rows
    first_empty_row.. without in-edges) for every {R: edge types} of `types`
    (relation 1 without edges when R > 1), att with ld_att = B + 2, with and
    without edge_norm, node-major and block-major, into NaN-filled outputs."""
    from mi355_mp import ops
    dst, src = edges[1], edges[0]
    dstd, srcd = edges[1].to(DEV), edges[0].to(DEV)
    g = torch.Generator().manual_seed(C * 1000 + B)
    x = torch.randn(n, C, generator=g)
    y = torch.randn(n, B, C, generator=g)
    p = torch.randn(n, B, C, generator=g)
    q = torch.randn(n, C, generator=g)
    bias = torch.randn(C, generator=g)
    xd, qd, bd = x.to(DEV), q.to(DEV), bias.to(DEV)
    y_node, y_block = y.view(n, B * C).to(DEV), y.permute(1, 0, 2).contiguous().to(DEV)
    p_node, p_block = p.view(n, B * C).to(DEV), p.permute(1, 0, 2).contiguous().to(DEV)
    for n_rel in sorted(types):
        assert ops.rgcn_ok(n_rel, B, C, C)
        et = types[n_rel]
        etd = et.to(DEV)
        plan = ops.rgcn_relation_plan(etd, n_rel)
        attw = torch.randn(n_rel, B + 2, generator=g)
        att = attw[:, :B]
        attd = attw.to(DEV)[:, :B]
        assert attd.stride(0) == B + 2
        for en in (None, norm):
            tag = "C=%d B=%d R=%d norm=%s" % (C, B, n_rel, en is not None)
            end = None if en is None else en.to(DEV)
            z_ref = R.bins(dst, src, n, et, en, att, x)
            z_abs = R.bins(dst, src, n, et, en, att.abs(), x.abs())
            Z = ops.rgcn_bins(csr, etd, end, attd, xd, out=_nan(n, B * C))
            assert Z.shape == (n, B * C)
            R.assert_bound(Z, z_ref.view(n, B * C), z_abs.view(n, B * C), "bins " + tag)
            assert float(Z[first_empty_row:].abs().max()) == 0.0      # rows without slots are zero
            assert torch.equal(ops.rgcn_bins(csr, etd, end, attd, xd), Z)
            Zb = _nan(B, n, C)
            ops.rgcn_bins(csr, etd, end, attd, xd, out=Zb)            # through the block stride
            assert torch.equal(Zb.permute(1, 0, 2).reshape(n, B * C), Z)
            o_ref = R.gather(dst, src, n, et, en, att, y)
            o_abs = R.gather(dst, src, n, et, en, att.abs(), y.abs())
            o = ops.rgcn_gather(csr, etd, end, attd, y_node, C, out=_nan(n, C))
            R.assert_bound(o, o_ref, o_abs, "gather " + tag)
            assert float(o[first_empty_row:].abs().max()) == 0.0
            assert torch.equal(ops.rgcn_gather(csr, etd, end, attd, y_node, C), o)
            assert torch.equal(ops.rgcn_gather(csr, etd, end, attd, y_block, out=_nan(n, C)), o)
            ob = ops.rgcn_gather(csr, etd, end, attd, y_block, bias=bd, out=_nan(n, C))
            R.assert_bound(ob, o_ref + bias.double(), o_abs + bias.double().abs(), "gather + bias " + tag)
            # att grad: P = dZ [n, B*C] by destination with Q = x by source (the featured backward), and
            # P = basis [B, n, C] in place by source with Q = g by destination (the featureless one)
            for rows, cols, rd, cd, pd in ((dst, src, dstd, srcd, p_node), (src, dst, srcd, dstd, p_block)):
                da = ops.rgcn_att_grad(plan, rd, cd, end, pd, qd, B, out=_nan(n_rel, B))
                assert da.shape == (n_rel, B)
                R.assert_bound(da, R.att_grad(et, en, rows, cols, p, q, n_rel),
                               R.att_grad(et, en, rows, cols, p.abs(), q.abs(), n_rel), "att_grad " + tag)
                assert torch.equal(ops.rgcn_att_grad(plan, rd, cd, end, pd, qd, B), da)
                if n_rel > 1:
                    assert float(da[1].abs().max()) == 0.0            # the relation without edges


@pytest.mark.parametrize("B", [1, 5, 30, 33])
@pytest.mark.parametrize("C", [1, 5, 16, 33, 64, 70])
def test_kernels_against_float64(edges, types, norm, graph, C, B):
    """bins (C: the flat mapping below 32 columns, the column mapping from 32 on,
    two column tiles at 70; B: one, part of one, two and three tiles of 16),
    gather (F = C) and att_grad (both roles), for R in {1, 7, 46}, att with
    ld_att = B + 2, with and without edge_norm, node-major and block-major."""
    check_kernels(edges, graph.dst, N, types, norm, C, B, 250)


@pytest.mark.parametrize("C", [5, 33])
def test_padded_outputs_come_back_untouched(edges, types, graph, C):
    """Strides above the row: the row's entries are written, the padding is not
    (both bins mappings under both stride settings, gather, att_grad's datt is
    the op's own)."""
    from mi355_mp import ops
    B, n_rel = 5, 7
    Q = B * C
    etd = types[n_rel].to(DEV)
    att = torch.randn(n_rel, B, device=DEV)
    x = torch.randn(N, C, device=DEV)
    y = torch.randn(N, Q, device=DEV)
    want = ops.rgcn_bins(graph.dst, etd, None, att, x)
    out = torch.full((N, Q + 3), 7.0, device=DEV)
    ops.rgcn_bins(graph.dst, etd, None, att, x, out=out)
    assert torch.equal(out[:, :Q], want) and float((out[:, Q:] - 7.0).abs().max()) == 0.0
    out = torch.full((B, N, C + 3), 7.0, device=DEV)
    ops.rgcn_bins(graph.dst, etd, None, att, x, out=out[:, :, :C])
    assert torch.equal(out[:, :, :C].permute(1, 0, 2).reshape(N, Q), want)
    assert float((out[:, :, C:] - 7.0).abs().max()) == 0.0
    out = torch.full((N, C + 3), 7.0, device=DEV)
    ops.rgcn_gather(graph.dst, etd, None, att, y, C, out=out)
    assert torch.equal(out[:, :C], ops.rgcn_gather(graph.dst, etd, None, att, y, C))
    assert float((out[:, C:] - 7.0).abs().max()) == 0.0


# 2. the layer ------------------------------------------------------------------

def _layer(c_in, c_out, n_rel, B, flow, seed, root=True, bias=True, cls=None):
    from torch_geometric.nn import RGCNConv
    torch.manual_seed(seed)
    return (cls or RGCNConv)(c_in, c_out, n_rel, B, root_weight=root, bias=bias, flow=flow)


def _reference(conv, x, ei, et, en, absolute=False, gout=None):
    """The restatement on float64 copies of the layer's parameters; with gout its
    autograd too.  absolute: sum |terms| -- every leaf by its magnitude.  Returns
    (out, {name: grad}) with the layer's parameter names, 'x' and 'edge_norm'."""
    cvt = (lambda t: t.detach().cpu().double().abs()) if absolute else (lambda t: t.detach().cpu().double())
    leaves = {n: cvt(p).requires_grad_(True) for n, p in conv.named_parameters()}
    if x is not None:
        leaves["x"] = cvt(x).requires_grad_(True)
    if en is not None:
        leaves["edge_norm"] = cvt(en).requires_grad_(True)
    out = R.rgcn_conv(leaves.get("x"), ei, et, leaves.get("edge_norm"), leaves["basis"], leaves["att"],
                      leaves.get("root"), leaves.get("bias"), conv.flow)
    grads = None
    if gout is not None:
        (out * (gout.double().abs() if absolute else gout.double())).sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return out.detach(), grads


def _check_layer(conv, x, ei, et, en, form, what, en_grad=False):
    """Forward and every gradient of one layer call on any graph against the
    restatement.  Returns (out, {name: grad}) of the device run."""
    conv = conv.to(DEV)
    n = conv.in_channels if x is None else x.shape[0]
    gout = torch.randn(n, conv.out_channels, generator=torch.Generator().manual_seed(5))
    xd = None if x is None else x.to(DEV).requires_grad_(True)
    end = None if en is None else en.to(DEV).requires_grad_(en_grad)
    kw = {} if form is None else {"form": form}
    out = conv(xd, ei.to(DEV), et.to(DEV), end, **kw)
    assert out.shape == (n, conv.out_channels)
    (out * gout.to(DEV)).sum().backward()
    ref, want = _reference(conv, x, ei, et, en, gout=gout)
    ref_abs, scale = _reference(conv, x, ei, et, en, absolute=True, gout=gout)
    R.assert_bound(out, ref, ref_abs, "forward " + what)
    got = {n: p.grad for n, p in conv.named_parameters()}
    if x is not None:
        got["x"] = xd.grad
    if en_grad:
        got["edge_norm"] = end.grad
    else:
        want.pop("edge_norm", None)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(got):
        assert got[name] is not None, name
        assert tuple(got[name].shape) == tuple(want[name].shape), name
        R.assert_bound(got[name], want[name], scale[name], "grad %s %s" % (name, what))
    return out, got


@pytest.mark.parametrize("root_bias", [True, False])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
@pytest.mark.parametrize("mode", ["bins", "gather", "chosen", "featureless"])
@pytest.mark.parametrize("shape", [(6, 10, 7, 5), (33, 4, 46, 30)])
def test_layer_forward_and_every_gradient(edges, types, norm, shape, mode, flow, root_bias):
    """out, d x, d basis, d att, d root and d bias: featured in both forms and with
    the chosen one (the flat and the column mapping of bins), featureless (x =
    None, Cin = N), both flows, with and without root and bias, with edge_norm."""
    c_in, c_out, n_rel, B = shape
    featureless = mode == "featureless"
    conv = _layer(N if featureless else c_in, c_out, n_rel, B, flow, 3, root=root_bias, bias=root_bias)
    x = None if featureless else torch.randn(N, c_in, generator=torch.Generator().manual_seed(4))
    form = mode if mode in ("bins", "gather") else None
    _check_layer(conv, x, edges, types[n_rel], norm, form, "%s %s %s root/bias=%s" % (shape, mode, flow, root_bias))


@pytest.mark.parametrize("featureless", [False, True])
def test_layer_without_edge_norm_and_the_chosen_form(edges, types, featureless):
    """edge_norm = None; the automatic form is bitwise the one rgcn_form names."""
    from mi355_mp import ops
    conv = _layer(N if featureless else 16, 8, 7, 5, "source_to_target", 7)
    x = None if featureless else torch.randn(N, 16, generator=torch.Generator().manual_seed(8))
    _check_layer(conv, x, edges, types[7], None, None, "no edge_norm, featureless=%s" % featureless)
    if featureless:
        return
    E = edges.shape[1]
    ei, et = edges.to(DEV), types[7].to(DEV)
    for c_in, c_out, B, want in ((6, 10, 5, "bins"), (70, 2, 5, "gather")):
        assert ops.rgcn_form(B, c_in, c_out, E, N) == want
        conv = _layer(c_in, c_out, 7, B, "source_to_target", 8).to(DEV)
        xd = torch.randn(N, c_in, device=DEV)
        assert torch.equal(conv(xd, ei, et), conv(xd, ei, et, form=want))


@pytest.mark.parametrize("case", ["edge_norm_grad", "message_override", "message_override_featureless"])
def test_generic_path_matches_the_restatement(edges, types, norm, case):
    """An edge_norm that requires a gradient and a subclass overriding message run
    upstream's message / update on the generic path: same result (and d
    edge_norm), no fused call."""
    from mi355_mp import ops
    from torch_geometric.nn import RGCNConv

    class Same(RGCNConv):
        def message(self, x_j, edge_index_j, edge_type, edge_norm):
            return super().message(x_j, edge_index_j, edge_type, edge_norm)

    featureless = case == "message_override_featureless"
    conv = _layer(N if featureless else 6, 5, 7, 3, "source_to_target", 13, cls=None if case == "edge_norm_grad" else Same)
    assert conv.fused_layer() == (case == "edge_norm_grad")
    x = None if featureless else torch.randn(N, 6, generator=torch.Generator().manual_seed(13))
    real = ops.rgcn_propagate
    ops.rgcn_propagate = None                                         # the generic path never touches it
    try:
        _check_layer(conv, x, edges, types[7], norm, None, "generic path: " + case, en_grad=case == "edge_norm_grad")
    finally:
        ops.rgcn_propagate = real


def test_gradient_launches_are_skipped_when_nothing_needs_them(edges, types):
    """With att and basis frozen the backward launches neither rgcn_att_grad nor
    the bins kernel for Z; d x still comes from the gather kernel."""
    from mi355_mp import ops
    conv = _layer(6, 10, 7, 5, "source_to_target", 17).to(DEV)
    conv.att.requires_grad_(False)
    conv.basis.requires_grad_(False)
    calls = []
    real_att, real_bins = ops.rgcn_att_grad, ops.rgcn_bins
    ops.rgcn_att_grad = lambda *a, **k: calls.append("att") or real_att(*a, **k)
    ops.rgcn_bins = lambda *a, **k: calls.append("bins") or real_bins(*a, **k)
    try:
        xd = torch.randn(N, 6, device=DEV, requires_grad=True)
        conv(xd, edges.to(DEV), types[7].to(DEV), form="gather").square().sum().backward()
        assert calls == [] and xd.grad is not None and conv.root.grad is not None
        conv.att.requires_grad_(True)
        conv(xd, edges.to(DEV), types[7].to(DEV), form="gather").square().sum().backward()
        assert calls == ["att"] and conv.att.grad is not None and conv.basis.grad is None
    finally:
        ops.rgcn_att_grad, ops.rgcn_bins = real_att, real_bins


# 3. bit-exact, determinism -------------------------------------------------------

def test_forward_bit_exact_on_small_integers(edges, types):
    """Integer x in [-3, 3], att, basis, root and bias in [-2, 2], edge_norm in {1, 2}:
    every product and every partial sum of the 700-slot row (at most 700 * 2 * 3 *
    2 * 4 * 3 * 2 < 2^24) is exact in fp32 in any order, so both forms and the
    featureless layer equal the restatement bit for bit."""
    from torch_geometric.nn import RGCNConv
    c_in, c_out, n_rel, B = 4, 6, 7, 3
    g = torch.Generator().manual_seed(9)
    E = edges.shape[1]
    en = torch.randint(1, 3, (E,), generator=g).float()
    x = torch.randint(-3, 4, (N, c_in), generator=g).float()
    ei, et = edges.to(DEV), types[n_rel].to(DEV)
    for cin, xin in ((c_in, x), (N, None)):
        conv = RGCNConv(cin, c_out, n_rel, B)
        with torch.no_grad():
            for p in conv.parameters():
                p.copy_(torch.randint(-2, 3, p.shape, generator=g).float())
        ref = _reference(conv, xin, edges, types[n_rel], en)[0]
        conv = conv.to(DEV)
        xd = None if xin is None else xin.to(DEV)
        forms = (None,) if xin is None else ("bins", "gather")
        for form in forms:
            out = conv(xd, ei, et, en.to(DEV), **({} if form is None else {"form": form}))
            assert torch.equal(out.detach().cpu().double(), ref), (cin, form)


def test_two_runs_bitwise_equal_and_forms_agree(edges, types, norm):
    ei, et, en = edges.to(DEV), types[46].to(DEV), norm.to(DEV)
    x = torch.randn(N, 33, generator=torch.Generator().manual_seed(21))
    outs = {}
    for mode in ("bins", "gather", "featureless"):
        conv = _layer(N if mode == "featureless" else 33, 20, 46, 30, "source_to_target", 21).to(DEV)
        runs = []
        for _ in range(2):
            conv.zero_grad()
            xd = None if mode == "featureless" else x.to(DEV).requires_grad_(True)
            o = conv(xd, ei, et, en, **({} if mode == "featureless" else {"form": mode}))
            o.square().sum().backward()
            runs.append([o.detach().clone()] + ([] if xd is None else [xd.grad.clone()])
                        + [p.grad.clone() for p in conv.parameters()])
            assert conv.att.grad is not None
        for a, b in zip(*runs):
            assert torch.equal(a, b), mode
        outs[mode] = runs[0][0]
    conv = _layer(33, 20, 46, 30, "source_to_target", 21)
    scale = _reference(conv, x, edges, types[46], norm, absolute=True)[0]
    R.assert_bound(outs["bins"], outs["gather"].cpu().double(), scale, "forms: bins against gather")


# 4. errors -------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [7, -1])
def test_out_of_range_edge_type_raises_index_error(edges, types, bad):
    conv = _layer(6, 10, 7, 5, "source_to_target", 1).to(DEV)
    et = types[7].clone()
    et[123] = bad
    with pytest.raises(IndexError, match="edge_type"):
        conv(torch.randn(N, 6, device=DEV), edges.to(DEV), et.to(DEV))
    first = _layer(N, 10, 7, 5, "source_to_target", 1).to(DEV)
    with pytest.raises(IndexError, match="edge_type"):
        first(None, edges.to(DEV), et.to(DEV))


def test_form_off_the_fused_path_raises_value_error(edges, types, norm):
    conv = _layer(6, 10, 7, 5, "source_to_target", 1).to(DEV)
    xd, ei, et = torch.randn(N, 6, device=DEV), edges.to(DEV), types[7].to(DEV)
    with pytest.raises(ValueError, match="fused path"):
        conv(xd, ei, et, norm.to(DEV).requires_grad_(True), form="bins")
    with pytest.raises(ValueError, match="form"):
        conv(xd, ei, et, form="other")
    with pytest.raises(ValueError, match="one form"):
        _layer(N, 10, 7, 5, "source_to_target", 1).to(DEV)(None, ei, et, form="gather")


# 5. no per-edge weight array, no [R * N, Cout] table -------------------------------------

def _peak_growth(run):
    run()                                                             # builds and caches the CSRs and the relation plan
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("form", ["bins", "gather"])
def test_no_per_edge_weight_array(edges, types, form):
    """E ~ 4000, Cin = Cout = 64, B = 5, R = 7: one [E, Cin, Cout] fp32 array is 65
    MB.  The fused path's own tensors, from their shapes -- Z, dZ and Y [N, B *
    64], out, its gradient twice (the loss's and the contiguous copy), d x, the
    parameter gradients and the att workspace -- come to under half of that;
    forward + backward must peak below the one array."""
    c, B, n_rel = 64, 5, 7
    E = edges.shape[1]
    conv = _layer(c, c, n_rel, B, "source_to_target", 31).to(DEV)
    xd = torch.randn(N, c, device=DEV, requires_grad=True)
    ei, et = edges.to(DEV), types[n_rel].to(DEV)

    def run():
        conv.zero_grad()
        xd.grad = None
        conv(xd, ei, et, form=form).square().sum().backward()

    per_edge = E * c * c * 4
    own = 4 * (3 * N * B * c + 5 * N * c + B * c * c + c * c + c + 2 * n_rel * B + (E // 64 + n_rel) * B)
    assert 2 * own < per_edge
    growth = _peak_growth(run)
    print("%s: peak growth %d bytes, own tensors %d, one per-edge weight array %d bytes" % (form, growth, own, per_edge))
    assert growth < per_edge


def test_featureless_builds_no_relation_node_table(edges, types):
    """x = None, N = 300, Cout = 64, B = 5, R = 46: upstream's att @ basis table
    [R * N, Cout] is 3.5 MB; the fused path holds out, its gradients and d basis
    [B, N, Cout] (0.4 MB): forward + backward must peak below the table."""
    c_out, B, n_rel = 64, 5, 46
    conv = _layer(N, c_out, n_rel, B, "source_to_target", 32).to(DEV)
    ei, et = edges.to(DEV), types[n_rel].to(DEV)

    def run():
        conv.zero_grad()
        conv(None, ei, et).square().sum().backward()

    table = n_rel * N * c_out * 4
    own = 4 * (5 * N * c_out + 2 * B * N * c_out + 2 * n_rel * B + (edges.shape[1] // 64 + n_rel) * B)
    assert 2 * own < table
    growth = _peak_growth(run)
    print("featureless: peak growth %d bytes, own tensors %d, one [R * N, Cout] table %d bytes" % (growth, own, table))
    assert growth < table


# 6. the example ------------------------------------------------------------------

def test_example_rgcn():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rgcn.py"), "--nodes", "3000", "--epochs", "30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(line.split("loss")[1].split(",")[0]) for line in r.stdout.splitlines() if "loss" in line]
    assert len(losses) == 30 and all(math.isfinite(v) for v in losses), losses
    assert sum(losses[-3:]) / 3 < sum(losses[:3]) / 3, losses
