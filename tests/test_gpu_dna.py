"""DNAConv on the GPU: the three kernels (packed and separate K, V; padded,
NaN-filled outputs), the layer's forward and every gradient on the fused and the
generic path, attention dropout under the exported mask, bit-exact and
determinism cases, skipped backward launches, the absence of any [E, T, C]
array, and the example, all against the float64 restatement tests/_dna_ref.py.

Every float comparison uses the project's bound |err| <= 1e-5 * sum |terms|
(sum |terms| = the restatement's `absolute` mode), on unit-scale inputs (randn
x, Q, K, V; weights randn / sqrt(C / G)).  One fixed graph: 300 nodes, about
4000 edges in random order with duplicate edges, self loops, node 5 with 700
in-edges, nodes 250.. without in-edges and nodes 280.. isolated.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import _dna_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 300


def _graph_edges():
    g = torch.Generator().manual_seed(1)
    n_random = 3200
    ei = torch.stack([torch.randint(0, 280, (n_random,), generator=g), torch.randint(0, 250, (n_random,), generator=g)])
    dup = ei[:, :40]                                                  # repeated (j, i) pairs
    loops = torch.randint(0, 250, (20,), generator=g).repeat(2, 1)    # self loops
    hub = torch.stack([torch.randint(0, 280, (700,), generator=g), torch.full((700,), 5, dtype=torch.int64)])
    ei = torch.cat([ei, dup, loops, hub], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()


@pytest.fixture(scope="module")
def edges():
    ei = _graph_edges()
    deg = torch.bincount(ei[1], minlength=N)
    assert int(deg[5]) >= 700 and int(deg[250:].sum()) == 0 and int((ei[0] == ei[1]).sum()) >= 20
    assert int(torch.bincount(ei[0], minlength=N)[280:].sum()) == 0  # isolated nodes
    assert torch.unique(ei[0] * N + ei[1]).numel() < ei.shape[1]      # duplicate edges
    return ei


@pytest.fixture(scope="module")
def norm(edges):
    return torch.rand(edges.shape[1], generator=torch.Generator().manual_seed(3)) + 0.5


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    return Graph(edges.to(DEV), N, N)


@pytest.fixture(scope="module")
def task_graphs(edges):
    """The same graph under a schedule of 64-unit tasks, the size from which the kernels walk tasks (about 70 tasks):
    as it is -- the 700 slots of row 5 of the destination CSR are cut into a dozen partials summed by the fix-up --
    and with its edges reversed, which puts that row into the source-keyed CSR."""
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    g = Graph(edges.to(DEV), N, N, chunk=ops.dna_split_chunk())
    gt = Graph(edges.flip(0).contiguous().to(DEV), N, N, chunk=ops.dna_split_chunk())
    assert g.dst.chunk == ops.dna_split_chunk() == 64 and g.dst.n_split >= 1 and gt.src.n_split >= 1
    return g, gt


# 1. the three kernels ---------------------------------------------------------

def _nan(*shape):
    """An output to hand to a kernel: an entry it leaves unwritten fails every comparison."""
    return torch.full(shape, float("nan"), device=DEV)


def _padded(rows, width, pad):
    """(view [rows, width] of a NaN-filled [rows, width + pad] buffer, the buffer)."""
    base = _nan(rows, width + pad)
    return base[:, :width], base


def check_kernels(edges, graph, norm, T, H, d, empty_dst=250, empty_src=280):
    """Forward, d Q and d K / d V for one (T, H, d) against the restatement: K and V
    as the halves of one [N, 2, T, C] buffer and as two tensors, outputs with row
    strides above the row, padding untouched, rows without slots (destinations
    empty_dst.., sources empty_src..) zero."""
    from mi355_mp import ops
    C = H * d
    assert ops.dna_ok(T, H, C)
    dst, src = edges[1], edges[0]
    g = torch.Generator().manual_seed(1000 * T + 10 * H + d)
    q = torch.randn(N, C, generator=g)
    kv = torch.randn(N, 2, T, C, generator=g)
    gout = torch.randn(N, C, generator=g)
    k, v = kv[:, 0], kv[:, 1]
    tag = "T=%d H=%d d=%d" % (T, H, d)
    ref = R.attention(q, k, v, norm, dst, src, N, H)
    ref_abs = R.attention_abs(q, k, v, norm, dst, src, N, H)
    want = R.attention_backward(q, k, v, norm, dst, src, N, H, gout)
    scale = R.attention_backward(q, k, v, norm, dst, src, N, H, gout, absolute=True)
    qd, kvd, gd, nd = q.to(DEV), kv.to(DEV), gout.to(DEV), norm.to(DEV)
    packed = (kvd[:, 0], kvd[:, 1])
    assert packed[0].stride(0) == 2 * T * C and not packed[0].is_contiguous() or N == 1
    separate = (kvd[:, 0].contiguous(), kvd[:, 1].contiguous())
    results = []
    for name, (kd, vd) in (("packed", packed), ("separate", separate)):
        out, out_base = _padded(N, C, 3)
        _, lse = ops.dna_aggregate(graph.dst, qd, kd, vd, nd, H, out=out, want_lse=True)
        R.assert_bound(out, ref, ref_abs, "out %s %s" % (tag, name))
        assert bool(torch.isnan(out_base[:, C:]).all())
        assert float(out[empty_dst:].abs().max()) == 0.0                    # rows without slots are zero
        assert lse.shape == (edges.shape[1], H) and bool(torch.isfinite(lse).all()) and float(lse.min()) >= 0.0
        assert torch.equal(ops.dna_aggregate(graph.dst, qd, kd, vd, nd, H), out)       # without lse, the op's own out
        dq, dq_base = _padded(N, C, 1)
        ops.dna_backward_dst(graph.dst, qd, kd, vd, nd, gd, lse, H, out=dq)
        R.assert_bound(dq, want[0], scale[0], "dQ %s %s" % (tag, name))
        assert bool(torch.isnan(dq_base[:, C:]).all()) and float(dq[empty_dst:].abs().max()) == 0.0
        dk_flat, dk_base = _padded(N, T * C, 5)
        dv_flat, dv_base = _padded(N, T * C, 2)
        dk, dv = dk_flat.unflatten(1, (T, C)), dv_flat.unflatten(1, (T, C))
        ops.dna_backward_src(graph.src, qd, kd, vd, nd, gd, lse, H, dk=dk, dv=dv)
        R.assert_bound(dk, want[1], scale[1], "dK %s %s" % (tag, name))
        R.assert_bound(dv, want[2], scale[2], "dV %s %s" % (tag, name))
        assert bool(torch.isnan(dk_base[:, T * C:]).all()) and bool(torch.isnan(dv_base[:, T * C:]).all())
        assert float(dk[empty_src:].abs().max()) == 0.0 and float(dv[empty_src:].abs().max()) == 0.0   # sources without edges
        results.append([t.clone() for t in (out, lse, dq, dk, dv)])
    for a, b in zip(*results):
        assert torch.equal(a, b), tag                                 # the layout of K | V changes no bit


@pytest.mark.parametrize("shape", [(1, 1, 8), (1, 1, 1), (2, 2, 2), (5, 8, 16), (7, 3, 22), (4, 1, 130), (3, 1, 65),
                                   (33, 16, 1), (9, 4, 64)])
def test_kernels_against_float64(edges, norm, graph, shape):
    """(T, H, d): one lane per head up to whole-wave heads, d no power of two, d above
    64 (two and three channels per lane), a long history of width-1 heads."""
    check_kernels(edges, graph, norm, *shape)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 8, 16), (7, 3, 22), (4, 1, 130), (33, 16, 1), (9, 4, 64)])
def test_kernels_over_tasks_against_float64(edges, norm, graph, task_graphs, shape, reverse):
    """The same checks on the schedule of 64-unit tasks: rows split across tasks leave partials in the slabs and
    the fix-up writes them (reverse: the long row is a source row, split in the d K / d V pass); the default
    schedule of this small graph (16-unit tasks) is walked by rows."""
    from mi355_mp import _lib
    nat = _lib.native()
    g = task_graphs[1 if reverse else 0]
    assert graph.dst.chunk < 64
    assert nat.mp_dna_workspace(graph.dst.struct("other"), 128) < nat.mp_dna_workspace(g.dst.struct("other"), 128)
    if reverse:
        check_kernels(edges.flip(0), g, norm, *shape, empty_dst=280, empty_src=250)
    else:
        check_kernels(edges, g, norm, *shape)


@pytest.mark.parametrize("hc", [(1, 130), (2, 8)])
def test_kernels_at_the_largest_history(edges, norm, graph, hc):
    from mi355_mp import ops
    H, C = hc
    T = ops.dna_max_layers(H, C)
    assert T >= 1 and ops.dna_ok(T, H, C) and not ops.dna_ok(T + 1, H, C)
    check_kernels(edges, graph, norm, T, H, C // H)


# 2. the layer ------------------------------------------------------------------

def _layer(C, H, G, flow, seed, bias=True, cls=None, **kw):
    from torch_geometric.nn import DNAConv
    torch.manual_seed(seed)
    conv = (cls or DNAConv)(C, heads=H, groups=G, bias=bias, flow=flow, **kw)
    with torch.no_grad():                                             # unit-scale weights, biases that matter
        for lin in (conv.multi_head.lin_q, conv.multi_head.lin_k, conv.multi_head.lin_v):
            lin.weight.copy_(torch.randn(lin.weight.shape) / math.sqrt(C // G))
            if bias:
                lin.bias.copy_(torch.randn(C))
    return conv


def _params(conv):
    mh = conv.multi_head
    prm = {"w" + l: getattr(mh, "lin_" + l).weight for l in "qkv"}
    prm.update({"b" + l: getattr(mh, "lin_" + l).bias for l in "qkv"})
    return prm


def _reference(conv, x, ei, ew, gout, keep=None, p=0.0, absolute=False, ew_grad=False):
    """(out, grads) of the restatement on float64 copies of the layer's parameters:
    grads by R.PARAMS names, 'x' and (ew_grad) 'edge_weight'."""
    prm = {k: (None if v is None else v.detach().cpu()) for k, v in _params(conv).items()}
    H = conv.multi_head.heads
    if not ew_grad:
        ei2, nrm = R.gcn_norm(ei, N, ew)
        return R.layer(x, ei2, nrm.detach(), prm, H, conv.flow, keep, p, gout, absolute)
    w = (ew.double().abs() if absolute else ew.double()).requires_grad_(True)
    ei2, nrm = R.gcn_norm(ei, N, w, absolute=absolute)
    out, grads = R.layer(x, ei2, nrm.detach(), prm, H, conv.flow, keep, p, gout, absolute)
    # d norm_e = <g_i, attention_e>: the layer is linear in norm, so it is the gradient of the same
    # restatement with norm as a leaf (absolute: of the sum |terms| form, which is linear in |norm| too)
    leaf = nrm.detach().clone().requires_grad_(True)
    dst, src = R._ends(ei2, conv.flow)
    p64 = {k: (None if v is None else v.double()) for k, v in prm.items()}
    q, k, v = R.project(x.double(), p64)
    if absolute:
        pa = {k_: (None if t is None else t.abs()) for k_, t in p64.items()}
        va = R.project(x.double().abs(), pa)[2]
        o = R.attention_abs(q, k, v, leaf, dst, src, N, H, keep, p, v_mag=va)
        (o * gout.double().abs()).sum().backward()
    else:
        (R.attention(q, k, v, leaf, dst, src, N, H, keep, p) * gout.double()).sum().backward()
    nrm.backward(leaf.grad)
    grads["edge_weight"] = w.grad
    return out, grads


def _check_layer(conv, x, ei, ew, what, ew_grad=False, keep=None, p=0.0):
    """Forward and every gradient of one layer call against the restatement.
    Returns (out, {name: grad}) of the device run."""
    conv = conv.to(DEV)
    C = conv.multi_head.out_channels
    gout = torch.randn(N, C, generator=torch.Generator().manual_seed(5))
    xd = x.to(DEV).requires_grad_(True)
    ewd = None if ew is None else ew.to(DEV).requires_grad_(ew_grad)
    out = conv(xd, ei.to(DEV), ewd)
    assert out.shape == (N, C)
    (out * gout.to(DEV)).sum().backward()
    ref, want = _reference(conv, x, ei, ew, gout, keep, p, ew_grad=ew_grad)
    ref_abs, scale = _reference(conv, x, ei, ew, gout, keep, p, absolute=True, ew_grad=ew_grad)
    R.assert_bound(out, ref, ref_abs, "forward " + what)
    got = {k: (None if v is None else v.grad) for k, v in _params(conv).items() if v is not None}
    got["x"] = xd.grad
    if ew_grad:
        got["edge_weight"] = ewd.grad
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(got):
        assert got[name] is not None, name
        assert tuple(got[name].shape) == tuple(want[name].shape), name
        R.assert_bound(got[name], want[name], scale[name], "grad %s %s" % (name, what))
    return out, got


def _x(T, C, seed=4):
    return torch.randn(N, T, C, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("case", [(5, 32, 8, 16, True), (5, 32, 8, 16, False), (3, 12, 4, 2, True), (4, 20, 1, 1, True),
                                  (1, 32, 8, 16, True), (2, 130, 1, 2, True)])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_layer_forward_and_every_gradient(edges, case, flow):
    """out, d x, the three d weight and the three d bias on the fused path: both
    flows, groups 1, 2 and 16, with and without bias, T = 1, a head of 130."""
    from mi355_mp import ops
    T, C, H, G, bias = case
    conv = _layer(C, H, G, flow, 3, bias=bias)
    calls = []
    real = ops.dna_propagate
    ops.dna_propagate = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        _check_layer(conv, _x(T, C), edges, None, "%s %s" % (case, flow))
    finally:
        ops.dna_propagate = real
    assert calls == [1]                                               # the fused path ran


@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_layer_walks_tasks_on_a_small_graph(edges, p, flow):
    """The layer asks for a schedule of 64-unit tasks even on this graph of 4600 rows + edges (default: 16), so the
    700-slot row is split over tasks (in the destination CSR, or with the other flow in the source-keyed one):
    forward and every gradient, with and without dropout; then the same call forced onto the default schedule,
    walked by rows; cached=False meets the same graph again on a second call."""
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    from torch_geometric.nn.conv import dna_conv as mod
    T, C, H, G = 5, 32, 8, 16
    graphs = []
    real_graph, real_seed = mod.graph_for, ops.dropout_seed

    def recording(*a, **k):
        graphs.append(real_graph(*a, **k))
        return graphs[-1]

    def by_rows(ei, n_dst, n_src, flow, target_tasks=None):
        graphs.append(Graph(ei, n_dst, n_src, flow))
        return graphs[-1]

    mod.graph_for = recording
    ops.dropout_seed = lambda device: 77
    try:
        keep = None
        if p:
            ei2, g2 = _normed_graph(edges)
            keep = ops.dna_dropout_keep(g2, 77, p, H, T).cpu()
        conv = _layer(C, H, G, flow, 3, dropout=p)
        _check_layer(conv, _x(T, C), edges, None, "tasks %s p=%g" % (flow, p), keep=keep, p=p)
        assert len(graphs) == 1 and graphs[0].dst.chunk == graphs[0].src.chunk == 64
        assert graphs[0].dst.n_split + graphs[0].src.n_split >= 1
        assert (graphs[0].dst if flow == "source_to_target" else graphs[0].src).n_split >= 1
        mod.graph_for = by_rows
        _check_layer(_layer(C, H, G, flow, 3, dropout=p), _x(T, C), edges, None, "rows %s p=%g" % (flow, p),
                     keep=keep, p=p)
        assert graphs[1].dst.chunk == 16
    finally:
        mod.graph_for, ops.dropout_seed = real_graph, real_seed


def test_uncached_layer_reuses_its_graph(edges):
    """cached=False: the normalised edge list is cached on the caller's edge_index, so graph_for returns the same
    Graph (CSRs and schedules built once) on every call with that tensor."""
    from torch_geometric.nn.conv import dna_conv as mod
    graphs = []
    real_graph = mod.graph_for
    mod.graph_for = lambda *a, **k: graphs.append(real_graph(*a, **k)) or graphs[-1]
    try:
        conv = _layer(12, 4, 2, "source_to_target", 5).to(DEV)
        ei, x = edges.to(DEV), _x(3, 12).to(DEV)
        a, b = conv(x, ei), conv(x, ei)
    finally:
        mod.graph_for = real_graph
    assert len(graphs) == 2 and graphs[0] is graphs[1] and graphs[0]._dst is not None and torch.equal(a, b)


def test_layer_with_edge_weight_fused_and_generic(edges):
    """edge_weight without a gradient stays on the fused path; with one the layer
    runs upstream's message on the generic path, and d edge_weight is checked."""
    from mi355_mp import ops
    ew = torch.rand(edges.shape[1], generator=torch.Generator().manual_seed(8)) + 0.5
    conv = _layer(12, 4, 2, "source_to_target", 9)
    _check_layer(conv, _x(3, 12), edges, ew, "edge_weight, fused")
    real = ops.dna_propagate
    ops.dna_propagate = None                                          # the generic path never touches it
    try:
        _check_layer(_layer(12, 4, 2, "source_to_target", 9), _x(3, 12), edges, ew, "edge_weight with grad, generic",
                     ew_grad=True)
    finally:
        ops.dna_propagate = real


@pytest.mark.parametrize("case", ["too_long", "message_override", "float64"])
def test_generic_path_matches_the_restatement(edges, case):
    """A history one longer than dna_max_layers, a subclass overriding message and a
    float64 layer run upstream's message on the generic path: same result, no
    fused call."""
    from mi355_mp import ops
    from torch_geometric.nn import DNAConv

    class Same(DNAConv):
        def message(self, x_i, x_j, norm):
            return super().message(x_i, x_j, norm)

    H, C = 2, 8
    T = ops.dna_max_layers(H, C) + 1 if case == "too_long" else 3
    conv = _layer(C, H, 2, "source_to_target", 13, cls=Same if case == "message_override" else None)
    assert conv.fused_layer() == (case != "message_override")
    real = ops.dna_propagate
    ops.dna_propagate = None
    try:
        if case == "float64":
            conv = conv.double().to(DEV)
            x = _x(T, C).double()
            out = conv(x.to(DEV), edges.to(DEV))
            assert out.dtype == torch.float64
            ref, _ = _reference(conv, x, edges, None, None)
            assert float((out.detach().cpu() - ref).abs().max()) <= 1e-11
        else:
            _check_layer(conv, _x(T, C), edges, None, "generic path: " + case)
    finally:
        ops.dna_propagate = real


def test_cached_layer_over_two_calls(edges):
    conv = _layer(12, 4, 2, "source_to_target", 11, cached=True).to(DEV)
    ei = edges.to(DEV)
    x = _x(3, 12).to(DEV)
    first = conv(x, ei)
    kept = conv.cached_result
    assert kept is not None and conv.cached_num_edges == edges.shape[1]
    second = conv(x, ei)
    assert conv.cached_result is kept and torch.equal(first, second)
    ref, _ = _reference(conv, x.cpu(), edges, None, None)
    ref_abs, _ = _reference(conv, x.cpu(), edges, None, None, absolute=True)
    R.assert_bound(second, ref, ref_abs, "cached, second call")
    with pytest.raises(RuntimeError, match="Cached %d number of edges, but found %d" % (edges.shape[1], edges.shape[1] - 1)):
        conv(x, ei[:, :-1])
    conv.reset_parameters()
    assert conv.cached_result is None
    conv(x, ei[:, :-1])
    assert conv.cached_num_edges == edges.shape[1] - 1
    with pytest.raises(ValueError, match="num_layers"):
        conv(x[:, 0], ei)


# 3. attention dropout ----------------------------------------------------------

def _normed_graph(edges):
    from mi355_mp.graph import Graph
    ei2, _ = R.gcn_norm(edges, N)
    return ei2, Graph(ei2.to(DEV), N, N)


@pytest.mark.parametrize("p", [0.5, 0.8])
def test_dropout_under_the_exported_mask(edges, p):
    """Training with 0 < p < 1: the restatement under the mask mp_dna_dropout_keep
    exports for the layer's seed gives the forward and every gradient; the mask
    keeps 1 - p of its bits within 4 standard deviations, repeats under its seed
    and changes with it; eval ignores p."""
    from mi355_mp import ops
    T, C, H, G = 5, 32, 8, 16
    ei2, g2 = _normed_graph(edges)
    keep = ops.dna_dropout_keep(g2, 1234, p, H, T)
    assert keep.dtype == torch.bool and keep.shape == (ei2.shape[1], H, T)
    n_bits = keep.numel()
    rate = float(keep.float().mean())
    print("p = %g: keep rate %.5f over %d bits" % (p, rate, n_bits))
    assert abs(rate - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n_bits)
    assert torch.equal(ops.dna_dropout_keep(g2, 1234, p, H, T), keep)
    assert not torch.equal(ops.dna_dropout_keep(g2, 1235, p, H, T), keep)
    conv = _layer(C, H, G, "source_to_target", 21, dropout=p)
    real = ops.dropout_seed
    ops.dropout_seed = lambda device: 1234
    try:
        assert conv.training
        out, _ = _check_layer(conv, _x(T, C), edges, None, "dropout p=%g" % p, keep=keep.cpu(), p=p)
    finally:
        ops.dropout_seed = real
    conv.eval()
    plain = _layer(C, H, G, "source_to_target", 21).to(DEV)
    xd = _x(T, C).to(DEV)
    evaluated = conv(xd, edges.to(DEV))
    assert torch.equal(evaluated, plain(xd, edges.to(DEV))) and not torch.equal(evaluated, out)
    # the kernels under the mask, away from the layer: lse carries no dropout
    q, kv = torch.randn(N, C, device=DEV), torch.randn(N, 2, T, C, device=DEV)
    nd = torch.rand(ei2.shape[1], device=DEV) + 0.5
    o, lse = ops.dna_aggregate(g2.dst, q, kv[:, 0], kv[:, 1], nd, H, p=p, seed=1234, want_lse=True)
    assert torch.equal(lse, ops.dna_aggregate(g2.dst, q, kv[:, 0], kv[:, 1], nd, H, want_lse=True)[1])
    ref = R.attention(q.cpu(), kv[:, 0].cpu(), kv[:, 1].cpu(), nd.cpu(), ei2[1], ei2[0], N, H, keep.cpu(), p)
    ref_abs = R.attention_abs(q.cpu(), kv[:, 0].cpu(), kv[:, 1].cpu(), nd.cpu(), ei2[1], ei2[0], N, H, keep.cpu(), p)
    R.assert_bound(o, ref, ref_abs, "kernel under dropout p=%g" % p)


def test_layer_draws_a_fresh_seed_per_call(edges):
    conv = _layer(12, 4, 2, "source_to_target", 23, dropout=0.5).to(DEV)
    x, ei = _x(3, 12).to(DEV), edges.to(DEV)
    torch.cuda.manual_seed(7)
    a, b = conv(x, ei), conv(x, ei)
    torch.cuda.manual_seed(7)
    c = conv(x, ei)
    assert torch.equal(a, c) and not torch.equal(a, b)


# 4. bit-exact plumbing ------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 3, 7])
def test_forward_bit_exact_on_zero_scores(edges, graph, task_graphs, T):
    """K = 0 makes every score 0 and a = 1 / (T + 1), a power of two; integer V in
    [-3, 3] and norm in {1, 2}: every product and every partial sum of the 700-slot
    row (at most 700 * 2 * 3 * 7 < 2^24) is exact in fp32 in any order, so out
    equals the restatement bit for bit, walked by rows and by tasks."""
    from mi355_mp import ops
    H, d = 4, 6
    C = H * d
    g = torch.Generator().manual_seed(9 + T)
    E = edges.shape[1]
    nrm = torch.randint(1, 3, (E,), generator=g).float()
    v = torch.randint(-3, 4, (N, T, C), generator=g).float()
    q = torch.randn(N, C, generator=g)
    k = torch.zeros(N, T, C)
    ref = R.attention(q, k, v, nrm, edges[1], edges[0], N, H)
    out, lse = ops.dna_aggregate(graph.dst, q.to(DEV), k.to(DEV), v.to(DEV), nrm.to(DEV), H, want_lse=True)
    assert torch.equal(out.cpu().double(), ref)
    assert torch.equal(ops.dna_aggregate(task_graphs[0].dst, q.to(DEV), k.to(DEV), v.to(DEV), nrm.to(DEV), H), out)
    assert float((lse.cpu().double() - math.log(T + 1.0)).abs().max()) <= 2e-7 * math.log(T + 1.0)   # m = 0, l = T + 1
    assert float(ref.abs().max()) > 10.0


# 5. determinism, skipped launches --------------------------------------------------

def test_two_runs_bitwise_equal(edges):
    from mi355_mp import ops
    ei = edges.to(DEV)
    x = _x(5, 32, seed=21)
    for p in (0.0, 0.5):
        conv = _layer(32, 8, 16, "source_to_target", 21, dropout=p).to(DEV)
        real = ops.dropout_seed
        ops.dropout_seed = lambda device: 99
        runs = []
        try:
            for _ in range(2):
                conv.zero_grad()
                xd = x.to(DEV).requires_grad_(True)
                o = conv(xd, ei)
                o.square().sum().backward()
                runs.append([o.detach().clone(), xd.grad.clone()] + [q.grad.clone() for q in conv.parameters()])
        finally:
            ops.dropout_seed = real
        assert len(runs[0]) == 8
        for a, b in zip(*runs):
            assert torch.equal(a, b), p


def test_gradient_launches_are_skipped_when_nothing_needs_them(edges):
    """d Q comes from the destination pass, d K and d V from the source pass: with x
    frozen, freezing lin_k and lin_v skips the source pass, freezing lin_q the
    destination pass; with x trainable both run."""
    from mi355_mp import ops
    conv = _layer(12, 4, 2, "source_to_target", 17).to(DEV)
    mh = conv.multi_head
    calls = []
    real_dst, real_src = ops.dna_backward_dst, ops.dna_backward_src
    ops.dna_backward_dst = lambda *a, **k: calls.append("dst") or real_dst(*a, **k)
    ops.dna_backward_src = lambda *a, **k: calls.append("src") or real_src(*a, **k)

    def freeze(q, kv):
        for lin, on in ((mh.lin_q, q), (mh.lin_k, kv), (mh.lin_v, kv)):
            for prm in lin.parameters():
                prm.requires_grad_(on)
                prm.grad = None

    try:
        ei = edges.to(DEV)
        x = _x(3, 12).to(DEV)
        freeze(True, False)
        conv(x, ei).square().sum().backward()
        assert calls == ["dst"] and mh.lin_q.weight.grad is not None and mh.lin_k.weight.grad is None
        del calls[:]
        freeze(False, True)
        conv(x, ei).square().sum().backward()
        assert calls == ["src"] and mh.lin_q.weight.grad is None and mh.lin_v.bias.grad is not None
        del calls[:]
        freeze(False, False)
        xd = x.clone().requires_grad_(True)
        conv(xd, ei).square().sum().backward()
        assert sorted(calls) == ["dst", "src"] and xd.grad is not None and mh.lin_k.weight.grad is None
        del calls[:]
        with torch.no_grad():
            conv(x, ei)
        assert calls == []
    finally:
        ops.dna_backward_dst, ops.dna_backward_src = real_dst, real_src


# 6. no per-edge array ------------------------------------------------------------------

def _peak_growth(run):
    run()                                                             # builds and caches the CSRs and the norm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_no_per_edge_history_array(edges):
    """C = 128, T = 5, H = 8, G = 16 (the example's layer): one [E, T, C] fp32 array of
    the ~4300 normalised edges is 11 MB; upstream holds three of them before the
    attention starts.  The fused path's own tensors, from their shapes -- Q, d Q,
    out, its gradient twice [N, C], K, V, d K, d V [N, T, C], lse [E, H] and the three
    slabs of the 64-unit task schedule (two slots per task) -- come to
    under half of one; forward + backward (the grouped Linears' node-level
    temporaries included) must peak below the one array."""
    T, C, H, G = 5, 128, 8, 16
    conv = _layer(C, H, G, "source_to_target", 31).to(DEV)
    xd = _x(T, C).to(DEV).requires_grad_(True)
    ei = edges.to(DEV)
    E2 = R.gcn_norm(edges, N)[0].shape[1]

    def run():
        conv.zero_grad()
        xd.grad = None
        conv(xd, ei).square().sum().backward()

    from mi355_mp import _lib, ops
    per_edge = E2 * T * C * 4
    assert ops.dna_target_tasks(N, E2) == (N + E2) // 64             # the layer's schedule: 64-unit tasks
    n_waves = int(_lib.native().mp_schedule_n_waves(N, E2, 64))      # of the destination and of the source CSR
    assert n_waves >= (N + E2) // 64
    slabs = 2 * n_waves * (2 * C + 2 * T * C)                        # forward, d Q; d K | d V
    own = 4 * (5 * N * C + 4 * N * T * C + E2 * H + slabs)
    assert 2 * own < per_edge
    growth = _peak_growth(run)
    print("peak growth %d bytes, own tensors %d, one [E, T, C] array %d bytes" % (growth, own, per_edge))
    assert growth < per_edge


# 7. the example ------------------------------------------------------------------

def test_example_dna():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dna.py"), "--nodes", "2708", "--epochs", "30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(line.split("loss")[1].split(",")[0]) for line in r.stdout.splitlines() if "loss" in line]
    assert len(losses) == 30 and all(math.isfinite(v) for v in losses), losses
    assert sum(losses[-3:]) / 3 < sum(losses[:3]) / 3, losses
