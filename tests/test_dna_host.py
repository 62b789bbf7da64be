"""CPU tests of the DNAConv feature: hand values and committed known answers of
the float64 restatement (tests/_dna_ref.py) that the GPU tests check the
kernels against, the two identities the fused path rests on (node-level
projections; the restricted softmax as an ordinary softmax over {0, s}), the
backward the kernels implement against autograd, the layer's host-side pieces
(parameter names, shapes, reset bounds, repr, errors, the fused-path predicate,
upstream's message on CPU tensors), and the C-ABI's rejection of every bad
argument of the DNA entry points -- from Python with fake device pointers and
from a C harness under the host-ASAN build of the library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _dna_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


# ---- the restatement ----------------------------------------------------------

def test_restatement_hand_values():
    """Three nodes, C = 2, one head (d = 2), T = 2, edges 0 -> 1 and 2 -> 1, identity
    projections.  r = sqrt(2), E = exp(-r)."""
    r = math.sqrt(2.0)
    ex = math.exp(-r)
    ei = torch.tensor([[0, 2], [1, 1]])
    q = torch.tensor([[0.0, 0.0], [2.0, 0.0], [0.0, 0.0]])
    k = torch.tensor([[[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]], [[-1.0, 0.0], [-1.0, 5.0]]])
    v = torch.tensor([[[1.0, 0.0], [0.0, 1.0]], [[9.0, 9.0], [9.0, 9.0]], [[3.0, 0.0], [0.0, 4.0]]])
    one = torch.ones(2)
    # edge 0 -> 1: s = (r, 0), m = r: a = (1, E) / (1 + E + E)
    # edge 2 -> 1: s = (-r, -r), all negative: m = 0, a = E / (2 E + 1) each -- not 1/2: the exp(-m) term
    a0, a1 = 1.0 / (1.0 + 2.0 * ex), ex / (1.0 + 2.0 * ex)
    b = ex / (2.0 * ex + 1.0)
    assert abs(b - 1.0 / (2.0 + math.exp(r))) < 1e-16 and b < 0.2
    out = R.attention(q, k, v, one, ei[1], ei[0], 3, 1)
    want = torch.tensor([[0.0, 0.0], [a0 + 3.0 * b, a1 + 4.0 * b], [0.0, 0.0]], dtype=torch.float64)
    assert float((out - want).abs().max()) < 1e-15
    s = R.scores(q.double(), k.double(), ei[1], ei[0], 1)
    assert float((s - torch.tensor([[[r, 0.0]], [[-r, -r]]], dtype=torch.float64)).abs().max()) < 1e-15
    for f in (R.softmax_clamp, R.softmax_extended):
        a = f(s)
        assert float((a - torch.tensor([[[a0, a1]], [[b, b]]], dtype=torch.float64)).abs().max()) < 1e-15
        assert float(a[1].sum()) < 0.4                                  # the restricted softmax does not sum to 1
    # norm scales a message; a dropped entry leaves, a kept one is scaled by 1 / (1 - p)
    out = R.attention(q, k, v, torch.tensor([2.0, 0.5]), ei[1], ei[0], 3, 1)
    assert float((out[1] - torch.tensor([2 * a0 + 1.5 * b, 2 * a1 + 2.0 * b], dtype=torch.float64)).abs().max()) < 1e-15
    keep = torch.tensor([[[True, False]], [[False, True]]])
    out = R.attention(q, k, v, one, ei[1], ei[0], 3, 1, keep=keep, p=0.75)
    assert float((out[1] - torch.tensor([4 * a0, 16.0 * b], dtype=torch.float64)).abs().max()) < 1e-15
    # sum |terms|: |v| under the same coefficients
    out = R.attention_abs(q, k, -v, -one, ei[1], ei[0], 3, 1)
    assert float((out - want).abs().max()) < 1e-15
    # two heads of width 1: each channel is its own head, d = 1
    out = R.attention(q, k, v, one, ei[1], ei[0], 3, 2)
    e2 = math.exp(-2.0)
    # head 0: edge 0: s = (2, 0) -> a = (1, e2) / (1 + 2 e2); edge 2: s = (-2, -2) -> a = e2 / (2 e2 + 1)
    # head 1: q = 0: s = 0 -> a = 1 / 3 everywhere
    assert abs(float(out[1, 0]) - (1.0 / (1.0 + 2.0 * e2) + 3.0 * e2 / (2.0 * e2 + 1.0))) < 1e-15
    assert abs(float(out[1, 1]) - (1.0 / 3.0 + 4.0 / 3.0)) < 1e-15
    # the loop with identity weights is the same computation
    eye = torch.eye(2).view(1, 2, 2)
    x = torch.stack([v[0], torch.tensor([[7.0, 7.0], [2.0, 0.0]]), v[2]])
    lo = R.dna_conv_loop(x, ei, one, {"wq": eye, "wk": eye, "wv": eye}, 1)
    assert float((lo - R.dna_conv(x, ei, one, {"wq": eye, "wk": eye, "wv": eye}, 1)).abs().max()) < 1e-15


def test_gcn_norm_hand_values():
    """Edges 0 -> 1 (w 2), 1 -> 1 (w 3), 1 -> 1 (w 5), 2 -> 0 (w 1), n = 3: the loops are
    dropped and re-added at the end, node 1 keeping the LAST loop's weight."""
    ei = torch.tensor([[0, 1, 1, 2], [1, 1, 1, 0]])
    w = torch.tensor([2.0, 3.0, 5.0, 1.0])
    ei2, norm = R.gcn_norm(ei, 3, w)
    assert ei2.tolist() == [[0, 2, 0, 1, 2], [1, 0, 0, 1, 2]]
    deg = [2.0 + 1.0, 5.0, 1.0 + 1.0]                                   # over row: w2 = (2, 1, 1, 5, 1)
    want = [2.0 / math.sqrt(deg[0] * deg[1]), 1.0 / math.sqrt(deg[2] * deg[0]), 1.0 / deg[0], 5.0 / deg[1], 1.0 / deg[2]]
    assert float((norm - torch.tensor(want, dtype=torch.float64)).abs().max()) < 1e-15
    # unweighted: deg = (2, 1, 2)
    assert float((R.gcn_norm(ei, 3)[1] - torch.tensor([1 / math.sqrt(2.0), 1 / 2.0, 1 / 2.0, 1.0, 1 / 2.0],
                                                      dtype=torch.float64)).abs().max()) < 1e-15


def _case(seed, n, E, T, C, G, bias=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, E), generator=g)
    prm = {}
    for name in ("wq", "wk", "wv"):
        prm[name] = torch.randn(G, C // G, C // G, generator=g) / math.sqrt(C // G)
    for name in ("bq", "bk", "bv"):
        prm[name] = torch.randn(C, generator=g) if bias else None
    return ei, torch.rand(E, generator=g) + 0.5, torch.randn(n, T, C, generator=g), prm


@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (3, 6, 2, 1), (4, 12, 3, 2), (2, 8, 8, 4), (5, 6, 1, 6)])
@pytest.mark.parametrize("drop", [False, True])
def test_recipe_factored_form_and_loop_agree(shape, drop):
    """Upstream's per-edge recipe (gather, project per edge, clamp softmax) equals the
    node-level factored form equals the literal loop, to 1e-12, in both flows."""
    T, C, H, G = shape
    n, E = 8, 40
    ei, norm, x, prm = _case(100 * T + C, n, E, T, C, G, bias=C != 8)
    keep = (torch.rand(E, H, T, generator=torch.Generator().manual_seed(5)) >= 0.5) if drop else None
    for flow in ("source_to_target", "target_to_source"):
        a = R.dna_conv_recipe(x, ei, norm, prm, H, flow, keep, 0.5)
        b = R.dna_conv(x, ei, norm, prm, H, flow, keep, 0.5)
        c = R.dna_conv_loop(x, ei, norm, prm, H, flow, keep, 0.5)
        assert float((a - b).abs().max()) <= 1e-12 and float((a - c).abs().max()) <= 1e-12, flow


@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (4, 12, 3, 2), (2, 8, 8, 4)])
@pytest.mark.parametrize("drop", [False, True])
def test_backward_formulas_are_the_recipes_autograd(shape, drop):
    """d Q, d K, d V as the kernels compute them (a recomputed; the plain softmax
    backward over the T real logits) carried through the Linears equal autograd
    through upstream's per-edge recipe: every gradient to 1e-12."""
    T, C, H, G = shape
    n, E = 8, 40
    ei, norm, x, prm = _case(7 * T + C, n, E, T, C, G)
    keep = (torch.rand(E, H, T, generator=torch.Generator().manual_seed(6)) >= 0.5) if drop else None
    gout = torch.randn(n, C, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    leaves = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    xr = x.double().requires_grad_(True)
    (R.dna_conv_recipe(xr, ei, norm, leaves, H, "source_to_target", keep, 0.5) * gout).sum().backward()
    q, k, v = R.project(xr, leaves)
    dq, dk, dv = R.attention_backward(q.detach(), k.detach(), v.detach(), norm, ei[1], ei[0], n, H, gout, keep, 0.5)
    want = {n_: t.grad.clone() for n_, t in leaves.items()}
    want["x"] = xr.grad.clone()
    for t in list(leaves.values()) + [xr]:
        t.grad = None
    ((q * dq).sum() + (k * dk).sum() + (v * dv).sum()).backward()
    for name, t in list(leaves.items()) + [("x", xr)]:
        assert float((t.grad - want[name]).abs().max()) <= 1e-12, name
    # and `layer` returns the same
    _, grads = R.layer(x, ei, norm, prm, H, keep=keep, p=0.5, gout=gout)
    for name in want:
        assert float((grads[name] - want[name]).abs().max()) <= 1e-12, name


def test_absolute_mode_bounds_every_term():
    """sum |terms| dominates the signed value, equals it when every leaf is positive
    (a's own nonlinearity aside: the scores stay the signed ones), and |ds| is taken
    as a (|d alpha| + sum a |d alpha|)."""
    T, C, H, G = 3, 8, 2, 2
    n, E = 8, 40
    ei, norm, x, prm = _case(11, n, E, T, C, G)
    gout = torch.randn(n, C, generator=torch.Generator().manual_seed(3))
    out, grads = R.layer(x, ei, norm, prm, H, gout=gout)
    sc_out, sc = R.layer(x, ei, norm, prm, H, gout=gout, absolute=True)
    assert bool((sc_out >= out.abs() - 1e-12).all())
    assert sorted(sc) == sorted(grads) == sorted(["x"] + list(R.PARAMS))
    for name in grads:
        assert bool((sc[name] >= grads[name].abs() - 1e-12).all()), name
    q, k, v = R.project(x.double(), {n_: p.double() for n_, p in prm.items()})
    dq, dk, dv = R.attention_backward(q, k, v, norm, ei[1], ei[0], n, H, gout)
    aq, ak, av = R.attention_backward(q, k, v, norm, ei[1], ei[0], n, H, gout, absolute=True)
    for a, s in ((dq, aq), (dk, ak), (dv, av)):
        assert bool((s >= a.abs() - 1e-12).all())
    pq, pk, pv = R.attention_backward(q, k, v.abs(), norm, ei[1], ei[0], n, H, gout.abs())
    assert float((pv - av).abs().max()) <= 1e-12                        # d V has no cancellation to lose


def test_restatement_matches_the_committed_known_answers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_dna",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_dna.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    kat = np.load(os.path.join(ROOT, "tests", "golden", "dna", "dna_kat.npz"))
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t)
    assert len(got) == 16
    for k, v in got.items():
        assert v.dtype == torch.float64 and np.abs(v.numpy() - kat[k]).max() <= 1e-13, k


# ---- the layer's host side ------------------------------------------------------

def test_layer_parameters_repr_and_init_bounds():
    from torch_geometric.nn import DNAConv
    import torch_geometric.nn.conv as conv
    from torch_geometric.nn.conv import dna_conv as mod
    from torch_geometric.nn.inits import kaiming_uniform
    assert conv.DNAConv is DNAConv and "DNAConv" in conv.__all__
    torch.manual_seed(0)
    c = DNAConv(128, heads=8, groups=16, dropout=0.8, cached=True)
    assert repr(c) == "DNAConv(128, heads=8, groups=16)"
    assert c.aggr == "add" and c.flow == "source_to_target" and c.cached and c.cached_result is None
    names = sorted(n for n, _ in c.named_parameters())
    assert names == ["multi_head.lin_%s.%s" % (l, p) for l in "kqv" for p in ("bias", "weight")]
    assert sorted(c.state_dict()) == names
    mh = c.multi_head
    assert isinstance(mh, mod.MultiHead) and isinstance(mh, mod.Attention) and isinstance(mh.lin_q, mod.Linear)
    assert (mh.in_channels, mh.out_channels, mh.heads, mh.groups, mh.dropout) == (128, 128, 8, 16, 0.8)
    bound = 1.0 / math.sqrt(128 // 16)          # kaiming_uniform(fan = in / G, a = sqrt(5)) = uniform(in / G)
    for lin in (mh.lin_q, mh.lin_k, mh.lin_v):
        assert lin.weight.shape == (16, 8, 8) and lin.bias.shape == (128,)
        for p in (lin.weight, lin.bias):
            top = float(p.detach().abs().max())
            assert 0.5 * bound < top <= bound
    w = torch.empty(1000)
    kaiming_uniform(w, fan=3, a=1.0)
    assert 0.9 < float(w.abs().max()) <= 1.0    # sqrt(6 / ((1 + 1) * 3)) = 1
    kaiming_uniform(None, fan=3, a=1.0)
    c = DNAConv(6, bias=False, flow="target_to_source")
    assert repr(c) == "DNAConv(6, heads=1, groups=1)" and c.flow == "target_to_source"
    assert sorted(n for n, _ in c.named_parameters()) == ["multi_head.lin_%s.weight" % l for l in "kqv"]
    assert c.multi_head.lin_q.weight.shape == (1, 6, 6) and c.multi_head.lin_q.bias is None
    with pytest.raises(AssertionError):
        DNAConv(6, heads=4)                     # channels % heads
    with pytest.raises(AssertionError):
        DNAConv(6, groups=4)                    # channels % groups
    with pytest.raises(TypeError):
        DNAConv(6, aggr="mean")                 # aggregation is "add", as upstream
    # the grouped Linear is block-diagonal; restricted_softmax is the clamp form
    lin = mod.Linear(6, 4, groups=2)
    xs = torch.randn(5, 3, 6)
    want = R.linear(xs.double(), lin.weight.detach().double(), lin.bias.detach().double())
    assert float((lin(xs).detach().double() - want).abs().max()) < 1e-5
    blk = torch.cat([xs[..., :3] @ lin.weight[0], xs[..., 3:] @ lin.weight[1]], dim=-1) + lin.bias
    assert float((lin(xs) - blk).detach().abs().max()) < 1e-5
    s = torch.randn(4, 2, 1, 5, dtype=torch.float64)
    assert float((mod.restricted_softmax(s) - R.softmax_extended(s)).abs().max()) < 1e-15


def test_forward_errors():
    from torch_geometric.nn import DNAConv
    c = DNAConv(4, cached=True)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match=r"\[num_nodes, num_layers, channels\]"):
        c(torch.ones(2, 4), ei)
    with pytest.raises(ValueError):
        c(torch.ones(2, 1, 2, 4), ei)
    # the cache holds the first call's edge count
    c.cached_result, c.cached_num_edges = (ei, torch.ones(2)), 2
    with pytest.raises(RuntimeError, match="Cached 2 number of edges, but found 3"):
        c(torch.ones(2, 3, 4), torch.tensor([[0, 1, 1], [1, 0, 1]]))
    c.reset_parameters()
    assert c.cached_result is None and c.cached_num_edges is None
    # host tensors: the normalisation and the aggregation have no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(torch.ones(2, 3, 4), ei)


def test_fused_path_predicate(lib):
    from torch_geometric.nn import DNAConv
    from mi355_mp import ops
    assert DNAConv(8, heads=2).fused_layer()
    assert DNAConv(8, heads=2, groups=4, bias=False, flow="target_to_source").fused_layer()
    assert not DNAConv(8, node_dim=1).fused_layer()

    class Doubled(DNAConv):
        def message(self, x_i, x_j, norm):
            return 2 * super().message(x_i, x_j, norm)

    class Shifted(DNAConv):
        def update(self, aggr_out):
            return aggr_out + 1

    class Mean(DNAConv):
        def aggregate(self, inputs, index, dim_size):
            return super().aggregate(inputs, index, dim_size)

    assert not Doubled(8).fused_layer() and not Shifted(8).fused_layer() and not Mean(8).fused_layer()
    # host tensors never take the fused path
    c = DNAConv(8, heads=2)
    ei = torch.tensor([[0, 1], [1, 0]])
    assert not c._fused_ok(torch.ones(2, 3, 8), ei, torch.ones(2))
    # the limits: T * ceil(d / 64) <= 48, d <= 256, C % H == 0
    assert ops.dna_ok(5, 8, 128) and ops.dna_ok(48, 8, 128) and not ops.dna_ok(49, 8, 128)
    assert ops.dna_max_layers(8, 128) == 48 and ops.dna_max_layers(1, 130) == 16 and ops.dna_max_layers(1, 65) == 24
    assert ops.dna_max_layers(1, 256) == 12 and ops.dna_max_layers(1, 257) == 0 and ops.dna_max_layers(3, 8) == 0
    for H, C in ((8, 128), (1, 130), (16, 16), (3, 66), (1, 256)):
        T = ops.dna_max_layers(H, C)
        assert ops.dna_ok(T, H, C) and not ops.dna_ok(T + 1, H, C), (H, C)
    # the layer's schedule: tasks of max(64, the default chunk) units, so long rows are split at any size
    from mi355_mp.graph import auto_chunk
    assert ops.dna_split_chunk() == 64
    for n, e in ((300, 4300), (2708, 13264), (10, 20), (100000, 1099710), (2000000, 60000000)):
        t = ops.dna_target_tasks(n, e)
        if auto_chunk(n, e) >= 64:
            assert t is None
        else:
            assert t == max((n + e) // 64, 1) and auto_chunk(n, e, t) == (64 if n + e >= 64 else 16)
    assert not ops.dna_ok(0, 1, 1) and not ops.dna_ok(1, 0, 1) and not ops.dna_ok(1, 1, 0) and not ops.dna_ok(1, 3, 8)


def test_message_on_cpu_tensors_matches_the_restatement():
    """The layer itself raises on CPU tensors (test_forward_errors: GCNConv.norm and
    propagate are device-only in this project), so "the layer on CPU tensors" is
    checked as far as it exists there: its message() called on CPU tensors.
    Upstream's message is plain torch: on CPU tensors, with the sum over the
    edges done by index_add, it is the restatement (groups, heads, bias or not,
    eval and -- p = 0 -- training)."""
    from torch_geometric.nn import DNAConv
    n, E = 9, 50
    for T, C, H, G, bias in ((3, 12, 4, 2, True), (1, 8, 8, 4, False), (4, 6, 1, 1, True)):
        ei, norm, x, _ = _case(3 * T + C, n, E, T, C, G)
        torch.manual_seed(1)
        c = DNAConv(C, heads=H, groups=G, bias=bias).double()
        mh = c.multi_head
        prm = {"w" + l: getattr(mh, "lin_" + l).weight.detach() for l in "qkv"}
        prm.update({"b" + l: (getattr(mh, "lin_" + l).bias.detach() if bias else None) for l in "qkv"})
        xd = x.double()
        for flow in ("source_to_target", "target_to_source"):
            dst, src = R._ends(ei, flow)
            msg = c.message(xd[dst], xd[src], norm.double())
            out = torch.zeros(n, C, dtype=torch.float64).index_add(0, dst, msg)
            want = R.dna_conv(x, ei, norm, prm, H, flow)
            assert float((out.detach() - want).abs().max()) <= 1e-12, (T, C, H, G, flow)
    c.multi_head.dropout = 1.0                  # training, p = 1: F.dropout zeroes every coefficient
    assert float(c.message(xd[dst], xd[src], norm.double()).detach().abs().max()) == 0.0


def test_no_cpu_fallback_and_documented_refusals(lib):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    ei = torch.tensor([[0, 1], [1, 0]])
    g = Graph(ei, 2, 2)
    q, k = torch.ones(2, 4), torch.ones(2, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dna_propagate(g, q, k, k, torch.ones(2), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dna_propagate(g, q, k, k, None, 2)


# ---- the C-ABI rejects every bad argument before any launch -------------------

def test_dna_entry_points_reject_bad_arguments(lib):
    from mi355_mp import _lib
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    N, M, E, T, H, C = 257, 300, 3000, 5, 3, 66
    RW = T * C
    QN, QM, KN, KM, LB = N * C * 4, M * C * 4, N * RW * 4, M * RW * 4, E * H * 4

    def csr(**kw):
        f = dict(rowptr=D, col=D, eid=D, n_rows=N, n_cols=M, n_ids=0)
        f.update(kw)
        return _lib.MpCsr(f["rowptr"], f["col"], f["eid"], None, None, None, f["n_rows"], E, 0, 0, 0, f["n_cols"],
                          f["n_ids"])

    g = csr()

    def agg(g=g, q=D, ldq=C, qb=QN, k=D, ldk=RW, kb=KM, v=D, ldv=RW, vb=KM, nrm=D, nn=E, T_=T, H_=H, C_=C, p=0.0,
            out=D, ldo=C, ob=QN, lse=D, lb=LB, ws=None, wsb=0):
        return lib.mp_dna_aggregate_f32(g, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, T_, H_, C_, 7, p, out, ldo, ob,
                                        lse, lb, ws, wsb, None)

    def dst(g=g, q=D, ldq=C, qb=QN, k=D, ldk=RW, kb=KM, v=D, ldv=RW, vb=KM, nrm=D, nn=E, go=D, ldg=C, gb=QN, lse=D,
            lb=LB, T_=T, H_=H, C_=C, p=0.0, out=D, ldo=C, ob=QN, ws=None, wsb=0):
        return lib.mp_dna_backward_dst_f32(g, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_,
                                           C_, 7, p, out, ldo, ob, ws, wsb, None)

    def src(g=g, q=D, ldq=C, qb=QM, k=D, ldk=RW, kb=KN, v=D, ldv=RW, vb=KN, nrm=D, nn=E, go=D, ldg=C, gb=QM, lse=D,
            lb=LB, T_=T, H_=H, C_=C, p=0.0, dk=D, lddk=RW, dkb=KN, dv=D, lddv=RW, dvb=KN, ws=None, wsb=0):
        return lib.mp_dna_backward_src_f32(g, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_,
                                           C_, 7, p, dk, lddk, dkb, dv, lddv, dvb, ws, wsb, None)

    def rejected(fn, kw, needle):
        rc = fn(**kw)
        err = lib.mp_last_error().decode()
        assert rc == -1 and needle in err, (fn.__name__, kw, rc, err)

    common = [(dict(g=None), "g is NULL"), (dict(q=None), "q is NULL"), (dict(k=None), "k is NULL"),
              (dict(v=None), "v is NULL"), (dict(ldq=C - 1), "ld of q = %d" % (C - 1)),
              (dict(ldk=RW - 1), "ld of k = %d" % (RW - 1)), (dict(ldv=RW - 1), "ld of v = %d" % (RW - 1)),
              (dict(nn=E - 1), "n_norm = %d" % (E - 1)), (dict(lb=LB - 1), "lse holds %d bytes, the call needs %d" % (LB - 1, LB)),
              (dict(T_=0), "T = 0"), (dict(H_=0), "H = 0"), (dict(C_=0), "C = 0"), (dict(H_=4), "no multiple"),
              (dict(T_=49, ldk=49 * C, ldv=49 * C, kb=1 << 40, vb=1 << 40), "above the limit"),
              (dict(p=1.0), "dropout p"), (dict(p=-0.1), "dropout p"),
              (dict(g=csr(col=None)), "col is NULL"), (dict(g=csr(eid=None)), "eid is NULL"),
              (dict(g=csr(rowptr=None)), "rowptr is NULL"), (dict(g=csr(n_cols=0)), "n_cols"),
              (dict(g=csr(n_ids=E + 1)), "n_norm")]
    for fn in (agg, dst, src):
        for kw, needle in common:
            rejected(fn, kw, needle)
    for fn in (agg, dst):
        rejected(fn, dict(qb=QN - 1), "q holds %d bytes, the call needs %d" % (QN - 1, QN))
        rejected(fn, dict(kb=KM - 1), "k holds %d bytes, the call needs %d" % (KM - 1, KM))
        rejected(fn, dict(vb=KN), "v holds")
        rejected(fn, dict(out=None), "%s is NULL" % ("out" if fn is agg else "dq"))
        rejected(fn, dict(ldo=C - 1), "ld of %s = %d" % ("out" if fn is agg else "dq", C - 1))
        rejected(fn, dict(ob=QN - 1), "%s holds" % ("out" if fn is agg else "dq"))
        rejected(fn, dict(ldo=C + 1), "%s holds" % ("out" if fn is agg else "dq"))
    for fn in (dst, src):
        rejected(fn, dict(lse=None), "lse is NULL")
        rejected(fn, dict(go=None), "gout is NULL")
        rejected(fn, dict(ldg=C - 1), "ld of gout")
    rejected(dst, dict(gb=QN - 1), "gout holds")
    rejected(src, dict(gb=QM - 1), "gout holds")
    rejected(src, dict(qb=QN), "q holds")                              # q by column: M rows
    rejected(src, dict(kb=KN - 1), "k holds")
    for name in ("dk", "dv"):
        rejected(src, {name: None}, "%s is NULL" % name)
        rejected(src, {"ld" + name: RW - 1}, "ld of %s" % name)
        rejected(src, {name + "b": KN - 1}, "%s holds %d bytes, the call needs %d" % (name, KN - 1, KN))
    # a CSR with a schedule of chunk >= mp_dna_split_chunk() is walked by tasks: the schedule arrays and the slab
    # (two slots per task; C floats a slot, 2 T C for the source backward) are then required
    assert lib.mp_dna_split_chunk() == 64
    NW = 40

    def sched(chunk=64, wave_row=D, wave_slot=D, split=D, n_waves=NW, n_split=3):
        return _lib.MpCsr(D, D, D, wave_row, wave_slot, split, N, E, chunk, n_waves, n_split, M, 0)

    small, large = lib.mp_dna_workspace(g, C), lib.mp_dna_workspace(sched(), C)
    assert large >= 2 * NW * C * 4 > small and lib.mp_dna_workspace(sched(chunk=32), C) == small
    assert lib.mp_dna_workspace(sched(wave_row=None), C) == small and lib.mp_dna_workspace(None, C) == small
    assert lib.mp_dna_workspace(sched(), 2 * RW) >= 2 * NW * 2 * RW * 4
    for fn, need in ((agg, large), (dst, large), (src, lib.mp_dna_workspace(sched(), 2 * RW))):
        rejected(fn, dict(g=sched(), ws=None, wsb=need), "ws is NULL")
        rejected(fn, dict(g=sched(), ws=D, wsb=need - 1), "ws holds %d bytes, the call needs %d" % (need - 1, need))
        rejected(fn, dict(g=sched(wave_slot=None), ws=D, wsb=need), "wave_slot is NULL")
        rejected(fn, dict(g=sched(split=None), ws=D, wsb=need), "split_waves is NULL")
        rejected(fn, dict(g=sched(n_waves=0), ws=D, wsb=need), "n_waves = 0")
        rejected(fn, dict(g=sched(n_split=NW + 1), ws=D, wsb=need), "n_split = %d" % (NW + 1))
    rejected(src, dict(g=sched(), ws=D, wsb=large), "ws holds")        # sized for the forward
    # K | V halves of one buffer [M, 2, T, C]: the extents run from each pointer on.  (The calls that pass every
    # check are made by the C harness only, where no device is visible: here they would launch on fake pointers.)
    rejected(agg, dict(ldk=2 * RW, ldv=2 * RW, kb=2 * KM, vb=2 * KM - RW * 4 - 1), "v holds")

    def keep(seed=1, p=0.5, H_=H, T_=T, ne=E, out=D, ob=E * H * T):
        return lib.mp_dna_dropout_keep(seed, p, H_, T_, ne, out, ob, None)

    for kw, needle in [(dict(p=0.0), "dropout p"), (dict(p=1.0), "dropout p"), (dict(H_=0), "H = 0"),
                       (dict(T_=0), "T = 0"), (dict(ne=-1), "n_edges"), (dict(out=None), "keep is NULL"),
                       (dict(ob=E * H * T - 1), "keep holds %d bytes, the call needs %d" % (E * H * T - 1, E * H * T)),
                       (dict(H_=1 << 20, T_=1 << 20, ob=1 << 60), "too large")]:
        rejected(keep, kw, needle)
    assert keep(ne=0, out=None, ob=0) == 0                             # nothing to write: no launch
    assert lib.mp_dna_ok(5, 8, 128) == 1 and lib.mp_dna_ok(49, 8, 128) == 0 and lib.mp_dna_max_layers(8, 128) == 48
    # the int64 returns are outside the symbols the raising view wraps: ops tests the sign
    for name in ("mp_dna_ok", "mp_dna_max_layers", "mp_dna_split_chunk", "mp_dna_aggregate_f32", "mp_dna_backward_dst_f32",
                 "mp_dna_backward_src_f32", "mp_dna_dropout_keep"):
        assert _lib.SIGNATURES[name][0] is _lib.i64 and name not in _lib.STATUS_RETURNING
    assert _lib.ABI_VERSION == 7 and lib.mp_abi_version() == 7
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match=r"mp_dna_dropout_keep failed \(code 1\): .*keep holds"):
        ops._count_call(_lib.native(), "mp_dna_dropout_keep", 1, 0.5, H, T, E, D, 3, None)


def test_dna_abi_rejections_under_asan():
    """tests/abi/abi_reject_dna.c against the host-AddressSanitizer build of the
    library (make asan_dna), run as a plain program: every rejection names its
    argument and the exact documented boundaries pass the checks."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_dna"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_dna")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_dna: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 109, r.stdout[-2000:]
