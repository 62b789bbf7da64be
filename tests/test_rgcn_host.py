"""CPU tests of the RGCNConv feature: hand values and committed known answers of
the float64 restatement (tests/_rgcn_ref.py) that the GPU tests check the
kernels against, the factorisation identity the fused path rests on, the
layer's host-side pieces (parameters, repr, the fused-path predicate, the form
chooser, upstream's message / update on CPU tensors), and the C-ABI's rejection
of every bad argument of the RGCN entry points -- from Python with fake device
pointers and from a C harness under the host-ASAN build of the library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _rgcn_ref as R

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
    """Three nodes, edges 0 -> 1 (type 0), 0 -> 1 (type 1), 2 -> 1 (type 1), Cin = 2,
    Cout = 1, B = 2: basis[0] = (1, 2)^T, basis[1] = (10, 20)^T, att = [[1, 0], [1, 1]],
    so W_0 = (1, 2)^T and W_1 = (11, 22)^T."""
    ei = torch.tensor([[0, 0, 2], [1, 1, 1]])
    et = torch.tensor([0, 1, 1])
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.0, 1.0]])
    basis = torch.tensor([[[1.0], [2.0]], [[10.0], [20.0]]])
    att = torch.tensor([[1.0, 0.0], [1.0, 1.0]])
    # messages: x0 . W_0 = 5; x0 . W_1 = 55; x2 . W_1 = 22
    assert R.rgcn_conv(x, ei, et, None, basis, att).tolist() == [[0.0], [82.0], [0.0]]
    en = torch.tensor([2.0, 1.0, 0.5])
    assert R.rgcn_conv(x, ei, et, en, basis, att).tolist() == [[0.0], [10.0 + 55.0 + 11.0], [0.0]]
    root, bias = torch.tensor([[1.0], [1.0]]), torch.tensor([0.5])
    assert R.rgcn_conv(x, ei, et, None, basis, att, root, bias).tolist() == [[3.5], [84.5], [1.5]]
    assert R.rgcn_conv(x, ei, et, None, basis, att, flow="target_to_source").tolist() == [[1.0 + 11.0], [0.0],
                                                                                          [11.0]]
    # x = None: Cin = N = 3 nodes, the message is row j of W_t; basis_n [B, N, Cout]
    basis_n = torch.tensor([[[1.0], [2.0], [3.0]], [[10.0], [20.0], [30.0]]])
    assert R.rgcn_conv(None, ei, et, None, basis_n, att).tolist() == [[0.0], [1.0 + 11.0 + 33.0], [0.0]]
    root_n = torch.tensor([[100.0], [200.0], [300.0]])
    assert R.rgcn_conv(None, ei, et, en, basis_n, att, root_n, bias).tolist() == [[100.5], [2.0 + 11.0 + 16.5 + 200.5],
                                                                                  [300.5]]
    # the kernel contracts: Z [n, B, C]
    assert R.bins(ei[1], ei[0], 3, et, None, att, x)[1].tolist() == [[1.0 + 1.0 + 0.0, 2.0 + 2.0 + 1.0],
                                                                     [0.0 + 1.0 + 0.0, 0.0 + 2.0 + 1.0]]
    assert R.bins(ei[1], ei[0], 3, et, en, att, x)[1].tolist() == [[2.0 + 1.0, 4.0 + 2.0 + 0.5], [1.0, 2.0 + 0.5]]
    y = torch.tensor([[[1.0], [2.0]], [[0.0], [0.0]], [[3.0], [4.0]]])                 # [n, B = 2, F = 1]
    assert R.gather(ei[1], ei[0], 3, et, None, att, y).tolist() == [[0.0], [1.0 + 3.0 + 7.0], [0.0]]
    dz = torch.tensor([[[0.0, 0.0], [0.0, 0.0]], [[1.0, 2.0], [5.0, 7.0]], [[0.0, 0.0], [0.0, 0.0]]])
    # per edge <dz[1, b], x_j>: x0 -> (5, 19), x2 -> (2, 7); relation 0 = edge 0, relation 1 = edges 1, 2
    assert R.att_grad(et, None, ei[1], ei[0], dz, x, 2).tolist() == [[5.0, 19.0], [7.0, 26.0]]
    assert R.att_grad(et, en, ei[1], ei[0], dz, x, 3).tolist() == [[10.0, 38.0], [6.0, 22.5], [0.0, 0.0]]


def _case(seed, n, E, NR, B, c_in, c_out):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, E), generator=g)
    return (ei, torch.randint(0, NR, (E,), generator=g), torch.rand(E, generator=g) + 0.5,
            torch.randn(n, c_in, generator=g), torch.randn(B, c_in, c_out, generator=g),
            torch.randn(NR, B, generator=g), torch.randn(c_in, c_out, generator=g), torch.randn(c_out, generator=g))


def test_restatement_is_the_per_edge_loop():
    ei, et, en, x, basis, att, root, bias = _case(3, 7, 40, 4, 3, 3, 2)
    g = torch.Generator().manual_seed(4)
    basis_n, root_n = torch.randn(3, 7, 2, generator=g), torch.randn(7, 2, generator=g)
    for flow in ("source_to_target", "target_to_source"):
        for norm in (None, en):
            out = R.rgcn_conv(x, ei, et, norm, basis, att, root, bias, flow)
            want = R.rgcn_conv_loop(x, ei, et, norm, basis, att, root, bias, flow)
            assert torch.allclose(out, want, rtol=0, atol=1e-12), (flow, norm is None)
            out = R.rgcn_conv(None, ei, et, norm, basis_n, att, root_n, bias, flow)
            want = R.rgcn_conv_loop(None, ei, et, norm, basis_n, att, root_n, bias, flow)
            assert torch.allclose(out, want, rtol=0, atol=1e-12), (flow, norm is None)
    assert torch.allclose(R.rgcn_conv(x, ei, et, None, basis, att), R.rgcn_conv_loop(x, ei, et, None, basis, att),
                          rtol=0, atol=1e-12)


def test_restatement_matches_the_committed_known_answers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_rgcn",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_rgcn.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    kat = np.load(os.path.join(ROOT, "tests", "golden", "rgcn", "rgcn_kat.npz"))
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t)
    assert len(got) == 9
    for k, v in got.items():
        assert v.dtype == torch.float64 and np.abs(v.numpy() - kat[k]).max() <= 1e-13, k


@pytest.mark.parametrize("shape", [(4, 3, 5), (1, 1, 4), (3, 6, 2), (2, 5, 5)])
@pytest.mark.parametrize("norm", [True, False])
def test_factorisation_identity(shape, norm):
    """The per-edge loop equals bins . V and equals gather of x . L' (float64,
    1e-12), at Cin != Cout, and the featureless layer equals gather of basis in
    place; the backward's pieces equal the restatement's autograd."""
    B, c_in, c_out = shape
    n, E, NR = 11, 60, 5
    ei, et, en, x, basis, att, _, _ = _case(10 * B + c_in, n, E, NR, B, c_in, c_out)
    en = en if norm else None
    dst, src = ei[1], ei[0]
    want = R.rgcn_conv_loop(x, ei, et, en, basis, att)
    V = basis.double().view(B * c_in, c_out)
    by_bins = R.bins(dst, src, n, et, en, att, x).view(n, B * c_in) @ V
    y = (x.double() @ basis.double().permute(1, 0, 2).reshape(c_in, B * c_out)).view(n, B, c_out)
    by_gather = R.gather(dst, src, n, et, en, att, y)
    assert float((by_bins - want).abs().max()) <= 1e-12
    assert float((by_gather - want).abs().max()) <= 1e-12
    # d x, d basis, d att of sum(out * g) from dZ = g V^T and Z
    xr, br, ar = (t.double().requires_grad_(True) for t in (x, basis, att))
    g = torch.randn(n, c_out, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (R.rgcn_conv(xr, ei, et, en, br, ar) * g).sum().backward()
    dz = (g @ V.t()).view(n, B, c_in)
    assert float((R.gather(src, dst, n, et, en, att, dz) - xr.grad).abs().max()) <= 1e-12
    assert float((R.att_grad(et, en, dst, src, dz, x, NR) - ar.grad).abs().max()) <= 1e-12
    Z = R.bins(dst, src, n, et, en, att, x).view(n, B * c_in)
    assert float(((Z.t() @ g).view(B, c_in, c_out) - br.grad).abs().max()) <= 1e-12
    # featureless: basis_n [B, N, Cout] read in place as y[j, b, :] = basis_n[b, j, :]
    basis_n = torch.randn(B, n, c_out, generator=torch.Generator().manual_seed(2))
    bn, an = basis_n.double().requires_grad_(True), att.double().requires_grad_(True)
    out = R.rgcn_conv(None, ei, et, en, bn, an)
    assert float((R.gather(dst, src, n, et, en, att, basis_n.permute(1, 0, 2)) - out.detach()).abs().max()) <= 1e-12
    assert float((out.detach() - R.rgcn_conv_loop(None, ei, et, en, basis_n, att)).abs().max()) <= 1e-12
    (out * g).sum().backward()
    d_basis = R.bins(src, dst, n, et, en, att, g).permute(1, 0, 2)    # the transposed pass with x := g
    assert float((d_basis - bn.grad).abs().max()) <= 1e-12
    assert float((R.att_grad(et, en, src, dst, basis_n.permute(1, 0, 2), g, NR) - an.grad).abs().max()) <= 1e-12


# ---- the layer's host side ------------------------------------------------------

def test_layer_parameters_repr_and_init_bounds():
    from torch_geometric.nn import RGCNConv
    import torch_geometric.nn.conv as conv
    assert conv.RGCNConv is RGCNConv and "RGCNConv" in conv.__all__
    torch.manual_seed(0)
    c = RGCNConv(16, 24, 46, num_bases=30)
    assert repr(c) == "RGCNConv(16, 24, num_relations=46)"
    assert c.aggr == "add" and c.flow == "source_to_target"
    assert c.basis.shape == (30, 16, 24) and c.att.shape == (46, 30)
    assert c.root.shape == (16, 24) and c.bias.shape == (24,)
    bound = 1.0 / math.sqrt(30 * 16)                                   # uniform(B * Cin, .) on all four
    for name in ("basis", "att", "root", "bias"):
        top = float(getattr(c, name).detach().abs().max())
        assert 0.5 * bound < top <= bound, name
    assert sorted(n for n, _ in c.named_parameters()) == ["att", "basis", "bias", "root"]
    c = RGCNConv(3, 4, 5, 2, root_weight=False, bias=False, flow="target_to_source")
    assert c.root is None and c.bias is None and c.flow == "target_to_source"
    assert sorted(n for n, _ in c.named_parameters()) == ["att", "basis"]
    with pytest.raises(TypeError):
        RGCNConv(3, 4, 5, 2, aggr="mean")                             # aggregation is "add", as upstream


def test_fused_path_predicate():
    from torch_geometric.nn import RGCNConv
    assert RGCNConv(3, 4, 5, 2).fused_layer()
    assert RGCNConv(3, 4, 5, 2, root_weight=False, bias=False, flow="target_to_source").fused_layer()
    assert not RGCNConv(3, 4, 5, 2, node_dim=1).fused_layer()

    class Doubled(RGCNConv):
        def message(self, x_j, edge_index_j, edge_type, edge_norm):
            return 2 * super().message(x_j, edge_index_j, edge_type, edge_norm)

    class Shifted(RGCNConv):
        def update(self, aggr_out, x):
            return super().update(aggr_out, x) + 1

    class Mean(RGCNConv):
        def aggregate(self, inputs, index, dim_size):
            return super().aggregate(inputs, index, dim_size)

    assert not Doubled(3, 4, 5, 2).fused_layer() and not Shifted(3, 4, 5, 2).fused_layer()
    assert not Mean(3, 4, 5, 2).fused_layer()
    # host tensors never take the fused path (and the generic one has no CPU fallback)
    c = RGCNConv(3, 4, 5, 2)
    ei, et = torch.tensor([[0, 1], [1, 0]]), torch.tensor([0, 4])
    assert not c._fused_ok(torch.ones(2, 3), ei, et, None, None)
    assert not c._fused_ok(None, ei, et, None, None)
    with pytest.raises(ValueError, match="fused path"):
        c(torch.ones(2, 3), ei, et, form="bins")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(torch.ones(2, 3), ei, et)


def test_form_chooser_and_limits(lib):
    from mi355_mp import ops
    # a pure function of (B, Cin, Cout, E, N): the lower float count, ties to bins
    for B, ci, co, E, N in ((30, 16, 2, 148454, 23644), (30, 64, 64, 148454, 23644), (30, 16, 16, 148454, 23644),
                            (5, 70, 2, 4000, 300), (5, 6, 10, 4000, 300), (1, 1, 1, 10, 10)):
        bins = E * (B + ci) + 2 * N * B * ci
        gather = E * (B + B * co) + N * B * co
        assert ops.rgcn_form(B, ci, co, E, N) == ("bins" if bins <= gather else "gather")
    assert ops.rgcn_form(30, 16, 2, 148454, 23644) == "gather" and ops.rgcn_form(30, 64, 64, 148454, 23644) == "bins"
    assert ops.rgcn_form(5, 70, 2, 4000, 300) == "gather" and ops.rgcn_form(5, 6, 10, 4000, 300) == "bins"
    assert ops.rgcn_form(1, 3, 3, 5, 0) == "bins"                      # 5 * 4 floats either way: a tie goes to bins
    assert ops.rgcn_ok(46, 30, 16, 2) and ops.rgcn_ok(46, 30, 64, 64) and ops.rgcn_ok(1, 1, 1, 1)
    assert not ops.rgcn_ok(0, 4, 4, 4) and not ops.rgcn_ok(4, 0, 4, 4) and not ops.rgcn_ok(4, 4, 0, 4)
    assert not ops.rgcn_ok(4, 1025, 1024, 4) and not ops.rgcn_ok(4, 1025, 4, 1024) and ops.rgcn_ok(4, 1024, 1024, 1024)
    assert not ops.rgcn_ok(65537, 1, 1, 1) and ops.rgcn_ok(65536, 1, 1, 1)
    assert ops.rgcn_att_chunk() == lib.mp_rgcn_att_chunk() >= 64


def test_message_and_update_on_cpu_tensors_match_the_restatement():
    """Upstream's message / update are plain torch: on CPU tensors, with the sum
    over the edges done by index_add, they are the restatement (featured and
    featureless, with and without edge_norm, root and bias)."""
    from torch_geometric.nn import RGCNConv
    n, E, NR, B, c_in, c_out = 9, 50, 4, 3, 5, 2
    ei, et, en, x, _, _, _, _ = _case(7, n, E, NR, B, c_in, c_out)
    torch.manual_seed(1)
    for featureless in (False, True):
        for root, bias in ((True, True), (False, False)):
            c = RGCNConv(n if featureless else c_in, c_out, NR, B, root_weight=root, bias=bias).double()
            xin = None if featureless else x.double()
            for norm in (None, en.double()):
                msg = c.message(None if featureless else xin[ei[0]], ei[0], et, norm)
                out = c.update(torch.zeros(n, c_out, dtype=torch.float64).index_add(0, ei[1], msg), xin)
                want = R.rgcn_conv(xin, ei, et, norm, c.basis.detach(), c.att.detach(),
                                   None if c.root is None else c.root.detach(),
                                   None if c.bias is None else c.bias.detach())
                assert float((out.detach() - want).abs().max()) <= 1e-12, (featureless, root, norm is None)


def test_no_cpu_fallback_and_documented_refusals(lib):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    ei = torch.tensor([[0, 1], [1, 0]])
    g = Graph(ei, 2, 2)
    x, et, att, basis = torch.ones(2, 3), torch.tensor([0, 1]), torch.ones(2, 2), torch.ones(2, 3, 4)
    with pytest.raises(ValueError, match="form"):
        ops.rgcn_propagate(g, x, et, None, att, basis, form="other")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgcn_propagate(g, x, et, None, att, basis)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgcn_relation_plan(et, 2)


# ---- the C-ABI rejects every bad argument before any launch -------------------

def test_rgcn_entry_points_reject_bad_arguments(lib):
    from mi355_mp import _lib
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    N, E, NR, B, C = 257, 3000, 7, 5, 33
    Q = B * C
    AB, ZB, BB = NR * B * 4, N * Q * 4, B * N * C * 4
    g = _lib.MpCsr(D, D, D, None, None, None, N, E, 0, 0, 0, N, 0)

    def bins(g=g, et=D, ne=E, att=D, lda=B, ab=AB, R_=NR, B_=B, x=D, ldx=C, C_=C, out=D, ldn=Q, ldb=C, ob=ZB):
        return lib.mp_rgcn_aggregate_bins_f32(g, et, None, ne, att, lda, ab, R_, B_, x, ldx, C_, out, ldn, ldb, ob, None)

    def gather(g=g, et=D, ne=E, att=D, lda=B, ab=AB, R_=NR, B_=B, x=D, ldn=Q, ldb=C, ob=ZB, C_=C, out=D, ldo=C):
        return lib.mp_rgcn_aggregate_gather_f32(g, et, None, ne, att, lda, ab, R_, B_, x, ldn, ldb, ob, C_, None, out,
                                                ldo, None)

    def variant(**kw):
        f = dict(rowptr=D, col=D, eid=D, n_cols=N, n_ids=0)
        f.update(kw)
        return _lib.MpCsr(f["rowptr"], f["col"], f["eid"], None, None, None, N, E, 0, 0, 0, f["n_cols"], f["n_ids"])

    def rejected(fn, kw, needle):
        rc = fn(**kw)
        err = lib.mp_last_error().decode()
        assert rc == -1 and needle in err, (fn.__name__, kw, rc, err)

    for fn, cname, xname in ((bins, "C", "x"), (gather, "F", "y")):
        for kw, needle in [
                (dict(et=None), "edge_type is NULL"), (dict(att=None), "att is NULL"),
                (dict(x=None), "%s is NULL" % xname), (dict(out=None), "out is NULL"),
                (dict(R_=0), "R = 0"), (dict(R_=65537, ab=1 << 30), "above the limit"), (dict(B_=0), "B = 0"),
                (dict(B_=-3), "B = -3"), (dict(C_=0), "%s = 0" % cname),
                (dict(B_=1025, lda=1025, ab=1 << 30, C_=1024, ldn=1025 * 1024, ldb=1024, ob=1 << 40),
                 "above the limit"),
                (dict(ne=E - 1), "n_type_edges = %d" % (E - 1)), (dict(lda=B - 1), "ld_att = %d" % (B - 1)),
                (dict(ab=AB - 1), "att holds %d bytes, the call needs %d" % (AB - 1, AB)),
                (dict(lda=B + 1), "att holds"),
                (dict(g=variant(n_ids=E + 1)), "n_type_edges"), (dict(g=variant(col=None)), "col is NULL"),
                (dict(g=variant(eid=None)), "eid is NULL"), (dict(g=variant(rowptr=None)), "rowptr is NULL"),
                (dict(g=variant(n_cols=0)), "n_cols"), (dict(g=None), "g is NULL")]:
            rejected(fn, kw, needle)
    rejected(bins, dict(ldx=C - 1), "ldx = %d" % (C - 1))
    rejected(bins, dict(ldn=Q - 1), "overlap")
    rejected(bins, dict(ldb=C - 1), "overlap")
    rejected(bins, dict(ldn=C, ldb=N * C - 1, ob=BB), "overlap")
    rejected(bins, dict(ob=ZB - 1), "out holds %d bytes, the call needs %d" % (ZB - 1, ZB))
    rejected(bins, dict(ldn=C, ldb=N * C, ob=BB - 1), "out holds %d bytes, the call needs %d" % (BB - 1, BB))
    rejected(bins, dict(ldn=Q + 1), "out holds")
    rejected(gather, dict(ldn=C - 1), "ld_node = %d" % (C - 1))
    rejected(gather, dict(ldb=C - 1), "ld_block = %d" % (C - 1))
    rejected(gather, dict(ldo=C - 1), "ldo = %d" % (C - 1))
    rejected(gather, dict(ob=ZB - 1), "y holds %d bytes, the call needs %d" % (ZB - 1, ZB))
    rejected(gather, dict(ldn=C, ldb=N * C, ob=BB - 1), "y holds %d bytes, the call needs %d" % (BB - 1, BB))

    WS = lib.mp_rgcn_att_grad_workspace(E, NR, B)
    assert WS >= (NR + 1) * 8 + (E // lib.mp_rgcn_att_chunk() + NR) * B * 4
    assert lib.mp_rgcn_att_grad_workspace(0, NR, B) < WS

    def att(perm=D, relptr=D, rows=D, cols=D, ne=E, P=D, ldpn=Q, ldpb=C, Q_=D, ldq=C, R_=NR, B_=B, C_=C, datt=D,
            ldd=B, db=AB, ws=D, wsb=WS):
        return lib.mp_rgcn_att_grad_f32(perm, relptr, rows, cols, ne, None, P, ldpn, ldpb, Q_, ldq, R_, B_, C_, datt,
                                        ldd, db, ws, wsb, None)

    for kw, needle in [(dict(perm=None), "perm is NULL"), (dict(relptr=None), "relptr is NULL"),
                       (dict(rows=None), "rows is NULL"), (dict(cols=None), "cols is NULL"),
                       (dict(P=None), "P is NULL"), (dict(Q_=None), "Q is NULL"), (dict(datt=None), "datt is NULL"),
                       (dict(ws=None), "ws is NULL"), (dict(ne=-1), "n_edges"),
                       (dict(ldpn=C - 1), "ldp_node = %d" % (C - 1)), (dict(ldpb=C - 1), "ldp_block = %d" % (C - 1)),
                       (dict(ldq=C - 1), "ldq = %d" % (C - 1)), (dict(ldd=B - 1), "ld_datt = %d" % (B - 1)),
                       (dict(db=AB - 1), "datt holds %d bytes, the call needs %d" % (AB - 1, AB)),
                       (dict(db=0), "datt holds 0 bytes"), (dict(ldd=B + 1), "datt holds"),
                       (dict(wsb=WS - 1), "ws holds %d bytes, the call needs %d" % (WS - 1, WS)),
                       (dict(wsb=lib.mp_rgcn_att_grad_workspace(0, NR, B)), "ws holds"),
                       (dict(R_=0), "R = 0"), (dict(B_=0), "B = 0"), (dict(C_=0), "C = 0"),
                       (dict(B_=1025, C_=1024, ldpn=1025 * 1024, ldpb=1024, ldq=1024, ldd=1025, db=1 << 30,
                             wsb=1 << 40), "above the limit")]:
        rejected(att, kw, needle)
    assert lib.mp_rgcn_ok(46, 30, 16, 2) == 1 and lib.mp_rgcn_ok(46, 30, 64, 64) == 1 and lib.mp_rgcn_ok(0, 1, 1, 1) == 0
    # the int64 returns are outside the symbols the raising view wraps: ops tests the sign
    for name in ("mp_rgcn_ok", "mp_rgcn_att_chunk", "mp_rgcn_aggregate_bins_f32", "mp_rgcn_aggregate_gather_f32",
                 "mp_rgcn_att_grad_f32"):
        assert _lib.SIGNATURES[name][0] is _lib.i64 and name not in _lib.STATUS_RETURNING
    assert _lib.ABI_VERSION == 7 and lib.mp_abi_version() == 7
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match=r"mp_rgcn_att_grad_f32 failed \(code 1\): .*ld_datt"):
        ops._count_call(_lib.native(), "mp_rgcn_att_grad_f32", D, D, D, D, E, None, D, Q, C, D, C, NR, B, C, D, B - 1,
                        AB, D, WS, None)


def test_rgcn_abi_rejections_under_asan():
    """tests/abi/abi_reject_rgcn.c against the host-AddressSanitizer build of
    the library (make asan_rgcn), run as a plain program: every rejection
    names its argument and the exact documented boundaries pass the checks."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_rgcn"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_rgcn")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_rgcn: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 70, r.stdout[-2000:]
