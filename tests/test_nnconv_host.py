"""CPU tests of the NNConv feature: hand values and committed known answers of
the float64 restatement (tests/_nnconv_ref.py) that the GPU tests check the
kernels against, the factorisation identity the fused path rests on, the
layer's host-side pieces (parameters, repr, the fused-path predicate, the form
chooser), and the C-ABI's rejection of every bad argument of the NNConv entry
points -- from Python with fake device pointers and from a C harness under the
host-ASAN build of the library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _nnconv_ref as R

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
    """Two nodes, edges 0 -> 1 twice and 1 -> 1, Cin = 2, Cout = 1, H = 1:
    W_e = [w0 h + b0, w1 h + b1] with w = (1, 2), b = (10, 20)."""
    ei = torch.tensor([[0, 0, 1], [1, 1, 1]])
    h = torch.tensor([[1.0], [2.0], [3.0]])
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0]])
    hw, hb = torch.tensor([[1.0], [2.0]]), torch.tensor([10.0, 20.0])
    # messages: x0 . (11, 22) = 55; x0 . (12, 24) = 60; x1 . (13, 26) = 13
    assert R.nn_conv(x, ei, h, hw, hb, 2, 1).tolist() == [[0.0], [128.0]]
    assert R.nn_conv(x, ei, h, hw, hb, 2, 1, aggr="mean").tolist() == [[0.0], [128.0 / 3]]
    assert R.nn_conv(x, ei, h, hw, hb, 2, 1, aggr="max").tolist() == [[0.0], [60.0]]
    assert R.nn_conv(x, ei, h, hw, None, 2, 1).tolist() == [[0.0], [5.0 + 10.0 + 3.0]]
    root, bias = torch.tensor([[1.0], [1.0]]), torch.tensor([0.5])
    assert R.nn_conv(x, ei, h, hw, hb, 2, 1, root, bias).tolist() == [[3.5], [130.5]]
    assert R.nn_conv(x, ei, h, hw, hb, 2, 1, flow="target_to_source").tolist() == [[11.0 * 3 - 22 + 12 * 3 - 24],
                                                                                   [13.0 * 3 - 26]]
    # the kernel contracts: Z[r, k*Cin + c], k = H the implicit 1
    assert R.bins(ei[1], ei[0], 2, h, x).tolist() == [[0.0] * 4, [1 + 2 + 9.0, 2 + 4 - 3.0, 1 + 1 + 3.0, 2 + 2 - 1.0]]
    y = torch.tensor([[1.0, 2.0], [3.0, 4.0]])                        # [n, H + 1 = 2, F = 1]
    assert R.gather(ei[1], ei[0], 2, h, y, 1).tolist() == [[0.0], [(1 + 2) + (2 + 2) + (9 + 4.0)]]
    dz = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 5.0, 7.0]])
    assert R.edge_grad(ei[1], ei[0], dz, x, 1).tolist() == [[5.0], [5.0], [1.0]]
    L = R.head_matrix(hw, hb, 2, 1)
    assert L.tolist() == [[1.0], [2.0], [10.0], [20.0]]
    assert R.gather_matrix(L, 1, 2, 1).tolist() == [[1.0, 10.0], [2.0, 20.0]]


def _case(seed, n, E, H, c_in, c_out):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, E), generator=g)
    return (ei, torch.randn(E, H, generator=g), torch.randn(n, c_in, generator=g),
            torch.randn(c_in * c_out, H, generator=g), torch.randn(c_in * c_out, generator=g),
            torch.randn(c_in, c_out, generator=g), torch.randn(c_out, generator=g))


def test_restatement_is_the_per_edge_loop():
    ei, h, x, hw, hb, root, bias = _case(3, 7, 40, 4, 3, 2)
    for aggr in ("add", "mean", "max"):
        for flow in ("source_to_target", "target_to_source"):
            out = R.nn_conv(x, ei, h, hw, hb, 3, 2, root, bias, aggr, flow)
            want = R.nn_conv_loop(x, ei, h, hw, hb, 3, 2, root, bias, aggr, flow)
            assert torch.allclose(out, want, rtol=0, atol=1e-12), (aggr, flow)
    assert torch.allclose(R.nn_conv(x, ei, h, hw, None, 3, 2), R.nn_conv_loop(x, ei, h, hw, None, 3, 2), rtol=0,
                          atol=1e-12)


def test_restatement_matches_the_committed_known_answers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_nnconv",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_nnconv.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    kat = np.load(os.path.join(ROOT, "tests", "golden", "nnconv", "nnconv_kat.npz"))
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t)
    assert len(got) == 10
    for k, v in got.items():
        assert v.dtype == torch.float64 and np.abs(v.numpy() - kat[k]).max() <= 1e-13, k


@pytest.mark.parametrize("shape", [(4, 3, 5), (1, 1, 4), (3, 6, 2), (2, 5, 5)])
@pytest.mark.parametrize("head_bias", [True, False])
def test_factorisation_identity(shape, head_bias):
    """The per-edge loop equals bins . L and equals gather of x . L' (float64,
    1e-12), head.weight's permutation at Cin != Cout included, for add and mean."""
    H, c_in, c_out = shape
    n, E = 11, 60
    ei, h, x, hw, hb, _, _ = _case(10 * H + c_in, n, E, H, c_in, c_out)
    hb = hb if head_bias else None
    dst, src = ei[1], ei[0]
    L = R.head_matrix(hw, hb, c_in, c_out)
    assert L.shape == ((H + 1) * c_in, c_out)
    for aggr in ("add", "mean"):
        scale = None
        if aggr == "mean":
            scale = 1.0 / torch.bincount(dst, minlength=n).clamp(min=1).double()
        want = R.nn_conv_loop(x, ei, h, hw, hb, c_in, c_out, aggr=aggr)
        by_bins = R.bins(dst, src, n, h, x, scale) @ L
        y = x.double() @ R.gather_matrix(L, H, c_in, c_out)
        by_gather = R.gather(dst, src, n, h, y, c_out, scale)
        assert float((by_bins - want).abs().max()) <= 1e-12, aggr
        assert float((by_gather - want).abs().max()) <= 1e-12, aggr
    # the backward's pieces: d h and d x of sum(out * g) from dZ = g L^T
    xr, hr = x.double().requires_grad_(True), h.double().requires_grad_(True)
    g = torch.randn(n, c_out, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (R.nn_conv(xr, ei, hr, hw, hb, c_in, c_out) * g).sum().backward()
    dz = g @ L.t()
    assert float((R.edge_grad(dst, src, dz, x, H) - hr.grad).abs().max()) <= 1e-12
    assert float((R.gather(src, dst, n, h, dz, c_in) - xr.grad).abs().max()) <= 1e-12


# ---- the layer's host side ------------------------------------------------------

def _seq(c_in, c_out, H=25, D=2):
    return torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, c_in * c_out))


def test_layer_parameters_repr_and_init_bounds():
    from torch_geometric.nn import NNConv
    import torch_geometric.nn.conv as conv
    assert conv.NNConv is NNConv
    torch.manual_seed(0)
    net = _seq(16, 24)
    before = net[2].weight.detach().clone()
    c = NNConv(16, 24, net)
    assert repr(c) == "NNConv(16, 24)"
    assert c.nn is net and c.aggr == "add" and c.flow == "source_to_target"
    assert c.root.shape == (16, 24) and c.bias.shape == (24,)
    assert not torch.equal(net[2].weight.detach(), before)           # nn was reset through its modules
    bound = 1.0 / math.sqrt(16)
    assert 0.9 * bound < float(c.root.detach().abs().max()) <= bound
    assert 0.5 * bound < float(c.bias.detach().abs().max()) <= bound
    assert sorted(n for n, _ in c.named_parameters()) == ["bias", "nn.0.bias", "nn.0.weight", "nn.2.bias",
                                                          "nn.2.weight", "root"]
    c = NNConv(3, 4, torch.nn.Linear(5, 12), aggr="mean", root_weight=False, bias=False, flow="target_to_source")
    assert c.root is None and c.bias is None and c.aggr == "mean" and c.flow == "target_to_source"
    assert sorted(n for n, _ in c.named_parameters()) == ["nn.bias", "nn.weight"]


def test_fused_path_predicate():
    from torch_geometric.nn import NNConv
    net = _seq(3, 4)
    trunk, head = NNConv(3, 4, net).fused_head()
    assert head is net[2] and len(trunk) == 2 and trunk[0] is net[0] and trunk[1] is net[1]
    lin = torch.nn.Linear(5, 12)
    assert NNConv(3, 4, lin).fused_head() == (None, lin)
    assert NNConv(3, 4, torch.nn.Sequential(lin)).fused_head() == (None, lin)
    assert NNConv(3, 4, lin, aggr="mean").fused_head() is not None
    assert NNConv(3, 4, torch.nn.Linear(5, 12, bias=False)).fused_head() is not None
    assert NNConv(3, 4, lin, aggr="max").fused_head() is None
    assert NNConv(3, 4, torch.nn.Linear(5, 13)).fused_head() is None             # wrong out_features
    assert NNConv(3, 4, torch.nn.Sequential(lin, torch.nn.ReLU())).fused_head() is None
    assert NNConv(3, 4, torch.nn.Sequential(torch.nn.Linear(5, 12), torch.nn.Tanh())).fused_head() is None

    class Scaled(torch.nn.Linear):
        pass

    assert NNConv(3, 4, Scaled(5, 12)).fused_head() is None                      # a subclass may compute anything
    for register in ("register_forward_hook", "register_forward_pre_hook", "register_full_backward_hook"):
        hooked = torch.nn.Linear(5, 12)
        handle = getattr(hooked, register)(lambda *a: None)
        c = NNConv(3, 4, torch.nn.Sequential(torch.nn.Linear(2, 5), hooked))
        assert c.fused_head() is None, register
        handle.remove()
        assert c.fused_head() is not None, register

    class Other(NNConv):
        def message(self, x_j, pseudo):
            return super().message(x_j, pseudo) * 2

    assert Other(3, 4, lin).fused_head() is None


def test_form_chooser_and_limits(lib):
    from mi355_mp import ops
    # a pure function of (H, Cin, Cout, E, N): the lower float count, ties to bins
    for H, ci, co, E, N in ((25, 1, 32, 38000, 4800), (25, 32, 64, 38000, 4800), (128, 64, 64, 4600, 2300),
                            (25, 64, 1, 10, 1000), (4, 70, 2, 3000, 257), (4, 6, 10, 3000, 257)):
        bins = E * (H + ci) + 2 * N * (H + 1) * ci
        gather = E * (H + (H + 1) * co) + N * (H + 1) * co
        assert ops.nnconv_form(H, ci, co, E, N) == ("bins" if bins <= gather else "gather")
    assert ops.nnconv_form(25, 1, 32, 38000, 4800) == "bins" and ops.nnconv_form(128, 64, 64, 4600, 2300) == "bins"
    assert ops.nnconv_form(25, 64, 1, 10, 1000) == "gather" and ops.nnconv_form(4, 70, 2, 3000, 257) == "gather"
    assert ops.nnconv_ok(25, 1, 32) and ops.nnconv_ok(25, 32, 64) and ops.nnconv_ok(128, 64, 64)
    assert not ops.nnconv_ok(0, 4, 4) and not ops.nnconv_ok(4, 0, 4) and not ops.nnconv_ok(1024, 1024, 4)
    assert not ops.nnconv_ok(1024, 4, 1024) and ops.nnconv_ok(1023, 1024, 1024)


def test_no_cpu_fallback_and_documented_refusals(lib):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    from torch_geometric.nn import NNConv
    ei = torch.tensor([[0, 1], [1, 0]])
    c = NNConv(2, 3, torch.nn.Linear(1, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(torch.ones(2, 2), ei, torch.rand(2))
    with pytest.raises(ValueError, match="fused path"):
        NNConv(2, 3, torch.nn.Linear(1, 6), aggr="max")(torch.ones(2, 2), ei, torch.rand(2), form="bins")
    g = Graph(ei, 2, 2)
    x, h, w = torch.ones(2, 2), torch.ones(2, 1), torch.ones(6, 1)
    with pytest.raises(NotImplementedError, match="max"):
        ops.nnconv_propagate(g, x, h, w, None, "max")
    with pytest.raises(ValueError, match="form"):
        ops.nnconv_propagate(g, x, h, w, None, "add", form="other")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nnconv_propagate(g, x, h, w, None, "add")


# ---- the C-ABI rejects every bad argument before any launch -------------------

def test_nnconv_entry_points_reject_bad_arguments(lib):
    from mi355_mp import _lib
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    N, E, H, C = 257, 3000, 25, 33
    Q = (H + 1) * C
    g = _lib.MpCsr(D, D, D, None, None, None, N, E, 0, 0, 0, N, 0)

    def bins(g=g, h=D, ne=E, ldh=H, H_=H, x=D, ldx=C, C_=C, out=D, ldo=Q):
        return lib.mp_nnconv_aggregate_bins_f32(g, h, ne, ldh, H_, x, ldx, C_, None, out, ldo, None)

    def gather(g=g, h=D, ne=E, ldh=H, H_=H, x=D, ldx=Q, C_=C, out=D, ldo=C):
        return lib.mp_nnconv_aggregate_gather_f32(g, h, ne, ldh, H_, x, ldx, C_, None, None, out, ldo, None)

    def variant(**kw):
        f = dict(rowptr=D, col=D, eid=D, n_cols=N, n_ids=0)
        f.update(kw)
        return _lib.MpCsr(f["rowptr"], f["col"], f["eid"], None, None, None, N, E, 0, 0, 0, f["n_cols"], f["n_ids"])

    def rejected(fn, kw, needle):
        rc = fn(**kw)
        err = lib.mp_last_error().decode()
        assert rc == -1 and needle in err, (fn.__name__, kw, rc, err)

    for fn, cname, xname in ((bins, "Cin", "x"), (gather, "F", "y")):
        for kw, needle in [
                (dict(h=None), "h is NULL"), (dict(x=None), "%s is NULL" % xname), (dict(out=None), "out is NULL"),
                (dict(H_=0), "H = 0"), (dict(H_=-3), "H = -3"), (dict(C_=0), "%s = 0" % cname),
                (dict(H_=1024, ldh=1024, C_=1024, ldx=1025 * 1024, ldo=1025 * 1024), "above the limit"),
                (dict(ne=E - 1), "n_h_edges = %d" % (E - 1)), (dict(ldh=H - 1), "ldh = %d" % (H - 1)),
                (dict(g=variant(n_ids=E + 1)), "n_h_edges"), (dict(g=variant(col=None)), "col is NULL"),
                (dict(g=variant(eid=None)), "eid is NULL"), (dict(g=variant(rowptr=None)), "rowptr is NULL"),
                (dict(g=variant(n_cols=0)), "n_cols"), (dict(g=None), "g is NULL")]:
            rejected(fn, kw, needle)
    rejected(bins, dict(ldo=Q - 1), "ldo = %d" % (Q - 1))
    rejected(bins, dict(ldx=C - 1), "ldx = %d" % (C - 1))
    rejected(gather, dict(ldx=Q - 1), "ldy = %d" % (Q - 1))
    rejected(gather, dict(ldo=C - 1), "ldo = %d" % (C - 1))

    need = ((E - 1) * H + H) * 4

    def edge(rows=D, cols=D, ne=E, dz=D, lddz=Q, x=D, ldx=C, H_=H, C_=C, dh=D, lddh=H, nbytes=need):
        return lib.mp_nnconv_edge_grad_f32(rows, cols, ne, dz, lddz, x, ldx, H_, C_, dh, lddh, nbytes, None)

    for kw, needle in [(dict(rows=None), "rows is NULL"), (dict(cols=None), "cols is NULL"),
                       (dict(dz=None), "dz is NULL"), (dict(x=None), "x is NULL"), (dict(dh=None), "dh is NULL"),
                       (dict(ne=-1), "n_edges"), (dict(lddz=Q - 1), "lddz = %d" % (Q - 1)),
                       (dict(ldx=C - 1), "ldx = %d" % (C - 1)), (dict(lddh=H - 1), "lddh = %d" % (H - 1)),
                       (dict(nbytes=need - 1), "dh holds %d bytes, the call needs %d" % (need - 1, need)),
                       (dict(nbytes=0), "dh holds 0 bytes"), (dict(lddh=H + 1), "dh holds"),
                       (dict(H_=0), "H = 0"), (dict(C_=0), "Cin = 0"),
                       (dict(H_=1024, C_=1024, lddz=1025 * 1024, ldx=1024, lddh=1024, nbytes=1 << 40),
                        "above the limit")]:
        rejected(edge, kw, needle)
    assert lib.mp_nnconv_edge_grad_f32(None, None, 0, None, Q, None, C, H, C, None, H, 0, None) == 0
    assert lib.mp_nnconv_ok(25, 1, 32) == 1 and lib.mp_nnconv_ok(128, 64, 64) == 1 and lib.mp_nnconv_ok(0, 1, 1) == 0
    # the int64 returns are outside the symbols the raising view wraps: ops tests the sign
    assert _lib.SIGNATURES["mp_nnconv_ok"][0] is _lib.i64
    for name in ("mp_nnconv_aggregate_bins_f32", "mp_nnconv_aggregate_gather_f32", "mp_nnconv_edge_grad_f32"):
        assert _lib.SIGNATURES[name][0] is _lib.i64 and name not in _lib.STATUS_RETURNING
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match=r"mp_nnconv_edge_grad_f32 failed \(code 1\): .*lddh"):
        ops._count_call(_lib.native(), "mp_nnconv_edge_grad_f32", D, D, E, D, Q, D, C, H, C, D, H - 1, need, None)


def test_nnconv_abi_rejections_under_asan():
    """tests/abi/abi_reject_nnconv.c against the host-AddressSanitizer build of
    the library (make asan_nnconv), run as a plain program: every rejection
    names its argument and the exact documented boundaries pass the checks."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_nnconv"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_nnconv")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_nnconv: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 50, r.stdout[-2000:]


# ---- which edge-gradient kernel a shape takes ------------------------------------------

def _width_restated(H, c_in):
    """The dispatch of nnconv_edge_grad, restated: the grouped kernel up to 32
    columns; above, the lanes W of 32 or 64 that waste the fewest lanes and
    values of h, ties to 64."""
    if c_in <= 32:
        return 0

    def used(W):
        return c_in / (-(-c_in // W) * W) * H / (-(-H // W) * W)
    return 32 if used(32) > used(64) else 64


def test_edge_grad_width_is_the_dispatch_restated(lib):
    from mi355_mp import ops
    seen = set()
    for c_in in range(1, 201):
        for H in range(1, 201):
            w = lib.mp_nnconv_edge_grad_width(H, c_in)
            assert w == _width_restated(H, c_in), (H, c_in, w)
            seen.add(w)
    assert seen == {0, 32, 64}
    assert ops.nnconv_edge_grad_width(40, 70) == 32 and ops.nnconv_edge_grad_width(40, 33) == 64
    assert ops.nnconv_edge_grad_width(128, 32) == 0
    assert lib.mp_nnconv_edge_grad_width(0, 33) == -1 and "H = 0" in lib.mp_last_error().decode()
    assert lib.mp_nnconv_edge_grad_width(5, 0) == -1 and lib.mp_nnconv_edge_grad_width(1024, 1024) == -1
    with pytest.raises(ValueError, match="H = 0"):
        ops.nnconv_edge_grad_width(0, 33)
    from mi355_mp import _lib
    assert _lib.SIGNATURES["mp_nnconv_edge_grad_width"][0] is _lib.i64
    assert "mp_nnconv_edge_grad_width" not in _lib.STATUS_RETURNING


def test_the_lane_shape_sweep_reaches_every_edge_grad_tile_shape(lib):
    """The coverage the GPU sweep (tests/test_gpu_conv_lane_shapes.py) claims, by the
    library's own dispatch: checked here too, where there is no GPU."""
    from tests import _conv_lane_cases as K
    width = lambda H, c_in: lib.mp_nnconv_edge_grad_width(H, c_in)     # noqa: E731
    assert K.edge_grad_reach(width, K.NNCONV_WIDTHS + K.NNCONV_EDGE_GRAD) >= K.EDGE_GRAD_REACHED
    assert K.edge_grad_reach(width, K.NNCONV_WIDTHS) == {"grouped", "w32 single partial tile", "w32 several c per lane"}
    for case, (w, tiles, last) in zip(K.NNCONV_EDGE_GRAD, ((64, 1, 40), (64, 1, 63), (64, 2, 36), (32, 2, 8),
                                                           (32, 3, 1), (64, 1, 33), (32, 1, 5))):
        c_in, H = case
        assert (width(H, c_in), -(-H // w), H - (-(-H // w) - 1) * w) == (w, tiles, last), case
    K.tiny_graph()
    assert torch.bincount(K.tiny_relations(3), minlength=3)[1] == 0
