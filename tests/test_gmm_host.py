"""CPU tests of the GMMConv feature: hand values and committed known answers of
the float64 restatement (tests/_gmm_ref.py) that the GPU tests check the
kernels against, the factorisation identity and the closed-form gradients the
fused path rests on, the layer's host-side pieces (parameters, repr, the
fused-path predicate, the form chooser), and the C-ABI's rejection of every bad
argument of the GMMConv entry points -- from Python with fake device pointers
and from a C harness under the host-ASAN build of the library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _gmm_ref as R

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
    # p = mu gives w = 1; |p - mu| = |sigma| in each of D dims gives w = e^{-D/2}
    for D in (1, 2, 3):
        mu = torch.tensor([[0.25] * D, [1.0] * D])
        sigma = torch.tensor([[0.5] * D, [-2.0] * D])
        p = torch.tensor([[0.25] * D, [0.75] * D, [-1.0] * D, [3.0] * D])
        w = R.weights(p, mu, sigma)
        assert w[0, 0] == 1.0
        assert abs(float(w[1, 0]) - math.exp(-D / 2)) < 1e-14          # |p - mu| = 0.5 = |sigma|
        assert abs(float(w[2, 1]) - math.exp(-D / 2)) < 1e-14          # |p - mu| = 2 = |sigma|, sign of sigma ignored
        assert abs(float(w[3, 1]) - math.exp(-D / 2)) < 1e-14
    # both g column layouts at Cin != Cout.  Cin = 2, M = 3, K = 2, every w = 1 (p = mu for all k)
    ei = torch.tensor([[0, 1, 1], [1, 1, 0]])
    p = torch.full((3, 1), 0.5)
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0]])
    g = torch.arange(12, dtype=torch.float32).view(2, 6)               # g[c, col] = 6 c + col
    mu, sigma = torch.full((2, 1), 0.5), torch.ones(2, 1)
    # shared: column k*M + m; m_e[m] = sum_k (x_j g)[k*3 + m]; x0 g = [12, 15, 18, 21, 24, 27], x1 g = [-6, -4, -2, 0, 2, 4]
    out = R.gmm_conv(x, ei, p, g, mu, sigma, 2, aggr="add")
    assert out.tolist() == [[-6.0, -2.0, 2.0], [33.0 - 6, 39.0 - 2, 45.0 + 2]]
    assert R.gmm_conv(x, ei, p, g, mu, sigma, 2, aggr="mean").tolist() == [[-6.0, -2.0, 2.0], [13.5, 18.5, 23.5]]
    assert R.gmm_conv(x, ei, p, g, mu, sigma, 2, aggr="max").tolist() == [[-6.0, -2.0, 2.0], [33.0, 39.0, 45.0]]
    # separate: column m*K + k; W[c, m] = g[c, 2m] + g[c, 2m + 1] = [[1, 5, 9], [13, 17, 21]]
    mus, sigmas = torch.full((2, 3, 2, 1), 0.5), torch.ones(2, 3, 2, 1)
    out = R.gmm_conv(x, ei, p, g, mus, sigmas, 2, aggr="add")
    assert out.tolist() == [[3.0 - 13, 15.0 - 17, 27.0 - 21], [27.0 - 10, 39.0 - 2, 51.0 + 6]]
    root, bias = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), torch.tensor([0.5, 0.0, 0.0])
    assert R.gmm_conv(x, ei, p, g, mu, sigma, 2, root, bias, "add").tolist() == [[-2.5, -2.0, 2.0], [29.5, 37.0, 47.0]]
    # target_to_source: node 0 receives from node 1, node 1 from nodes 1 and 0 -- the same sums here
    assert R.gmm_conv(x, ei, p, g, mu, sigma, 2, aggr="add", flow="target_to_source").tolist() == [
        [-6.0, -2.0, 2.0], [27.0, 37.0, 47.0]]
    assert R.gmm_conv(x, ei[:, :2], p[:2], g, mu, sigma, 2, aggr="add", flow="target_to_source").tolist() == [
        [-6.0, -2.0, 2.0], [-6.0, -2.0, 2.0]]
    # the kernel contracts
    assert R.bins(ei[1], ei[0], 2, p, mu, sigma, x).tolist() == [[3.0, -1.0, 3.0, -1.0], [4.0, 1.0, 4.0, 1.0]]
    assert R.mix_matrix(g, 2, 2, 3).tolist() == [[0.0, 1.0, 2.0], [6.0, 7.0, 8.0], [3.0, 4.0, 5.0], [9.0, 10.0, 11.0]]
    y = torch.tensor([[1.0, 2.0], [3.0, 4.0]])                         # [n, K = 2, F = 1]
    assert R.gather(ei[1], ei[0], 2, p, mu, sigma, y, 1).tolist() == [[7.0], [10.0]]


def _case(seed, n, E, K, D, c_in, c_out, separate=False):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, E), generator=g)
    shape = (c_in, c_out, K, D) if separate else (K, D)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (ei, torch.rand(E, D, generator=g), torch.randn(n, c_in, generator=g),
            torch.randn(c_in, K * c_out, generator=g), torch.rand(shape, generator=g),
            (torch.rand(shape, generator=g) + 0.5) * sign,
            torch.randn(c_in, c_out, generator=g), torch.randn(c_out, generator=g))


def test_restatement_is_the_per_edge_loop():
    for separate in (False, True):
        ei, p, x, g, mu, sigma, root, bias = _case(3, 7, 30, 3, 2, 3, 2, separate)
        for aggr in ("add", "mean", "max"):
            for flow in ("source_to_target", "target_to_source"):
                out = R.gmm_conv(x, ei, p, g, mu, sigma, 3, root, bias, aggr, flow)
                want = R.gmm_conv_loop(x, ei, p, g, mu, sigma, 3, root, bias, aggr, flow)
                assert torch.allclose(out, want, rtol=0, atol=1e-12), (separate, aggr, flow)
        assert torch.allclose(R.gmm_conv(x, ei, p, g, mu, sigma, 3), R.gmm_conv_loop(x, ei, p, g, mu, sigma, 3),
                              rtol=0, atol=1e-12)


def test_restatement_matches_the_committed_known_answers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_gmm",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_gmm.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    kat = np.load(os.path.join(ROOT, "tests", "golden", "gmm", "gmm_kat.npz"))
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t)
    assert len(got) == 14
    for k, v in got.items():
        assert v.dtype == torch.float64 and np.abs(v.numpy() - kat[k]).max() <= 1e-13, k


@pytest.mark.parametrize("K", [1, 3, 25])
@pytest.mark.parametrize("D", [1, 3])
def test_factorisation_identity_and_gradient_formulas(K, D):
    """The per-edge loop equals bins . G' and equals gather of x g (float64,
    1e-12), g's permutation at Cin != Cout included, for add and mean; and the
    closed forms of d mu, d sigma, d pseudo, d x equal float64 autograd."""
    c_in, c_out, n, E = 3, 5, 11, 50
    ei, p, x, g, mu, sigma, _, _ = _case(10 * K + D, n, E, K, D, c_in, c_out)
    dst, src = ei[1], ei[0]
    Gp = R.mix_matrix(g, K, c_in, c_out)
    assert Gp.shape == (K * c_in, c_out)
    for aggr in ("add", "mean"):
        scale = None
        if aggr == "mean":
            scale = 1.0 / torch.bincount(dst, minlength=n).clamp(min=1).double()
        want = R.gmm_conv_loop(x, ei, p, g, mu, sigma, K, aggr=aggr)
        by_bins = R.bins(dst, src, n, p, mu, sigma, x, scale) @ Gp
        by_gather = R.gather(dst, src, n, p, mu, sigma, x.double() @ g.double(), c_out, scale)
        assert float((by_bins - want).abs().max()) <= 1e-12, aggr
        assert float((by_gather - want).abs().max()) <= 1e-12, aggr
    xr, pr = x.double().requires_grad_(True), p.double().requires_grad_(True)
    mur, sr = mu.double().requires_grad_(True), sigma.double().requires_grad_(True)
    go = torch.randn(n, c_out, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (R.gmm_conv(xr, ei, pr, g, mur, sr, K, aggr="add") * go).sum().backward()
    dz = go @ Gp.t()
    dmu, dsigma, dpseudo = R.param_grad(dst, src, p, mu, sigma, dz, x)
    assert float((dmu - mur.grad).abs().max()) <= 1e-12
    assert float((dsigma - sr.grad).abs().max()) <= 1e-12
    assert float((dpseudo - pr.grad).abs().max()) <= 1e-12
    assert float((R.gather(src, dst, n, p, mu, sigma, dz, c_in) - xr.grad).abs().max()) <= 1e-12


def test_underflowed_weights_contribute_zero_in_the_restatement():
    ei, p, x, g, mu, sigma, _, _ = _case(5, 6, 20, 3, 2, 2, 2)
    sigma[1] = 1e-4                                                      # every weight of kernel 1 underflows
    assert bool((R.weights(p, mu, sigma)[:, 1] == 0).all())
    dz = torch.randn(6, 3 * 2, generator=torch.Generator().manual_seed(0))
    dmu, dsigma, dpseudo = R.param_grad(ei[1], ei[0], p, mu, sigma, dz, x)
    assert bool(torch.isfinite(dmu).all() and torch.isfinite(dsigma).all() and torch.isfinite(dpseudo).all())
    assert bool((dmu[1] == 0).all() and (dsigma[1] == 0).all())


# ---- the layer's host side ------------------------------------------------------

def test_layer_parameters_repr_and_init_bounds():
    from torch_geometric.nn import GMMConv
    import torch_geometric.nn as nn
    import torch_geometric.nn.conv as conv
    assert conv.GMMConv is GMMConv and "GMMConv" in conv.__all__ and "GMMConv" in nn.__all__
    torch.manual_seed(0)
    c = GMMConv(16, 24, dim=2, kernel_size=25)
    assert repr(c) == "GMMConv(16, 24)"
    assert c.aggr == "mean" and c.flow == "source_to_target" and not c.separate_gaussians
    assert c.g.shape == (16, 24 * 25) and c.mu.shape == (25, 2) and c.sigma.shape == (25, 2)
    assert c.root.shape == (16, 24) and c.bias.shape == (24,)
    for t in (c.g, c.mu, c.sigma, c.root):
        bound = math.sqrt(6.0 / (t.shape[-2] + t.shape[-1]))
        assert 0.9 * bound < float(t.detach().abs().max()) <= bound
    assert bool((c.bias.detach() == 0).all())
    assert sorted(n for n, _ in c.named_parameters()) == ["bias", "g", "mu", "root", "sigma"]
    c = GMMConv(3, 4, 2, 5, separate_gaussians=True, aggr="add", root_weight=False, bias=False,
                flow="target_to_source")
    assert c.root is None and c.bias is None and c.aggr == "add" and c.flow == "target_to_source"
    assert c.g.shape == (3, 4 * 5) and c.mu.shape == (3, 4, 5, 2) and c.sigma.shape == (3, 4, 5, 2)
    bound = math.sqrt(6.0 / (5 + 2))
    assert 0.9 * bound < float(c.mu.detach().abs().max()) <= bound
    assert sorted(n for n, _ in c.named_parameters()) == ["g", "mu", "sigma"]


def test_fused_path_predicate():
    from torch_geometric.nn import GMMConv
    assert GMMConv(3, 4, 2, 5).fused() and GMMConv(3, 4, 2, 5, aggr="add").fused()
    assert GMMConv(3, 4, 2, 5, root_weight=False, bias=False, flow="target_to_source").fused()
    assert not GMMConv(3, 4, 2, 5, aggr="max").fused()
    assert not GMMConv(3, 4, 2, 5, separate_gaussians=True).fused()
    assert not GMMConv(3, 4, 2, 5, node_dim=1).fused()

    class Other(GMMConv):
        def message(self, x_j, pseudo):
            return super().message(x_j, pseudo) * 2

    class Updated(GMMConv):
        def update(self, aggr_out):
            return aggr_out + 1

    class Aggregated(GMMConv):
        def aggregate(self, inputs, index, dim_size):
            return super().aggregate(inputs, index, dim_size)

    class Plain(GMMConv):
        pass

    assert not Other(3, 4, 2, 5).fused() and not Updated(3, 4, 2, 5).fused() and not Aggregated(3, 4, 2, 5).fused()
    assert Plain(3, 4, 2, 5).fused()


def test_form_chooser_and_limits(lib):
    from mi355_mp import ops
    # a pure function of (K, D, Cin, Cout, E, N): the lower float count, ties to bins
    for K, D, ci, co, E, N in ((25, 2, 1, 32, 38000, 4800), (25, 2, 32, 64, 38000, 4800), (25, 3, 64, 64, 10 ** 6, 10 ** 5),
                               (25, 2, 64, 1, 10, 1000), (4, 3, 70, 2, 3000, 257), (5, 2, 6, 10, 3000, 257),
                               (1, 1, 1, 1, 1, 1), (2, 1, 3, 3, 0, 5)):
        want, b, g = R.gmm_form(K, D, ci, co, E, N)
        assert b == E * (D + ci) + 2 * N * K * ci and g == E * (D + K * co) + N * K * co
        assert ops.gmm_form(K, D, ci, co, E, N) == want
    assert ops.gmm_form(25, 2, 1, 32, 38000, 4800) == "bins" and ops.gmm_form(25, 2, 32, 64, 38000, 4800) == "bins"
    assert ops.gmm_form(25, 2, 64, 1, 10, 1000) == "gather" and ops.gmm_form(4, 3, 70, 2, 3000, 257) == "gather"
    assert ops.gmm_form(1, 1, 2, 4, 2, 1) == R.gmm_form(1, 1, 2, 4, 2, 1)[0]
    b, g = R.gmm_form(1, 1, 2, 4, 2, 1)[1:]
    assert (b, g) == (2 * 3 + 4, 2 * 5 + 4) and ops.gmm_form(1, 1, 2, 4, 2, 1) == "bins"
    assert R.gmm_form(2, 1, 1, 1, 2, 2)[1:] == (12, 10) and R.gmm_form(2, 1, 1, 2, 2, 2)[1:] == (12, 18)
    assert R.gmm_form(1, 3, 2, 3, 4, 4)[1:] == (36, 36) and ops.gmm_form(1, 3, 2, 3, 4, 4) == "bins"   # the tie
    # the limits at their edges
    assert ops.gmm_ok(25, 2, 1, 32) and ops.gmm_ok(25, 2, 32, 64) and ops.gmm_ok(25, 3, 64, 64) and ops.gmm_ok(1, 1, 1, 1)
    assert not ops.gmm_ok(0, 1, 1, 1) and not ops.gmm_ok(1, 0, 1, 1) and not ops.gmm_ok(1, 1, 0, 1)
    assert not ops.gmm_ok(1, 1, 1, 0) and not ops.gmm_ok(-2, 1, 1, 1)
    assert ops.gmm_ok(128, 8, 5, 5) and not ops.gmm_ok(128, 9, 5, 5) and not ops.gmm_ok(129, 8, 5, 5)
    assert ops.gmm_ok(1024, 1, 1024, 1024) and not ops.gmm_ok(1024, 1, 1025, 1) and not ops.gmm_ok(1024, 1, 1, 1025)
    assert ops.gmm_ok(1, 1, 1 << 20, 1 << 20) and not ops.gmm_ok(1, 1, (1 << 20) + 1, 1)
    # the chunk of the parameter gradient: a pure function of the shape, at least 1024 edges, bounded chunks
    assert ops.gmm_grad_chunk(0, 25, 2) == ops.gmm_grad_chunk(1, 25, 2) == ops.gmm_grad_chunk(4096 * 1024, 25, 2) == 1024
    assert ops.gmm_grad_chunk(4096 * 1024 + 1, 25, 2) == 1280
    for E, K, D in ((10 ** 7, 25, 3), (2 ** 31 - 1, 128, 8), (5000, 1, 1), (10 ** 9, 1, 1)):
        chunk = ops.gmm_grad_chunk(E, K, D)
        chunks = -(-E // chunk)
        assert chunk >= 1024 and chunks <= 4096 and chunks * 2 * K * D * 4 <= 8 << 20, (E, K, D, chunk)
        assert lib.mp_gmm_param_grad_workspace(E, K, D) >= chunks * 2 * K * D * 4
    with pytest.raises(ValueError, match="K \\* D"):
        ops.gmm_grad_chunk(10, 128, 9)


def test_no_cpu_fallback_and_documented_refusals(lib):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    from torch_geometric.nn import GMMConv
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="fused path"):
        GMMConv(2, 3, 1, 4, aggr="max")(torch.ones(2, 2), ei, torch.rand(2), form="bins")
    with pytest.raises(ValueError, match="fused path"):
        GMMConv(2, 3, 1, 4, separate_gaussians=True)(torch.ones(2, 2), ei, torch.rand(2), form="gather")
    with pytest.raises(ValueError, match="fused path"):
        GMMConv(2, 3, 1, 4)(torch.ones(2, 2), ei, torch.rand(2), form="bins")      # CPU tensors: not the fused path
    g = Graph(ei, 2, 2)
    x, p, mu, sigma, w = torch.ones(2, 2), torch.ones(2, 1), torch.ones(4, 1), torch.ones(4, 1), torch.ones(2, 12)
    with pytest.raises(NotImplementedError, match="max"):
        ops.gmm_propagate(g, x, p, mu, sigma, w, "max")
    with pytest.raises(ValueError, match="form"):
        ops.gmm_propagate(g, x, p, mu, sigma, w, "add", form="other")
    with pytest.raises(ValueError, match="reduce"):
        ops.gmm_propagate(g, x, p, mu, sigma, w, "min")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gmm_propagate(g, x, p, mu, sigma, w, "add")


# ---- the C-ABI rejects every bad argument before any launch -------------------

def test_gmm_entry_points_reject_bad_arguments(lib):
    from mi355_mp import _lib
    P = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    N, E, K, D, C = 257, 3000, 25, 3, 33
    Q = K * C
    g = _lib.MpCsr(P, P, P, None, None, None, N, E, 0, 0, 0, N, 0)

    def bins(g=g, p=P, ne=E, ldp=D, D_=D, mu=P, sigma=P, K_=K, x=P, ldx=C, C_=C, out=P, ldo=Q):
        return lib.mp_gmm_aggregate_bins_f32(g, p, ne, ldp, D_, mu, sigma, K_, x, ldx, C_, None, out, ldo, None)

    def gather(g=g, p=P, ne=E, ldp=D, D_=D, mu=P, sigma=P, K_=K, x=P, ldx=Q, C_=C, out=P, ldo=C):
        return lib.mp_gmm_aggregate_gather_f32(g, p, ne, ldp, D_, mu, sigma, K_, x, ldx, C_, None, None, out, ldo,
                                               None)

    def variant(**kw):
        f = dict(rowptr=P, col=P, eid=P, n_cols=N, n_ids=0)
        f.update(kw)
        return _lib.MpCsr(f["rowptr"], f["col"], f["eid"], None, None, None, N, E, 0, 0, 0, f["n_cols"], f["n_ids"])

    def rejected(fn, kw, needle):
        rc = fn(**kw)
        err = lib.mp_last_error().decode()
        assert rc == -1 and needle in err, (fn.__name__, kw, rc, err)

    for fn, cname, xname in ((bins, "Cin", "x"), (gather, "F", "y")):
        for kw, needle in [
                (dict(p=None), "pseudo is NULL"), (dict(mu=None), "mu is NULL"), (dict(sigma=None), "sigma is NULL"),
                (dict(x=None), "%s is NULL" % xname), (dict(out=None), "out is NULL"),
                (dict(K_=0), "K = 0"), (dict(K_=-3), "K = -3"), (dict(D_=0), "D = 0"), (dict(C_=0), "%s = 0" % cname),
                (dict(K_=128, D_=9, ldp=9, ldx=128 * C, ldo=128 * C), "K * D = 1152 above the limit K * D <= 1024"),
                (dict(K_=1025, D_=1, ldx=1025 * C, ldo=1025 * C), "K * D = 1025"),
                (dict(K_=1024, D_=1, C_=1025, ldx=1024 * 1025, ldo=1024 * 1025), "K * %s = 1049600" % cname),
                (dict(ne=E - 1), "n_p_edges = %d" % (E - 1)), (dict(ldp=D - 1), "ldp = %d" % (D - 1)),
                (dict(g=variant(n_ids=E + 1)), "n_p_edges"), (dict(g=variant(col=None)), "col is NULL"),
                (dict(g=variant(eid=None)), "eid is NULL"), (dict(g=variant(rowptr=None)), "rowptr is NULL"),
                (dict(g=variant(n_cols=0)), "n_cols"), (dict(g=None), "g is NULL")]:
            rejected(fn, kw, needle)
    rejected(bins, dict(ldo=Q - 1), "ldo = %d" % (Q - 1))
    rejected(bins, dict(ldx=C - 1), "ldx = %d" % (C - 1))
    rejected(gather, dict(ldx=Q - 1), "ldy = %d" % (Q - 1))
    rejected(gather, dict(ldo=C - 1), "ldo = %d" % (C - 1))

    WS = lib.mp_gmm_param_grad_workspace(E, K, D)
    assert WS >= 3 * 2 * K * D * 4 and lib.mp_gmm_param_grad_workspace(0, K, D) < WS

    def grad(rows=P, cols=P, ne=E, p=P, ldp=D, D_=D, mu=P, sigma=P, K_=K, dz=P, lddz=Q, x=P, ldx=C, C_=C, dmu=P,
             dsigma=P, dp=None, lddp=0, ws=P, wsb=WS):
        return lib.mp_gmm_param_grad_f32(rows, cols, ne, p, ldp, D_, mu, sigma, K_, dz, lddz, x, ldx, C_, dmu, dsigma,
                                         dp, lddp, ws, wsb, None)

    for kw, needle in [(dict(rows=None), "rows is NULL"), (dict(cols=None), "cols is NULL"),
                       (dict(p=None), "pseudo is NULL"), (dict(mu=None), "mu is NULL"),
                       (dict(sigma=None), "sigma is NULL"), (dict(dz=None), "dz is NULL"), (dict(x=None), "x is NULL"),
                       (dict(dmu=None), "dmu is NULL"), (dict(dsigma=None), "dsigma is NULL"),
                       (dict(ws=None), "ws is NULL"), (dict(ne=-1), "n_edges"),
                       (dict(ldp=D - 1), "ldp = %d" % (D - 1)), (dict(lddz=Q - 1), "lddz = %d" % (Q - 1)),
                       (dict(ldx=C - 1), "ldx = %d" % (C - 1)), (dict(dp=P, lddp=D - 1), "lddp = %d" % (D - 1)),
                       (dict(wsb=WS - 1), "ws holds %d bytes, the call needs %d" % (WS - 1, WS)),
                       (dict(wsb=0), "ws holds 0 bytes"),
                       (dict(wsb=lib.mp_gmm_param_grad_workspace(0, K, D)), "ws holds"),
                       (dict(K_=0), "K = 0"), (dict(D_=0), "D = 0"), (dict(C_=0), "Cin = 0"),
                       (dict(K_=128, D_=9, ldp=9, lddz=128 * C, wsb=1 << 40), "K * D = 1152")]:
        rejected(grad, kw, needle)
    assert lib.mp_gmm_ok(25, 2, 1, 32) == 1 and lib.mp_gmm_ok(128, 8, 5, 5) == 1 and lib.mp_gmm_ok(128, 9, 5, 5) == 0
    # the int64 returns are outside the symbols the raising view wraps: ops tests the sign
    assert _lib.SIGNATURES["mp_gmm_ok"][0] is _lib.i64 and _lib.SIGNATURES["mp_gmm_grad_chunk"][0] is _lib.i64
    for name in ("mp_gmm_aggregate_bins_f32", "mp_gmm_aggregate_gather_f32", "mp_gmm_param_grad_f32"):
        assert _lib.SIGNATURES[name][0] is _lib.i64 and name not in _lib.STATUS_RETURNING
    assert lib.mp_abi_version() == 7
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match=r"mp_gmm_param_grad_f32 failed \(code 1\): .*lddz"):
        ops._count_call(_lib.native(), "mp_gmm_param_grad_f32", P, P, E, P, D, D, P, P, K, P, Q - 1, P, C, C, P, P,
                        None, 0, P, WS, None)


def test_gmm_abi_rejections_under_asan():
    """tests/abi/abi_reject_gmm.c against the host-AddressSanitizer build of the
    library (make asan_gmm), run as a plain program: every rejection names its
    argument and the exact documented boundaries pass the checks."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_gmm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_gmm")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_gmm: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 60, r.stdout[-2000:]


def test_the_build_lists_the_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "mp_gmm.hip" in srcs and os.path.exists(os.path.join(CSRC, "mp_gmm.hip"))
    assert re.search(r"^asan_gmm: \$\(ASAN_DIR\)/abi_reject_gmm$", mk, re.M)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"asan_gmm"' in entry
    from mi355_mp import _lib
    for name in ("mp_gmm_ok", "mp_gmm_aggregate_bins_f32", "mp_gmm_aggregate_gather_f32", "mp_gmm_grad_chunk",
                 "mp_gmm_param_grad_workspace", "mp_gmm_param_grad_f32"):
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "mi355_mp.h")).read()
    assert "mp_gmm_param_grad_f32" in header and "upstream's autograd yields NaN" in header
