"""CPU tests of the SplineConv feature: hand known answers of the float64
restatement (tests/_spline_ref.py) that the GPU tests check the kernels against,
the small host-side pieces (repeat, Cartesian, the layer's parameters), and the
C-ABI's rejection of every bad argument of the spline entry points -- from
Python with fake device pointers and from a C harness under the host-ASAN
build of the library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _spline_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


# ---- the restatement: hand known answers ------------------------------------

def test_restatement_hand_values():
    b, wi = R.basis(torch.tensor([[0.5, 1.0]]), [5, 5], [1, 1], 1)
    assert b.tolist() == [[1.0, 0.0, 0.0, 0.0]] and wi.tolist() == [[22, 23, 2, 3]]
    b, wi = R.basis(torch.tensor([[0.25]]), [2], [1], 1)
    assert b.tolist() == [[0.75, 0.25]] and wi.tolist() == [[0, 1]]
    b, wi = R.basis(torch.tensor([[1.0]]), [5], [0], 1)           # closed: index 5 wraps to 0
    assert b.tolist() == [[1.0, 0.0]] and wi.tolist() == [[0, 1]]
    b, wi = R.basis(torch.tensor([[0.3]], dtype=torch.float32), [5], [1], 2)
    assert wi.tolist() == [[0, 1, 2]]
    assert np.allclose(b.numpy(), [[0.005, 0.59, 0.405]], rtol=0, atol=1e-6)


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_restatement_partition_of_unity_and_index_range(D, M):
    ks, op = [5, 3, 4][:D], [1, 0, 1][:D]
    g = torch.Generator().manual_seed(10 * D + M)
    u = torch.rand(400, D, generator=g)
    u[0], u[1] = 0.0, 1.0
    u[2:2 + D] = torch.eye(D)
    b, wi = R.basis(u, ks, op, M)
    K = int(np.prod(ks))
    assert b.shape == (400, (M + 1) ** D) and wi.shape == b.shape
    assert int(wi.min()) >= 0 and int(wi.max()) < K
    assert float(b.min()) >= 0.0
    assert torch.allclose(b.sum(1), torch.ones(400, dtype=torch.float64), rtol=0, atol=1e-12)


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "spline", "spline_kat.npz"))
    for D in (1, 2, 3):
        u = torch.from_numpy(kat["pseudo_d%d" % D])
        for M in (1, 2, 3):
            b, wi = R.basis(u, [5, 3, 4][:D], [1, 0, 1][:D], M)
            assert np.array_equal(wi.numpy(), kat["index_d%d_m%d" % (D, M)]), (D, M)
            assert np.abs(b.numpy() - kat["basis_d%d_m%d" % (D, M)]).max() <= 1e-15, (D, M)


def test_restatement_layer_is_the_per_edge_loop():
    """spline_conv (vectorised) against the literal per-edge, per-s loop."""
    g = torch.Generator().manual_seed(3)
    n, E, fi, fo = 7, 40, 3, 2
    ei = torch.randint(0, n, (2, E), generator=g)
    u = torch.rand(E, 2, generator=g)
    x = torch.randn(n, fi, generator=g)
    W = torch.randn(6, fi, fo, generator=g)
    root, bias = torch.randn(fi, fo, generator=g), torch.randn(fo, generator=g)
    for aggr in ("add", "mean"):
        for flow in ("source_to_target", "target_to_source"):
            out = R.spline_conv(x, ei, u, W, root, bias, [3, 2], [1, 0], 1, aggr, flow)
            b, wi = R.basis(u, [3, 2], [1, 0], 1)
            i, j = (1, 0) if flow == "source_to_target" else (0, 1)
            want = torch.zeros(n, fo, dtype=torch.float64)
            deg = torch.zeros(n)
            for e in range(E):
                for s in range(4):
                    want[ei[i, e]] += b[e, s] * (x[ei[j, e]].double() @ W[wi[e, s]].double())
                deg[ei[i, e]] += 1
            if aggr == "mean":
                want = want / deg.clamp(min=1).double().view(-1, 1)
            want = want + x.double() @ root.double() + bias.double()
            assert torch.allclose(out, want, rtol=0, atol=1e-12), (aggr, flow)


# ---- small host-side pieces -------------------------------------------------

def test_repeat():
    from torch_geometric.utils import repeat
    assert repeat(5, 3) == [5, 5, 5]
    assert repeat([1, 2], 4) == [1, 2, 2, 2]
    assert repeat([1, 2, 3], 2) == [1, 2]
    assert repeat([True, False], 2) == [True, False]
    assert repeat(None, 2) is None


def test_cartesian_hand_values():
    from torch_geometric.data import Data
    from torch_geometric.transforms import Cartesian
    pos = torch.tensor([[0.0, 0.0], [2.0, 0.0], [0.0, -4.0]])
    ei = torch.tensor([[0, 1, 0], [1, 0, 2]])
    d = Cartesian()(Data(pos=pos, edge_index=ei))                  # pos[col] - pos[row], / (2 * 4) + 0.5
    assert torch.equal(d.edge_attr, torch.tensor([[0.75, 0.5], [0.25, 0.5], [0.5, 0.0]]))
    d = Cartesian(norm=False)(Data(pos=pos, edge_index=ei))
    assert torch.equal(d.edge_attr, torch.tensor([[2.0, 0.0], [-2.0, 0.0], [0.0, -4.0]]))
    d = Cartesian(max_value=8.0)(Data(pos=pos, edge_index=ei, edge_attr=torch.tensor([1.0, 2.0, 3.0])))
    assert torch.equal(d.edge_attr, torch.tensor([[1.0, 0.625, 0.5], [2.0, 0.375, 0.5], [3.0, 0.5, 0.25]]))
    d = Cartesian(cat=False)(Data(pos=pos, edge_index=ei, edge_attr=torch.ones(3)))
    assert d.edge_attr.shape == (3, 2)


def test_layer_parameters_repr_and_init_bounds():
    from torch_geometric.nn import SplineConv
    import torch_geometric.nn.conv as conv
    assert conv.SplineConv is SplineConv
    torch.manual_seed(0)
    c = SplineConv(3, 8, dim=2, kernel_size=5)
    assert repr(c) == "SplineConv(3, 8, dim=2)"
    assert c.weight.shape == (25, 3, 8) and c.root.shape == (3, 8) and c.bias.shape == (8,)
    assert c.kernel_size.tolist() == [5, 5] and c.is_open_spline.tolist() == [1, 1]
    assert set(dict(c.named_buffers())) == {"kernel_size", "is_open_spline"}
    bound = 1.0 / math.sqrt(3 * 25)
    assert float(c.weight.detach().abs().max()) <= bound and float(c.weight.detach().abs().max()) > 0.9 * bound
    assert float(c.root.detach().abs().max()) <= bound and float(c.bias.detach().abs().max()) == 0.0
    c = SplineConv(1, 4, dim=3, kernel_size=[5, 3], is_open_spline=[True, False], degree=2, aggr="add",
                   root_weight=False, bias=False)
    assert c.kernel_size.tolist() == [5, 3, 3] and c.is_open_spline.tolist() == [1, 0, 0]
    assert c.weight.shape == (45, 1, 4) and c.root is None and c.bias is None and c.aggr == "add"


def test_loaded_buffers_are_the_geometry_the_kernels_get():
    """kernel_size / is_open_spline are buffers: a state dict with other
    per-dimension values (same K) must change what the layer launches with."""
    from torch_geometric.nn import SplineConv
    a = SplineConv(2, 3, dim=2, kernel_size=[6, 2], is_open_spline=[False, True])
    b = SplineConv(2, 3, dim=2, kernel_size=[3, 4], is_open_spline=True)
    assert (b._kernel_size, b._is_open_spline) == ([3, 4], [1, 1])
    b.load_state_dict(a.state_dict())
    assert b.kernel_size.tolist() == [6, 2] and b.is_open_spline.tolist() == [0, 1]
    assert (b._kernel_size, b._is_open_spline) == ([6, 2], [0, 1])


def test_no_cpu_fallback_and_documented_refusals(lib):
    from mi355_mp import ops
    from mi355_mp.graph import Graph
    from torch_geometric.nn import SplineConv
    ei = torch.tensor([[0, 1], [1, 0]])
    c = SplineConv(2, 3, dim=1, kernel_size=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c(torch.ones(2, 2), ei, torch.rand(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spline_basis(torch.rand(4, 2), [5, 5], [1, 1], 1)
    g = Graph(ei, 2, 2)
    x, w, u = torch.ones(2, 2), torch.ones(2, 2, 3), torch.rand(2, 1)
    with pytest.raises(NotImplementedError, match="max"):
        ops.spline_propagate(g, x, w, u, [2], [1], 1, "max")
    with pytest.raises(NotImplementedError, match="pseudo"):
        ops.spline_propagate(g, x, w, u.clone().requires_grad_(True), [2], [1], 1, "mean")
    # the limits of the fused path, each named
    for ks, op, deg, D, needle in (([7, 7, 7], [1, 1, 1], 1, 3, "K <= 256"), ([3], [1], 3, 1, "< 1"),
                                   ([5], [1], 4, 1, "degree"), ([2, 2, 2, 2], [1, 1, 1, 1], 1, 4, "D = 4")):
        with pytest.raises(NotImplementedError, match=needle):
            ops._spline_geom(ks, op, deg, D)
    ks_a, op_a, K, S = ops._spline_geom(torch.tensor([5, 5]), torch.tensor([1, 0], dtype=torch.uint8), 2, 2)
    assert (list(ks_a), list(op_a), K, S) == ([5, 5], [1, 0], 25, 9)
    assert ops.spline_form(2, 1433, 16, 2) == "bins" and ops.spline_form(4, 1, 32, 25) == "bins"
    assert ops.spline_form(4, 32, 64, 25) == "bins" and ops.spline_form(2, 16, 7, 2) == "bins"
    assert ops.spline_form(8, 64, 64, 125) == "gather" and ops.spline_form(8, 1, 32, 125) == "bins"


# ---- the C-ABI rejects every bad argument before any launch -------------------

def test_spline_entry_points_reject_bad_arguments(lib):
    import ctypes
    from mi355_mp import _lib
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    N, E, F, K = 257, 3000, 33, 25
    g = _lib.MpCsr(D, D, D, None, None, None, N, E, 0, 0, 0, N, 0)
    ks = (ctypes.c_int32 * 2)(5, 5)
    op = (ctypes.c_int32 * 2)(1, 1)
    big = (ctypes.c_int32 * 3)(7, 7, 7)
    op3 = (ctypes.c_int32 * 3)(1, 1, 1)
    small = (ctypes.c_int32 * 1)(3)
    op1 = (ctypes.c_int32 * 1)(1)

    def bins(g=g, pseudo=D, ne=E, D_=2, ks=ks, op=op, deg=1, x=D, ldx=F, F_=F, out=D, ldo=K * F):
        return lib.mp_spline_aggregate_bins_f32(g, pseudo, ne, D_, ks, op, deg, x, ldx, F_, None, out, ldo, None)

    def gather(g=g, pseudo=D, ne=E, D_=2, ks=ks, op=op, deg=1, x=D, ldx=K * F, F_=F, out=D, ldo=F):
        return lib.mp_spline_aggregate_gather_f32(g, pseudo, ne, D_, ks, op, deg, x, ldx, F_, None, None, out, ldo,
                                                  None)

    def variant(**kw):
        f = dict(rowptr=D, col=D, eid=D, n_cols=N, n_ids=0)
        f.update(kw)
        return _lib.MpCsr(f["rowptr"], f["col"], f["eid"], None, None, None, N, E, 0, 0, 0, f["n_cols"], f["n_ids"])

    for fn in (bins, gather):
        cases = [
            (dict(pseudo=None), "pseudo is NULL"), (dict(x=None), "x is NULL"), (dict(out=None), "out is NULL"),
            (dict(ks=None), "kernel_size is NULL"), (dict(op=None), "is_open is NULL"),
            (dict(D_=0), "D = 0"), (dict(D_=4, ks=big, op=op3), "D = 4"), (dict(deg=0), "degree = 0"),
            (dict(deg=4), "degree = 4"), (dict(D_=3, ks=big, op=op3), "K <= 256"),
            (dict(D_=1, ks=small, op=op1, deg=3), "< 1"), (dict(F_=0), "F = 0"),
            (dict(ne=E - 1), "n_pseudo_edges = %d" % (E - 1)),
            (dict(g=variant(n_ids=E + 1)), "n_pseudo_edges"),
            (dict(g=variant(col=None)), "col is NULL"), (dict(g=variant(eid=None)), "eid is NULL"),
            (dict(g=variant(rowptr=None)), "rowptr is NULL"), (dict(g=variant(n_cols=0)), "n_cols"),
            (dict(g=None), "g is NULL"),
        ]
        for kw, needle in cases:
            rc = fn(**kw)
            err = lib.mp_last_error().decode()
            assert rc == 1 and needle in err, (fn.__name__, kw, rc, err)
    for fn, kw, needle in ((bins, dict(ldo=K * F - 1), "ldo = %d" % (K * F - 1)), (bins, dict(ldx=F - 1), "ldx"),
                           (gather, dict(ldx=K * F - 1), "ldx = %d" % (K * F - 1)), (gather, dict(ldo=F - 1), "ldo")):
        rc = fn(**kw)
        err = lib.mp_last_error().decode()
        assert rc == 1 and needle in err, (fn.__name__, kw, rc, err)

    # the standalone basis: extents of both outputs (S = 4)
    need_b, need_w = E * 4 * 4, E * 4 * 8
    for bb, wb, what, need in ((need_b - 1, need_w, "basis", need_b), (0, need_w, "basis", need_b),
                               (need_b, need_w - 1, "weight_index", need_w)):
        rc = lib.mp_spline_basis_f32(D, E, 2, ks, op, 1, D, bb, D, wb, None)
        err = lib.mp_last_error().decode()
        assert rc == 1 and what in err and str(need) in err, (bb, wb, rc, err)
    for args, needle in (((None, E, 2, ks, op, 1, D, need_b, D, need_w, None), "pseudo is NULL"),
                         ((D, E, 2, ks, op, 1, None, need_b, D, need_w, None), "basis is NULL"),
                         ((D, E, 2, ks, op, 1, D, need_b, None, need_w, None), "weight_index is NULL"),
                         ((D, -1, 2, ks, op, 1, D, need_b, D, need_w, None), "n_edges"),
                         ((D, E, 3, big, op3, 1, D, need_b * 2, D, need_w * 2, None), "K <= 256")):
        rc = lib.mp_spline_basis_f32(*args)
        assert rc == 1 and needle in lib.mp_last_error().decode(), (args, lib.mp_last_error())
    assert lib.mp_spline_ok(2, 1, ks, op, 1) == 1 and lib.mp_spline_ok(3, 1, big, op3, 1) == 0
    assert lib.mp_spline_ok(1, 3, small, op1, 1) == 0 and lib.mp_spline_ok(2, 1, ks, op, 0) == 0


def test_spline_abi_rejections_under_asan():
    """tests/abi/abi_reject_spline.c against the host-AddressSanitizer build of
    the library (make asan_spline), run as a plain program: every rejection
    names its argument, the exact documented boundaries pass the checks, and
    the D-entry kernel_size / is_open host arrays are never read past their end."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_spline"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_spline")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_spline: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 45, r.stdout[-2000:]


def test_makefile_variant_rule_links_the_spline_object():
    """An A/B variant library must hold every unit of the main one (without
    mp_spline.o or mp_gemm.o it lacks symbols and _lib.load() fails on it), each
    compiled with the variant's DEFS: a knob may live in any unit."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = [u[:-len(".hip")] for u in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()]
    assert "mp_spline" in units and "mp_gemm" in units
    assert sorted(u + ".hip" for u in units) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    r = subprocess.run(["make", "-n", "-C", CSRC, "variant", "NAME=t", "DEFS=-DMP_TEST_KNOB=3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    link = [ln for ln in lines if "-shared" in ln and "lib_t.so" in ln]
    assert len(link) == 1, r.stdout[-4000:]
    objs = [w for w in link[0].split() if w.endswith(".o")]
    assert sorted(objs) == sorted(["build/v_t/%s.o" % u for u in units] + ["build/mp_version.o"]), link[0]
    for u in units:
        cc = [ln for ln in lines if " -c %s.hip " % u in ln]
        assert len(cc) == 1, (u, cc)
        assert "-DMP_TEST_KNOB=3" in cc[0].split() and "build/v_t/%s.o" % u in cc[0].split(), cc[0]
