"""CPU tests of the nearest-neighbour feature (knn, knn_graph, nearest,
knn_interpolate, EdgeConv, DynamicEdgeConv): hand known answers of the restatement
(tests/_knn_ref.py) that the GPU tests check the kernels against, the committed
known-answer file, the public surface (exports, upstream's signatures and reprs,
refusals on the CPU), the bindings, and the C-ABI's rejection of every bad argument
of the mp_knn_* entry points from a C harness under the host-ASAN build of the
library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _knn_ref as R
from tests.golden import make_golden_knn as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def test_knn_on_a_line():
    x = np.asarray([0.0, 1.0, 4.0, 7.0, 10.0], dtype=np.float32)
    y = np.asarray([0.9, 8.0], dtype=np.float32)
    # 0.9: 1 (0.01), 0 (0.81), 4 (9.61); 8: 7 (1), 10 (4), 4 (16)
    assert R.knn(x, y, 3).tolist() == [[0, 0, 0, 1, 1, 1], [1, 0, 2, 3, 4, 2]]
    assert R.knn(x, y, 1).tolist() == [[0, 1], [1, 3]]
    pairs, d2 = R.knn_with_d2(x, y[1:], 2)
    assert pairs.tolist() == [[0, 0], [3, 4]] and d2.tolist() == [1.0, 4.0] and d2.dtype == np.float32


def test_ties_go_to_the_lower_index_on_a_lattice():
    gx, gy = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    x = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)     # index = 3 * x0 + x1
    centre = np.asarray([[1, 1]], dtype=np.float32)
    # itself, then the four at distance 1 in index order, then the four corners in index order
    assert R.knn(x, centre, 9)[1].tolist() == [4, 1, 3, 5, 7, 0, 2, 6, 8]
    assert R.knn(x, centre, 3)[1].tolist() == [4, 1, 3]
    # a cell centre is equally far from its four corners
    assert R.knn(x, np.asarray([[0.5, 0.5]], dtype=np.float32), 2)[1].tolist() == [0, 1]
    # the order of the rows decides, not the coordinates
    assert R.knn(x[::-1], centre, 3)[1].tolist() == [4, 1, 3]


def test_k_above_the_graph_gives_the_graph():
    x = np.asarray([0.0, 1.0, 2.0, 10.0, 11.0], dtype=np.float32)
    y = np.asarray([0.4, 10.6, 5.0], dtype=np.float32)
    bx, by = np.asarray([0, 0, 0, 2, 2]), np.asarray([0, 2, 1])
    # graph 0 has 3 points, graph 2 has 2, graph 1 has none on the x side
    assert R.knn(x, y, 4, bx, by).tolist() == [[0, 0, 0, 1, 1], [0, 1, 2, 4, 3]]
    assert R.knn(x, y, 4, bx, np.asarray([1, 1, 3])).shape == (2, 0)
    assert R.knn(x, y, 64).shape == (2, 15)


def test_knn_graph_keeps_upstreams_quirk():
    # k = 1: nodes 0 and 1 find themselves among their first k + 1 = 2 hits (the tie at distance 0 goes to the
    # lower index); node 2's two hits are 0 and 1 -- k + 1 coincident points of lower index -- so it keeps both
    x = np.asarray([[1, 1], [1, 1], [1, 1], [5, 5]], dtype=np.float32)
    ei = R.knn_graph(x, 1)
    assert ei.tolist() == [[1, 0, 0, 1, 0], [0, 1, 2, 2, 3]]
    assert np.bincount(ei[1]).tolist() == [1, 1, 2, 1]
    assert R.knn_graph(x, 1, flow="target_to_source").tolist() == [[0, 1, 2, 2, 3], [1, 0, 0, 1, 0]]
    assert R.knn_graph(x, 1, loop=True).tolist() == [[0, 0, 0, 3], [0, 1, 2, 3]]
    line = np.asarray([0.0, 1.0, 3.0], dtype=np.float32)
    assert R.knn_graph(line, 1).tolist() == [[1, 0, 1], [0, 1, 2]]
    assert R.knn_graph(line, 2, np.asarray([0, 0, 1])).tolist() == [[1, 0], [0, 1]]


def test_nearest_is_knn_with_the_roles_swapped():
    x = np.asarray([0.1, 4.9, 5.1, 2.5], dtype=np.float32)
    y = np.asarray([0.0, 5.0], dtype=np.float32)
    assert R.nearest(x, y).tolist() == [0, 1, 1, 0]                       # 2.5: a tie, the lower index
    assert np.array_equal(R.nearest(x, y), R.knn(y, x, 1)[1])
    bx, by = np.asarray([0, 0, 1, 1]), np.asarray([0, 1])
    assert R.nearest(x, y, bx, by).tolist() == [0, 0, 1, 1]
    with pytest.raises(ValueError):
        R.nearest(x, y, bx, np.asarray([0, 0]))                           # graph 1 has no y


def test_interpolation_by_hand():
    pos_x = np.asarray([0.0, 1.0, 3.0], dtype=np.float32)
    x = np.asarray([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], dtype=np.float32)
    out, scale, pairs, wn = R.knn_interpolate(x, pos_x, np.asarray([2.0, 1.0], dtype=np.float32), k=2)
    # y = 2: neighbours 1 and 2 at d2 = 1 each (the tie to the lower index first): the mean; y = 1 coincides
    # with point 1: w = 1e16 against 1, the point's own value to 1e-16
    assert pairs.tolist() == [[0, 0, 1, 1], [1, 2, 1, 0]]
    assert np.allclose(out[0], [3.0, 30.0]) and np.allclose(out[1], [2.0, 20.0], rtol=1e-15)
    assert scale.tolist() == [[4.0, 40.0], [2.0, 20.0]] and np.allclose(wn[:2], [0.5, 0.5])
    grad, gscale, deg = R.knn_interpolate_grad(np.ones((2, 2)), pairs, wn, 3)
    assert deg.tolist() == [1, 2, 1] and np.allclose(grad.sum(0), [2.0, 2.0])
    # a y whose graph holds no x: zeros
    out, _, pairs, _ = R.knn_interpolate(x, pos_x, np.asarray([2.0], dtype=np.float32), np.asarray([0, 0, 0]),
                                         np.asarray([1]), 2)
    assert pairs.shape == (2, 0) and out.tolist() == [[0.0, 0.0]]


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "knn", "knn_kat.npz"))
    ins = G.inputs()
    for name, v in zip(G.NAMES, ins):
        assert np.array_equal(kat[name], v) and kat[name].dtype == v.dtype, name
    want = G.answers(*ins)
    assert sorted(want) == sorted(k for k in kat.files if k not in G.NAMES)
    for k, v in want.items():
        assert np.array_equal(kat[k], v) and kat[k].dtype == v.dtype == np.int64, k
    # what the file is for: ties, duplicates, a graph missing on each side
    assert kat["lattice_centres_k1"][1].tolist() == [0, 1, 5, 10] == kat["nearest_lattice"].tolist()
    assert kat["lattice_self_k1"][1].tolist() == list(range(16))
    assert len(np.unique(kat["dups"], axis=0)) <= 5 and kat["dups_k1"][1].tolist() != list(range(24))
    per_y = np.bincount(kat["batch_k16"][0], minlength=sum(G.Y_SIZES))
    assert per_y.tolist() == [9] * 4 + [0] * 3 + [14] * 5
    assert kat["batch_k3"].shape == (2, 27) and not (kat["batch"] == 1).any() and not (kat["batch_y"] == 3).any()
    assert np.bincount(kat["graph_dups_k2"][1]).max() == 3                # the quirk: k + 1 neighbours


def test_exports_signatures_and_reprs():
    import torch_geometric.nn as nn
    import torch_geometric.nn.conv as conv
    import torch_geometric.nn.pool as pool
    import torch_geometric.nn.unpool as unpool
    for name in ("knn", "knn_graph", "nearest"):
        assert getattr(nn, name) is getattr(pool, name) and name in nn.__all__ and name in pool.__all__
    assert nn.knn_interpolate is unpool.knn_interpolate
    assert "knn_interpolate" in nn.__all__ and "knn_interpolate" in unpool.__all__
    for name in ("EdgeConv", "DynamicEdgeConv"):
        assert getattr(nn, name) is getattr(conv, name) and name in nn.__all__ and name in conv.__all__

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(nn.knn) == [("x", E), ("y", E), ("k", E), ("batch_x", None), ("batch_y", None), ("cosine", False)]
    assert params(nn.knn_graph) == [("x", E), ("k", E), ("batch", None), ("loop", False),
                                    ("flow", "source_to_target"), ("cosine", False)]
    assert params(nn.nearest) == [("x", E), ("y", E), ("batch_x", None), ("batch_y", None)]
    assert params(nn.knn_interpolate) == [("x", E), ("pos_x", E), ("pos_y", E), ("batch_x", None), ("batch_y", None),
                                          ("k", 3)]
    assert params(nn.EdgeConv.__init__)[1:3] == [("nn", E), ("aggr", "max")]
    assert params(nn.DynamicEdgeConv.__init__)[1:4] == [("nn", E), ("k", E), ("aggr", "max")]
    lin = torch.nn.Linear(6, 4)
    layer = nn.EdgeConv(lin)
    assert repr(layer) == "EdgeConv(nn=%r)" % lin and layer.aggr == "max"
    assert list(inspect.signature(layer.forward).parameters) == ["x", "edge_index"]
    assert list(inspect.signature(layer.message).parameters) == ["x_i", "x_j"]
    dyn = nn.DynamicEdgeConv(lin, 6, aggr="add")
    assert repr(dyn) == "DynamicEdgeConv(nn=%r, k=6)" % lin and dyn.aggr == "add" and dyn.k == 6
    assert isinstance(dyn, nn.EdgeConv) and list(inspect.signature(dyn.forward).parameters) == ["x", "batch"]
    assert inspect.signature(dyn.forward).parameters["batch"].default is None
    before = lin.weight.detach().clone()
    torch.manual_seed(1)
    layer.reset_parameters()
    assert not torch.equal(before, lin.weight)


def test_no_cpu_fallback(lib):
    from mi355_mp import ops
    from torch_geometric.nn import DynamicEdgeConv, knn, knn_graph, knn_interpolate, nearest
    pos = torch.rand(6, 3)
    batch = torch.zeros(6, dtype=torch.int64)
    for call in (lambda: knn(pos, pos, 2), lambda: knn(pos, pos, 2, batch, batch), lambda: knn_graph(pos, 2),
                 lambda: nearest(pos, pos), lambda: knn_interpolate(torch.rand(6, 4), pos, pos),
                 lambda: ops.knn_search(pos, pos, 2), lambda: ops.knn_slab(pos, pos, 2),
                 lambda: ops.knn_interpolate(torch.rand(6, 4), pos, pos),
                 lambda: DynamicEdgeConv(torch.nn.Linear(6, 4), 2)(pos)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # cosine is refused before anything else
    for call in (lambda: knn(pos, pos, 2, cosine=True), lambda: knn_graph(pos, 2, cosine=True)):
        with pytest.raises(NotImplementedError, match="cosine"):
            call()


def test_paths_and_limits(lib):
    from mi355_mp import ops
    assert ops.KNN_MAX_K == lib.mp_knn_max_k() == 64
    max_d = ops.knn_max_d()
    assert max_d == lib.mp_knn_max_d() >= 256
    paths = [ops.knn_path(D) for D in range(1, max_d + 1)]
    assert paths == [0] * 8 + [1] * (max_d - 8)
    for D in (0, -1, max_d + 1):
        with pytest.raises(ValueError, match="1 to %d columns" % max_d):
            ops.knn_path(D)
    assert ops.POINT_MAX_D == 8                                           # the point ops keep their own limit


def test_bindings(lib):
    from mi355_mp import _lib, ops
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("mp_knn_"))
    assert names == ["mp_knn_fill", "mp_knn_interpolate_f32", "mp_knn_max_d", "mp_knn_max_k", "mp_knn_path",
                     "mp_knn_search_f32", "mp_knn_workspace"]
    nat = _lib.native()
    # like the point-set calls they return int64_t, launches or -(code): not status symbols, the wrapper tests the sign
    for name in ("mp_knn_search_f32", "mp_knn_fill", "mp_knn_interpolate_f32", "mp_knn_path", "mp_knn_max_k",
                 "mp_knn_max_d"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int64 and name not in _lib.STATUS_RETURNING
        assert getattr(nat, name) is getattr(lib, name) and getattr(lib, name).errcheck is None
    assert _lib.SIGNATURES["mp_knn_workspace"][0] is ctypes.c_size_t
    assert lib.mp_abi_version() == 7 == _lib.ABI_VERSION
    # the pinned point-set names are untouched
    assert not [n for n in names if n.startswith(("mp_fps_", "mp_radius_", "mp_point_"))]
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    ws = lib.mp_knn_workspace(10, 4)
    with pytest.raises(RuntimeError, match=r"mp_knn_search_f32 failed \(code 1\): mp_knn_search_f32: k = 65 is outside "
                                           r"\[1, 64\]"):
        ops._count_call(nat, "mp_knn_search_f32", D, 3, 10, D, 3, 10, 3, None, D, 1, 65, D, 32, D, 1 << 20, None)
    with pytest.raises(RuntimeError, match=r"D = %d is outside \[1, %d\]" % (ops.knn_max_d() + 1, ops.knn_max_d())):
        ops._count_call(nat, "mp_knn_search_f32", D, 1000, 10, D, 1000, 10, ops.knn_max_d() + 1, None, D, 1, 4, D, 32, D,
                        1 << 20, None)
    with pytest.raises(RuntimeError, match="ws holds %d bytes" % (ws - 1)):
        ops._count_call(nat, "mp_knn_search_f32", D, 3, 10, D, 3, 10, 3, None, D, 1, 4, D, 32, D, ws - 1, None)
    assert lib.mp_knn_fill(10, 4, 41, D, D, 41 * 8, None, 0, D, 1 << 20, None) == -1
    assert "n_edges = 41" in lib.mp_last_error().decode()
    assert lib.mp_knn_interpolate_f32(D, 4, 10, 5, 10, 4, D, 1 << 20, D, 5, 10 * 5 * 4, None) == -1
    assert "ldx = 4 < C = 5" in lib.mp_last_error().decode()
    assert lib.mp_knn_path(9) == 1 and lib.mp_knn_path(0) == -1


def test_knn_abi_rejections_under_asan():
    """tests/abi/abi_reject_knn.c against the host-AddressSanitizer build of the
    library (make asan_knn), run as a plain program with nothing preloaded: every
    NULL pointer, every extent and workspace one byte short, negative sizes,
    n_y * k not below 2^31, D outside [1, MP_KNN_MAX_D] and k outside [1, 64], each
    answered with -(MP_ERR_ARG) and its text."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_knn"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_knn")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_knn: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 80, r.stdout[-2000:]


def test_makefile_lists_the_knn_unit_and_build_makes_the_harness():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "mp_knn.hip" in units
    assert "-ffp-contract=off" in mk                     # the distance arithmetic depends on it
    assert re.search(r"^asan_knn:", mk, flags=re.M)
    assert '"asan_knn"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
