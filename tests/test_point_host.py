"""CPU tests of the point-set feature (fps, radius, radius_graph, PointConv): hand
known answers of the restatement (tests/_point_ref.py) that the GPU tests check
the kernels against, the committed known-answer file, the keep count against
TopKPooling's rule, the path thresholds, the public surface (exports, refusals on
the CPU) and the C-ABI's rejection of every bad argument of the point-set entry
points from a C harness under the host-ASAN build of the library."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _point_ref as R
from tests import _pool_ref as P
from tests.golden import make_golden_point as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def test_fps_on_a_line():
    # from 0 the far end comes first, then the middle (4 is nearer to 0 than to 10: m = 16 against
    # m[7] = 9), then the points in order of their gap
    line = np.asarray([0.0, 1.0, 4.0, 7.0, 10.0], dtype=np.float32)
    assert R.fps_graph(line, 5, 0) == [0, 4, 2, 3, 1]
    assert R.fps_graph(line, 3, 4) == [4, 0, 2]
    assert R.fps_graph(line, 1, 2) == [2]
    # equal distances go to the lower index: from the middle both ends are 5 away
    assert R.fps_graph(np.asarray([0.0, 5.0, 10.0], dtype=np.float32), 3, 1) == [1, 0, 2]
    # two graphs: the output is grouped by graph and offset by its first row
    both = np.concatenate([line, line + 100])
    batch = np.asarray([0] * 5 + [1] * 5)
    assert R.fps(both, batch, 0.6).tolist() == [0, 4, 2, 5, 9, 7]
    assert R.fps(both, batch, 0.6, [4, 1]).tolist() == [4, 0, 2, 6, 9, 7]
    assert R.fps(both, batch, 1e-3).tolist() == [0, 5]


def test_fps_selects_duplicates_twice():
    # two distinct points, five rows, ratio 1.0: once both are taken every m is 0 and the argmax is row 0
    pos = np.asarray([[1, 1], [1, 1], [3, 3], [1, 1], [3, 3]], dtype=np.float32)
    assert R.fps(pos, None, 1.0).tolist() == [0, 2, 0, 0, 0]
    assert R.fps(pos, None, 1.0, [4]).tolist() == [4, 0, 0, 0, 0]
    assert R.fps(np.zeros((4, 3), dtype=np.float32), None, 1.0).tolist() == [0, 0, 0, 0]


def test_radius_boundary_is_inclusive_on_the_lattice():
    # the 3-4-5 triangle: (3, 4) lies exactly 5 from the origin
    x = np.asarray([[0, 0], [3, 0], [3, 4], [6, 8]], dtype=np.float32)
    y = np.asarray([[0, 0]], dtype=np.float32)
    assert R.radius(x, y, 5.0).tolist() == [[0, 0, 0], [0, 1, 2]]
    below = float(np.nextafter(np.float32(5), np.float32(0)))
    assert R.radius(x, y, below).tolist() == [[0, 0], [0, 1]]
    assert R.radius(x, y, 0.0).tolist() == [[0], [0]]
    assert R.d2(x, y[0]).tolist() == [0.0, 9.0, 25.0, 100.0]


def test_radius_cap_keeps_the_lowest_indices():
    x = np.asarray([0.0, 0.1, 0.2, 5.0, 0.3], dtype=np.float32)
    y = np.asarray([0.1, 5.0, 9.0], dtype=np.float32)
    assert R.radius(x, y, 1.0, max_num_neighbors=1).tolist() == [[0, 1], [0, 3]]
    assert R.radius(x, y, 1.0, max_num_neighbors=3).tolist() == [[0, 0, 0, 1], [0, 1, 2, 3]]
    assert R.radius(x, y, 1.0, max_num_neighbors=64).tolist() == [[0, 0, 0, 0, 1], [0, 1, 2, 4, 3]]
    # graphs pair by number; a graph may be missing on either side
    bx, by = np.asarray([0, 0, 0, 2, 2]), np.asarray([0, 1, 2])
    assert R.radius(x, y, 10.0, bx, by, 64).tolist() == [[0, 0, 0, 2, 2], [0, 1, 2, 3, 4]]
    assert R.radius(x, y, 10.0, bx, np.asarray([1, 1, 3]), 64).shape == (2, 0)


def test_radius_graph_keeps_upstreams_quirk():
    x = np.asarray([0.0, 0.1, 0.2, 0.3], dtype=np.float32)
    # the first two hits of nodes 2 and 3 are 0 and 1: their own index is not among them, so they keep both
    ei = R.radius_graph(x, 1.0, None, False, 1)
    assert ei.tolist() == [[1, 0, 0, 1, 0, 1], [0, 1, 2, 2, 3, 3]]
    assert R.radius_graph(x, 1.0, None, False, 1, "target_to_source").tolist() == [[0, 1, 2, 2, 3, 3],
                                                                                  [1, 0, 0, 1, 0, 1]]
    assert R.radius_graph(x, 1.0, None, True, 1).tolist() == [[0, 0, 0, 0], [0, 1, 2, 3]]


def test_edge_features_by_hand():
    ps = np.asarray([[1, 2], [3, 5]], dtype=np.float32)
    pd = np.asarray([[10, 20]], dtype=np.float32)
    xs = np.asarray([[7], [8]], dtype=np.float32)
    assert R.edge_features(xs, ps, pd, [1, 0], [0, 0]).tolist() == [[8, -7, -15], [7, -9, -18]]
    assert R.edge_features(None, ps, pd, [1], [0]).tolist() == [[-7, -15]]


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "point", "point_kat.npz"))
    names = ("pos", "y", "feat", "batch", "batch_y", "start")
    ins = G.inputs()
    for name, v in zip(names, ins):
        assert np.array_equal(kat[name], v) and kat[name].dtype == v.dtype, name
    want = G.answers(*ins)
    assert sorted(want) == sorted(k for k in kat.files if k not in names)
    for k, v in want.items():
        assert np.array_equal(kat[k], v) and kat[k].dtype == v.dtype, k
    assert kat["fps_half"].tolist() != kat["fps_half_start"].tolist()
    assert len(kat["fps_all"]) == sum(G.SIZES) and len(set(kat["fps_all"].tolist())) < sum(G.SIZES)   # duplicates
    full, capped = kat["radius_cap32"], kat["radius_cap2"]
    assert capped.shape[1] < full.shape[1] and np.bincount(capped[0]).max() == 2
    assert len(set(full[0].tolist())) < sum(G.Y_SIZES)                                               # a query finds nothing
    assert kat["edge_features"].shape == (full.shape[1], 7) and kat["edge_features"].dtype == np.float32


def test_keep_count_is_the_topk_rule():
    sizes = [0, 1, 2, 3, 63, 64, 65, 130, 257, 1000, 1025, 4097, (1 << 24) + 1]
    for ratio in (1.0, 0.5, 0.25, 0.1, 1e-3, 0.3, 0.7, 1.0 / 3.0):
        want = torch.minimum(P.keep_counts(ratio, torch.tensor(sizes)), torch.tensor(sizes)).tolist()
        assert [R.keep_count(ratio, s) for s in sizes] == want, ratio
    assert R.keep_count(1e-3, 1025) == 2 and R.keep_count(1e-3, 1000) == 1 and R.keep_count(0.5, 1) == 1


def test_fps_path_is_monotone(lib):
    from mi355_mp import ops
    paths = [ops.fps_path(n) for n in range(0, 20000)]
    assert all(a <= b for a, b in zip(paths, paths[1:])) and sorted(set(paths)) == [0, 1, 2]
    assert paths[1] == 0 and paths[64] == 0 and ops.fps_path(1 << 30) == 2
    assert lib.mp_fps_path(65) == paths[65]


def test_exports():
    import torch_geometric.nn as nn
    import torch_geometric.nn.conv as conv
    import torch_geometric.nn.pool as pool
    for name in ("fps", "radius", "radius_graph"):
        assert getattr(nn, name) is getattr(pool, name) and name in nn.__all__ and name in pool.__all__
    assert nn.PointConv is conv.PointConv and "PointConv" in nn.__all__ and "PointConv" in conv.__all__
    assert list(inspect.signature(nn.fps).parameters) == ["x", "batch", "ratio", "random_start"]
    assert list(inspect.signature(nn.radius).parameters) == ["x", "y", "r", "batch_x", "batch_y", "max_num_neighbors"]
    assert list(inspect.signature(nn.radius_graph).parameters) == ["x", "r", "batch", "loop", "max_num_neighbors",
                                                                   "flow"]
    assert inspect.signature(nn.fps).parameters["ratio"].default == 0.5
    assert inspect.signature(nn.radius).parameters["max_num_neighbors"].default == 32
    lin = torch.nn.Linear(3, 4)
    layer = nn.PointConv(lin, None)
    assert repr(layer) == "PointConv(local_nn=%r, global_nn=None)" % lin and layer.aggr == "max"
    assert list(inspect.signature(layer.forward).parameters) == ["x", "pos", "edge_index"]
    before = lin.weight.detach().clone()
    torch.manual_seed(1)
    layer.reset_parameters()
    assert not torch.equal(before, lin.weight)


def test_no_cpu_fallback(lib):
    from mi355_mp import ops
    from torch_geometric.nn import PointConv, fps, radius, radius_graph
    pos = torch.rand(6, 3)
    ei = torch.tensor([[0, 1], [1, 0]])
    for call in (lambda: fps(pos), lambda: radius(pos, pos, 0.5), lambda: radius_graph(pos, 0.5),
                 lambda: ops.point_edge_features(None, pos, pos, ei[0], ei[1]),
                 lambda: PointConv()(None, (pos, pos), ei)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bindings(lib):
    from mi355_mp import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("mp_fps_", "mp_radius_", "mp_point_")))
    assert names == ["mp_fps_f32", "mp_fps_path", "mp_fps_workspace", "mp_point_edge_features_f32", "mp_radius_fill",
                     "mp_radius_search_f32", "mp_radius_workspace"]
    nat = _lib.native()
    # like the graclus calls they return int64_t, a count or -(code): not status symbols, the wrapper tests the sign
    for name in ("mp_fps_f32", "mp_radius_search_f32", "mp_radius_fill", "mp_point_edge_features_f32"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int64 and name not in _lib.STATUS_RETURNING
        assert getattr(nat, name) is getattr(lib, name) and getattr(lib, name).errcheck is None
    # the path is an answer, not a status: int64_t, so the raising view leaves it alone
    assert _lib.SIGNATURES["mp_fps_path"][0] is ctypes.c_int64 and "mp_fps_path" not in _lib.STATUS_RETURNING
    assert _lib.native().mp_fps_path is lib.mp_fps_path and lib.mp_fps_path.errcheck is None
    assert _lib.SIGNATURES["mp_fps_workspace"][0] is ctypes.c_size_t
    assert lib.mp_abi_version() == 7
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match=r"mp_fps_f32 failed \(code 1\): mp_fps_f32: D = 9 is outside \[1, 8\]"):
        ops._count_call(nat, "mp_fps_f32", D, 9, 10, 9, D, 1, 10, D, None, D, 80, D, 32, D, 256, None)
    with pytest.raises(RuntimeError, match="negative or not finite"):
        ops._count_call(nat, "mp_radius_search_f32", D, 3, 10, D, 3, 10, 3, None, D, 1, float("nan"), 4, D, 32, D,
                        1 << 20, None)
    assert lib.mp_radius_fill(10, 4, 41, D, D, 41 * 8, D, 1 << 20, None) == -1
    assert "n_edges = 41" in lib.mp_last_error().decode()


def test_point_abi_rejections_under_asan():
    """tests/abi/abi_reject_point.c against the host-AddressSanitizer build of the
    library (make asan_point), run as a plain program with nothing preloaded: every
    NULL pointer, every extent and workspace one byte short, sizes negative or not
    below 2^31, D outside [1, 8], a radius negative, NaN or infinite and a cap of 0,
    each answered with -(MP_ERR_ARG) and its text."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_point"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_point")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_point: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 90, r.stdout[-2000:]


def test_makefile_lists_the_point_unit_and_build_makes_the_harness():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "mp_point.hip" in units
    assert "-ffp-contract=off" in mk                     # the distance arithmetic depends on it
    assert "asan_point" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
