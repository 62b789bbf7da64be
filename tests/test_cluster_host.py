"""CPU tests of the cluster-pooling feature: hand known answers of the restatement
(tests/_cluster_ref.py) that the GPU tests check the kernels against, the committed
known-answer file, the public surface (exports, refusals on the CPU), and the
C-ABI's rejection of every bad argument of the cluster entry points from a C
harness under the host-ASAN build of the library."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _cluster_ref as R
from tests.golden import make_golden_cluster as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def test_voxel_grid_hand_values():
    pos = torch.tensor([[0.0, 0.0], [4.99, 27.9], [5.0, 5.0], [27.99, 27.99], [28.0, 0.0], [-0.5, 3.0], [-5.0, 3.0]])
    batch = torch.tensor([0, 0, 0, 1, 1, 1, 1])
    # m = (6, 6, 2): key = cx + 6 * cy + 36 * b; -0.5 / 5 truncates to 0 (collides), -5 / 5 = -1 (negative term)
    assert R.voxel_grid(pos, batch, 5, 0, 28).tolist() == [0, 30, 7, 36 + 5 + 30, 36 + 5, 36, 36 - 1]
    # 1-D positions; start / end None: the column minimum / maximum (the batch column too)
    p1 = torch.tensor([1.0, 2.0, 3.5, 9.0])
    b1 = torch.tensor([1, 1, 2, 2])
    assert R.voxel_grid(p1, b1, 2.0).tolist() == [0, 0, 1 + 5, 4 + 5]
    # 0.1 is not a float32: the quotient of float32 operands decides the cell
    q = (torch.tensor([0.3, 0.7], dtype=torch.float32) / torch.tensor(0.1, dtype=torch.float32)).long().tolist()
    assert R.voxel_grid(torch.tensor([0.3, 0.7]), torch.zeros(2, dtype=torch.int64), 0.1, 0, 1).tolist() == q


def test_consecutive_cluster_hand_values():
    src = torch.tensor([7, -3, 7, 1 << 40, -3, 7, 0])
    inv, perm = R.consecutive_cluster(src)
    assert inv.tolist() == [2, 0, 2, 3, 0, 2, 1] and perm.tolist() == [4, 6, 5, 3]


def test_pool_hand_graph():
    cluster = torch.tensor([5, 5, 9, 2, 9, 5])                       # -> inv [1, 1, 2, 0, 2, 1]
    x = torch.tensor([[1.0, -20000.0], [1.0, -30000.0], [0.5, 2.0], [-1.0, 0.0], [0.5, 3.0], [0.0, -20000.0]])
    pos = torch.arange(12.0).view(6, 2)
    batch = torch.tensor([0, 0, 0, 1, 1, 1])
    ei = torch.tensor([[0, 1, 2, 3, 4, 0, 5, 2], [1, 2, 3, 0, 3, 4, 4, 4]])
    attr = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    p = R.pool(cluster, x, pos, batch, ei, attr)
    assert p["inv"].tolist() == [1, 1, 2, 0, 2, 1] and p["perm"].tolist() == [3, 5, 4]
    assert p["x"].tolist() == [[-1.0, 0.0], [1.0, 0.0], [0.5, 3.0]]          # -20000 wins cluster 1, then masked
    assert p["arg"].tolist() == [[3, 3], [0, 0], [2, 4]]                      # ties: the lowest node index
    assert p["pos"].tolist() == [[6.0, 7.0], [4.0, 5.0], [6.0, 7.0]] and p["batch"].tolist() == [1, 1, 1]
    # edges: (1,1) loop, (1,2), (2,0), (0,1), (2,0), (1,2), (1,2), (2,2) loop -> sorted distinct pairs
    assert p["edge_index"].tolist() == [[0, 1, 2], [1, 2, 0]]
    assert p["edge_attr"].tolist() == [8.0, 2.0 + 32.0 + 64.0, 4.0 + 16.0]
    assert p["edge_slot"].tolist() == [-1, 1, 2, 0, 2, 1, 1, -1]
    # every edge a loop: nothing is coalesced, the attributes are an empty selection
    q = R.pool(torch.zeros(6, dtype=torch.int64), x, pos, None, ei, attr)
    assert q["edge_index"].shape == (2, 0) and q["edge_attr"].shape == (0,) and q["batch"] is None
    with pytest.raises(IndexError):
        R.pool(cluster, x, pos, batch, torch.tensor([[0], [6]]), None)


def test_float64_form_is_the_forward():
    pos, batch, x, ei, attr = G.inputs()
    key = R.voxel_grid(pos, batch, 5, 0, 28)
    p = R.pool(key, x, pos, batch, ei, attr)
    M, Ep = p["perm"].numel(), p["edge_index"].size(1)
    for reduce in ("max", "mean"):
        want = p["x"] if reduce == "max" else R.scatter_mean(x, p["inv"], M)
        xo, po, ao = R.pool_f64(x.double(), pos.double(), attr.double(), p["inv"], p["arg"], p["edge_slot"], M, Ep,
                                reduce)
        assert torch.allclose(xo, want.double(), rtol=1e-6, atol=1e-6)
        assert torch.allclose(po, p["pos"].double(), rtol=1e-6, atol=1e-5)
        assert torch.allclose(ao, p["edge_attr"].double(), rtol=1e-6, atol=1e-6)


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "cluster", "cluster_kat.npz"))
    pos, batch, x, ei, attr = G.inputs()
    for name, t in (("pos", pos), ("batch", batch), ("x", x), ("edge_index", ei), ("edge_attr", attr)):
        assert np.array_equal(kat[name], t.numpy()), name
    for i, (size, start, end) in enumerate(G.SETTINGS):
        assert np.array_equal(R.voxel_grid(pos, batch, size, start, end).numpy(), kat["key_%d" % i]), i
    assert np.array_equal(R.voxel_grid(pos, batch, [5, 0.1]).numpy(), kat["key_auto"])
    p = R.pool(torch.from_numpy(kat["key_0"]), x, pos, batch, ei, attr)
    for k in ("inv", "perm", "x", "arg", "pos", "batch", "edge_index", "edge_attr", "edge_slot"):
        assert np.array_equal(p[k].numpy(), kat["pool_" + k]), k
    assert 1 < p["perm"].numel() < pos.size(0) and 0 < p["edge_index"].size(1) < ei.size(1)


def test_exports():
    from torch_geometric.nn import voxel_grid, max_pool, max_pool_x, avg_pool, avg_pool_x
    import torch_geometric.nn as nn
    import torch_geometric.nn.pool as pool
    for name in ("voxel_grid", "consecutive_cluster", "max_pool", "max_pool_x", "avg_pool", "avg_pool_x", "pool_edge",
                 "pool_batch", "pool_pos"):
        assert getattr(nn, name) is getattr(pool, name) and name in nn.__all__ and name in pool.__all__
    assert callable(voxel_grid) and callable(max_pool) and callable(max_pool_x)
    assert callable(avg_pool) and callable(avg_pool_x)


def test_no_cpu_fallback(lib):
    from torch_geometric.data import Data
    from torch_geometric.nn import (avg_pool_x, consecutive_cluster, max_pool, max_pool_x, pool_edge, pool_pos,
                                    voxel_grid)
    pos = torch.rand(4, 2)
    batch = torch.zeros(4, dtype=torch.int64)
    cluster = torch.tensor([0, 1, 0, 1])
    ei = torch.tensor([[0, 1], [1, 0]])
    data = Data(x=torch.ones(4, 2), pos=pos, edge_index=ei)
    data.batch = batch
    for call in (lambda: voxel_grid(pos, batch, 0.5), lambda: consecutive_cluster(cluster),
                 lambda: max_pool(cluster, data), lambda: max_pool_x(cluster, data.x, batch),
                 lambda: max_pool_x(cluster, data.x, batch, size=2), lambda: avg_pool_x(cluster, data.x, batch),
                 lambda: pool_edge(cluster, ei), lambda: pool_pos(cluster, pos)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bindings_and_launch_cap(lib):
    from mi355_mp import _lib
    names = [n for n in _lib.SIGNATURES if n.startswith(("mp_cluster_", "mp_voxel_"))]
    assert sorted(names) == ["mp_cluster_build", "mp_cluster_build_workspace", "mp_cluster_edge_attr_bwd_f32",
                             "mp_cluster_edge_attr_f32", "mp_cluster_edges", "mp_cluster_edges_workspace",
                             "mp_cluster_max_blocks", "mp_cluster_reduce_f32", "mp_voxel_keys_f32"]
    assert lib.mp_cluster_max_blocks() == 2048
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    for n, needle in ((-1, "n = -1"), (1 << 31, "not below 2^31")):
        assert lib.mp_voxel_keys_f32(D, 2, n, 2, D, D, D, D, D, 1 << 40, None) == 1
        assert needle in lib.mp_last_error().decode()
        assert lib.mp_cluster_build(D, n, D, 1 << 40, D, 1 << 40, D, 1 << 40, D, 1 << 40, D, D, 1 << 40, None) == 1
        assert needle in lib.mp_last_error().decode()
    assert lib.mp_voxel_keys_f32(D, 9, 10, 9, D, D, D, D, D, 80, None) == 1
    assert "D = 9" in lib.mp_last_error().decode()
    assert lib.mp_voxel_keys_f32(D, 2, 10, 2, D, D, D, D, None, 80, None) == 1
    assert "key is NULL" in lib.mp_last_error().decode()
    assert lib.mp_voxel_keys_f32(D, 2, 10, 2, D, D, D, D, D, 79, None) == 1
    assert "key holds 79" in lib.mp_last_error().decode()


def test_cluster_abi_rejections_under_asan():
    """tests/abi/abi_reject_cluster.c against the host-AddressSanitizer build of the
    library (make asan_cluster), run as a plain program with nothing preloaded: NULL
    outputs, short extents, D > 8, negative n and n >= 2^31 of every entry point."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_cluster"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_cluster")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_cluster: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 100, r.stdout[-2000:]


def test_makefile_lists_the_cluster_unit_and_build_makes_the_harness():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "mp_cluster.hip" in units
    assert "asan_cluster" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
