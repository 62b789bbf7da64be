"""CPU tests of the graclus feature: hand known answers of the restatement
(tests/_graclus_ref.py) that the GPU tests check the kernels against, pinned
values of the priority's two words, handshake == greedy on random graphs with
heavy weight ties, the committed known-answer file, the public surface (exports,
refusals on the CPU), normalized_cut by hand, and the C-ABI's rejection of every
bad argument of the graclus entry points from a C harness under the host-ASAN
build of the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _graclus_ref as R
from tests.golden import make_golden_graclus as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")

HAND = R.HAND


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


@pytest.mark.parametrize("name,ei,w,n,want", HAND, ids=[h[0] for h in HAND])
def test_hand_answers(name, ei, w, n, want):
    for seed in (0, 1, 12345):
        assert R.greedy(ei, w, n, seed).tolist() == want
        cluster, rounds = R.handshake(ei, w, n, seed)
        assert cluster.tolist() == want
        assert (rounds == 0) == all(u == v for u, v in zip(*ei))
        R.check_matching(cluster, ei)


def test_unweighted_answers_follow_the_hash():
    # a path of 3: the hash of (0, 1) against that of (1, 2) decides, and differs between seeds 0 and 1
    path = [[0, 1], [1, 2]]
    assert R.pair_hash(0, 0, 1) < R.pair_hash(0, 1, 2) and R.pair_hash(1, 0, 1) > R.pair_hash(1, 1, 2)
    assert R.greedy(path, None, 3, 0).tolist() == [0, 1, 1] and R.greedy(path, None, 3, 1).tolist() == [0, 0, 2]
    # equal weights leave it to the hash as well
    assert R.greedy(path, [2.0, 2.0], 3, 0).tolist() == [0, 1, 1]
    assert R.greedy([[0, 3], [1, 2]], None, None, 0).tolist() == [0, 0, 2, 2]       # num_nodes from the index
    with pytest.raises(IndexError):
        R.greedy(path, None, 2, 0)
    with pytest.raises(IndexError):
        R.handshake([[0], [-1]], None, 2, 0)


def test_priority_words_are_pinned():
    for w, want in ((0.0, 0x80000000), (-0.0, 0x7FFFFFFF), (1.0, 0xBF800000), (-1.0, 0x407FFFFF),
                    (1e-45, 0x80000001), (-1e-45, 0x7FFFFFFE), (float("inf"), 0xFF800000),
                    (-float("inf"), 0x007FFFFF)):
        assert R.wkey(w) == want, w
    ws = [-float("inf"), -3.5, -1e-45, -0.0, 0.0, 1e-45, 0.1, 3.5, float("inf")]
    assert [R.wkey(w) for w in ws] == sorted(R.wkey(w) for w in ws) and len(set(map(R.wkey, ws))) == len(ws)
    assert R.mix64(0) == 0xE220A8397B1DCDAF and R.mix64(1) == 0x910A2DEC89025CC1
    for seed, a, b, want in ((0, 0, 1, 0x08B4FDA8), (0, 1, 2, 0x64A28FC2), (1, 0, 1, 0xE9FD6049),
                             (7, 123, 456789, 0x35A76F49), ((1 << 64) - 1, 0, (1 << 31) - 1, 0x6024251E),
                             (-1, 5, 6, 0x908C770D)):
        assert R.pair_hash(seed, a, b) == want, (seed, a, b)
    from mi355_mp import ops
    assert all(ops._mix64(z) == R.mix64(z) for z in (0, 1, 0xDEADBEEF, (1 << 64) - 1))
    keys = R.priorities([[3, 1, 2], [1, 3, 2]], [0.5, -0.5, 1.0], 7)
    assert keys == [(R.wkey(0.5), R.pair_hash(7, 1, 3), 1, 3), (R.wkey(-0.5), R.pair_hash(7, 1, 3), 1, 3), None]


def test_handshake_equals_greedy_on_random_graphs():
    rng = np.random.default_rng(5)
    most = 0
    for case in range(300):
        n = int(rng.integers(1, 30))
        E = int(rng.integers(0, 4 * n + 1))
        ei = rng.integers(0, n, (2, E))
        w = None if case % 3 == 0 else (rng.integers(0, 3, E) - 1).astype(np.float32)      # three values: ties abound
        seed = int(rng.integers(0, 1 << 62))
        want = R.greedy(ei, w, n, seed)
        got, rounds = R.handshake(ei, w, n, seed)
        assert np.array_equal(got, want), case
        R.check_matching(got, ei)
        most = max(most, rounds)
    assert most >= 3
    # one round per pair on a path whose weights increase along it
    n = 40
    ei = [list(range(n - 1)), list(range(1, n))]
    got, rounds = R.handshake(ei, np.arange(n - 1, dtype=np.float32), n, 0)
    assert rounds == n // 2 and got.tolist() == [i - i % 2 for i in range(n)]


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "graclus", "graclus_kat.npz"))
    ei, w, n = G.inputs()
    assert np.array_equal(kat["edge_index"], ei) and np.array_equal(kat["weight"], w) and int(kat["num_nodes"]) == n
    want = G.answers(ei, w, n)
    assert sorted(want) == sorted(k for k in kat.files if k not in ("edge_index", "weight", "num_nodes"))
    for k, v in want.items():
        assert np.array_equal(kat[k], v) and kat[k].dtype == v.dtype, k
    assert not np.array_equal(kat["cluster_unweighted_0"], kat["cluster_unweighted_1"])
    assert int((kat["cluster_weighted_0"] != np.arange(n)).sum()) >= n // 4
    assert bool((ei[0] == ei[1]).any())                                   # the batch has loops
    for seed in G.SEEDS:
        assert np.array_equal(R.greedy(ei, w, n, seed), kat["cluster_weighted_%d" % seed])


def test_normalized_cut_hand_values():
    ei = [[0, 0, 1, 2], [1, 2, 0, 0]]                                     # deg = (2, 1, 1)
    out = R.normalized_cut(ei, [1.0, 2.0, 4.0, 8.0])
    assert out.tolist() == [1.5, 3.0, 6.0, 12.0]
    # a node that starts no edge has degree 0: 1 / 0 = inf, as upstream
    assert R.normalized_cut([[0], [1]], [1.0], 2).tolist() == [float("inf")]


def test_exports():
    from torch_geometric.nn import graclus
    from torch_geometric.utils import normalized_cut
    import torch_geometric.nn as nn
    import torch_geometric.nn.pool as pool
    import torch_geometric.utils as utils
    assert nn.graclus is pool.graclus is graclus and "graclus" in nn.__all__ and "graclus" in pool.__all__
    assert utils.normalized_cut is normalized_cut and "normalized_cut" in utils.__all__
    import inspect
    sig = inspect.signature(graclus)
    assert list(sig.parameters) == ["edge_index", "weight", "num_nodes", "seed"]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["seed"].default == 0


def test_no_cpu_fallback(lib):
    from mi355_mp import ops
    from torch_geometric.nn import graclus
    from torch_geometric.utils import normalized_cut
    ei = torch.tensor([[0, 1], [1, 0]])
    w = torch.ones(2)
    for call in (lambda: graclus(ei), lambda: graclus(ei, w, 2, seed=1), lambda: normalized_cut(ei, w),
                 lambda: ops.graclus_match(ei, None, 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bindings(lib):
    from mi355_mp import _lib
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("mp_graclus_"))
    assert names == ["mp_graclus_init", "mp_graclus_rounds", "mp_graclus_workspace"]
    assert _lib.SIGNATURES["mp_graclus_workspace"][0] is ctypes.c_size_t
    nat = _lib.native()
    for name in ("mp_graclus_init", "mp_graclus_rounds"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int64 and name not in _lib.STATUS_RETURNING
        assert getattr(nat, name) is getattr(lib, name) and getattr(lib, name).errcheck is None
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    ws = lib.mp_graclus_workspace(10, 20)
    assert ws >= 10 * 4 + 10 + 40 * 8
    assert lib.mp_graclus_init(D, D, None, 0, 20, 10, 0, D, 160, D, 80, D, 32, D, ws - 1, None) == -1
    assert "ws holds %d" % (ws - 1) in lib.mp_last_error().decode()
    assert lib.mp_graclus_rounds(D, 44, D, 160, 20, 1 << 30, 0, 8, D, 80, D, 32, D, ws, None) == -1
    assert "not below 2^30" in lib.mp_last_error().decode()
    # the Python wrapper raises on the sign itself, in the raising view's format
    from mi355_mp import ops
    with pytest.raises(RuntimeError) as e:
        ops._graclus_call(nat, "mp_graclus_rounds", D, 44, D, 160, 20, 10, 0, 4097, D, 80, D, 32, D, ws, None)
    assert str(e.value) == "mp_graclus_rounds failed (code 1): " + lib.mp_last_error().decode()
    assert "n_rounds = 4097" in str(e.value)


def test_graclus_abi_rejections_under_asan():
    """tests/abi/abi_reject_graclus.c against the host-AddressSanitizer build of the
    library (make asan_graclus), run as a plain program with nothing preloaded:
    every NULL pointer, every extent and the workspace one byte short, negative
    sizes and sizes >= 2^30 of both entry points, each answered with -(code) and
    its text."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_graclus"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_graclus")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_graclus: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 40, r.stdout[-2000:]


def test_makefile_lists_the_graclus_unit_and_build_makes_the_harness():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "mp_graclus.hip" in units
    assert "asan_graclus" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
