"""CPU tests of the attention readout feature: the float64 restatement
(tests/_glob_ref.py) against its literal per-graph loop and the committed known
answers, graphs without nodes, the fp32 fact that lets the kernels divide by den
alone, the path query, the C-ABI's rejection of every bad argument (a C harness
under the host-ASAN build of the library, run as a plain program), the Compose
and Distance transforms, and the two layers' host-side pieces."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _glob_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def _starts(sizes):
    return torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)


@pytest.mark.parametrize("sizes", [[3, 1, 4], [0, 2, 5], [2, 0, 0, 5], [2, 5, 0, 0], [0], [6]])
@pytest.mark.parametrize("mode", ["q", "s"])
def test_restatement_is_the_per_graph_loop(sizes, mode):
    """Graphs without nodes first, in the middle and last: r = 0, m = den = 0."""
    g = torch.Generator().manual_seed(len(sizes) * 10 + sum(sizes))
    n, C = sum(sizes), 3
    x = torch.randn(n, C, generator=g)
    kw = {"q": torch.randn(len(sizes), C, generator=g)} if mode == "q" else {"score": torch.randn(n, generator=g)}
    got, want = R.readout(x, _starts(sizes), **kw), R.readout_loop(x, _starts(sizes), **kw)
    for a, b in zip(got, want):
        assert a.dtype == torch.float64 and a.shape == b.shape
        assert a.numel() == 0 or float((a - b).abs().max()) <= 1e-13
    r, _, m, den, a = got
    for i, s in enumerate(sizes):
        if s == 0:
            assert float(r[i].abs().max()) == 0.0 and float(m[i]) == 0.0 and float(den[i]) == 0.0
        else:
            assert float(den[i]) >= 1.0
            assert abs(float(a[int(_starts(sizes)[i]):int(_starts(sizes)[i + 1])].sum()) - 1.0) <= 1e-12


def test_restatement_hand_values():
    """Two nodes with scores 0 and ln 3: a = (1/4, 3/4)."""
    x = torch.tensor([[4.0, 0.0], [0.0, 8.0]])
    r, e, m, den, a = R.readout(x, [0, 2], score=torch.tensor([0.0, np.log(3.0)]))
    assert torch.allclose(a, torch.tensor([0.25, 0.75], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(r, torch.tensor([[1.0, 6.0]], dtype=torch.float64), atol=1e-12)
    assert abs(float(m[0]) - np.log(3.0)) < 1e-7 and abs(float(den[0]) - 4.0 / 3.0) < 1e-7
    # query mode: e = x . q
    r, e, *_ = R.readout(x, [0, 1, 2], q=torch.tensor([[1.0, 1.0], [0.5, 0.25]]))
    assert e.tolist() == [4.0, 2.0] and r.tolist() == x.tolist()        # one node per graph: r = x


def test_restatement_gradients_match_the_formulas():
    """Float64 autograd through readout gives the backward the header states."""
    sizes = [4, 0, 3]
    g = torch.Generator().manual_seed(2)
    x, q, dr = (torch.randn(7, 5, generator=g).double(), torch.randn(3, 5, generator=g).double(),
                torch.randn(3, 5, generator=g).double())
    got = R.readout_grads(x, _starts(sizes), dr, q=q)
    r, e, m, den, a = R.readout(x, _starts(sizes), q=q)
    batch = torch.tensor([0] * 4 + [2] * 3)
    s = (dr * r).sum(-1)
    de = a * ((dr[batch] * x).sum(-1) - s[batch])
    dx = a[:, None] * dr[batch] + de[:, None] * q[batch]
    dq = torch.zeros(3, 5, dtype=torch.float64).index_add(0, batch, de[:, None] * x)
    assert float((got["dx"] - dx).abs().max()) <= 1e-12 and float((got["dq"] - dq).abs().max()) <= 1e-12
    score = torch.randn(7, generator=g).double()
    got = R.readout_grads(x, _starts(sizes), dr, score=score)
    r, e, m, den, a = R.readout(x, _starts(sizes), score=score)
    de = a * ((dr[batch] * x).sum(-1) - (dr * r).sum(-1)[batch])
    assert float((got["dx"] - a[:, None] * dr[batch]).abs().max()) <= 1e-12
    assert float((got["dscore"] - de).abs().max()) <= 1e-12


def test_restatement_matches_the_committed_known_answers():
    spec = importlib.util.spec_from_file_location("make_golden_glob",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_glob.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    kat = np.load(os.path.join(ROOT, "tests", "golden", "glob", "glob_kat.npz"))
    t = {k: torch.from_numpy(kat[k]) for k in mk.inputs()}
    for k, v in mk.inputs().items():
        assert torch.equal(t[k], v), k                              # the generator still draws the committed inputs
    got = mk.answers(t, R.readout)
    assert len(got) == 5 * len(mk.CASES)
    for k, v in got.items():
        assert v.dtype == torch.float64 and (v.numel() == 0 or np.abs(v.numpy() - kat[k]).max() <= 1e-13), k


def test_layers_restatement_on_a_shuffled_batch():
    """set2set and global_attention are set functions: a permuted batch gives the same rows."""
    g = torch.Generator().manual_seed(4)
    batch = torch.tensor([0, 0, 0, 2, 2, 3])
    x = torch.randn(6, 3, generator=g).double()
    lstm = torch.nn.LSTM(6, 3).double()
    perm = torch.tensor([5, 2, 0, 4, 1, 3])
    with torch.no_grad():
        a, b = R.set2set(x, batch, lstm, 3), R.set2set(x[perm], batch[perm], lstm, 3)
    assert a.shape == (4, 6) and float((a - b).abs().max()) <= 1e-12
    assert float(a[1, 3:].abs().max()) == 0.0                         # graph 1 has no node: r = 0
    gate = torch.nn.Linear(3, 1).double()
    with torch.no_grad():
        o = R.global_attention(x, batch, 5, gate)
        r = R.readout(x, [0, 3, 3, 5, 6, 6], score=gate(x).view(-1))[0]
    assert o.shape == (5, 3) and float((o - r).abs().max()) <= 1e-12


def test_one_plus_1e_16_is_one_in_fp32():
    """Upstream divides by den + 1e-16; den >= 1 for a graph with a node, so in
    fp32 that is den itself and the kernels divide by den."""
    one = np.float32(1) + np.float32(1e-16)
    assert one == np.float32(1) and one.dtype == np.float32
    for den in (1.0, 1.5, 3.0, 1e6):
        assert np.float32(den) + np.float32(1e-16) == np.float32(den)
    assert bool(torch.tensor(1.0) + 1e-16 == torch.tensor(1.0))


def test_readout_path_query(lib):
    from mi355_mp import ops
    for C in (1, 3, 4, 33, 64, 65, 200, 260, 5000):
        paths = [lib.mp_readout_path(n, C) for n in list(range(0, 3000)) + [1 << 14, 1 << 17, 1 << 24]]
        assert paths == sorted(paths) and set(paths) == {0, 1, 2}, C      # monotone in n_g, every path taken
        assert paths[0] == 0 and paths[1] == 0
        chunk = lib.mp_readout_chunk(C)
        assert chunk >= 1 and lib.mp_readout_path(chunk, C) < 2          # a split graph has more than one chunk
        assert ops.readout_path(40, C) == lib.mp_readout_path(40, C) and ops.readout_chunk(C) == chunk
    assert lib.mp_readout_path(29, 64) == 0 and lib.mp_readout_path(33, 128) == 0   # QM9, ENZYMES: a wave per graph
    assert lib.mp_readout_path(1 << 17, 64) == 2
    for C in (0, -1):
        assert lib.mp_readout_path(5, C) == -1 and b"C" in lib.mp_last_error()   # -MP_ERR_ARG
        assert lib.mp_readout_chunk(C) == -1
        with pytest.raises(ValueError):
            ops.readout_path(5, C)
    assert lib.mp_readout_path(-1, 4) == -1


def test_workspace_one_byte_short_is_rejected(lib):
    D = 0x7F0000000000                                                # fake device pointer: never dereferenced
    n, G, C, mx = 5000, 7, 33, 3000
    need = lib.mp_readout_workspace(n, G, mx, C)
    assert need >= (n // lib.mp_readout_chunk(C) + G) * (C + 2) * 4
    assert lib.mp_readout_workspace(n, G, 8, C) < need                # no split graph: no chunk slots
    ob = ((G - 1) * C + C) * 4
    rc = lib.mp_attention_readout_f32(D, C, n, C, D, G, mx, D, C, None, D, C, ob, None, 0, D, n * 4, D, G * 8, None, 0,
                                      D, need - 1, None)
    assert rc == -1 and b"ws holds %d bytes, the call needs %d" % (need - 1, need) in lib.mp_last_error()
    rc = lib.mp_attention_readout_bwd_f32(D, C, D, C, n, C, D, G, mx, D, C, D, D, D, C, D, C, ((n - 1) * C + C) * 4, D, C,
                                          ob, None, 0, D, need - 1, None)
    assert rc == -1 and b"ws holds" in lib.mp_last_error()


def test_abi_rejections_as_a_plain_program():
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_glob"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", HIP_VISIBLE_DEVICES="",
               ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_glob")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_glob: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 50, r.stdout[-500:]
    assert r.stdout.count("holds") >= 10                              # every extent, one byte short


def test_compose_and_distance():
    from torch_geometric.data import Data
    from torch_geometric.transforms import Cartesian, Compose, Distance
    pos = torch.tensor([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0]])
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    d = Distance(norm=False)(Data(pos=pos, edge_index=ei))
    assert torch.allclose(d.edge_attr, torch.tensor([[5.0], [18.0 ** 0.5], [1.0]]))
    d = Distance()(Data(pos=pos, edge_index=ei))
    assert torch.allclose(d.edge_attr, torch.tensor([[1.0], [18.0 ** 0.5 / 5], [0.2]]))
    d = Distance(max_value=10.0)(Data(pos=pos, edge_index=ei, edge_attr=torch.tensor([7.0, 8.0, 9.0])))
    assert torch.allclose(d.edge_attr, torch.tensor([[7.0, 0.5], [8.0, 18.0 ** 0.5 / 10], [9.0, 0.1]]))
    d = Distance(norm=False, cat=False)(Data(pos=pos, edge_index=ei, edge_attr=torch.ones(3, 2)))
    assert d.edge_attr.shape == (3, 1)
    d = Distance()(Data(pos=pos, edge_index=torch.zeros((2, 0), dtype=torch.int64)))
    assert d.edge_attr.shape == (0, 1)
    both = Compose([Cartesian(norm=False), Distance(norm=False)])
    d = both(Data(pos=pos, edge_index=ei))
    assert torch.allclose(d.edge_attr, torch.tensor([[3.0, 4.0, 5.0], [-3.0, -3.0, 18.0 ** 0.5], [0.0, -1.0, 1.0]]))
    assert repr(Distance(norm=False)) == "Distance(norm=False, max_value=None)"
    assert repr(both).startswith("Compose([\n    Cartesian(") and repr(both).endswith("\n])")


def test_layers_import_and_repr():
    from torch_geometric.nn import GlobalAttention, Set2Set
    from torch_geometric.nn.glob import GlobalAttention as GA2, Set2Set as S2
    assert GA2 is GlobalAttention and S2 is Set2Set
    s = Set2Set(64, processing_steps=3)
    assert repr(s) == "Set2Set(64, 128)" and s.out_channels == 128 and s.processing_steps == 3
    assert isinstance(s.lstm, torch.nn.LSTM) and (s.lstm.input_size, s.lstm.hidden_size, s.lstm.num_layers) == (128, 64, 1)
    assert Set2Set(4, 2, num_layers=2).lstm.num_layers == 2
    before = s.lstm.weight_ih_l0.clone()
    s.reset_parameters()
    assert not torch.equal(before, s.lstm.weight_ih_l0)
    gate, nn = torch.nn.Linear(4, 1), torch.nn.Linear(4, 2)
    assert repr(GlobalAttention(gate)) == "GlobalAttention(gate_nn=%r, nn=None)" % gate
    assert repr(GlobalAttention(gate, nn)) == "GlobalAttention(gate_nn=%r, nn=%r)" % (gate, nn)
    # no GPU here: the layers hand a host tensor to the engine's recipe ops, which refuse it
    with pytest.raises(RuntimeError, match="ROCm"):
        GlobalAttention(gate)(torch.randn(3, 4), torch.tensor([0, 0, 1]), 2)
