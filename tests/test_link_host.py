"""CPU tests of the link-prediction feature (GAE, VGAE, InnerProductDecoder,
negative_sampling, structured_negative_sampling, to_undirected,
train_test_split_edges): hand known answers of the restatement (tests/_link_ref.py)
that the GPU tests check the kernels against, the committed known-answer file, the
host-side pieces of the public surface (the split, the metrics, VGAE's formulas,
exports, upstream's signatures and reprs, refusals on the CPU), the bindings, and
the C-ABI's rejection of every bad argument of the link entry points from a C
harness under the host-ASAN build of the library."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _link_ref as R
from tests.golden import make_golden_link as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def _pairs(ei):
    return [(int(a), int(b)) for a, b in np.asarray(ei).T]


def test_hash_is_the_engines_key_mix():
    from mi355_mp import ops
    for z in (0, 1, 0x5EED, (1 << 64) - 1, 0x0123456789ABCDEF):
        assert R.mix64(z) == ops._mix64(z)
    assert R.mix64(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0
    assert all(0 <= R.draw(3, s, 7) < 7 for s in range(200))
    assert {R.draw(3, s, 7) for s in range(200)} == set(range(7))
    assert R.draw(3, 5, 1) == 0 and R.draw(1, 0, 1 << 62) != R.draw(2, 0, 1 << 62)


def test_kth_missing_against_brute_force():
    rng = np.random.default_rng(5)
    for n in list(range(1, 13)) + [31, 64, 65]:
        total = n * n
        for density in (0.0, 0.2, 0.9):
            keys = sorted(int(k) for k in np.nonzero(rng.random(total) < density)[0])
            if len(keys) == total:
                keys = keys[:-1]
            missing = [t for t in range(total) if t not in set(keys)]
            for r in sorted({0, len(missing) // 2, len(missing) - 1}):
                assert R.kth_missing(keys, r) == missing[r] == R.kth_missing_brute(keys, r, total)
    # a single non-edge: every draw lands on it
    keys = [t for t in range(49) if t != 30]
    assert {R.kth_missing(keys, R.draw(9, s, 1)) for s in range(50)} == {30}
    # a segment with a base, as the row mode searches it
    assert [R.kth_missing([20, 21, 23], r, base=20) for r in range(3)] == [2, 4, 5]


def test_path_graph_only_non_edges():
    row, col = [0, 1, 2, 3], [1, 2, 3, 4]
    edges = set(zip(row, col))
    out = R.negative_sample(row, col, 5, seed=1, num_neg_samples=21)
    assert out.shape == (2, 21) and not (set(_pairs(out)) & edges)     # the cap: min(21, 25 - 4)
    seen = set()
    for seed in range(40):
        seen |= set(_pairs(R.negative_sample(row, col, 5, seed, num_neg_samples=21)))
    assert seen == {(i, j) for i in range(5) for j in range(5)} - edges
    # upper: the pairs i < j joined in neither direction, each with its mirror
    up = R.negative_sample(row, col, 5, seed=1, upper=True)
    assert up.shape == (2, 4) and np.array_equal(up[:, :2], up[::-1, 2:])
    assert all(i < j and abs(i - j) > 1 for i, j in _pairs(up[:, :2]))
    # the loop rewrite: no (i, i) comes back, and the count follows E - loops + N = 9
    lp = R.negative_sample(row, col, 5, seed=1, loops=True)
    assert lp.shape == (2, 9) and all(i != j for i, j in _pairs(lp)) and not (set(_pairs(lp)) & edges)


def test_complete_minus_one_returns_the_missing_pair():
    full = [(i, j) for i in range(6) for j in range(6) if (i, j) != (4, 2)]
    row, col = [p[0] for p in full], [p[1] for p in full]
    out = R.negative_sample(row, col, 6, seed=3)
    assert out.shape == (2, 1) and _pairs(out) == [(4, 2)]                 # min(35, 36 - 35)
    keys, _ = R.key_table(row, col, 6)
    assert {R.kth_missing(keys, R.draw(seed, s, 1)) for seed in range(5) for s in range(20)} == {4 * 6 + 2}
    # upper: (2, 4) is joined by (2, 4) itself, so nothing is missing and nothing is drawn
    assert R.negative_sample(row, col, 6, seed=3, upper=True).shape == (2, 0)
    # rows: node 4 misses column 2 only; every other node is linked to all: -1
    k = R.structured_negative_sample(row, col, 6, seed=3)
    assert [int(v) for v, i in zip(k, row) if i == 4] == [2] * 5
    assert all(int(v) == -1 for v, i in zip(k, row) if i != 4)


def test_full_row_gives_minus_one():
    row, col = [0, 0, 0, 1], [0, 1, 2, 2]
    k = R.structured_negative_sample(row, col, 3, seed=11)
    assert k[:3].tolist() == [-1, -1, -1] and int(k[3]) in (0, 1)
    for seed in range(30):
        assert int(R.structured_negative_sample(row, col, 3, seed)[3]) in (0, 1)


def test_triangular_inverse():
    assert [R.tri_inverse(t) for t in range(6)] == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]
    assert [R.tri_key(i, j) for i, j in ((0, 1), (0, 2), (1, 2))] == [0, 1, 2]
    wrong = 0
    for j in (1 << 31, (1 << 31) + 1, 3037000498, 2147483647, 1518500250):
        for i in (0, 1, j // 2, j - 2, j - 1):
            t = R.tri_key(i, j)
            assert R.tri_inverse(t) == (i, j)
            wrong += R.tri_inverse_float_only(t) != (i, j)
    assert abs(R.tri_key(0, 1 << 31) - (1 << 61)) <= 1 << 30
    assert wrong > 0                                              # the float inverse alone is off near 2^61
    for t in (0, 1, 2, (1 << 61) - 1, 1 << 61, (1 << 61) + 1, (1 << 62) - 1):
        i, j = R.tri_inverse(t)
        assert 0 <= i < j and R.tri_key(i, j) == t


def test_to_undirected_and_split():
    from torch_geometric.data import Data
    from torch_geometric.utils import to_undirected, train_test_split_edges
    ei = torch.tensor([[3, 0, 0, 2, 3], [1, 2, 2, 0, 3]])
    want = [[0, 1, 2, 3, 3], [2, 3, 0, 1, 3]]
    assert to_undirected(ei, 4).tolist() == want == R.to_undirected(ei.numpy(), 4).tolist()
    assert to_undirected(ei).tolist() == want and to_undirected(ei).dtype == torch.int64
    rng = np.random.default_rng(3)
    for n, m, vr, tr in ((30, 60, 0.05, 0.1), (12, 60, 0.2, 0.3), (6, 15, 0.4, 0.4), (40, 0, 0.05, 0.1)):
        pairs = {(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (m, 2)) if a != b}
        if n == 6:
            pairs = {(i, j) for i in range(6) for j in range(6) if i < j}        # complete: no negatives at all
        pr = torch.tensor(sorted(pairs), dtype=torch.int64).reshape(-1, 2)
        und = torch.cat([pr.t(), pr.t().flip(0)], dim=1)
        data = Data(x=torch.zeros(n, 2), edge_index=und)
        torch.manual_seed(n)
        out = train_test_split_edges(data, vr, tr)
        assert out is data
        n_v, n_t = R.check_split(und.numpy(), n, data, vr, tr)
        assert data.val_pos_edge_index.shape == (2, n_v) and data.test_pos_edge_index.shape == (2, n_t)


def test_auc_and_ap_with_ties_by_hand():
    from torch_geometric.nn.models.autoencoder import average_precision_score, roc_auc_score
    y = [1, 0, 1, 1, 0, 0, 1, 0]
    s = [0.9, 0.9, 0.5, 0.4, 0.4, 0.1, 0.4, 0.9]
    # positives 0.9 0.5 0.4 0.4 against negatives 0.9 0.4 0.1 0.9: wins 2 + 2 + 1 + 1 = 6, ties 2 + 0 + 1 + 1 = 4 -> 8 / 16
    assert roc_auc_score(y, s) == pytest.approx(8 / 16, abs=1e-15) == pytest.approx(R.roc_auc(y, s), abs=1e-15)
    # thresholds 0.9 (tp 1 of 3), 0.5 (2 of 4), 0.4 (4 of 7), 0.1 (4 of 8): recall 1/4, 2/4, 1, 1
    ap = 0.25 * (1 / 3) + 0.25 * (2 / 4) + 0.5 * (4 / 7)
    assert average_precision_score(y, s) == pytest.approx(ap, abs=1e-15) == pytest.approx(R.average_precision(y, s),
                                                                                        abs=1e-15)
    assert roc_auc_score([1, 1, 0], [3.0, 2.0, 1.0]) == 1.0 and roc_auc_score([0, 0, 1], [3.0, 2.0, 1.0]) == 0.0
    assert roc_auc_score([1, 0], [0.5, 0.5]) == 0.5 and average_precision_score([1, 0], [0.5, 0.5]) == 0.5
    with pytest.raises(ValueError):
        roc_auc_score([1, 1], [0.1, 0.2])
    rng = np.random.default_rng(2)
    for _ in range(5):
        yy = rng.integers(0, 2, 60)
        yy[:2] = (0, 1)
        ss = rng.integers(0, 12, 60) / 12.0
        assert roc_auc_score(yy, ss) == pytest.approx(R.roc_auc(yy, ss), abs=1e-13)
        assert average_precision_score(yy, ss) == pytest.approx(R.average_precision(yy, ss), abs=1e-13)


def test_auc_and_ap_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    from torch_geometric.nn.models.autoencoder import average_precision_score, roc_auc_score
    rng = np.random.default_rng(4)
    for n in (2, 17, 300):
        y = rng.integers(0, 2, n)
        y[:2] = (0, 1)
        s = np.round(rng.random(n), 1 if n > 17 else 3)
        assert roc_auc_score(y, s) == pytest.approx(metrics.roc_auc_score(y, s), abs=1e-12)
        assert average_precision_score(y, s) == pytest.approx(metrics.average_precision_score(y, s), abs=1e-12)


def test_loss_terms_by_hand():
    t, c = R.loss_terms([0.0, 0.0], True)
    assert t == pytest.approx([math.log(2)] * 2, abs=1e-14) and c == pytest.approx([-0.25, -0.25], abs=1e-14)
    t, c = R.loss_terms([0.0], False)
    assert t == pytest.approx([math.log(2)], abs=1e-14) and c == pytest.approx([0.5], abs=1e-14)
    t, c = R.loss_terms([-100.0], True)
    assert t == pytest.approx([-math.log(1e-15)], rel=1e-12) and abs(c[0]) < 1e-25
    z = np.asarray([[1.0, 2.0], [0.5, -1.0], [3.0, 0.0]])
    assert R.score(z, [0, 1, 2], [1, 1, 0]).tolist() == [-1.5, 1.25, 3.0]
    dz = R.grad_z(z, np.asarray([0, 1]), np.asarray([1, 1]), [2.0, 10.0])
    assert dz.tolist() == [[1.0, -2.0], [2.0 + 10.0, 4.0 - 20.0], [0.0, 0.0]]      # the loop counts twice
    assert math.isnan(R.side_loss(z, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), True)[0])


def test_restatement_matches_the_committed_known_answers():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "link", "link_kat.npz"))
    ins = G.inputs()
    for name, v in zip(G.NAMES, ins):
        assert kat[name].dtype == v.dtype and kat[name].tobytes() == v.tobytes(), name
    want = G.answers(*ins)
    assert sorted(want) == sorted(k for k in kat.files if k not in G.NAMES)
    for k, v in want.items():
        assert kat[k].dtype == v.dtype and kat[k].shape == v.shape and kat[k].tobytes() == v.tobytes(), k
    # what the file is for
    assert kat["almost_full_s0"].T.tolist() == [[4, 2]] == kat["almost_full_s1"].T.tolist()
    assert kat["almost_upper_s0"].shape == (2, 0) and kat["edges_full_17"].shape == (2, 17)
    assert len(kat["edges_full_keys"]) < 40 and kat["edges_full_s0"].shape == (2, 40)
    assert not np.array_equal(kat["edges_full_s0"], kat["edges_full_s1"])
    edges = set(_pairs(kat["edges"]))
    for tag in ("edges_full_s0", "edges_full_s1", "edges_upper_s0", "edges_loops_s0"):
        assert not (set(_pairs(kat[tag])) & edges), tag
    assert all(i != j for i, j in _pairs(kat["edges_loops_s0"]))
    half = kat["edges_upper_s0"].shape[1] // 2
    assert half == 20 and (kat["edges_upper_s0"][0, :half] < kat["edges_upper_s0"][1, :half]).all()
    assert sorted(_pairs(kat["path_undirected"])) == sorted([(i, i + 1) for i in range(4)] + [(i + 1, i) for i in range(4)])
    rows = kat["edges_rows_s0"]
    assert all((int(i), int(k)) not in edges for i, k in zip(kat["edges"][0], rows))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "link", "link_kat.npz")) < 64 * 1024


def test_vgae_formulas_and_gae_plumbing():
    from torch_geometric.nn import GAE, VGAE, InnerProductDecoder
    from torch_geometric.nn.models import autoencoder as A
    assert A.MAX_LOGVAR == 10 and A.EPS == 1e-15

    class Enc(torch.nn.Module):
        def __init__(self):
            super(Enc, self).__init__()
            self.lin = torch.nn.Linear(3, 4)

        def forward(self, x):
            h = self.lin(x)
            return h, 6 * h

    torch.manual_seed(0)
    m = VGAE(Enc())
    x = torch.randn(5, 3) * 3
    m.eval()
    z = m.encode(x)
    mu, raw = m.encoder(x)
    assert torch.equal(z, mu) and raw.max() > 10                   # eval: the mean; and the clamp is exercised
    logvar = raw.clamp(max=10)
    assert torch.equal(m.__logvar__, logvar) and torch.equal(m.__mu__, mu)
    want = -0.5 * torch.mean(torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1))
    assert torch.equal(m.kl_loss(), want) and torch.equal(m.kl_loss(mu, raw), want)
    m.train()
    torch.manual_seed(5)
    z = m.encode(x)
    torch.manual_seed(5)
    mu, raw = m.encoder(x)
    logvar = raw.clamp(max=10)
    assert torch.equal(z, mu + torch.randn_like(logvar) * torch.exp(logvar))
    dec = InnerProductDecoder()
    zz = torch.randn(4, 3)
    assert torch.equal(dec.forward_all(zz), torch.sigmoid(zz @ zz.t()))
    assert torch.equal(dec.forward_all(zz, sigmoid=False), zz @ zz.t())
    g = GAE(Enc())
    assert isinstance(g.decoder, InnerProductDecoder) and g.encode(x)[0].shape == (5, 4)
    before = g.encoder.lin.weight.detach().clone()
    g.reset_parameters()
    assert not torch.equal(before, g.encoder.lin.weight)
    own = torch.nn.Bilinear(2, 2, 1)
    assert GAE(Enc(), own).decoder is own


def test_exports_signatures_and_reprs():
    import torch_geometric.nn as nn
    import torch_geometric.nn.models as models
    import torch_geometric.utils as utils
    for name in ("InnerProductDecoder", "GAE", "VGAE"):
        assert getattr(nn, name) is getattr(models, name) and name in nn.__all__ and name in models.__all__
    for name in ("negative_sampling", "structured_negative_sampling", "to_undirected", "train_test_split_edges"):
        assert callable(getattr(utils, name)) and name in utils.__all__

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(utils.negative_sampling) == [("edge_index", E), ("num_nodes", None), ("num_neg_samples", None),
                                               ("force_undirected", False)]
    assert params(utils.structured_negative_sampling) == [("edge_index", E), ("num_nodes", None)]
    assert params(utils.to_undirected) == [("edge_index", E), ("num_nodes", None)]
    assert params(utils.train_test_split_edges) == [("data", E), ("val_ratio", 0.05), ("test_ratio", 0.1)]
    assert params(nn.InnerProductDecoder.forward)[1:] == [("z", E), ("edge_index", E), ("sigmoid", True)]
    assert params(nn.InnerProductDecoder.forward_all)[1:] == [("z", E), ("sigmoid", True)]
    assert params(nn.GAE.__init__)[1:] == [("encoder", E), ("decoder", None)] == params(nn.VGAE.__init__)[1:]
    assert params(nn.GAE.split_edges)[1:] == [("data", E), ("val_ratio", 0.05), ("test_ratio", 0.1)]
    assert params(nn.GAE.recon_loss)[1:] == [("z", E), ("pos_edge_index", E)]
    assert params(nn.GAE.test)[1:] == [("z", E), ("pos_edge_index", E), ("neg_edge_index", E)]
    assert params(nn.VGAE.kl_loss)[1:] == [("mu", None), ("logvar", None)]
    assert params(nn.VGAE.reparametrize)[1:] == [("mu", E), ("logvar", E)]
    assert issubclass(nn.VGAE, nn.GAE)
    for name in ("reset_parameters", "encode", "decode"):
        assert callable(getattr(nn.GAE, name))
    lin = torch.nn.Linear(3, 2)
    assert repr(nn.InnerProductDecoder()) == "InnerProductDecoder()"
    assert repr(nn.GAE(lin)) == "GAE(\n  (encoder): %r\n  (decoder): InnerProductDecoder()\n)" % lin
    assert repr(nn.VGAE(lin)).startswith("VGAE(\n  (encoder): Linear")


def test_no_cpu_fallback(lib):
    from mi355_mp import ops
    from torch_geometric.nn import GAE, InnerProductDecoder
    from torch_geometric.utils import negative_sampling, structured_negative_sampling
    z = torch.randn(6, 4)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    gae = GAE(torch.nn.Identity())
    for call in (lambda: InnerProductDecoder()(z, ei), lambda: ops.edge_score(z, ei), lambda: ops.link_loss(z, ei, ei),
                 lambda: negative_sampling(ei, 6), lambda: negative_sampling(ei, 6, force_undirected=True),
                 lambda: structured_negative_sampling(ei, 6), lambda: ops.negative_sample(ei, 6, loops=True),
                 lambda: gae.recon_loss(z, ei), lambda: gae.test(z, ei, ei)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bindings(lib):
    from mi355_mp import _lib, ops
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("mp_link_", "mp_edge_score", "mp_neg_sample")))
    assert names == ["mp_edge_score_f32", "mp_link_grad_rows_f32", "mp_link_lanes", "mp_link_loss_f32",
                     "mp_link_loss_workspace", "mp_neg_sample", "mp_neg_sample_rows"]
    header = open(os.path.join(ROOT, "include", "mi355_mp.h")).read()
    nat = _lib.native()
    for name in names:
        assert re.search(r"^(int64_t|size_t) %s\(" % name, header, flags=re.M), name
        decl = re.search(r"^(?:int64_t|size_t) %s\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        decl = " ".join(decl.split())
        assert len(_lib.SIGNATURES[name][1]) == len(decl.split(",")), name      # one ctypes type per parameter
        # every caller-allocated array travels with its extent: a *_bytes follows it
        for arr in re.findall(r"\b(v|coef|loss|ws|keys|out)\b(?=,)", decl):
            assert re.search(r"\b%s, size_t \w*bytes" % arr, decl) or arr == "coef" and "n_coef" in decl, (name, arr)
        if name == "mp_link_loss_workspace":
            assert _lib.SIGNATURES[name][0] is ctypes.c_size_t
            continue
        assert _lib.SIGNATURES[name][0] is ctypes.c_int64 and name not in _lib.STATUS_RETURNING
        assert getattr(nat, name) is getattr(lib, name) and getattr(lib, name).errcheck is None
    assert lib.mp_abi_version() == 7 == _lib.ABI_VERSION
    assert [ops.link_lanes(C) for C in (1, 3, 4, 16, 17, 64, 65, 128, 256, 260)] == [1, 4, 1, 4, 32, 16, 64, 16, 16, 16]
    assert [ops.link_lanes(C, vec4=False) for C in (4, 16, 64, 65)] == [4, 16, 64, 64]
    D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first
    with pytest.raises(RuntimeError, match=r"mp_edge_score_f32 failed \(code 1\): mp_edge_score_f32: ldz = 3 < C = 4"):
        ops._count_call(nat, "mp_edge_score_f32", D, D, 10, D, 3, 5, 4, 0, 0, D, 40, None)
    with pytest.raises(RuntimeError, match="v holds 39 bytes, the call needs 40"):
        ops._count_call(nat, "mp_edge_score_f32", D, D, 10, D, 4, 5, 4, 0, 0, D, 39, None)
    ws = lib.mp_link_loss_workspace(10)
    with pytest.raises(RuntimeError, match="ws holds %d bytes" % (ws - 1)):
        ops._count_call(nat, "mp_link_loss_f32", D, D, 10, D, 4, 5, 4, 1, 0, D, 40, D, 4, D, ws - 1, None)
    assert lib.mp_link_grad_rows_f32(D, D, D, 5, 20, D, 9, D, 4, 5, 4, 0, D, 4, 80, None) == -1
    assert "n_coef = 9" in lib.mp_last_error().decode()
    assert lib.mp_neg_sample(D, 80, D, 5, 3, 1, 4, D, D, 32, None) == -1
    assert "mode = 3" in lib.mp_last_error().decode()
    assert lib.mp_neg_sample_rows(D, 80, D, 5, 1, D, 4, D, 31, None) == -1
    assert "out holds 31 bytes" in lib.mp_last_error().decode()
    assert lib.mp_link_lanes(0, 1) == -1


def test_link_abi_rejections_under_asan():
    """tests/abi/abi_reject_link.c against the host-AddressSanitizer build of the
    library (make asan_link), run as a plain program with nothing preloaded: every
    NULL pointer, every extent and workspace one byte short, sizes that are negative
    or beyond the int32 CSR limits, a lane count that is no power of two, a
    misaligned z or workspace, a mode or side flag outside its values and N beyond
    the 64-bit key space, each answered with -(MP_ERR_ARG) and its text."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC, "asan_link"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "abi_reject_link")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.match(r"abi_reject_link: (\d+) cases, 0 failures", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) >= 100, r.stdout[-2000:]


def test_makefile_lists_the_link_unit_and_build_makes_the_harness():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "mp_link.hip" in units
    assert "-ffp-contract=off" in mk                     # the score's bitwise position independence depends on it
    assert re.search(r"^asan_link:", mk, flags=re.M)
    assert '"asan_link"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
