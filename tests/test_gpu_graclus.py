"""GPU tests of graclus and normalized_cut (csrc/mp_graclus.hip) against the CPU
restatement tests/_graclus_ref.py.

Clusters are integers and must equal the restatement exactly, everywhere; the
rounds the kernels took must equal the handshake's.  normalized_cut is compared
with its float64 form under |err| <= 4 * 2^-24 * |ref|: three fp32 roundings (the
reciprocal, the sum, the product) and the rounding of the reference to fp32 scale.

No kernel of the unit caps its grid and strides: every launch has one thread per
node or per incidence entry, so there is no size past a cap to test.  The two
paths of the round kernel are a row of at most 64 entries (one lane) and a longer
one (the wave): the star and the hub below cover a row longer than a wave (200)
and one longer than a workgroup's 256 threads (5000), the batches the short rows.
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import _cluster_ref as C
from tests import _graclus_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = [1, 64, 75, 130]


def _match(ei, w, n, seed=0, **kw):
    from mi355_mp import ops
    ei = torch.as_tensor(np.asarray(ei, dtype=np.int64).reshape(2, -1)).to(DEV)
    w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.float32)).to(DEV)
    m = ops.graclus_match(ei, w, n, seed=seed, **kw)
    torch.cuda.synchronize()
    return m


def _assert_is_the_restatement(ei, w, n, seed=0):
    m = _match(ei, w, n, seed)
    want, rounds = R.handshake(ei, w, n, seed)
    got = m.cluster.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (n,)
    assert np.array_equal(got, want), "seed %d: %d of %d nodes differ" % (seed, int((got != want).sum()), n)
    assert m.rounds == rounds
    return m, want


def _knn_batch(seed, k=8):
    """Graphs of 1, 64, 75 and 130 random points on [0, 28)^2, every node linked from
    its k nearest neighbours (one direction, as the superpixel graphs are stored)."""
    g = torch.Generator().manual_seed(seed)
    rows, cols, poss, off = [], [], [], 0
    for s in SIZES:
        pos = torch.rand(s, 2, generator=g) * 28
        if s > 1:
            d = torch.cdist(pos, pos)
            d.fill_diagonal_(float("inf"))
            nbr = d.topk(min(k, s - 1), largest=False).indices
            rows.append(nbr.reshape(-1) + off)
            cols.append(torch.arange(s).view(-1, 1).expand_as(nbr).reshape(-1) + off)
        poss.append(pos)
        off += s
    return torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(poss), off


@pytest.fixture(scope="module")
def batch():
    from torch_geometric.utils import normalized_cut
    ei, pos, n = _knn_batch(3)
    length = (pos[ei[0]] - pos[ei[1]]).norm(dim=1)
    cut = normalized_cut(ei.to(DEV), length.to(DEV), n).cpu()
    quant = (length / length.max() * 4.999).floor() / 4                     # five values: the hash decides within each
    assert quant.unique().numel() == 5
    return {"ei": ei.numpy(), "pos": pos, "n": n, "length": length,
            "weights": {"unweighted": None, "normalized_cut": cut.numpy(), "five_values": quant.numpy()}}


@pytest.mark.parametrize("name,ei,w,n,want", R.HAND, ids=[h[0] for h in R.HAND])
def test_hand_graphs(name, ei, w, n, want):
    for seed in (0, 1):
        m = _match(ei, w, n, seed)
        assert m.cluster.dtype == torch.int64 and m.cluster.cpu().tolist() == want
        assert m.rounds == R.handshake(ei, w, n, seed)[1]


@pytest.mark.parametrize("weights", ["unweighted", "normalized_cut", "five_values"])
def test_superpixel_batch_is_the_restatement(batch, weights):
    w = batch["weights"][weights]
    out = []
    for seed in (0, 1):
        m, want = _assert_is_the_restatement(batch["ei"], w, batch["n"], seed)
        R.check_matching(m.cluster.cpu().numpy(), batch["ei"])
        assert int((want != np.arange(batch["n"])).sum()) > batch["n"] // 4 and want[0] == 0        # graph 0: one node
        print("%s seed %d: %d rounds, %d host reads" % (weights, seed, m.rounds, m.host_reads))
        out.append(want)
    if weights == "unweighted":
        assert not np.array_equal(out[0], out[1])                          # another seed, another valid matching


def test_public_graclus_and_num_nodes(batch):
    from torch_geometric.nn import graclus
    ei = torch.from_numpy(batch["ei"]).to(DEV)
    w = torch.from_numpy(batch["weights"]["normalized_cut"]).to(DEV)
    n = batch["n"]
    w_np = batch["weights"]["normalized_cut"]
    for seed in (0, 1):
        assert np.array_equal(graclus(ei, w, n, seed=seed).cpu().numpy(), R.greedy(batch["ei"], w_np, n, seed))
    assert np.array_equal(graclus(ei).cpu().numpy(), R.greedy(batch["ei"], None, n, 0))       # num_nodes: max + 1
    assert np.array_equal(graclus(ei, None, n + 3).cpu().numpy()[n:], np.arange(n, n + 3))    # trailing isolated nodes
    assert np.array_equal(graclus(ei, w.requires_grad_(True), n).cpu().numpy(), R.greedy(batch["ei"], w_np, n, 0))


def test_result_does_not_depend_on_edge_order_or_direction(batch):
    g = torch.Generator().manual_seed(9)
    ei = torch.from_numpy(batch["ei"])
    E = ei.size(1)
    for name in ("unweighted", "five_values"):
        w = batch["weights"][name]
        first = _match(ei, w, batch["n"], 1).cluster
        again = _match(ei, w, batch["n"], 1).cluster
        assert torch.equal(first, again)                                    # two runs: bitwise equal
        perm = torch.randperm(E, generator=g)
        flip = torch.rand(E, generator=g) < 0.5
        ei2 = ei[:, perm]
        ei2 = torch.where(flip[perm], ei2.flip(0), ei2)
        assert not torch.equal(ei2, ei)
        w2 = None if w is None else w[perm.numpy()]
        assert torch.equal(_match(ei2, w2, batch["n"], 1).cluster, first)


def test_long_rows():
    # a star: the hub's row of 200 is scanned by the wave, the leaves' by one lane each
    star = [[0] * 200, list(range(1, 201))]
    m, want = _assert_is_the_restatement(star, None, 201)
    assert int((want != np.arange(201)).sum()) == 1 and m.rounds == 2
    # a hub of 5000 leaves in the middle of a few ordinary nodes, weights with ties; the leaves'
    # edges point at the hub, so its row is long only through the reversed entries
    rng = np.random.default_rng(4)
    hub, n = 7, 5020
    row = list(range(20, n)) + rng.integers(0, 20, 60).tolist()
    col = [hub] * 5000 + rng.integers(0, 20, 60).tolist()
    w = rng.integers(0, 4, len(row)).astype(np.float32)
    for seed in (0, 1):
        _assert_is_the_restatement([row, col], w, n, seed)
    _assert_is_the_restatement([row, col], None, n, 2)
    # two hubs in one wave (nodes 0 and 1), each with a row past the threshold, sharing their leaves
    leaves = list(range(2, 102))
    two = [[0] * 100 + [1] * 100, leaves + leaves]
    _assert_is_the_restatement(two, rng.random(200).astype(np.float32), 102)


def test_many_rounds_and_batched_host_reads():
    from mi355_mp import ops
    n = 300
    path = [list(range(n - 1)), list(range(1, n))]
    w = np.arange(n - 1, dtype=np.float32)
    m, want = _assert_is_the_restatement(path, w, n)
    R_ = ops.GRACLUS_ROUNDS_PER_READ
    assert m.rounds == 150 > R_ and want.tolist() == [i - i % 2 for i in range(n)]
    assert m.host_reads == math.ceil(m.rounds / R_)
    for r in (1, 7, 150, 151):
        m2 = _match(path, w, n, rounds_per_read=r)
        assert torch.equal(m2.cluster, m.cluster) and m2.rounds == 150 and m2.host_reads == math.ceil(150 / r)


def test_errors(batch):
    import torch_geometric
    from torch_geometric.nn import graclus
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    w = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    for bad in (torch.tensor([[0, 1, 2], [1, 2, 4]]), torch.tensor([[0, -1, 2], [1, 2, 3]])):
        with pytest.raises(IndexError):
            graclus(bad.to(DEV), w, 4)
    with pytest.raises(TypeError, match="float32"):
        graclus(ei, w.double(), 4)
    with pytest.raises(ValueError):
        graclus(ei, w[:2], 4)
    nan = torch.tensor([1.0, float("nan"), 3.0], device=DEV)
    with torch_geometric.debug():
        with pytest.raises(ValueError, match="NaN"):
            graclus(ei, nan, 4)
        assert graclus(ei, w, 4).cpu().tolist() == [0, 0, 2, 2]
    assert graclus(ei, w, 4).cpu().tolist() == [0, 0, 2, 2]                 # and the layer still works afterwards


def test_normalized_cut_against_float64(batch):
    from torch_geometric.utils import normalized_cut
    ei, n = batch["ei"], batch["n"]
    g = torch.Generator().manual_seed(2)
    for attr in (batch["length"], torch.randn(ei.shape[1], generator=g) * 100):
        ref = R.normalized_cut(ei, attr.numpy(), n)
        got = normalized_cut(torch.from_numpy(ei).to(DEV), attr.to(DEV), n)
        assert got.dtype == torch.float32 and tuple(got.shape) == (ei.shape[1],)
        fin = np.isfinite(ref)                                               # a node that starts no edge: 1 / 0 = inf
        got64 = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(got64[~fin], ref[~fin])
        err = np.abs(got64[fin] - ref[fin])
        ratio = float((err / np.abs(ref[fin])).max())
        print("normalized_cut: max |err| / |ref| = %.3g (bound %.3g), %d infinite"
              % (ratio, 4 * 2.0 ** -24, int((~fin).sum())))
        assert bool((err <= 4 * 2.0 ** -24 * np.abs(ref[fin])).all()), ratio
    # num_nodes from the row index; an end outside it raises
    sub = torch.tensor([[0, 1, 1], [1, 0, 0]], device=DEV)
    assert normalized_cut(sub, torch.ones(3, device=DEV)).cpu().tolist() == [1.5, 1.5, 1.5]
    with pytest.raises(IndexError):
        normalized_cut(torch.tensor([[0, 1], [1, 2]], device=DEV), torch.ones(2, device=DEV))


def test_graclus_then_max_pool_end_to_end(batch):
    from torch_geometric.data import Batch
    from torch_geometric.nn import graclus, max_pool
    ei, n, pos = torch.from_numpy(batch["ei"]), batch["n"], batch["pos"]
    w = torch.from_numpy(batch["weights"]["normalized_cut"])
    g = torch.Generator().manual_seed(6)
    x = torch.randint(-2, 3, (n, 5), generator=g).float() * 0.5
    attr = torch.rand(ei.size(1), 2, generator=g)
    b = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(SIZES)])
    cluster = graclus(ei.to(DEV), w.to(DEV), n)
    out = max_pool(cluster, Batch(batch=b.to(DEV), x=x.to(DEV), pos=pos.to(DEV), edge_index=ei.to(DEV),
                                  edge_attr=attr.to(DEV)))
    ref = C.pool(torch.from_numpy(R.greedy(batch["ei"], w.numpy(), n)), x, pos, b, ei, attr)
    M = ref["perm"].numel()
    assert n // 2 <= M < n and tuple(out.x.shape) == (M, 5)
    assert torch.equal(out.x.cpu(), ref["x"]) and torch.equal(out.batch.cpu(), ref["batch"])
    assert torch.equal(out.edge_index.cpu(), ref["edge_index"]) and torch.equal(out.edge_attr.cpu(), ref["edge_attr"])
    # a cluster has one or two members: the mean of two fp32 numbers is one rounding of the exact value
    p64 = C.pool_f64(None, pos.double(), None, ref["inv"], None, None, M, 0, "mean")[1]
    assert bool(((out.pos.cpu().double() - p64).abs() <= 2.0 ** -24 * p64.abs()).all())


def _example():
    spec = importlib.util.spec_from_file_location("mnist_graclus", os.path.join(ROOT, "examples", "mnist_graclus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_trains():
    torch.manual_seed(0)   # weights and dropout masks (the example itself is unseeded, as the reference's)
    losses = _example().main(["--epochs", "2", "--graphs", "256"])
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
