"""GPU tests of the link-prediction kernels (csrc/mp_link.hip) and the layers on top
(mi355_mp.ops edge_score / link_loss / negative_sample, torch_geometric.nn GAE, VGAE,
InnerProductDecoder, torch_geometric.utils negative_sampling,
structured_negative_sampling) against the float64 / integer restatement
tests/_link_ref.py.  u = 2^-24 throughout.

Bounds (each from the arithmetic, none from what the kernels give):

  score     |v - v64| <= dv = 2 C u sum_c |z_ic z_jc|: an fp32 dot product of C rounded
            products added in any order is within gamma_C of the exact one; doubled,
            as elsewhere in the suite.  With the sigmoid: its slope is at most 1/4,
            and expf, the add and the divide cost under 4 u on a value below 1:
            0.25 dv + 4 u.
  loss      |L - L64| <= mean_e dv_e + 8 u (1 + mean_e |t_e|): |dt/dv| <= 1, the
            sigmoid's and logf's roundings are a few u absolute and 2 u relative on
            t, and the sum is carried in fp64, so it adds only the last rounding.
            Inputs are scaled to |v| <= 12 so that nothing saturates.
  gradient  dz_ic = sum over the d_i edge ends e at node i of coef_e z_oc (o the
            other end).  Each product is rounded once and the d_i terms are added
            in fp32 in some fixed order: |coef_e z_oc| (d_i + 8) u per term covers
            the products, the d_i - 1 additions, the scaling of coef by the incoming
            gradient and the second pass adding into the first.  coef_e itself is
            off by dcoef_e: 0 for a raw score (it is the incoming gradient), |g_e|
            (0.25 dv_e + 8 u) for a sigmoid score (the slope of p (1 - p) is below
            1/4) and (0.25 dv_e + 8 u) / E_side for the loss (|d coef / dv| <= 1/4 /
            E_side, its own arithmetic a few u of a value below 1 / E_side).  Per
            element: sum_{e at i} |z_oc| (|coef_e| (d_i + 8) u + dcoef_e).
  sampler   integers: equal to the restatement exactly.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import _link_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SCORE_C = (1, 3, 4, 16, 17, 64, 65, 256, 260)
SCORE_E = (0, 1, 15, 16, 17, 63, 64, 65, 1025)


@pytest.fixture(scope="module")
def dev():
    import mi355_mp
    mi355_mp.load_native()
    return torch.device("cuda:0")


def _edges(rng, n, e, loops=2, repeats=2):
    ei = rng.integers(0, n, (2, e)).astype(np.int64)
    for k in range(min(loops, e)):
        ei[1, k] = ei[0, k]                                   # row == col
    for k in range(min(repeats, max(e - 3, 0))):
        ei[:, e - 1 - k] = ei[:, 2]                           # a repeated edge
    return ei


def _z(rng, n, c):
    return rng.standard_normal((n, c)).astype(np.float32)


def _scaled_z(rng, n, c, ei, vmax=12.0):
    """z with max |v| just below vmax over the edges of ei."""
    z = _z(rng, n, c)
    top = np.abs(R.score(z, ei[0], ei[1])).max() if ei.shape[1] else 1.0
    return (z * np.float32(math.sqrt(vmax / max(top, 1e-6)) * 0.99)).astype(np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("C", SCORE_C)
def test_score_against_float64(dev, C):
    from mi355_mp import ops
    rng = np.random.default_rng(100 + C)
    n = 37
    z = _z(rng, n, C)
    zd = _t(z, dev)
    worst = 0.0
    for E in SCORE_E:
        ei = _edges(rng, n, E)
        eid = _t(ei, dev)
        v64, dv = R.score(z, ei[0], ei[1]), R.score_bound(z, ei[0], ei[1])
        v = ops.edge_score(zd, eid).cpu().numpy().astype(np.float64)
        p = ops.edge_score(zd, eid, sigmoid=True).cpu().numpy().astype(np.float64)
        assert v.shape == (E,) and p.shape == (E,)
        if E:
            worst = max(worst, float((np.abs(v - v64) / np.maximum(dv, 1e-300)).max()))
        assert (np.abs(v - v64) <= dv).all(), (C, E)
        assert (np.abs(p - R.sigmoid(v64)) <= 0.25 * dv + 4 * U).all(), (C, E)
    print("score C=%d: worst |v - v64| / bound = %.3f over E in %s" % (C, worst, SCORE_E))


def test_score_one_node_and_lane_override(dev):
    from mi355_mp import ops
    rng = np.random.default_rng(7)
    for C in (1, 4, 17):
        z = _z(rng, 1, C)
        ei = np.zeros((2, 5), dtype=np.int64)
        v = ops.edge_score(_t(z, dev), _t(ei, dev)).cpu().numpy().astype(np.float64)
        assert (np.abs(v - R.score(z, ei[0], ei[1])) <= R.score_bound(z, ei[0], ei[1])).all()
        assert len(set(v.tolist())) == 1
    # every forced lane mapping computes the same score to the bound (tools/bench_link.py sweeps them)
    z = _z(rng, 50, 64)
    ei = _edges(rng, 50, 130)
    zd, row, col = _t(z, dev), _t(ei[0], dev), _t(ei[1], dev)
    v64, dv = R.score(z, ei[0], ei[1]), R.score_bound(z, ei[0], ei[1])
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        v = ops.edge_score_forward(zd, row, col, lanes=lanes).cpu().numpy().astype(np.float64)
        assert (np.abs(v - v64) <= dv).all(), lanes


def test_score_strided_and_misaligned_z(dev):
    from mi355_mp import ops
    rng = np.random.default_rng(8)
    n, E = 29, 70
    ei = _edges(rng, n, E)
    eid = _t(ei, dev)
    for C, ld in ((16, 20), (16, 19), (64, 64), (260, 264), (5, 9)):
        z = _z(rng, n, C)
        v64, dv = R.score(z, ei[0], ei[1]), R.score_bound(z, ei[0], ei[1])
        wide = torch.zeros((n, ld), dtype=torch.float32, device=dev)
        wide[:, :C] = _t(z, dev)
        view = wide[:, :C]                                     # ldz > C; 16-byte rows when ld % 4 == 0
        assert view.stride(0) == ld and view.data_ptr() % 16 == 0
        # a base one float past a 16-byte boundary: the scalar form whatever C
        buf = torch.zeros(n * ld + 1, dtype=torch.float32, device=dev)
        off = buf[1:].view(n, ld)[:, :C]
        off.copy_(_t(z, dev))
        assert off.data_ptr() % 16 == 4
        for zz in (view, off):
            v = ops.edge_score(zz, eid).cpu().numpy().astype(np.float64)
            assert (np.abs(v - v64) <= dv).all(), (C, ld)
        if C % 4 == 0 and ld % 4 == 0:
            # the two load forms add the products in different orders: both are inside the bound, and the
            # aligned view is the contiguous tensor's bits (same form, same mapping)
            assert torch.equal(ops.edge_score(view, eid), ops.edge_score(_t(z, dev), eid))


@pytest.mark.parametrize("C", (16, 17, 260))
def test_score_does_not_depend_on_position(dev, C):
    from mi355_mp import ops
    rng = np.random.default_rng(9)
    n = 41
    zd = _t(_z(rng, n, C), dev)
    short = _edges(rng, n, 65)
    long_ = _edges(rng, n, 1025)
    where = rng.permutation(1025)[:65]
    long_[:, where] = short
    a = ops.edge_score(zd, _t(short, dev))
    b = ops.edge_score(zd, _t(long_, dev))
    assert torch.equal(a, b[_t(where, dev)])                    # bitwise: another position, another length
    assert torch.equal(ops.edge_score(zd, _t(short[:, :1], dev)), a[:1])


@pytest.mark.parametrize("C", (16, 17))
def test_loss_against_float64(dev, C):
    from mi355_mp import ops
    rng = np.random.default_rng(200 + C)
    n = 33
    for E in (1, 2, 65, 1025):
        ei = _edges(rng, n, E, loops=1, repeats=1)
        z = _scaled_z(rng, n, C, ei)
        v64, dv = R.score(z, ei[0], ei[1]), R.score_bound(z, ei[0], ei[1])
        assert np.abs(v64).max() <= 12.0
        zd, row, col = _t(z, dev), _t(ei[0], dev), _t(ei[1], dev)
        for positive in (True, False):
            L64, c64, t64 = R.side_loss(z, ei[0], ei[1], positive)
            loss, coef = ops.link_loss_side(zd, row, col, positive)
            loss2, coef2 = ops.link_loss_side(zd, row, col, positive)
            assert torch.equal(loss, loss2) and torch.equal(coef, coef2)      # run to run: the same bits
            L = float(loss)
            bound = dv.mean() + 8 * U * (1 + np.abs(t64).mean())
            print("loss C=%d E=%d %s: |L - L64| = %.3g, bound %.3g" % (C, E, "pos" if positive else "neg",
                                                                      abs(L - L64), bound))
            assert abs(L - L64) <= bound, (C, E, positive)
            dc = (0.25 * dv + 8 * U) / E
            assert (np.abs(coef.cpu().numpy().astype(np.float64) - c64) <= dc).all(), (C, E, positive)


def test_loss_saturated_and_empty(dev):
    from mi355_mp import ops
    z = _t(np.asarray([[10.0, 0.0], [10.0, 0.0], [-10.0, 0.0]], dtype=np.float32), dev)
    want = -np.log(np.float32(1e-15), dtype=np.float32)
    # positive side at v = -100, negative side at v = +100: p + EPS (1 - p + EPS) is EPS itself
    for positive, pair in ((True, (0, 2)), (False, (0, 1))):
        row, col = _t(np.asarray([pair[0]]), dev), _t(np.asarray([pair[1]]), dev)
        loss, coef = ops.link_loss_side(z, row, col, positive)
        assert abs(float(loss) - float(want)) <= 2 * float(np.spacing(want)), (float(loss), float(want))
        assert float(coef[0]) == 0.0
    # the other way round nothing is lost: t = -log(1 + EPS) = 0
    loss, coef = ops.link_loss_side(z, _t(np.asarray([0]), dev), _t(np.asarray([1]), dev), True)
    assert float(loss) == 0.0 and float(coef[0]) == 0.0
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    for positive in (True, False):
        loss, coef = ops.link_loss_side(z, empty, empty, positive)
        assert math.isnan(float(loss)) and coef.shape == (0,)
    ei0 = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    assert math.isnan(float(ops.link_loss(z, ei0, ei0)))


def _hub_graph(rng, n, e):
    """Random edges plus a hub (node 0: 160 edges as row, 160 as col), a loop, a
    repeated edge; node n - 1 is an end of nothing."""
    ei = rng.integers(0, n - 1, (2, e)).astype(np.int64)
    ei[0, :160] = 0
    ei[1, 160:320] = 0
    ei[:, 320] = (5, 5)
    ei[:, 321] = ei[:, 322]
    return ei


def _check_grad(got, z, rows, cols, coefs, dcoefs, what):
    row, col = np.concatenate(rows), np.concatenate(cols)
    coef, dcoef = np.concatenate(coefs), np.concatenate(dcoefs)
    want = R.grad_z(z, row, col, coef)
    bound = R.grad_bound(z, row, col, coef, dcoef)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst |dz - dz64| / bound = %.3f" % (what, ratio))
    assert (err <= bound).all(), what
    return want


@pytest.mark.parametrize("C", (16, 17, 5))
def test_score_gradients(dev, C):
    from mi355_mp import ops
    rng = np.random.default_rng(300 + C)
    n, E = 400, 1500
    ei = _hub_graph(rng, n, E)
    deg = np.bincount(ei.ravel(), minlength=n)
    assert deg[0] >= 300 and deg[n - 1] == 0
    z = _scaled_z(rng, n, C, ei)
    g = rng.standard_normal(E).astype(np.float32)
    v64, dv = R.score(z, ei[0], ei[1]), R.score_bound(z, ei[0], ei[1])
    eid, gd = _t(ei, dev), _t(g, dev)
    for sigmoid in (False, True):
        if sigmoid:
            p = R.sigmoid(v64)
            coef, dcoef = g * p * (1 - p), np.abs(g) * (0.25 * dv + 8 * U)
        else:
            coef, dcoef = g.astype(np.float64), np.zeros(E)
        grads = []
        for cached in (True, False):                            # the engine path, then mp_link_grad_rows_f32
            for _ in range(2):
                zd = _t(z, dev).requires_grad_(True)
                ops.edge_score(zd, eid, sigmoid=sigmoid, cached=cached).backward(gd)
                grads.append(zd.grad)
            assert torch.equal(grads[-1], grads[-2])            # run to run: the same bits
            got = grads[-1].cpu().numpy()
            _check_grad(got, z, [ei[0]], [ei[1]], [coef], [dcoef],
                        "edge_score C=%d sigmoid=%s cached=%s" % (C, sigmoid, cached))
            assert not got[n - 1].any()                           # the isolated node


@pytest.mark.parametrize("C", (16, 17))
def test_link_loss_gradient(dev, C):
    from mi355_mp import ops
    rng = np.random.default_rng(400 + C)
    n = 400
    pos, neg = _hub_graph(rng, n, 1500), _hub_graph(rng, n, 700)
    z = _scaled_z(rng, n, C, np.concatenate([pos, neg], axis=1))
    posd, negd = _t(pos, dev), _t(neg, dev)
    Lp, cp, tp = R.side_loss(z, pos[0], pos[1], True)
    Ln, cn, tn = R.side_loss(z, neg[0], neg[1], False)
    dvp, dvn = R.score_bound(z, pos[0], pos[1]), R.score_bound(z, neg[0], neg[1])
    outs = []
    for _ in range(2):
        zd = _t(z, dev).requires_grad_(True)
        loss = ops.link_loss(zd, posd, negd)
        (3.0 * loss).backward()                                  # an incoming gradient other than one
        outs.append((loss.detach(), zd.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    bound = dvp.mean() + dvn.mean() + 8 * U * (2 + np.abs(tp).mean() + np.abs(tn).mean())
    assert abs(float(outs[0][0]) - (Lp + Ln)) <= bound
    _check_grad(outs[0][1].cpu().numpy(), z, [pos[0], neg[0]], [pos[1], neg[1]], [3 * cp, 3 * cn],
                [3 * (0.25 * dvp + 8 * U) / pos.shape[1], 3 * (0.25 * dvn + 8 * U) / neg.shape[1]],
                "link_loss C=%d" % C)
    assert not outs[0][1][n - 1].any()


def test_recon_loss_gradient_with_sampled_negatives(dev):
    from mi355_mp import ops
    from torch_geometric.nn import GAE
    rng = np.random.default_rng(11)
    n, C = 300, 16
    pos = _hub_graph(rng, n, 900)
    posd = _t(pos, dev)
    model = GAE(torch.nn.Identity())
    torch.cuda.manual_seed(123)
    neg = ops.negative_sample(posd, n, loops=True).cpu().numpy()
    loops = int((pos[0] == pos[1]).sum())
    assert loops >= 1 and neg.shape == (2, 900 - loops + n)      # the loops out, one per node in
    z = _scaled_z(rng, n, C, np.concatenate([pos, neg], axis=1))
    torch.cuda.manual_seed(123)
    zd = _t(z, dev).requires_grad_(True)
    loss = model.recon_loss(zd, posd)
    loss.backward()
    Lp, cp, tp = R.side_loss(z, pos[0], pos[1], True)
    Ln, cn, tn = R.side_loss(z, neg[0], neg[1], False)
    dvp, dvn = R.score_bound(z, pos[0], pos[1]), R.score_bound(z, neg[0], neg[1])
    bound = dvp.mean() + dvn.mean() + 8 * U * (2 + np.abs(tp).mean() + np.abs(tn).mean())
    assert abs(float(loss.detach()) - (Lp + Ln)) <= bound
    _check_grad(zd.grad.cpu().numpy(), z, [pos[0], neg[0]], [pos[1], neg[1]], [cp, cn],
                [(0.25 * dvp + 8 * U) / pos.shape[1], (0.25 * dvn + 8 * U) / neg.shape[1]], "recon_loss")


def _graphs(n, rng):
    """name -> edge list [2, E] of the sampler's cases on n nodes."""
    out = {"empty": np.zeros((2, 0), dtype=np.int64)}
    if n >= 2:
        sparse = rng.integers(0, n, (2, max(3 * n if n > 100 else n, 2))).astype(np.int64)
        out["sparse"] = sparse
        dup = np.concatenate([sparse[:, : max(sparse.shape[1] // 2, 1)]] * 3, axis=1)
        dup[:, 0] = (n - 1, n - 1)
        out["duplicated"] = dup
    if n <= 65:
        full = np.asarray([(i, j) for i in range(n) for j in range(n)], dtype=np.int64).reshape(-1, 2).T
        out["complete"] = full
        if n >= 2:
            hole = (n - 1) * n + (n // 2)                        # the pair (n - 1, n // 2)
            out["complete_minus_one"] = np.delete(full, hole, axis=1)
    return out


@pytest.mark.parametrize("n", (1, 2, 5, 64, 65, 1000))
def test_sampler_equals_the_restatement(dev, n):
    from mi355_mp import ops
    rng = np.random.default_rng(500 + n)
    seeds = (0, 12345, (1 << 64) - 1)
    for name, ei in _graphs(n, rng).items():
        eid = _t(ei, dev)
        edges = {(int(a), int(b)) for a, b in ei.T}
        E = ei.shape[1]
        for seed in seeds[: (3 if n < 1000 else 1)]:
            for kw in (dict(), dict(num_neg_samples=7), dict(force_undirected=True), dict(loops=True),
                       dict(force_undirected=True, num_neg_samples=50)):
                got = ops.negative_sample(eid, n, seed=seed, **kw).cpu().numpy()
                rkw = dict(num_neg_samples=kw.get("num_neg_samples"), upper=kw.get("force_undirected", False),
                           loops=kw.get("loops", False))
                want = R.negative_sample(ei[0], ei[1], n, seed, **rkw)
                assert got.shape == want.shape and np.array_equal(got, want), (name, seed, kw)
                pairs = {(int(a), int(b)) for a, b in got.T}
                assert not (pairs & edges), (name, kw)
                if kw.get("force_undirected"):
                    h = got.shape[1] // 2
                    assert (got[0, :h] < got[1, :h]).all() and np.array_equal(got[:, :h], got[::-1, h:])
                    assert not ({(b, a) for a, b in pairs} & edges)
                    assert h == (0 if name.startswith("complete") else
                                 max(min(kw.get("num_neg_samples") or E, n * n - E), 0) // 2) or n < 3
                elif kw.get("loops"):
                    assert all(a != b for a, b in pairs)
                else:
                    cap = max(min(kw.get("num_neg_samples") or E, n * n - E), 0)
                    assert got.shape[1] == cap, (name, kw)
            k = ops.structured_negative_sample(eid, n, seed=seed).cpu().numpy()
            assert np.array_equal(k, R.structured_negative_sample(ei[0], ei[1], n, seed)), (name, seed)
            assert all((int(i), int(c)) not in edges for i, c in zip(ei[0], k) if c >= 0)
            if name == "complete":
                assert (k == -1).all()
        if name == "complete_minus_one":
            got = ops.negative_sample(eid, n, seed=5).cpu().numpy()
            assert got.T.tolist() == [[n - 1, n // 2]]
        if n >= 64 and name == "sparse":
            a = ops.negative_sample(eid, n, seed=1)
            assert not torch.equal(a, ops.negative_sample(eid, n, seed=2))       # two seeds differ
            assert torch.equal(a, ops.negative_sample(eid, n, seed=1))


def test_public_sampling_follows_the_device_seed(dev):
    from mi355_mp import ops
    from torch_geometric.utils import negative_sampling, structured_negative_sampling
    rng = np.random.default_rng(12)
    n = 200
    ei = rng.integers(0, n, (2, 600)).astype(np.int64)
    eid = _t(ei, dev)
    edges = {(int(a), int(b)) for a, b in ei.T}
    torch.cuda.manual_seed(77)
    a1, a2 = negative_sampling(eid, n), negative_sampling(eid, n)
    i, j, k = structured_negative_sampling(eid, n)
    torch.cuda.manual_seed(77)
    b1, b2 = negative_sampling(eid, n), negative_sampling(eid, n)
    i2, j2, k2 = structured_negative_sampling(eid)             # num_nodes from the edge list
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)
    assert a1.shape == (2, 600) and not ({(int(p), int(q)) for p, q in a1.cpu().numpy().T} & edges)
    assert torch.equal(i, eid[0]) and torch.equal(j, eid[1]) and k.shape == (600,)
    if int(ei.max()) == n - 1:
        assert torch.equal(k, k2)
    torch.cuda.manual_seed(78)
    assert not torch.equal(negative_sampling(eid, n), a1)
    und = negative_sampling(eid, n, num_neg_samples=100, force_undirected=True)
    assert und.shape == (2, 100) and torch.equal(und[:, :50], und[:, 50:].flip(0))
    with pytest.raises(IndexError):
        ops.negative_sample(eid, n - 150)                        # an end outside [0, N)
    with pytest.raises(IndexError):
        ops.edge_score(torch.zeros((10, 4), device=dev), eid)


def test_known_answer_file(dev):
    from mi355_mp import ops
    from tests.golden import make_golden_link as G
    kat = np.load(os.path.join(ROOT, "tests", "golden", "link", "link_kat.npz"))
    for name, n in (("edges", G.N), ("path", 5), ("almost", 6)):
        eid = _t(kat[name], dev)
        for q, seed in enumerate(G.SEEDS):
            assert np.array_equal(ops.negative_sample(eid, n, seed=seed).cpu().numpy(), kat["%s_full_s%d" % (name, q)])
            got = ops.negative_sample(eid, n, seed=seed, force_undirected=True).cpu().numpy()
            assert np.array_equal(got, kat["%s_upper_s%d" % (name, q)])
        assert np.array_equal(ops.negative_sample(eid, n, seed=G.SEEDS[0], loops=True).cpu().numpy(),
                              kat[name + "_loops_s0"])
        assert np.array_equal(ops.structured_negative_sample(eid, n, seed=G.SEEDS[0]).cpu().numpy(),
                              kat[name + "_rows_s0"])
        from torch_geometric.utils import to_undirected
        assert np.array_equal(to_undirected(eid, n).cpu().numpy(), kat[name + "_undirected"])
    z, ei = kat["z"], kat["edges"]
    v = ops.edge_score(_t(z, dev), _t(ei, dev)).cpu().numpy()
    assert np.array_equal(v.astype(np.float64), kat["v"])        # quarter-integer z: every sum is exact


def test_training_step_reads_nothing_back(dev):
    from torch_geometric.nn import GAE
    rng = np.random.default_rng(13)
    n, C = 500, 16
    posd = _t(_hub_graph(rng, n, 2000), dev)
    model = GAE(torch.nn.Identity())
    z0 = _t(_z(rng, n, C) * np.float32(0.3), dev)

    def step():
        zd = z0.clone().requires_grad_(True)
        loss = model.recon_loss(zd, posd)
        loss.backward()
        return loss.detach(), zd.grad

    step()                                                       # warm-up: the caches of pos_edge_index are built
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, grad = step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all()) and bool(grad.abs().sum() > 0)


def test_custom_decoder_equals_the_stock_path(dev):
    """Upstream's composition forms 1 - sigmoid(v) by an fp32 subtraction, which loses
    digits as v grows; the comparison therefore runs at |v| <= 0.5, where that
    costs a few u, on 65 edges, where torch's fp32 mean adds no more."""
    from mi355_mp import ops
    from torch_geometric.nn import GAE, InnerProductDecoder

    class Mine(InnerProductDecoder):
        pass

    rng = np.random.default_rng(14)
    n, C = 40, 16
    pos = _edges(rng, n, 65)
    posd = _t(pos, dev)
    torch.cuda.manual_seed(5)
    neg = ops.negative_sample(posd, n, loops=True).cpu().numpy()
    z = _scaled_z(rng, n, C, np.concatenate([pos, neg], axis=1), vmax=0.5)
    losses, grads = [], []
    for model in (GAE(torch.nn.Identity()), GAE(torch.nn.Identity(), Mine())):
        torch.cuda.manual_seed(5)
        zd = _t(z, dev).requires_grad_(True)
        loss = model.recon_loss(zd, posd)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(zd.grad.cpu().numpy().astype(np.float64))
    _, cp, tp = R.side_loss(z, pos[0], pos[1], True)
    _, cn, tn = R.side_loss(z, neg[0], neg[1], False)
    dvp, dvn = R.score_bound(z, pos[0], pos[1]), R.score_bound(z, neg[0], neg[1])
    bound = dvp.mean() + dvn.mean() + 8 * U * (2 + np.abs(tp).mean() + np.abs(tn).mean())
    print("custom decoder: |L_stock - L_custom| = %.3g, bound %.3g" % (abs(losses[0] - losses[1]), bound))
    assert abs(losses[0] - losses[1]) <= bound
    gb = R.grad_bound(z, np.concatenate([pos[0], neg[0]]), np.concatenate([pos[1], neg[1]]), np.concatenate([cp, cn]),
                      np.concatenate([(0.25 * dvp + 8 * U) / 65, (0.25 * dvn + 8 * U) / neg.shape[1]]))
    assert (np.abs(grads[0] - grads[1]) <= 2 * gb).all()         # each within its bound of the float64 gradient
    auc, ap = GAE(torch.nn.Identity()).test(_t(z, dev), posd, _t(neg, dev))
    s = np.concatenate([R.sigmoid(R.score(z, pos[0], pos[1])), R.sigmoid(R.score(z, neg[0], neg[1]))])
    y = np.concatenate([np.ones(65), np.zeros(neg.shape[1])])
    assert 0.0 <= auc <= 1.0 and 0.0 <= ap <= 1.0
    assert abs(auc - R.roc_auc(y, s)) <= 0.02 and abs(ap - R.average_precision(y, s)) <= 0.02


def test_vgae_on_the_device(dev):
    from torch_geometric.nn import VGAE
    from torch_geometric.nn.models.autoencoder import MAX_LOGVAR

    class Enc(torch.nn.Module):
        def __init__(self):
            super(Enc, self).__init__()
            self.mu, self.lv = torch.nn.Linear(6, 8), torch.nn.Linear(6, 8)

        def forward(self, x):
            return self.mu(x), 9 * self.lv(x)

    torch.manual_seed(3)
    model = VGAE(Enc()).to(dev)
    x = torch.randn(50, 6, device=dev) * 2
    mu, raw = model.encoder(x)
    assert float(raw.detach().max()) > MAX_LOGVAR
    logvar = raw.clamp(max=MAX_LOGVAR)
    model.eval()
    assert torch.equal(model.encode(x), mu)
    kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1))
    assert torch.equal(model.kl_loss(), kl) and torch.equal(model.kl_loss(mu, raw), kl)
    assert math.isfinite(float(kl.detach()))
    model.train()
    torch.cuda.manual_seed(9)
    z = model.encode(x)
    torch.cuda.manual_seed(9)
    assert torch.equal(z, mu + torch.randn_like(logvar) * torch.exp(logvar))
    # the whole model trains through the fused loss
    ei = torch.randint(0, 50, (2, 120), device=dev)
    loss = model.recon_loss(z, ei) + 0.001 * model.kl_loss()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
