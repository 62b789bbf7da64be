"""GPU tests of knn, knn_graph, nearest, knn_interpolate, EdgeConv and
DynamicEdgeConv (csrc/mp_knn.hip) against the numpy restatement tests/_knn_ref.py.

Indices are an ordering of (fp32 d2, index) pairs, and the d2 are single fp32
operations, so they must equal the restatement exactly, everywhere.  The
interpolation is two fp32 sums and a division: per element it is held to
|out - ref| <= 4 * (k + 2) * 2^-24 * max_t |x[i_t, c]| against the float64
restatement from the float32 d2 (the weights carry one rounding each, the
numerator k products and k - 1 sums, the denominator k - 1 sums, one division:
about (2k + 3) half-ulps of a convex combination; the bound is doubled).

Shapes.  One wave searches for one query, 64 candidates at a time, and a workgroup
of four queries stages tiles of 256 candidates when its queries search the same
rows: graphs of 0, 1, k - 1, k, k + 1, 63, 64, 65, 129 and 257 points put a graph
below, at and above k, a tile's and a wave's edge, with a graph missing on either
side; graphs of one to three queries make the waves of a workgroup search
different rows.  Widths 1, 2, 3, 8 run with the points in registers, 9, 64, 70
on the general path.
"""
import numpy as np
import pytest
import torch

from tests import _knn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _batch(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def _cloud(n, D, kind, rng):
    if kind == "random":
        return (rng.random((n, D)) * 2 - 1).astype(np.float32)
    if kind == "lattice":                                # many equal distances
        return rng.integers(0, 8 if D <= 3 else 3, (n, D)).astype(np.float32)
    assert kind == "duplicates"                          # a handful of distinct points
    return rng.integers(0, 2, (n, min(D, 3))).astype(np.float32)[:, np.arange(D) % min(D, 3)]


_REF = {}


def _ref(key, make):
    """Every reference is computed once and shared between the tests that need it."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _knn(x, y, k, bx=None, by=None):
    from torch_geometric.nn import knn
    out = knn(x if torch.is_tensor(x) else _dev(x), y if torch.is_tensor(y) else _dev(y), k, _dev(bx), _dev(by))
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] == 2
    return out.cpu().numpy()


# ---- knn: the grid -------------------------------------------------------------------------------

def _grid_case(k, D):
    """x: graphs of 0, 1, k - 1, k, k + 1, 63, 64, 65, 129, 257 points (graph 0 is missing from
    x); y: a few queries per graph, none in graph 6, and two in a graph past the last of x.
    Lattice coordinates for every other case: ties abound."""
    def make():
        rng = np.random.default_rng(100 * k + D)
        xs = [0, 1, k - 1, k, k + 1, 63, 64, 65, 129, 257]
        ys = [2, 3, 5, 4, 6, 7, 0, 9, 5, 6, 2]
        kind = "lattice" if (k + D) % 2 == 0 else "random"
        x, y = _cloud(sum(xs), D, kind, rng), _cloud(sum(ys), D, kind, rng)
        bx, by = _batch(xs), _batch(ys)
        return x, y, bx, by, R.knn(x, y, k, bx, by)
    return _ref(("grid", k, D), make)


@pytest.mark.parametrize("k", [1, 3, 16, 63, 64])
@pytest.mark.parametrize("D", [1, 2, 3, 8, 9, 64, 70])
def test_knn_is_the_restatement(D, k):
    from mi355_mp import ops
    assert ops.knn_path(D) == (0 if D <= 8 else 1)
    x, y, bx, by, want = _grid_case(k, D)
    got = _knn(x, y, k, bx, by)
    assert got.shape == want.shape and np.array_equal(got, want), \
        "%d of %d pairs differ" % (int((got != want).any(0).sum()) if got.shape == want.shape else -1, want.shape[1])
    per_query = np.bincount(want[0], minlength=len(y))
    sizes = np.bincount(bx, minlength=11)[by]
    assert np.array_equal(per_query, np.minimum(sizes, k)) and per_query.min() == 0 and per_query.max() == k
    assert ((bx[got[1]] == by[got[0]])).all()             # never outside the query's graph


@pytest.mark.parametrize("D", [3, 8, 64])
def test_knn_with_row_strides_and_no_batch(D):
    rng = np.random.default_rng(30 + D)
    wide_x = _cloud(700, D + 5, "random", rng)
    wide_y = _cloud(133, D + 3, "random", rng)
    x, y = wide_x[:, 2:2 + D], wide_y[:, 1:1 + D]
    xs, ys = _dev(wide_x)[:, 2:2 + D], _dev(wide_y)[:, 1:1 + D]
    assert not xs.is_contiguous() and not ys.is_contiguous()
    for k in (5, 64):
        want = R.knn(x, y, k)
        got = _knn(xs, ys, k)
        assert np.array_equal(got, want) and got.shape == (2, 133 * k)
        assert (np.diff(got[0]) >= 0).all()
    # the point itself comes first
    same = _knn(xs, xs[:10], 1)
    assert same.tolist() == [list(range(10)), list(range(10))]
    # a vector of coordinates is a cloud of width 1
    if D == 3:
        assert np.array_equal(_knn(np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(y[:, 0]), 4),
                              R.knn(x[:, 0], y[:, 0], 4))


@pytest.mark.parametrize("kind", ["lattice", "duplicates"])
@pytest.mark.parametrize("D", [2, 3, 9])
def test_ties_go_to_the_lower_index(kind, D):
    rng = np.random.default_rng(40 + D)
    sizes = [70, 200, 300]
    x = _cloud(sum(sizes), D, kind, rng)
    y = x[::3].copy()                                     # queries on the points themselves
    bx, by = _batch(sizes), _batch(sizes)[::3]
    for k in (4, 33):
        pairs, d2 = R.knn_with_d2(x, y, k, bx, by)
        got = _knn(x, y, k, bx, by)
        assert np.array_equal(got, pairs)
        # what the case is for: equal distances inside a query's selection, and at its edge
        tied = (np.diff(d2) == 0) & (np.diff(pairs[0]) == 0)
        assert tied.mean() > 0.2
        assert (np.diff(pairs[1])[tied] > 0).all()


def test_every_candidate_is_closer_than_the_last():
    # points on a line in index order, the query beyond the far end: the candidates arrive in descending
    # distance, so every one of them is inserted at the front of the selection
    x = np.arange(257, dtype=np.float32)
    for D in (1, 9):
        xs = np.repeat(x[:, None], D, axis=1)
        far, near = np.full((1, D), 300, dtype=np.float32), np.full((1, D), -10, dtype=np.float32)
        got = _knn(xs, np.concatenate([far, near, far]), 64)
        assert got[1][:64].tolist() == list(range(256, 192, -1))
        assert got[1][64:128].tolist() == list(range(64))             # and the best case: nothing after the first tile
        assert np.array_equal(got, R.knn(xs, np.concatenate([far, near, far]), 64))


@pytest.mark.parametrize("D", [3, 9])
def test_a_workgroup_straddling_graphs(D):
    rng = np.random.default_rng(50 + D)
    ys = [1 + g % 3 for g in range(41)]                   # one to three queries per graph: four waves, several graphs
    xs = [int(v) for v in rng.integers(0, 90, 41)]
    xs[5], xs[17] = 0, 300
    x, y = _cloud(sum(xs), D, "lattice", rng), _cloud(sum(ys), D, "lattice", rng)
    bx, by = _batch(xs), _batch(ys)
    for k in (3, 40):
        assert np.array_equal(_knn(x, y, k, bx, by), R.knn(x, y, k, bx, by))


def test_known_answers():
    import os
    from torch_geometric.nn import knn, knn_graph, nearest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kat = np.load(os.path.join(root, "tests", "golden", "knn", "knn_kat.npz"))
    lattice, centres, dups, pos, y, batch, batch_y = (_dev(kat[k]) for k in ("lattice", "centres", "dups", "pos", "y",
                                                                            "batch", "batch_y"))
    for k in (1, 3, 16):
        assert np.array_equal(knn(lattice, lattice, k).cpu().numpy(), kat["lattice_self_k%d" % k])
        assert np.array_equal(knn(lattice, centres, k).cpu().numpy(), kat["lattice_centres_k%d" % k])
        assert np.array_equal(knn(dups, dups, k).cpu().numpy(), kat["dups_k%d" % k])
        assert np.array_equal(knn(pos, y, k, batch, batch_y).cpu().numpy(), kat["batch_k%d" % k])
    assert np.array_equal(knn_graph(pos, 3, batch).cpu().numpy(), kat["graph_k3"])
    assert np.array_equal(knn_graph(pos, 3, batch, True, "target_to_source").cpu().numpy(), kat["graph_k3_loop_t2s"])
    assert np.array_equal(knn_graph(dups, 2).cpu().numpy(), kat["graph_dups_k2"])
    assert np.array_equal(nearest(centres, lattice).cpu().numpy(), kat["nearest_lattice"])
    has_x = torch.as_tensor(np.isin(kat["batch_y"], np.unique(kat["batch"]))).to(DEV)
    assert np.array_equal(nearest(y[has_x], pos, batch_y[has_x], batch).cpu().numpy(), kat["nearest_batch"])


# ---- knn_graph, nearest --------------------------------------------------------------------------

@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_knn_graph_is_the_restatement(loop, flow):
    from torch_geometric.nn import knn_graph
    sizes = [1, 2, 65, 300]
    x = _ref("kg_cloud", lambda: _cloud(sum(sizes), 3, "duplicates", np.random.default_rng(60)))
    batch = _batch(sizes)
    want = R.knn_graph(x, 4, batch, loop, flow)
    got = knn_graph(_dev(x), 4, _dev(batch), loop, flow).cpu().numpy()
    assert np.array_equal(got, want)
    target = want[1] if flow == "source_to_target" else want[0]
    assert np.bincount(target).max() == (4 if loop else 5)   # upstream's quirk: coincident points of lower index


def test_knn_graph_quirk_and_its_limit():
    from torch_geometric.nn import knn_graph
    x = np.asarray([[1, 1], [1, 1], [1, 1], [5, 5]], dtype=np.float32)
    got = knn_graph(_dev(x), 1).cpu().numpy()
    assert got.tolist() == [[1, 0, 0, 1, 0], [0, 1, 2, 2, 3]] == R.knn_graph(x, 1).tolist()
    cloud = _dev(_cloud(100, 3, "random", np.random.default_rng(61)))
    assert knn_graph(cloud, 63).shape == (2, 100 * 63)   # k + 1 = 64 is the limit without loops
    assert knn_graph(cloud, 64, loop=True).shape == (2, 100 * 64)
    with pytest.raises(ValueError, match="64"):
        knn_graph(cloud, 64)


def test_nearest_and_an_x_without_a_y():
    from torch_geometric.nn import nearest
    rng = np.random.default_rng(62)
    xs, ys = [40, 0, 130, 7], [3, 5, 66, 1]
    x, y = _cloud(sum(xs), 3, "lattice", rng), _cloud(sum(ys), 3, "lattice", rng)
    bx, by = _batch(xs), _batch(ys)
    got = nearest(_dev(x), _dev(y), _dev(bx), _dev(by)).cpu().numpy()
    assert got.shape == (sum(xs),) and np.array_equal(got, R.nearest(x, y, bx, by))
    assert np.array_equal(got, R.knn(y, x, 1, by, bx)[1])
    assert np.array_equal(nearest(_dev(x), _dev(y)).cpu().numpy(), R.nearest(x, y))
    ys[2] = 0                                             # graph 2 of x now has no y
    y2, by2 = y[:sum(ys)], _batch(ys)
    with pytest.raises(ValueError, match="130 rows of x"):
        nearest(_dev(x), _dev(y2), _dev(bx), _dev(by2))


# ---- knn_interpolate -----------------------------------------------------------------------------

def _interp_case():
    """Coarse points in four graphs (graph 1 has none), fine points in all four; every
    fifth fine point coincides with a coarse point of its graph (d2 = 0: the clamp)."""
    def make():
        rng = np.random.default_rng(70)
        xs, ys = [30, 0, 9, 200], [50, 6, 33, 260]
        pos_x, pos_y = _cloud(sum(xs), 3, "random", rng), _cloud(sum(ys), 3, "random", rng)
        bx, by = _batch(xs), _batch(ys)
        sx = np.concatenate([[0], np.cumsum(xs)])
        for j in range(0, len(pos_y), 5):
            g = by[j]
            if xs[g]:
                pos_y[j] = pos_x[sx[g] + j % xs[g]]
        feat = rng.standard_normal((sum(xs), 130)).astype(np.float32)
        return pos_x, pos_y, bx, by, feat
    return _ref("interp", make)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 5, 64, 130])
def test_interpolation_forward_and_gradient(C, k):
    from torch_geometric.nn import knn_interpolate
    pos_x, pos_y, bx, by, feat = _interp_case()
    x = np.ascontiguousarray(feat[:, :C])
    want, scale, pairs, wn = _ref(("interp", C, k), lambda: R.knn_interpolate(x, pos_x, pos_y, bx, by, k))
    _, dist = R.knn_with_d2(pos_x, pos_y, k, bx, by)
    assert (dist == 0).sum() >= 40                        # coincident points: the clamp
    xd = _dev(x).requires_grad_(True)
    out = knn_interpolate(xd, _dev(pos_x), _dev(pos_y), _dev(bx), _dev(by), k=k)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(pos_y), C)
    got = out.detach().cpu().numpy().astype(np.float64)
    err, bound = np.abs(got - want), 4 * (k + 2) * U * scale
    print("forward C=%d k=%d: worst |err| / bound = %.3f" % (C, k, float((err[bound > 0] / bound[bound > 0]).max())))
    assert (err <= bound).all(), float((err - bound).max())
    assert (got[by == 1] == 0).all() and (want[by == 1] == 0).all()   # a y whose graph holds no x: zeros
    # gradient to x: d x[i] = sum_j wn_ji g[j]; the bound with g in place of x and the in-degree in place of k
    g = np.random.default_rng(71).standard_normal(want.shape).astype(np.float32)
    out.backward(_dev(g))
    gref, gscale, deg = R.knn_interpolate_grad(g, pairs, wn, len(pos_x))
    gerr, gbound = np.abs(xd.grad.cpu().numpy().astype(np.float64) - gref), 4 * (deg[:, None] + 2) * U * gscale
    live = gbound > 0
    print("backward C=%d k=%d: worst |err| / bound = %.3f, largest in-degree %d"
          % (C, k, float((gerr[live] / gbound[live]).max()), int(deg.max())))
    assert (gerr <= gbound).all(), float((gerr - gbound).max())
    assert (xd.grad[torch.as_tensor(deg == 0).to(DEV)] == 0).all()
    # two backward runs give equal bits
    first_grad = xd.grad.clone()
    xd.grad = None
    knn_interpolate(xd, _dev(pos_x), _dev(pos_y), _dev(bx), _dev(by), k=k).backward(_dev(g))
    assert torch.equal(xd.grad, first_grad)


def test_interpolation_without_a_batch_with_a_row_stride_and_no_gradient_to_positions():
    from torch_geometric.nn import knn_interpolate
    rng = np.random.default_rng(72)
    pos_x, pos_y = _cloud(90, 3, "random", rng), _cloud(400, 3, "random", rng)
    wide = rng.standard_normal((90, 40)).astype(np.float32)
    x = wide[:, 4:36]
    want, scale, _, _ = R.knn_interpolate(x, pos_x, pos_y)
    px, py = _dev(pos_x).requires_grad_(True), _dev(pos_y).requires_grad_(True)
    xd = _dev(wide)[:, 4:36].requires_grad_(True)
    assert not xd.is_contiguous()
    out = knn_interpolate(xd, px, py)                     # k = 3
    assert (np.abs(out.detach().cpu().numpy() - want) <= 4 * 5 * U * scale).all()
    out.sum().backward()
    assert px.grad is None and py.grad is None
    # every row of weights sums to one: the gradient of sum(out) is the total weight a source carries
    assert abs(float(xd.grad.sum()) / (400 * 32) - 1) < 1e-5


# ---- host reads ----------------------------------------------------------------------------------

def test_host_reads():
    """knn with both batch vectors None reads nothing from the device (E = n_y * min(k, n_x));
    knn_interpolate's forward reads nothing beyond the batch layouts, which the first call
    caches.  torch's sync debug mode raises on any synchronising call."""
    from torch_geometric.nn import knn, knn_interpolate
    rng = np.random.default_rng(80)
    sizes_x, sizes_y = [50, 70], [20, 30]
    x, y = _dev(_cloud(120, 3, "random", rng)), _dev(_cloud(50, 3, "random", rng))
    bx, by = _dev(_batch(sizes_x)), _dev(_batch(sizes_y))
    feat = torch.randn(120, 16, device=DEV)
    warm = (knn(x, y, 4), knn_interpolate(feat, x, y, bx, by), knn(x, y, 4, bx, by), knn(x[:3], y, 4))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pairs = knn(x, y, 4)
        few = knn(x[:3], y, 4)                            # k above n_x: E = n_y * n_x
        out = knn_interpolate(feat, x, y, bx, by)
        with pytest.raises(RuntimeError):                 # with batch vectors knn reads E: the mode does notice
            knn(x, y, 4, bx, by)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(pairs, warm[0]) and torch.equal(out, warm[1]) and tuple(few.shape) == (2, 150)
    assert torch.equal(knn(x, y, 4, bx, by), warm[2])


# ---- EdgeConv, DynamicEdgeConv -------------------------------------------------------------------

def _mlp(c_in, c_out):
    return torch.nn.Sequential(torch.nn.Linear(2 * c_in, 16), torch.nn.ReLU(), torch.nn.Linear(16, c_out))


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_edge_conv_agrees_with_a_plain_message_passing_subclass(aggr):
    import copy
    from torch_geometric.nn import EdgeConv, MessagePassing

    class PlainEdgeConv(MessagePassing):
        def __init__(self, mlp, aggr):
            super(PlainEdgeConv, self).__init__(aggr=aggr)
            self.mlp = mlp

        def forward(self, x, edge_index):
            return self.propagate(edge_index, x=x)

        def message(self, x_i, x_j):
            return self.mlp(torch.cat([x_i, x_j - x_i], dim=1))

    rng = np.random.default_rng(90)
    n, E, C = 150, 1200, 5
    x = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(DEV)
    edge_index = torch.from_numpy(np.stack([rng.integers(0, n, E), rng.integers(0, n - 1, E)])).to(DEV)
    torch.manual_seed(0)
    layer = EdgeConv(_mlp(C, 7), aggr=aggr).to(DEV)
    plain = PlainEdgeConv(copy.deepcopy(layer.nn), aggr).to(DEV)
    outs = []
    for mod in (layer, plain):
        xin = x.clone().requires_grad_(True)
        out = mod(xin, edge_index)
        out.square().sum().backward()
        outs.append((out.detach(), xin.grad, [q.grad for q in mod.parameters()]))
    (out, gx, gp), (rout, rgx, rgp) = outs
    assert tuple(out.shape) == (n, 7) and bool((out[n - 1] == 0).all())     # the node without an edge
    # the same operations in the same order on deterministic kernels
    assert torch.equal(out, rout) and torch.equal(gx, rgx)
    for a, b in zip(gp, rgp):
        assert torch.equal(a, b)
    assert float(gx.abs().sum()) > 0 and all(float(a.abs().sum()) > 0 for a in gp)


@pytest.mark.parametrize("D", [3, 64])
def test_dynamic_edge_conv_is_edge_conv_on_the_knn_graph(D):
    from torch_geometric.nn import DynamicEdgeConv, EdgeConv, knn_graph
    rng = np.random.default_rng(91 + D)
    sizes = [40, 7, 130]
    xn = _cloud(sum(sizes), D, "random", rng)
    x, batch = _dev(xn), _dev(_batch(sizes))
    torch.manual_seed(0)
    dyn = DynamicEdgeConv(_mlp(D, 6), k=6).to(DEV)
    static = EdgeConv(dyn.nn)                             # the two share the network (and its reset)
    edge_index = knn_graph(x, 6, batch)
    assert np.array_equal(edge_index.cpu().numpy(), R.knn_graph(xn, 6, _batch(sizes)))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = dyn(xa, batch)
    out.square().sum().backward()
    ga = [q.grad.clone() for q in dyn.parameters()]
    for q in dyn.parameters():
        q.grad = None
    ref = static(xb, edge_index)
    ref.square().sum().backward()
    assert tuple(out.shape) == (sum(sizes), 6) and torch.equal(out, ref) and torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(a, q.grad) for a, q in zip(ga, static.parameters()))
    # without a batch vector the neighbours come from the whole set
    assert torch.equal(dyn(x), static(x, knn_graph(x, 6)))


# ---- errors --------------------------------------------------------------------------------------

def test_bad_arguments_raise_and_leave_the_device_healthy():
    from mi355_mp import ops
    from torch_geometric.nn import knn, knn_graph, knn_interpolate, nearest
    pos = _dev(_cloud(40, 3, "lattice", np.random.default_rng(95)))
    y = pos[:7].contiguous()
    batch = _dev(_batch([15, 25]))
    by = _dev(np.asarray([0, 0, 0, 1, 1, 1, 1]))
    unsorted = batch.flip(0).contiguous()
    too_wide = torch.zeros(40, ops.knn_max_d() + 1, device=DEV)
    feat = torch.randn(40, 8, device=DEV)
    good = knn(pos, y, 5, batch, by)
    good_interp = knn_interpolate(feat, pos, y, batch, by)
    bad = [lambda: knn(pos, y, 5, unsorted, by),
           lambda: knn(pos, y, 5, batch, by.flip(0).contiguous()),
           lambda: knn(pos, y, 5, batch, None),
           lambda: knn(pos, y, 5, None, by),
           lambda: knn(pos, y, 0, batch, by),
           lambda: knn(pos, y, -1),
           lambda: knn(pos, y, 65, batch, by),
           lambda: knn(pos, y[:, :2], 5, batch, by),
           lambda: knn(too_wide, too_wide[:7], 5, batch, by),
           lambda: knn_graph(pos, 0, batch, loop=True),
           lambda: knn_graph(pos, 64, batch),
           lambda: knn_graph(pos, 5, unsorted),
           lambda: nearest(pos, y, batch, None),
           lambda: knn_interpolate(feat, pos, y, unsorted, by),
           lambda: knn_interpolate(feat, pos, y, batch, by, k=65),
           lambda: knn_interpolate(feat, pos, y, batch, by, k=0),
           lambda: knn_interpolate(feat[:30], pos, y, batch, by)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
    for call in (lambda: knn(pos, y, 5, batch, by, cosine=True), lambda: knn_graph(pos, 5, batch, cosine=True)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="limit of 64"):
        knn(pos, y, 65)
    assert torch.equal(knn(pos, y, 5, batch, by), good)
    assert torch.equal(knn_interpolate(feat, pos, y, batch, by), good_interp)
    assert np.array_equal(good.cpu().numpy(),
                          R.knn(pos.cpu().numpy(), y.cpu().numpy(), 5, batch.cpu().numpy(), by.cpu().numpy()))
    at_the_limit = knn(torch.zeros(40, ops.knn_max_d(), device=DEV), torch.zeros(7, ops.knn_max_d(), device=DEV), 2)
    assert at_the_limit[1].tolist() == [0, 1] * 7         # every distance is 0: the lowest indices
