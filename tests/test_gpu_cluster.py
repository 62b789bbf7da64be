"""GPU tests of cluster pooling (voxel_grid, consecutive_cluster, max_pool / avg_pool
and their _x forms; csrc/mp_cluster.hip) against the CPU restatement
tests/_cluster_ref.py.

Integer outputs (voxel keys, cluster ids, perm, arg, batch, the coalesced edge
index) and the max are exact.  Means and edge-attribute sums follow the project's
fp32 rule: |err| <= 1e-5 * sum |terms| of the float64 restatement (for a mean, the
terms are the members' |values| / count); the edge-attribute sums are in addition
bitwise equal to the float32 CPU sum in ascending original edge position.
"""
import importlib.util
import os

import pytest
import torch

from tests import _cluster_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOUND = 1e-5
SIZES = [1, 64, 75, 130]
GRAPH_IDS = [0, 1, 2, 4]                                   # id 3 is unused


def _assert_bound(got, ref, scale, what):
    err = (got.detach().cpu().double() - ref.detach()).abs()
    ratio = float((err / scale.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert err.numel() == 0 or float((err - BOUND * scale).max()) <= 0.0, "%s: max ratio %.3g" % (what, ratio)


def _batch():
    return torch.cat([torch.full((n,), g, dtype=torch.int64) for n, g in zip(SIZES, GRAPH_IDS)])


def _graph_case(F, attr_mode, seed=0):
    """Graphs of 1, 64, 75 and 130 nodes (graph id 3 unused) on [0, 28)^2 under 5-wide
    voxels: the 130-node graph sits inside one voxel (a cluster of > 64 members, all
    of its edges loops), the others give clusters of one and of a few members.  x
    takes five values (ties) and some entries below -10000; the single node of graph
    0 holds nothing else in column 0."""
    g = torch.Generator().manual_seed(seed)
    n = sum(SIZES)
    batch = _batch()
    pos = torch.rand(n, 2, generator=g) * 28
    pos[-130:] = 10.5 + torch.rand(130, 2, generator=g) * 4
    x = torch.randint(-2, 3, (n, F), generator=g).float() * 0.5
    x[torch.rand(n, F, generator=g) < 0.05] = -20000.0
    x[0, 0] = -20000.0
    parts, off = [], 0
    for s in SIZES:
        parts.append(torch.randint(0, s, (2, 8 * s), generator=g) + off)
        off += s
    ei = torch.cat(parts, dim=1)[:, torch.randperm(8 * n, generator=g)]
    E = ei.size(1)
    attr = {"none": None, "vec": torch.rand(E, generator=g) - 0.3, "mat": torch.rand(E, 2, generator=g) - 0.3}[attr_mode]
    cluster = R.voxel_grid(pos, batch, 5, 0, 28)
    return cluster, x, pos, batch, ei, attr


def _data(x, pos, batch, ei, attr):
    from torch_geometric.data import Batch
    return Batch(batch=None if batch is None else batch.to(DEV), x=x.to(DEV), pos=None if pos is None else pos.to(DEV),
                 edge_index=ei.to(DEV), edge_attr=None if attr is None else attr.to(DEV))


def _selection(cluster, x, pos, batch, ei, attr, reduce="max"):
    """The ops-level stage (what max_pool runs), with arg and edge_slot kept."""
    from mi355_mp import ops
    sel = ops.cluster_build(cluster.to(DEV))
    x_out, arg, pos_out, batch_out = ops.cluster_reduce(sel, x.to(DEV), reduce, pos=pos.to(DEV),
                                                        batch=None if batch is None else batch.to(DEV))
    ep = ops.pool_edges(ei.to(DEV), sel)
    a = None if attr is None else ops.pool_edge_attr_sum(attr.to(DEV), ep, sel)
    M, kept, _ = ops.cluster_read_counts(sel)
    return {"inv": sel.inv, "perm": sel.perm[:M], "x": x_out[:M], "arg": None if arg is None else arg[:M],
            "pos": pos_out[:M], "batch": None if batch_out is None else batch_out[:M], "edge_index": ep.out[:, :kept],
            "edge_attr": None if a is None else a[:kept], "edge_slot": ep.edge_slot}


def _mean_scale(v, inv, M):
    """sum |terms| of a cluster mean: the members' |values| / count (float64)."""
    v = v.double().abs()
    cnt = torch.zeros(M, dtype=torch.float64).index_add_(0, inv, torch.ones(inv.numel(), dtype=torch.float64))
    return torch.zeros((M,) + tuple(v.shape[1:]), dtype=torch.float64).index_add_(0, inv, v) / cnt.view(-1, 1)


def _attr_scale(attr, slot, Ep):
    keep = slot >= 0
    a = attr.double().abs()
    return torch.zeros((Ep,) + tuple(a.shape[1:]), dtype=torch.float64).index_add_(0, slot[keep], a[keep])


def _check_stage(got, ref, x, pos, attr, reduce="max"):
    M, Ep = ref["perm"].numel(), ref["edge_index"].size(1)
    assert torch.equal(got["inv"].cpu(), ref["inv"]) and torch.equal(got["perm"].cpu(), ref["perm"])
    if reduce == "max":
        assert torch.equal(got["x"].cpu(), ref["x"])
        if got.get("arg") is not None:
            assert torch.equal(got["arg"].cpu(), ref["arg"])
    else:
        r64 = R.pool_f64(x.double(), None, None, ref["inv"], None, None, M, 0, "mean")[0]
        _assert_bound(got["x"], r64, _mean_scale(x, ref["inv"], M), "mean of x")
    if ref["batch"] is None:
        assert got["batch"] is None
    else:
        assert torch.equal(got["batch"].cpu(), ref["batch"])
    assert got["edge_index"].dtype == torch.int64 and tuple(got["edge_index"].shape) == (2, Ep)
    assert torch.equal(got["edge_index"].cpu(), ref["edge_index"])
    if got.get("edge_slot") is not None:
        assert torch.equal(got["edge_slot"].cpu(), ref["edge_slot"])
    p64 = R.pool_f64(None, pos.double(), None, ref["inv"], None, None, M, 0, "mean")[1]
    _assert_bound(got["pos"], p64, _mean_scale(pos, ref["inv"], M), "pos_out")
    if attr is None:
        assert got["edge_attr"] is None
    else:
        assert tuple(got["edge_attr"].shape) == (Ep,) + tuple(attr.shape[1:])
        a64 = R.pool_edge(ref["inv"], EI_OF[id(ref)], attr.double(), M)[1]
        _assert_bound(got["edge_attr"], a64, _attr_scale(attr, ref["edge_slot"], Ep), "edge_attr_out")
        assert torch.equal(got["edge_attr"].cpu(), ref["edge_attr"]), "edge_attr_out is not the ordered float32 sum"


EI_OF = {}


def _ref(cluster, x, pos, batch, ei, attr, reduce="max"):
    ref = R.pool(cluster, x, pos, batch, ei, attr, reduce)
    EI_OF[id(ref)] = ei
    return ref


# ---- voxel keys ------------------------------------------------------------------

def _voxel_points(D, seed):
    """~300 nodes in 4 graphs of unequal size (ids 0, 1, 2, 4), positions in [0, 28)^D,
    some placed exactly on cell edges fl32(k * size), at `end`, and outside [start, end]."""
    g = torch.Generator().manual_seed(seed)
    sizes = [100, 120, 77, 3]
    batch = torch.cat([torch.full((n,), b, dtype=torch.int64) for n, b in zip(sizes, GRAPH_IDS)])
    n = sum(sizes)
    pos = torch.rand(n, D, generator=g) * 28
    return pos, batch, g


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("size,start,end", [(5, 0, 28), (7, 0, 28), (14, 0, 27.99), (0.1, 0, 28), ([5, 0.1, 3], 0, 28),
                                             (5, None, None), ([0.1, 7], None, 28), (2.5, [1, 2, 3], [20, 27, 28])])
def test_voxel_keys_are_exact(D, size, start, end):
    from torch_geometric.nn import voxel_grid
    pos, batch, g = _voxel_points(D, 3 + D)
    n = pos.size(0)
    sz = torch.tensor(R.repeat(size, D), dtype=torch.float32)
    k = torch.randint(0, 12, (40, D), generator=g).float()
    pos[10:50] = k * sz                                            # exactly on cell edges: fl32(k * size)
    if end is not None:
        pos[50:60] = torch.tensor(R.repeat(end, D), dtype=torch.float32)      # at end
    pos[60:70] = -15 - torch.rand(10, D, generator=g) * 25         # below start (graph 0): negative keys
    pos[70:80] = 28 + torch.rand(10, D, generator=g) * 40          # above end: cells past the grid, collisions
    pos_in = pos[:, 0].contiguous() if D == 1 else pos
    want = R.voxel_grid(pos_in, batch, size, start, end)
    got = voxel_grid(pos_in.to(DEV), batch.to(DEV), size, start, end)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n,)
    assert torch.equal(got.cpu(), want)
    if start is not None and end is not None:
        assert int(want.min()) < 0 and want.unique().numel() < n
    # size / start / end as tensors, and a strided position view
    wide = torch.zeros(n, D + 2)
    wide[:, 1:D + 1] = pos
    got2 = voxel_grid(wide.to(DEV)[:, 1:D + 1], batch.to(DEV), torch.tensor(R.repeat(size, D)),
                      None if start is None else torch.tensor(R.repeat(start, D), dtype=torch.float32), end)
    assert torch.equal(got2.cpu(), want)


def test_voxel_grid_debug_mode_rejects_non_finite_positions():
    import torch_geometric
    from torch_geometric.nn import voxel_grid
    pos = torch.tensor([[0.0, 1.0], [float("nan"), 2.0]], device=DEV)
    batch = torch.zeros(2, dtype=torch.int64, device=DEV)
    with torch_geometric.debug():
        with pytest.raises(ValueError, match="finite"):
            voxel_grid(pos, batch, 1.0, 0, 4)
    with pytest.raises(TypeError, match="float32"):
        voxel_grid(pos.double(), batch, 1.0, 0, 4)


# ---- consecutive_cluster ------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_consecutive_cluster_is_exact(N):
    from torch_geometric.nn import consecutive_cluster
    g = torch.Generator().manual_seed(N)
    pool = torch.cat([torch.randint(-(1 << 40), 1 << 40, (max(N // 8, 1),), generator=g),
                      torch.tensor([-1, 0, 1, (1 << 40) + 3, -(1 << 40) - 3, (1 << 62) + 5, -(1 << 62)])])
    src = pool[torch.randint(0, pool.numel(), (N,), generator=g)]
    inv, perm = consecutive_cluster(src.to(DEV))
    uniq, want = torch.unique(src, sorted=True, return_inverse=True)
    assert torch.equal(inv.cpu(), want) and perm.dtype == torch.int64 and perm.numel() == uniq.numel()
    last = torch.zeros(uniq.numel(), dtype=torch.int64).scatter_reduce_(0, want, torch.arange(N), "amax",
                                                                        include_self=False)
    assert torch.equal(perm.cpu(), last)
    rinv, rperm = R.consecutive_cluster(src)
    assert torch.equal(rinv, want) and torch.equal(rperm, last)


# ---- max_pool end to end -------------------------------------------------------------

@pytest.mark.parametrize("F,attr_mode", [(1, "vec"), (3, "none"), (32, "mat"), (33, "vec"), (64, "none"), (130, "mat")])
def test_max_pool_end_to_end(F, attr_mode):
    from torch_geometric.nn import max_pool
    cluster, x, pos, batch, ei, attr = _graph_case(F, attr_mode, seed=F)
    ref = _ref(cluster, x, pos, batch, ei, attr)
    members = torch.bincount(ref["inv"])
    assert int(members.min()) == 1 and int(members.max()) > 64 and int(((members > 1) & (members < 10)).sum()) > 5
    keep = ref["edge_slot"] >= 0
    assert int((~keep).sum()) >= 8 * 130 and ref["edge_index"].size(1) < int(keep.sum())   # loops and duplicates
    assert bool((x < -10000).any()) and float(ref["x"][ref["batch"] == 0][0, 0]) == 0.0     # a masked maximum
    got = _selection(cluster, x, pos, batch, ei, attr)
    _check_stage(got, ref, x, pos, attr)
    out = max_pool(cluster.to(DEV), _data(x, pos, batch, ei, attr))
    layer = {"inv": got["inv"], "perm": got["perm"], "x": out.x, "pos": out.pos, "batch": out.batch,
             "edge_index": out.edge_index, "edge_attr": out.edge_attr}
    _check_stage(layer, ref, x, pos, attr)
    assert out.x.is_contiguous() and out.edge_index.is_contiguous()


def test_max_pool_small_cases():
    from torch_geometric.nn import max_pool
    from torch_geometric.transforms import Cartesian
    cluster, x, pos, batch, ei, attr = _graph_case(3, "vec", seed=5)
    none = torch.empty((2, 0), dtype=torch.int64)
    # E = 0
    out = max_pool(cluster.to(DEV), _data(x, pos, batch, none, None))
    ref = _ref(cluster, x, pos, batch, none, None)
    assert tuple(out.edge_index.shape) == (2, 0) and out.edge_attr is None and torch.equal(out.x.cpu(), ref["x"])
    out = max_pool(cluster.to(DEV), _data(x, pos, batch, none, torch.empty(0, 2)))
    assert tuple(out.edge_attr.shape) == (0, 2)
    # every edge collapses to a loop (E' = 0): one cluster per graph
    out = max_pool(batch.to(DEV), _data(x, pos, batch, ei, attr))
    ref = _ref(batch, x, pos, batch, ei, attr)
    assert tuple(out.edge_index.shape) == (2, 0) and tuple(out.edge_attr.shape) == (0,)
    assert torch.equal(out.x.cpu(), ref["x"]) and torch.equal(out.batch.cpu(), ref["batch"])
    assert out.batch.tolist() == GRAPH_IDS
    # data.batch = None; 1-D x
    d = _data(x[:, 0].contiguous(), pos, None, ei, attr)
    out = max_pool(cluster.to(DEV), d)
    ref = _ref(cluster, x[:, 0].contiguous(), pos, None, ei, attr)
    assert out.batch is None and out.x.dim() == 1 and torch.equal(out.x.cpu(), ref["x"])
    assert torch.equal(out.edge_index.cpu(), ref["edge_index"]) and torch.equal(out.edge_attr.cpu(), ref["edge_attr"])
    # the transform runs on the pooled graph
    out = max_pool(cluster.to(DEV), _data(x, pos, batch, ei, None), transform=Cartesian(cat=False))
    assert tuple(out.edge_attr.shape) == (out.edge_index.size(1), 2)
    assert float(out.edge_attr.min()) >= 0.0 and float(out.edge_attr.max()) <= 1.0
    # an edge end >= n
    bad = ei.clone()
    bad[1, 7] = x.size(0)
    with pytest.raises(IndexError):
        max_pool(cluster.to(DEV), _data(x, pos, batch, bad, None))
    bad[1, 7] = -1
    with pytest.raises(IndexError):
        max_pool(cluster.to(DEV), _data(x, pos, batch, bad, attr))
    with pytest.raises(TypeError, match="float32"):
        max_pool(cluster.to(DEV), _data(x, pos, batch, ei, attr.double()))


def test_pool_helpers():
    from torch_geometric.nn import consecutive_cluster, pool_batch, pool_edge, pool_pos
    cluster, x, pos, batch, ei, attr = _graph_case(3, "mat", seed=9)
    ref = _ref(cluster, x, pos, batch, ei, attr)
    inv, perm = consecutive_cluster(cluster.to(DEV))
    index, a = pool_edge(inv, ei.to(DEV), attr.to(DEV))
    assert torch.equal(index.cpu(), ref["edge_index"]) and torch.equal(a.cpu(), ref["edge_attr"])
    index, a = pool_edge(inv, ei.to(DEV))
    assert torch.equal(index.cpu(), ref["edge_index"]) and a is None
    assert torch.equal(pool_batch(perm, batch.to(DEV)).cpu(), ref["batch"])
    M = ref["perm"].numel()
    p64 = R.pool_f64(None, pos.double(), None, ref["inv"], None, None, M, 0, "mean")[1]
    _assert_bound(pool_pos(inv, pos.to(DEV)), p64, _mean_scale(pos, ref["inv"], M), "pool_pos")


# ---- max_pool_x / avg_pool -------------------------------------------------------------

def _last_stage(F=64, graphs=6, seed=2):
    """The example's last stage: a few nodes per graph on [0, 28)^2 under 14-wide
    voxels (size=4 slots per graph, some of them empty)."""
    g = torch.Generator().manual_seed(seed)
    sizes = [1, 2, 3, 5, 7, 9][:graphs]
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)])
    pos = torch.rand(sum(sizes), 2, generator=g) * 27.9
    x = torch.randint(-2, 3, (sum(sizes), F), generator=g).float() * 0.5
    x[torch.rand(x.shape, generator=g) < 0.1] = -20000.0
    return x, pos, batch


def test_max_pool_x():
    from torch_geometric.nn import max_pool_x, voxel_grid
    x, pos, batch = _last_stage()
    G = int(batch.max()) + 1
    cluster = voxel_grid(pos.to(DEV), batch.to(DEV), 14, 0, 27.99)
    assert torch.equal(cluster.cpu(), R.voxel_grid(pos, batch, 14, 0, 27.99))
    out, b = max_pool_x(cluster, x.to(DEV), batch.to(DEV), size=4)
    want = R.pool_x_sized(cluster.cpu(), x, batch, 4)
    assert b is None and tuple(out.shape) == (G * 4, x.size(1)) and torch.equal(out.cpu(), want)
    assert cluster.unique().numel() < G * 4 and bool((want == 0).all(dim=1).any())       # empty voxels: zero rows
    out, b = max_pool_x(cluster, x.to(DEV), batch.to(DEV))
    ref = R.pool(cluster.cpu(), x, None, batch, torch.empty((2, 0), dtype=torch.int64), None)
    assert torch.equal(out.cpu(), ref["x"]) and torch.equal(b.cpu(), ref["batch"])
    bad = cluster.clone()
    bad[3] = G * 4
    with pytest.raises(IndexError):
        max_pool_x(bad, x.to(DEV), batch.to(DEV), size=4)
    bad[3] = -1
    with pytest.raises(IndexError):
        max_pool_x(bad, x.to(DEV), batch.to(DEV), size=4)


def test_avg_pool_and_avg_pool_x():
    from torch_geometric.nn import avg_pool, avg_pool_x
    cluster, x, pos, batch, ei, attr = _graph_case(33, "mat", seed=4)
    x = x.clamp(min=-2)
    ref = _ref(cluster, x, pos, batch, ei, attr, "mean")
    out = avg_pool(cluster.to(DEV), _data(x, pos, batch, ei, attr))
    got = {"inv": torch.unique(cluster, return_inverse=True)[1], "perm": ref["perm"], "x": out.x, "pos": out.pos,
           "batch": out.batch, "edge_index": out.edge_index, "edge_attr": out.edge_attr}
    _check_stage(got, ref, x, pos, attr, "mean")
    M = ref["perm"].numel()
    o, b = avg_pool_x(cluster.to(DEV), x.to(DEV), batch.to(DEV))
    r64 = R.pool_f64(x.double(), None, None, ref["inv"], None, None, M, 0, "mean")[0]
    _assert_bound(o, r64, _mean_scale(x, ref["inv"], M), "avg_pool_x")
    assert torch.equal(b.cpu(), ref["batch"])
    xs, ps, bs = _last_stage(F=5)
    cl = R.voxel_grid(ps, bs, 14, 0, 27.99)
    xs = xs.clamp(min=-2)
    o, b = avg_pool_x(cl.to(DEV), xs.to(DEV), bs.to(DEV), size=4)
    rows = (int(bs.max()) + 1) * 4
    cnt = torch.bincount(cl, minlength=rows).clamp(min=1).double().view(-1, 1)
    r64 = torch.zeros((rows, 5), dtype=torch.float64).index_add_(0, cl, xs.double()) / cnt
    sc = torch.zeros((rows, 5), dtype=torch.float64).index_add_(0, cl, xs.double().abs()) / cnt
    assert b is None
    _assert_bound(o, r64, sc, "avg_pool_x(size=4)")


# ---- gradients ---------------------------------------------------------------------------

@pytest.mark.parametrize("reduce,F,attr_mode", [("max", 33, "mat"), ("max", 3, "vec"), ("mean", 64, "vec")])
def test_gradients_against_float64(reduce, F, attr_mode):
    """d x (through the max: routed to arg, exact; through the mean), d pos and d
    edge_attr (through the coalesce) against the float64 restatement run with the
    device's inv / arg / edge_slot.  sum |terms| of a gradient entry = the same
    computation on absolute values."""
    from torch_geometric.nn import avg_pool, max_pool
    cluster, x, pos, batch, ei, attr = _graph_case(F, attr_mode, seed=20 + F)
    ref = _ref(cluster, x, pos, batch, ei, attr, reduce)
    M, Ep = ref["perm"].numel(), ref["edge_index"].size(1)
    g = torch.Generator().manual_seed(1)
    wx = torch.randn(M, F, generator=g)
    wp = torch.randn(M, 2, generator=g)
    wa = torch.randn((Ep,) + tuple(attr.shape[1:]), generator=g)
    d = _data(x, pos, batch, ei, attr)
    for t in (d.x, d.pos, d.edge_attr):
        t.requires_grad_(True)
    out = (max_pool if reduce == "max" else avg_pool)(cluster.to(DEV), d)
    if reduce == "max":
        assert torch.equal(out.x.detach().cpu(), ref["x"])
    loss = (out.x * wx.to(DEV)).sum() + (out.pos * wp.to(DEV)).sum() + (out.edge_attr * wa.to(DEV)).sum()
    loss.backward()

    def f64(xv, pv, av, ws):
        xo, po, ao = R.pool_f64(xv, pv, av, ref["inv"], ref["arg"], ref["edge_slot"], M, Ep, reduce)
        return (xo * ws[0]).sum() + (po * ws[1]).sum() + (ao * ws[2]).sum()

    leaves = [t.double().requires_grad_(True) for t in (x, pos, attr)]
    f64(*leaves, [wx.double(), wp.double(), wa.double()]).backward()
    scales = [t.double().requires_grad_(True) for t in (x, pos, attr)]
    f64(*scales, [wx.double().abs(), wp.double().abs(), wa.double().abs()]).backward()
    for name, got, want, sc in zip(("d x", "d pos", "d edge_attr"), (d.x.grad, d.pos.grad, d.edge_attr.grad),
                                   leaves, scales):
        assert got is not None and tuple(got.shape) == tuple(want.shape)
        _assert_bound(got, want.grad, sc.grad.abs(), "%s (%s)" % (name, reduce))
    if reduce == "max":
        assert torch.equal(d.x.grad.cpu().double(), leaves[0].grad)                  # a routing: exact
    assert torch.equal(d.edge_attr.grad.cpu().double(), leaves[2].grad)              # a gather: exact


# ---- determinism, launch shapes, the example ----------------------------------------------

def test_two_runs_are_bitwise_equal():
    cluster, x, pos, batch, ei, attr = _graph_case(33, "mat", seed=6)
    for reduce in ("max", "mean"):
        a = _selection(cluster, x, pos, batch, ei, attr, reduce)
        b = _selection(cluster, x, pos, batch, ei, attr, reduce)
        for k in a:
            if a[k] is not None:
                assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                   b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), (reduce, k)


def test_launch_shape_past_the_grid_cap():
    """More clusters and more output edges than one sweep of the capped grids covers:
    the row kernels stride over their rows from at most mp_cluster_max_blocks()
    workgroups of four waves (16 clusters per wave at F = 4, 64 output edges per wave
    for a one-column edge_attr)."""
    from mi355_mp import _lib
    cap = int(_lib.load().mp_cluster_max_blocks())
    M = cap * 4 * 16 + 4000
    n = M + 5000
    E = cap * 4 * 64 + 80000
    g = torch.Generator().manual_seed(0)
    cluster = torch.cat([torch.arange(M), torch.randint(0, M, (n - M,), generator=g)]) * 3 - 7
    cluster = cluster[torch.randperm(n, generator=g)]
    x = torch.randint(-2, 3, (n, 4), generator=g).float()
    pos = torch.rand(n, 2, generator=g)
    batch = torch.zeros(n, dtype=torch.int64)
    ei = torch.randint(0, n, (2, E), generator=g)
    attr = torch.rand(E, generator=g)
    ref = _ref(cluster, x, pos, batch, ei, attr)
    assert ref["perm"].numel() == M > cap * 4 * 16 and ref["edge_index"].size(1) > cap * 4 * 64
    got = _selection(cluster, x, pos, batch, ei, attr)
    _check_stage(got, ref, x, pos, attr)


def _example():
    spec = importlib.util.spec_from_file_location("mnist_voxel_grid", os.path.join(ROOT, "examples",
                                                                                   "mnist_voxel_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_trains():
    from torch_geometric.data import Batch
    mod = _example()
    losses = mod.main(["--epochs", "1", "--graphs", "128"])
    assert len(losses) == 2 and all(torch.isfinite(torch.tensor(losses)))
    torch.manual_seed(0)
    net = mod.Net().to(DEV).eval()
    data = Batch.from_data_list(mod.superpixel_graphs(64, 3)).to(DEV)
    out = net(data)
    assert tuple(out.shape) == (64, 10) and bool(torch.isfinite(out).all())
