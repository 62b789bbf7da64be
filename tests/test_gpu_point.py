"""GPU tests of fps, radius, radius_graph, the edge-feature kernel and PointConv
(csrc/mp_point.hip) against the numpy restatement tests/_point_ref.py.

Indices are integers and the edge features are single fp32 operations, so they
must equal the restatement exactly, everywhere.  Gradients are sums: they are
compared with float64 under the project's bound |err| <= 1e-5 * sum |terms|, the
sums of magnitudes written out next to each use.

Shapes.  fps takes one of three paths by graph size (ops.fps_path): the batches
hold graphs of 1, 2, 63, 64, 65, 130, 257 and 1025 points, and one graph just
below and one just above every threshold the library reports; the largest ones run
at a ratio that gives about a thousand steps.  radius has one kernel whose
workgroup of four queries either stages candidates through LDS (the four search
the same rows) or reads them directly (they do not): graphs with fewer than four
queries, and queries of a graph that x lacks, give both, and caps of 1, 3, 64 and
200 stop a wave inside a tile, at its end and past a wave's width.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _point_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOUND = 1e-5
SIZES = [1, 2, 63, 64, 65, 130, 257, 1025]
Y_SIZES = [1, 1, 5, 7, 3, 11, 13, 17]


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _batch(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def _cloud(n, D, kind, rng):
    if kind == "random":
        return (rng.random((n, D)) * 2 - 1).astype(np.float32)
    if kind == "lattice":                                # many equal distances
        return rng.integers(0, 8, (n, D)).astype(np.float32)
    assert kind == "duplicates"                          # at most 2^D distinct points
    return rng.integers(0, 2, (n, D)).astype(np.float32)


_REF = {}


def _ref(key, make):
    """Every reference is computed once and shared between the tests that need it."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _thresholds():
    from mi355_mp import ops
    paths = [ops.fps_path(n) for n in range(1, 20001)]
    return [n for n, (a, b) in enumerate(zip(paths, paths[1:]), start=1) if a != b]


def _fps(pos, batch, ratio, start=None):
    from mi355_mp import ops
    out = ops.fps(_dev(pos), _dev(batch), ratio, _dev(start))
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and out.dim() == 1
    return out.cpu().numpy()


# ---- fps -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ratio", [("random", 1.0), ("random", 0.5), ("random", 0.25), ("random", 1e-3),
                                        ("lattice", 1.0), ("lattice", 0.5), ("lattice", 0.25), ("lattice", 1e-3),
                                        ("duplicates", 1.0)])
def test_fps_is_the_restatement(kind, ratio):
    pos = _ref(("cloud", kind), lambda: _cloud(sum(SIZES), 3, kind, np.random.default_rng(11)))
    batch = _batch(SIZES)
    want = _ref(("fps", kind, ratio), lambda: R.fps(pos, batch, ratio))
    got = _fps(pos, batch, ratio)
    assert np.array_equal(got, want), "%d of %d selections differ" % (int((got != want).sum()), len(want))
    if ratio == 1e-3:
        starts = np.concatenate([[0], np.cumsum(SIZES)])
        assert got.tolist() == starts[:-1].tolist() + [starts[-2] + int(np.argmax(R.d2(pos[starts[-2]:], pos[starts[-2]])))]
    if kind == "duplicates":
        assert len(set(got.tolist())) < len(got)          # points are selected twice


@pytest.mark.parametrize("kind", ["random", "lattice"])
def test_fps_on_both_sides_of_every_threshold(kind):
    from mi355_mp import ops
    ts = _thresholds()
    assert len(ts) == 2 and [ops.fps_path(t) for t in ts] == [0, 1] and [ops.fps_path(t + 1) for t in ts] == [1, 2]
    sizes = [s for t in ts for s in (t, t + 1)]
    ratio = 1024.5 / (ts[-1] + 1)                        # about a thousand steps in the largest graph
    pos = _ref(("tcloud", kind), lambda: _cloud(sum(sizes), 3, kind, np.random.default_rng(12)))
    batch = _batch(sizes)
    want = _ref(("tfps", kind), lambda: R.fps(pos, batch, ratio))
    assert 1000 <= R.keep_count(ratio, sizes[-1]) <= 1100
    got = _fps(pos, batch, ratio)
    assert np.array_equal(got, want), "%d of %d selections differ" % (int((got != want).sum()), len(want))


def test_fps_from_given_starts():
    pos = _ref(("cloud", "lattice"), lambda: _cloud(sum(SIZES), 3, "lattice", np.random.default_rng(11)))
    batch = _batch(SIZES)
    start = np.asarray([0, 1, 62, 0, 64, 77, 256, 1024], dtype=np.int64)        # the last point of five graphs
    want = R.fps(pos, batch, 0.5, start)
    got = _fps(pos, batch, 0.5, start)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, _ref(("fps", "lattice", 0.5), lambda: R.fps(pos, batch, 0.5)))


def test_fps_random_start_draws_inside_every_graph():
    from torch_geometric.nn import fps
    pos = _ref(("cloud", "random"), lambda: _cloud(sum(SIZES), 3, "random", np.random.default_rng(11)))
    batch = _batch(SIZES)
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    torch.manual_seed(5)
    seen = set()
    for _ in range(3):
        got = fps(_dev(pos), _dev(batch), ratio=0.25).cpu().numpy()
        ks = [R.keep_count(0.25, s) for s in SIZES]
        assert len(got) == sum(ks)
        firsts, o = [], 0
        for g, k in enumerate(ks):
            seg = got[o:o + k]
            assert ((seg >= starts[g]) & (seg < starts[g + 1])).all()
            firsts.append(int(seg[0] - starts[g]))
            o += k
        assert np.array_equal(got, R.fps(pos, batch, 0.25, firsts))
        seen.add(tuple(firsts))
    assert len(seen) > 1                                  # the draws differ between calls


@pytest.mark.parametrize("D", [1, 2, 8])
def test_fps_widths_and_a_row_stride(D):
    rng = np.random.default_rng(13)
    sizes = [5, 64, 300]
    wide = _cloud(sum(sizes), D + 3, "lattice", rng)
    pos = wide[:, 2:2 + D]
    batch = _batch(sizes)
    want = R.fps(pos, batch, 0.5)
    from mi355_mp import ops
    strided = _dev(wide)[:, 2:2 + D]
    assert D == 1 or not strided.is_contiguous()
    got = ops.fps(strided, _dev(batch), 0.5).cpu().numpy()
    assert np.array_equal(got, want)
    if D == 1:                                            # a vector of coordinates is a cloud of width 1
        assert np.array_equal(ops.fps(_dev(np.ascontiguousarray(pos[:, 0])), _dev(batch), 0.5).cpu().numpy(), want)


def test_known_answers():
    from torch_geometric.nn import fps, radius, radius_graph
    from mi355_mp import ops
    kat = np.load(os.path.join(ROOT, "tests", "golden", "point", "point_kat.npz"))
    pos, y, feat, batch, batch_y, start = (_dev(kat[k]) for k in ("pos", "y", "feat", "batch", "batch_y", "start"))
    for name, ratio in (("half", 0.5), ("all", 1.0)):
        assert np.array_equal(fps(pos, batch, ratio, random_start=False).cpu().numpy(), kat["fps_%s" % name])
        assert np.array_equal(ops.fps(pos, batch, ratio, start).cpu().numpy(), kat["fps_%s_start" % name])
    from tests.golden import make_golden_point as G
    for cap in (2, 32):
        assert np.array_equal(radius(pos, y, G.RADIUS, batch, batch_y, cap).cpu().numpy(), kat["radius_cap%d" % cap])
    assert np.array_equal(radius_graph(pos, G.RADIUS, batch, False, 3).cpu().numpy(), kat["radius_graph"])
    assert np.array_equal(radius_graph(pos, G.RADIUS, batch, True, 3, "target_to_source").cpu().numpy(),
                          kat["radius_graph_loop_t2s"])
    row, col = _dev(kat["radius_cap32"])
    assert np.array_equal(ops.point_edge_features(feat, pos, y, col, row).cpu().numpy(), kat["edge_features"])
    assert np.array_equal(ops.point_edge_features(None, pos, y, col, row).cpu().numpy(), kat["edge_features_pos_only"])


# ---- radius --------------------------------------------------------------------------------------

def _radius_case(D):
    """x: the graphs of SIZES (graph 2 left out of x), y: fewer points per graph (graph 5
    left out of y, and two queries of a graph past the last of x).  Lattice coordinates
    put points exactly on the boundary; a few queries lie far from everything."""
    def make():
        rng = np.random.default_rng(20 + D)
        xs = list(SIZES)
        ys = list(Y_SIZES) + [2]
        xs[2], ys[5] = 0, 0
        kind, r = ("duplicates", 2.0) if D == 8 else ("lattice", 3.0)
        x = _cloud(sum(xs), D, kind, rng)
        y = _cloud(sum(ys), D, kind, rng)
        y[::7] += 100                                    # these find nothing
        return x, y, _batch(xs), _batch(ys), r
    return _ref(("radius_case", D), make)


@pytest.mark.parametrize("cap", [1, 3, 64, 200])
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_radius_is_the_restatement(D, cap):
    from torch_geometric.nn import radius
    x, y, bx, by, r = _radius_case(D)
    want = _ref(("radius", D, cap), lambda: R.radius(x, y, r, bx, by, cap))
    got = radius(_dev(x), _dev(y), r, _dev(bx), _dev(by), max_num_neighbors=cap)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # what the case is for: queries at the cap, queries with nothing, a point exactly on the boundary
    per_query = np.bincount(want[0], minlength=len(y))
    assert per_query.min() == 0 and per_query[by == 2].sum() == 0 and per_query[by == len(SIZES)].sum() == 0
    if cap <= 64:
        assert per_query.max() == cap
    elif D <= 3:
        assert per_query.max() > 64                      # more than a wave's width of hits
    r2 = np.float32(r) * np.float32(r)
    assert any((R.d2(x[bx == by[j]], y[j]) == r2).any() for j in range(len(y)))


def test_radius_on_random_clouds_a_row_stride_and_no_batch():
    from torch_geometric.nn import radius
    rng = np.random.default_rng(30)
    wide_x = (rng.random((1500, 6)) * 2 - 1).astype(np.float32)
    wide_y = (rng.random((333, 5)) * 2 - 1).astype(np.float32)
    x, y = wide_x[:, 2:5], wide_y[:, 1:4]
    want = R.radius(x, y, 0.35, None, None, 32)
    xs, ys = _dev(wide_x)[:, 2:5], _dev(wide_y)[:, 1:4]
    assert not xs.is_contiguous() and not ys.is_contiguous()
    got = radius(xs, ys, 0.35).cpu().numpy()
    assert np.array_equal(got, want)
    per_query = np.bincount(want[0], minlength=333)
    assert per_query.max() == 32 and per_query.min() < 32
    # sorted by y, then x
    assert (np.diff(got[0]) >= 0).all() and (np.diff(got[1])[np.diff(got[0]) == 0] > 0).all()
    # r = 0 finds the coinciding points only
    same = radius(xs, xs[:10].contiguous(), 0.0).cpu().numpy()
    assert same.tolist() == [list(range(10)), list(range(10))]


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_radius_graph_is_the_restatement(loop, flow):
    from torch_geometric.nn import radius_graph
    sizes = [1, 2, 65, 300]
    x = _ref("rg_cloud", lambda: _cloud(sum(sizes), 3, "lattice", np.random.default_rng(40)))
    batch = _batch(sizes)
    want = R.radius_graph(x, 1.5, batch, loop, 4, flow)
    got = radius_graph(_dev(x), 1.5, _dev(batch), loop, 4, flow).cpu().numpy()
    assert np.array_equal(got, want)
    target = want[1] if flow == "source_to_target" else want[0]
    most = np.bincount(target).max()
    assert most == (4 if loop else 5)                     # upstream's quirk: a node may keep max_num_neighbors + 1


# ---- edge features -------------------------------------------------------------------------------

def _edge_case(F, D, shuffled):
    rng = np.random.default_rng(50 + F + D)
    n_src, n_dst, E = 300, 70, 2000
    x = None if F == 0 else rng.standard_normal((n_src, F + 3)).astype(np.float32)
    ps = rng.standard_normal((n_src, D)).astype(np.float32)
    pd = rng.standard_normal((n_dst, D)).astype(np.float32)
    src = rng.integers(0, n_src, E)
    dst = np.sort(rng.integers(0, n_dst - 1, E))          # the last target has no edge
    if shuffled:
        p = rng.permutation(E)
        src, dst = src[p], dst[p]
    return x, ps, pd, src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("F,D", [(0, 3), (5, 3), (128, 3), (4, 4), (13, 3), (64, 8), (3, 1)])
def test_edge_features_forward_and_gradients(F, D, shuffled):
    from mi355_mp import ops
    x, ps, pd, src, dst = _edge_case(F, D, shuffled)
    xs = None if x is None else x[:, :F]                  # a column slice: rows with a stride
    want = R.edge_features(xs, ps, pd, src, dst)
    xd = None if x is None else _dev(x)[:, :F].requires_grad_(True)
    psd, pdd = _dev(ps).requires_grad_(True), _dev(pd).requires_grad_(True)
    out = ops.point_edge_features(xd, psd, pdd, _dev(src), _dev(dst))
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(src), F + D)
    assert np.array_equal(out.detach().cpu().numpy(), want)
    # gradients of sum(out * w): g_x[s] = sum_{e: src = s} w[e, :F], g_pos_src[s] = sum w[e, F:],
    # g_pos_dst[t] = -sum_{e: dst = t} w[e, F:]; sum |terms| = the same sums over |w|
    w = torch.from_numpy(np.random.default_rng(3).standard_normal(want.shape)).double()
    (out * w.float().to(DEV)).sum().backward()
    s, t = torch.from_numpy(src), torch.from_numpy(dst)
    w32 = w.float().double()
    for got, index, n, cols, sign in ((None if xd is None else xd.grad, s, len(ps), slice(0, F), 1.0),
                                      (psd.grad, s, len(ps), slice(F, F + D), 1.0),
                                      (pdd.grad, t, len(pd), slice(F, F + D), -1.0)):
        if got is None:
            continue
        ref = torch.zeros(n, w32[:, cols].shape[1], dtype=torch.float64).index_add_(0, index, w32[:, cols]) * sign
        terms = torch.zeros_like(ref).index_add_(0, index, w32[:, cols].abs())
        err = (got.cpu().double() - ref).abs()
        assert bool((err <= BOUND * terms).all()), float((err - BOUND * terms).max())
    assert bool((pdd.grad[-1] == 0).all())                # the target without an edge


def test_edge_features_reject_an_index_out_of_range():
    from mi355_mp import ops
    ps, pd = torch.rand(10, 3, device=DEV), torch.rand(4, 3, device=DEV)
    good = ops.point_edge_features(None, ps, pd, _dev(np.asarray([9])), _dev(np.asarray([3])))
    for src, dst in (([10], [0]), ([-1], [0]), ([0], [4])):
        with pytest.raises(IndexError):
            ops.point_edge_features(None, ps, pd, _dev(np.asarray(src)), _dev(np.asarray(dst)))
    again = ops.point_edge_features(None, ps, pd, _dev(np.asarray([9])), _dev(np.asarray([3])))
    assert torch.equal(good, again) and torch.equal(good[0], ps[9] - pd[3])


# ---- PointConv -----------------------------------------------------------------------------------

def _reference_layer():
    from torch_geometric.nn import PointConv

    class GenericPointConv(PointConv):
        """The same layer through MessagePassing's generic path: overriding message()
        is what turns the fused edge-feature kernel off."""

        def message(self, x_j, pos_i, pos_j):
            msg = pos_j - pos_i
            if x_j is not None:
                msg = torch.cat([x_j, msg], dim=1)
            self.feat = msg
            if msg.requires_grad:
                msg.retain_grad()
            return msg if self.local_nn is None else self.local_nn(msg)

    return GenericPointConv


class _LinearTerms(object):
    """sum |terms| of every Linear's weight and bias gradient (|g|^T |a| and sum |g|)
    and of its output (|a| |W|^T + |b|), recorded while the reference layer runs."""

    def __init__(self, module):
        self.grad, self.out = {}, {}
        for lin in (m for m in module.modules() if isinstance(m, torch.nn.Linear)):
            lin.register_forward_hook(self._forward(lin))

    def _forward(self, lin):
        def hook(mod, inputs, output):
            a = inputs[0].detach().double()
            self.out[lin] = a.abs() @ lin.weight.detach().double().abs().t() + lin.bias.detach().double().abs()

            def on_grad(g):
                g = g.detach().double()
                self.grad[lin.weight] = g.abs().t() @ a.abs()
                self.grad[lin.bias] = g.abs().sum(0)
            if output.requires_grad:
                output.register_hook(on_grad)
        return hook


def _within(got, ref, terms, what):
    err = (got.double() - ref.double()).abs()
    assert bool((err <= BOUND * terms).all()), "%s: %g over" % (what, float((err - BOUND * terms).max()))


@pytest.mark.parametrize("form", ["tuple", "tuple_no_x", "tensor", "tensor_no_x"])
def test_pointconv_agrees_with_the_generic_path(form):
    from torch_geometric.nn import PointConv
    rng = np.random.default_rng(60)
    n, m, F = 200, 40, 6
    pos = torch.from_numpy(_cloud(n, 3, "random", rng)).to(DEV)
    x = None if form.endswith("no_x") else torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32)).to(DEV)
    width = 3 + (0 if x is None else F)
    torch.manual_seed(0)
    local_nn = torch.nn.Sequential(torch.nn.Linear(width, 16), torch.nn.ReLU(), torch.nn.Linear(16, 8)).to(DEV)
    global_nn = torch.nn.Linear(8, 5).to(DEV)
    if form.startswith("tuple"):
        dst_pos = pos[:m].clone()
        src = torch.from_numpy(rng.integers(0, n, 600))
        dst = torch.from_numpy(np.sort(rng.integers(0, m - 1, 600)))      # target m - 1 has no neighbour
        edge_index = torch.stack([src, dst]).to(DEV)
    else:
        from torch_geometric.nn import radius_graph
        edge_index = radius_graph(pos, 0.4, None, loop=True, max_num_neighbors=8)   # its loops are removed, then added
        assert int((edge_index[0] == edge_index[1]).sum()) > 0

    def run(layer):
        leaves = [pos.clone().requires_grad_(True)]
        if form.startswith("tuple"):
            leaves.append(dst_pos.clone().requires_grad_(True))
        if x is not None:
            leaves.append(x.clone().requires_grad_(True))
        p = (leaves[0], leaves[1]) if form.startswith("tuple") else leaves[0]
        xin = None if x is None else ((leaves[-1], None) if form == "tuple" else leaves[-1])
        for q in layer.parameters():
            q.grad = None
        out = layer(xin, p, edge_index)
        out.square().sum().backward()
        return out.detach(), [t.grad for t in leaves], [q.grad.clone() for q in layer.parameters()]

    # both layers first: a constructor resets the networks the two share
    ref_layer, layer = _reference_layer()(local_nn, global_nn), PointConv(local_nn, global_nn)
    terms = _LinearTerms(ref_layer)
    ref_out, ref_leaves, ref_params = run(ref_layer)
    out, leaves, params = run(layer)
    assert tuple(out.shape) == ((m if form.startswith("tuple") else n), 5)
    _within(out, ref_out, terms.out[global_nn], "out")
    for q, got, ref in zip(ref_layer.parameters(), params, ref_params):
        _within(got, ref, terms.grad[q], "parameter gradient")
    # the leaves' gradients are sums of the per-edge gradient rows the reference kept
    g = ref_layer.feat.grad.double().abs()
    if form.startswith("tensor"):                         # the edge list the layer really used: loops re-added
        from torch_geometric.utils import remove_self_loops, add_self_loops
        used, _ = remove_self_loops(edge_index)
        used, _ = add_self_loops(used, num_nodes=n)
    else:
        used = edge_index
    assert used.shape[1] == g.shape[0]
    by_src = torch.zeros(n, g.shape[1], dtype=torch.float64, device=DEV).index_add_(0, used[0], g)
    n_dst = m if form.startswith("tuple") else n
    by_dst = torch.zeros(n_dst, g.shape[1], dtype=torch.float64, device=DEV).index_add_(0, used[1], g)
    if form.startswith("tuple"):
        _within(leaves[0], ref_leaves[0], by_src[:, -3:], "pos_src gradient")
        _within(leaves[1], ref_leaves[1], by_dst[:, -3:], "pos_dst gradient")
        assert bool((leaves[1][m - 1] == 0).all())
    else:
        _within(leaves[0], ref_leaves[0], by_src[:, -3:] + by_dst[:, -3:], "pos gradient")
    if x is not None:
        _within(leaves[-1], ref_leaves[-1], by_src[:, :F], "x gradient")


def test_pointconv_without_networks_is_exact_and_an_isolated_target_is_zero():
    from torch_geometric.nn import PointConv
    rng = np.random.default_rng(61)
    n, m = 50, 9
    pos, centre = torch.from_numpy(_cloud(n, 3, "random", rng)).to(DEV), torch.from_numpy(_cloud(m, 3, "random", rng)).to(DEV)
    x = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32)).to(DEV)
    src = torch.from_numpy(rng.integers(0, n, 100))
    dst = torch.from_numpy(rng.integers(0, m - 1, 100))                   # unsorted; target m - 1 has no neighbour
    edge_index = torch.stack([src, dst]).to(DEV)
    out = PointConv()(x, (pos, centre), edge_index)
    ref = _reference_layer()()(x, (pos, centre), edge_index)
    assert tuple(out.shape) == (m, 7) and torch.equal(out, ref)
    assert bool((out[m - 1] == 0).all())
    feat = R.edge_features(x.cpu().numpy(), pos.cpu().numpy(), centre.cpu().numpy(), src.numpy(), dst.numpy())
    want = np.zeros((m, 7), dtype=np.float32)
    for t in range(m - 1):
        want[t] = feat[dst.numpy() == t].max(0)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- errors --------------------------------------------------------------------------------------

def test_bad_arguments_raise_and_leave_the_device_healthy():
    from mi355_mp import ops
    from torch_geometric.nn import fps, radius, radius_graph
    pos = _dev(_cloud(40, 3, "lattice", np.random.default_rng(70)))
    y = pos[:7].contiguous()
    batch = _dev(_batch([15, 25]))
    by = _dev(np.asarray([0, 0, 0, 1, 1, 1, 1]))
    unsorted = batch.flip(0).contiguous()
    nine = torch.zeros(40, 9, device=DEV)
    good_fps = fps(pos, batch, 0.5, random_start=False)
    good_radius = radius(pos, y, 3.0, batch, by, 8)
    bad = [lambda: fps(pos, unsorted, 0.5),
           lambda: fps(nine, batch, 0.5),
           lambda: fps(pos, batch, 0.0),
           lambda: ops.fps(pos, batch, 0.5, _dev(np.asarray([15, 0]))),          # one past the last point
           lambda: ops.fps(pos, batch, 0.5, _dev(np.asarray([0, -1]))),
           lambda: radius(pos, y, 3.0, unsorted, by, 8),
           lambda: radius(pos, y, 3.0, batch, by.flip(0).contiguous(), 8),
           lambda: radius(nine, nine[:7], 3.0, batch, by, 8),
           lambda: radius(pos, y, -1.0, batch, by, 8),
           lambda: radius(pos, y, float("nan"), batch, by, 8),
           lambda: radius(pos, y, float("inf"), batch, by, 8),
           lambda: radius(pos, y, 3.0, batch, by, 0),
           lambda: radius(pos, y[:, :2], 3.0, batch, by, 8),
           lambda: radius_graph(pos, -1.0, batch)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
    assert torch.equal(fps(pos, batch, 0.5, random_start=False), good_fps)
    assert torch.equal(radius(pos, y, 3.0, batch, by, 8), good_radius)
    assert np.array_equal(good_fps.cpu().numpy(), R.fps(pos.cpu().numpy(), batch.cpu().numpy(), 0.5))
    assert np.array_equal(good_radius.cpu().numpy(),
                          R.radius(pos.cpu().numpy(), y.cpu().numpy(), 3.0, batch.cpu().numpy(), by.cpu().numpy(), 8))
    last = ops.fps(pos, batch, 0.5, _dev(np.asarray([14, 24])))                  # the last point of each graph is fine
    assert np.array_equal(last.cpu().numpy(), R.fps(pos.cpu().numpy(), batch.cpu().numpy(), 0.5, [14, 24]))


# ---- the example ---------------------------------------------------------------------------------

def test_example_pointnet_one_training_step():
    spec = importlib.util.spec_from_file_location("example_pointnet", os.path.join(ROOT, "examples", "pointnet++.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from torch_geometric.data import DataLoader
    torch.manual_seed(0)
    data = next(iter(DataLoader(mod.synthetic_clouds(2, 3), batch_size=2))).to(DEV)
    assert tuple(data.pos.shape) == (2048, 3) and float(data.pos.abs().max()) <= 1.0
    model = mod.Net().to(DEV).train()
    loss = torch.nn.functional.nll_loss(model(data), data.y)
    loss.backward()
    assert bool(torch.isfinite(loss))
    assert model.kept == (2 * 512, 2 * 128)
    for name, q in model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    assert sum(float(q.grad.abs().sum()) for q in model.sa1.parameters()) > 0    # the first stage learns too
