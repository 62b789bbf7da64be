"""CPU tests of the shared fuzz generators (tests/_fuzz_cases.py): every generator
kind is driven through the restatements alone (tests/_pool_ref.py,
tests/_cluster_ref.py, tests/_spline_ref.py), which shows without a GPU that the
references accept the edge cases the GPU fuzz tests feed them (empty graphs,
N = 1, E = 0, every edge a loop, int64 keys of either sign, no root / bias)
and agree with each other."""
import pytest
import torch

from tests import _cluster_ref as C, _fuzz_cases as Z, _pool_ref as P, _spline_ref as S
from tests.test_gpu_pool import RATIOS

SEEDS = range(6)


# ---- the generators themselves ---------------------------------------------------

@pytest.mark.parametrize("kind", Z.BATCH_KINDS)
def test_batch_sizes_stay_in_their_sets(kind):
    allowed = {"tiny": {0, 1, 2, 3}, "wave": {25, 63, 64}, "edge": {0, 1, 64, 65, 100, 101, 130},
               "random": set(range(1, 41))}[kind]
    lengths = set()
    for seed in range(40):
        sizes = Z.batch_sizes(kind, seed)
        assert 1 <= len(sizes) <= 12 and set(sizes) <= allowed and sum(sizes) >= 1
        capped = Z.batch_sizes(kind, seed, cap=250)
        assert capped == sizes[:len(capped)] and 1 <= sum(capped) and (sum(capped) <= 250 or len(capped) == 1)
        assert sizes == Z.batch_sizes(kind, seed)                     # a seed replays
        lengths.add(len(sizes))
    assert len(lengths) > 4
    assert Z.visible([0, 3, 0, 0]) == [0, 3] and Z.visible([0, 0]) == []


def test_scores_kinds():
    for n in (0, 1, 50):
        d = Z.scores("distinct", n, 1)
        assert d.dtype == torch.float32 and d.unique().numel() == n
        assert Z.scores("ties", n, 1).unique().numel() <= 4
        assert Z.scores("equal", n, 1).unique().numel() == min(n, 1)
        assert Z.scores("five", n, 1).shape == (n,)
    five = Z.scores("five", 400, 2)
    assert bool(torch.isnan(five).any()) and bool(torch.isinf(five).any()) and bool((five == 0).any())
    assert bool(torch.signbit(five[five == 0]).any()) and not bool(torch.signbit(five[five == 0]).all())


def test_pseudo_and_graph_recipes():
    u = Z.pseudo(100, 2, [5, 3], 0)
    assert float(u.min()) == 0.0 and float(u.max()) == 1.0 and u.shape == (100, 2)
    assert Z.pseudo(0, 3, [2, 2, 2], 0).shape == (0, 3)
    ei, _ = Z.graph(50, 6.0, 0.2, 3)
    assert ei.shape == (2, 300) and int((ei[0] == ei[1]).sum()) >= 40
    assert int(torch.bincount(ei[1], minlength=50).max()) >= 75                # the hub
    assert Z.graph(1, 0.0, 0.0, 0)[0].shape == (2, 0)


@pytest.mark.parametrize("kind", Z.CLUSTER_KINDS)
def test_cluster_kinds(kind):
    for seed in SEEDS:
        sizes = Z.batch_sizes("random", seed)
        batch = P.batch_of(sizes)
        n = batch.numel()
        cluster, pos, size = Z.clusters(kind, n, batch, seed)
        assert cluster.dtype == torch.int64 and cluster.shape == (n,) and pos.shape == (n, 2)
        assert float(pos.min()) >= 0.0 and float(pos.max()) < 28.0
        m = cluster.unique().numel()
        if kind == "one":
            assert m == 1
        elif kind == "each":
            assert m == n
        elif kind == "wide":
            assert m <= max(1, n // 3) and (n < 30 or (int(cluster.min()) < 0 < int(cluster.max())))
            assert n < 30 or int(cluster.abs().max()) > 1 << 40
        else:
            assert size in Z.VOXEL_SIZES and torch.equal(cluster, C.voxel_grid(pos, batch, size, 0, 28.0))
        inside = Z.cluster_edges("inside", n, cluster, seed)
        assert inside.shape[1] > 0 and torch.equal(cluster[inside[0]], cluster[inside[1]])
        assert Z.cluster_edges("none", n, cluster, seed).shape == (2, 0)
        assert Z.cluster_edges("pairs", n, cluster, seed).unique(dim=1).shape[1] <= 3
        rnd = Z.cluster_edges("random", n, cluster, seed)
        assert int((rnd[0] == rnd[1]).sum()) > 0 and rnd.unique(dim=1).shape[1] < rnd.shape[1]


# ---- TopKPooling: the two restatement forms agree ------------------------------------

@pytest.mark.parametrize("kind", Z.BATCH_KINDS)
def test_topk_stable_equals_dense_on_distinct_scores(kind):
    for seed in SEEDS:
        sizes = Z.batch_sizes(kind, seed)
        batch = P.batch_of(sizes)
        s = Z.scores("distinct", batch.numel(), seed)
        for ratio in RATIOS:
            perm, starts = P.topk_stable(s, ratio, sizes)
            assert torch.equal(P.topk_dense(s, ratio, batch), perm), (sizes, ratio)
            assert torch.equal(starts.diff(), P.keep_counts(ratio, sizes)) and int(starts[-1]) == perm.numel()
            # trailing empty graphs change nothing the batch vector can show
            seen = Z.visible(sizes)
            perm2, starts2 = P.topk_stable(s, ratio, seen)
            assert torch.equal(perm2, perm) and torch.equal(starts2, starts[:len(seen) + 1])


@pytest.mark.parametrize("kind", ["ties", "five", "equal"])
def test_topk_stable_tie_rule(kind):
    """Within a graph: descending, equal scores by ascending index; NaN first, -0.0 = +0.0."""
    sizes = [0, 5, 64, 0, 101]
    s = Z.scores(kind, sum(sizes), 4)
    perm, starts = P.topk_stable(s, 1.0, sizes)
    assert torch.equal(perm.sort()[0], torch.arange(sum(sizes)))

    def key(i):
        v = float(s[i])
        return (2, 0.0) if v != v else ((1, 0.0) if v == float("inf") else (0, v))

    for g in range(len(sizes)):
        p = perm[int(starts[g]):int(starts[g + 1])].tolist()
        for a, b in zip(p[:-1], p[1:]):
            assert key(a) > key(b) or (key(a) == key(b) and a < b), (kind, g, a, b)


# ---- cluster pooling: the float64 form reproduces the forward --------------------------

@pytest.mark.parametrize("edges", Z.CLUSTER_EDGE_KINDS)
@pytest.mark.parametrize("kind", Z.CLUSTER_KINDS)
def test_pool_f64_reproduces_pool(kind, edges):
    for seed, bkind in zip(SEEDS, ("tiny", "wave", "edge", "random", "tiny", "random")):
        sizes = Z.visible(Z.batch_sizes(bkind, seed, cap=250))
        batch = P.batch_of(sizes)
        n = batch.numel()
        cluster, pos, _ = Z.clusters(kind, n, batch, seed)
        ei = Z.cluster_edges(edges, n, cluster, seed)
        E = ei.shape[1]
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, 3, generator=g)
        x[torch.rand(n, 3, generator=g) < 0.1] = -20000.0
        for attr in (None, torch.rand(E, generator=g) - 0.3, torch.rand(E, 2, generator=g) - 0.3):
            a64 = None if attr is None else attr.double()
            p = C.pool(cluster, x, pos.double(), batch, ei, a64, "max")
            M, Ep = p["perm"].numel(), p["edge_index"].size(1)
            assert M == cluster.unique().numel() and tuple(p["x"].shape) == (M, 3)
            if edges in ("none", "inside") or kind == "one":
                assert Ep == 0
            if edges == "inside":
                assert E > 0 and bool((p["edge_slot"] == -1).all())
            xo, po, ao = C.pool_f64(x.double(), pos.double(), a64, p["inv"], p["arg"], p["edge_slot"], M, Ep, "max")
            assert torch.equal(xo, p["x"].double())                                 # the max is exact
            assert float((po - p["pos"]).abs().max()) <= 1e-12
            if attr is None:
                assert ao is None and p["edge_attr"] is None
            else:
                assert tuple(ao.shape) == tuple(p["edge_attr"].shape) == (Ep,) + tuple(attr.shape[1:])
                assert Ep == 0 or float((ao - p["edge_attr"]).abs().max()) <= 1e-12
            q = C.pool(cluster, x.clamp(min=-2).double(), pos.double(), batch, ei, a64, "mean")
            xm = C.pool_f64(x.clamp(min=-2).double(), None, None, q["inv"], None, None, M, 0, "mean")[0]
            assert float((xm - q["x"]).abs().max()) <= 1e-12
            assert torch.equal(q["edge_index"], p["edge_index"]) and torch.equal(q["batch"], batch[p["perm"]])


def test_pool_x_sized_on_relabelled_voxels():
    sizes = [3, 0, 40, 7]
    batch = P.batch_of(sizes)
    cluster, pos, _ = Z.clusters("voxel", batch.numel(), batch, 5)
    x = torch.randn(batch.numel(), 4, generator=torch.Generator().manual_seed(0))
    size = 9
    local = torch.unique(cluster, return_inverse=True)[1] % size + batch * size
    out = C.pool_x_sized(local, x, batch, size)
    assert tuple(out.shape) == (len(sizes) * size, 4)
    assert bool((out[size:2 * size] == 0).all())                      # the empty graph's rows


# ---- SplineConv: the restatement at the edges ------------------------------------------

@pytest.mark.parametrize("N,deg,loops", [(1, 0.0, 0.0), (1, 3.0, 1.0), (5, 0.0, 0.0), (40, 0.2, 0.0), (30, 5.0, 0.2)])
@pytest.mark.parametrize("root,bias", [(True, True), (False, False), (True, False)])
def test_spline_restatement_at_the_edges(N, deg, loops, root, bias):
    ei, g = Z.graph(N, deg, loops, 3)
    E = ei.shape[1]
    ks, op, M, f_in, f_out = [3, 2], [1, 0], 1, 3, 4
    u = Z.pseudo(E, 2, ks, 1)
    x = torch.randn(N, f_in, generator=g)
    w = torch.randn(6, f_in, f_out, generator=g)
    r = torch.randn(f_in, f_out, generator=g) if root else None
    b = torch.randn(f_out, generator=g) if bias else None
    for aggr in ("mean", "add"):
        for flow in ("source_to_target", "target_to_source"):
            out = S.spline_conv(x, ei, u, w, r, b, ks, op, M, aggr, flow)
            assert tuple(out.shape) == (N, f_out) and out.dtype == torch.float64
            want = torch.zeros(N, f_out, dtype=torch.float64)
            if root:
                want = want + x.double() @ r.double()
            if bias:
                want = want + b.double()
            if E == 0:
                assert torch.equal(out, want)
            scale = S.spline_conv(x, ei, u, w, r, b, ks, op, M, aggr, flow, absolute=True)
            assert bool((scale >= out.abs() - 1e-12).all())
            gout = torch.randn(N, f_out, generator=g)
            sc = S.abs_grad_scale(w, r, b, x, ei, u, ks, op, M, aggr, gout, flow)
            assert set(sc) == {"x", "weight"} | ({"root"} if root else set()) | ({"bias"} if bias else set())
            assert sc["x"].shape == x.shape and sc["weight"].shape == w.shape
    if N == 1 and E:
        # only self loops: the one node aggregates its own row through every edge
        bs, wi = S.basis(u, ks, op, M)
        msg = sum((bs[:, s:s + 1] * torch.einsum("f,efo->eo", x[0].double(), w.double()[wi[:, s]])) for s in range(4))
        want = msg.mean(0, keepdim=True) + (x.double() @ r.double() if root else 0) + (b.double() if bias else 0)
        got = S.spline_conv(x, ei, u, w, r, b, ks, op, M, "mean")
        assert float((got - want).abs().max()) <= 1e-12


# ---- NNConv / RGCNConv: the generators, and the restatements on the pinned examples ------------

from tests import _nnconv_ref as NR, _rgcn_ref as RR  # noqa: E402

F64_BOUND = 1e-12          # float64 restatements against each other: 1e-12 * sum |terms|


def _close64(a, b, scale, what):
    assert tuple(a.shape) == tuple(b.shape) == tuple(scale.shape), what
    if a.numel():
        excess = float(((a - b).abs() - F64_BOUND * scale).max())
        assert excess <= 0.0, "%s: exceeds 1e-12 * sum|terms| by %.3g" % (what, excess)


@pytest.mark.parametrize("kind", Z.RELATION_KINDS)
def test_relation_kinds(kind):
    for E, n_rel in ((0, 1), (0, 7), (1, 1), (5, 2), (300, 1), (300, 2), (300, 3), (300, 7), (640, 30)):
        for seed in SEEDS:
            et = Z.relations(kind, E, n_rel, seed)
            assert et.dtype == torch.int64 and tuple(et.shape) == (E,)
            assert torch.equal(et, Z.relations(kind, E, n_rel, seed))              # a seed replays
            if not E:
                continue
            assert 0 <= int(et.min()) and int(et.max()) < n_rel
            count = torch.bincount(et, minlength=n_rel)
            if kind == "one":
                assert int(count.max()) == E and (n_rel == 1 or int(count[0]) == 0)
            if kind == "skewed" and n_rel > 2:
                assert int(count[1]) == 0                                           # an empty relation
                if E >= 300:
                    assert int(count[0]) == int(count.max()) and int((count > 0).sum()) >= min(n_rel - 1, 5)
            if kind == "uniform" and E >= 300 and n_rel <= 7:
                assert int(count.min()) > 0
    assert len({int(Z.relations("one", 4, 7, seed)[0]) for seed in range(12)}) == 6   # every relation but 0


def test_edge_norm_and_edge_attr_kinds():
    assert Z.NORM_KINDS == (None, "rand", "signed") and Z.edge_norm(None, 9, 1) is None
    for E in (0, 1, 2, 50):
        for seed in SEEDS:
            r, s = Z.edge_norm("rand", E, seed), Z.edge_norm("signed", E, seed)
            assert r.dtype == s.dtype == torch.float32 and tuple(r.shape) == tuple(s.shape) == (E,)
            assert torch.equal(r, Z.edge_norm("rand", E, seed)) and torch.equal(s, Z.edge_norm("signed", E, seed))
            if E:
                assert 0.5 <= float(r.min()) and float(r.max()) < 1.5 and float(s[0]) == 0.0
            if E == 50:
                assert int((s == 0).sum()) >= 17 and int((s == 1).sum()) >= 17 and int((s < 0).sum()) >= 8
                assert int(((s > 0) & (s < 1)).sum()) > 0
            for D in (1, 3):
                u = Z.edge_attr(E, D, seed)
                assert u.dtype == torch.float32 and tuple(u.shape) == (E, D) and torch.equal(u, Z.edge_attr(E, D, seed))
                if E:
                    assert 0.0 <= float(u.min()) and float(u.max()) <= 1.0 and float(u[0].abs().max()) == 0.0
                if E == 50:
                    assert bool((u == 1).all(1).any()) and bool((u == 0).all(1).any())


def test_pinned_conv_examples_are_what_their_comments_say():
    from tests import _conv_lane_cases as K
    nn = [(p, Z.nnconv_inputs(p)) for p in Z.NNCONV_PINNED]
    rg = [(p, Z.rgcn_inputs(p)) for p in Z.RGCN_PINNED]
    for p, (ei, x, ea) in nn:
        E = ei.shape[1]
        assert tuple(x.shape) == (p["N"], p["c_in"]) and ea.shape[0] == E == int(p["N"] * p["deg"])
        assert ea.shape[1] == (p["H"] if p["nn"] == "linear" else p["D"])
        if p["loops"] == 1.0:
            assert bool((ei[0] == ei[1]).all())
    for p, (ei, x, et, en) in rg:
        assert et.shape[0] == ei.shape[1] and (x is None) == (p["mode"] == "featureless")
        assert (en is None) == (p["nkind"] is None)
        if p["loops"] == 1.0:
            assert bool((ei[0] == ei[1]).all())
    shapes = lambda rows: [(p["N"], i[0].shape[1]) for p, i in rows]                 # noqa: E731
    for rows in (nn, rg):
        assert (1, 0) in shapes(rows) and (5, 0) in shapes(rows)
        assert any(p["loops"] == 1.0 and i[0].shape[1] > 10 for p, i in rows)      # every edge a loop
    assert any(p["N"] == 1 and i[0].shape[1] > 0 for p, i in nn)                     # N = 1, self loops only
    assert any(p["aggr"] == "mean" and int((torch.bincount(i[0][0], minlength=p["N"])
                                            + torch.bincount(i[0][1], minlength=p["N"]) == 0).sum()) > 5
               for p, i in nn)                                                       # mean with isolated nodes
    assert any(p["form"] == "gather" and not p["head_bias"] for p, _ in nn)
    linear = {(p["c_in"], p["H"]) for p, _ in nn if p["nn"] == "linear" and p["N"] > 5}
    assert linear == {(33, 40), (70, 40), (32, 25)}
    modes = {(p["N"], p["mode"] == "featureless") for p, i in rg if i[0].shape[1] == 0}
    assert modes >= {(1, False), (1, True), (5, False)}
    assert any(p["R"] == 1 for p, _ in rg) and any(p["B"] == 65 and p["c_in"] == 3 for p, _ in rg)
    assert any(p["nkind"] == "signed" for p, _ in rg)
    assert any(p["rkind"] == "one" and (p["N"], p["deg"]) == (80, 8.0) and int(torch.bincount(i[2]).max()) == 640
               for p, i in rg)
    assert K.N_EDGES == 203                                                          # (the sweep's graph, for scale)


@pytest.mark.parametrize("k", range(len(Z.NNCONV_PINNED)))
def test_nnconv_restatements_agree_on_the_pinned_examples(k):
    """nn_conv against its literal loop, and bins(h, x) @ L against gather(h, x @
    L'): the identity the two kernel forms rest on (E = 0 and N = 1 included)."""
    p = Z.NNCONV_PINNED[k]
    ei, x, ea = Z.nnconv_inputs(p)
    N, c_in, c_out, H = p["N"], p["c_in"], p["c_out"], p["H"]
    g = torch.Generator().manual_seed(p["seed"])
    if p["nn"] == "linear":
        h = ea.double()
    else:
        h = torch.relu(ea.double() @ torch.randn(p["D"], H, generator=g, dtype=torch.float64)
                       + torch.randn(H, generator=g, dtype=torch.float64))
    hw = torch.randn(c_in * c_out, H, generator=g, dtype=torch.float64)
    hb = torch.randn(c_in * c_out, generator=g, dtype=torch.float64) if p["head_bias"] else None
    root = torch.randn(c_in, c_out, generator=g, dtype=torch.float64) if p["root"] else None
    bias = torch.randn(c_out, generator=g, dtype=torch.float64) if p["bias"] else None
    out = NR.nn_conv(x, ei, h, hw, hb, c_in, c_out, root, bias, p["aggr"], p["flow"])
    scale = NR.nn_conv(x, ei, h, hw, hb, c_in, c_out, root, bias, p["aggr"], p["flow"], absolute=True)
    assert tuple(out.shape) == (N, c_out)
    _close64(out, NR.nn_conv_loop(x, ei, h, hw, hb, c_in, c_out, root, bias, p["aggr"], p["flow"]), scale, "loop")
    i, j = (1, 0) if p["flow"] == "source_to_target" else (0, 1)
    dst, src = ei[i], ei[j]
    L = NR.head_matrix(hw, hb, c_in, c_out)
    Z_ = NR.bins(dst, src, N, h, x)
    assert tuple(Z_.shape) == (N, (H + 1) * c_in)
    by_bins = Z_ @ L
    by_gather = NR.gather(dst, src, N, h, x.double() @ NR.gather_matrix(L, H, c_in, c_out), c_out)
    terms = NR.bins(dst, src, N, h.abs(), x.abs()) @ L.abs()
    _close64(by_bins, by_gather, terms, "bins @ L against gather")
    plain = NR.nn_conv(x, ei, h, hw, hb, c_in, c_out, None, None, "add", p["flow"])
    _close64(by_bins, plain, terms, "bins @ L against the layer")
    dz = torch.randn(N, (H + 1) * c_in, generator=g, dtype=torch.float64)
    assert tuple(NR.edge_grad(dst, src, dz, x, H).shape) == (ei.shape[1], H)
    if ei.shape[1] == 0:
        assert float(Z_.abs().sum()) == 0.0 and float(by_gather.abs().sum()) == 0.0


@pytest.mark.parametrize("k", range(len(Z.RGCN_PINNED)))
def test_rgcn_restatements_agree_on_the_pinned_examples(k):
    """rgcn_conv against its literal loop, and bins(x) @ V against gather(x @ L'),
    featured and featureless (x = the identity), with att_grad's shape."""
    p = Z.RGCN_PINNED[k]
    ei, x, et, en = Z.rgcn_inputs(p)
    N, c_out, n_rel, B = p["N"], p["c_out"], p["R"], p["B"]
    c_in = N if x is None else p["c_in"]
    g = torch.Generator().manual_seed(p["seed"])
    basis = torch.randn(B, c_in, c_out, generator=g, dtype=torch.float64)
    att = torch.randn(n_rel, B, generator=g, dtype=torch.float64)
    root = torch.randn(c_in, c_out, generator=g, dtype=torch.float64) if p["root"] else None
    bias = torch.randn(c_out, generator=g, dtype=torch.float64) if p["bias"] else None
    out = RR.rgcn_conv(x, ei, et, en, basis, att, root, bias, p["flow"])
    scale = RR.rgcn_conv(x, ei, et, en, basis, att, root, bias, p["flow"], absolute=True)
    assert tuple(out.shape) == (N, c_out)
    _close64(out, RR.rgcn_conv_loop(x, ei, et, en, basis, att, root, bias, p["flow"]), scale, "loop")
    i, j = (1, 0) if p["flow"] == "source_to_target" else (0, 1)
    dst, src = ei[i], ei[j]
    xe = torch.eye(N, dtype=torch.float64) if x is None else x.double()
    ena = None if en is None else en.abs()
    Z_ = RR.bins(dst, src, N, et, en, att, xe)
    assert tuple(Z_.shape) == (N, B, c_in)
    by_bins = Z_.reshape(N, B * c_in) @ basis.view(B * c_in, c_out)
    y = torch.einsum("nc,bcf->nbf", xe, basis)                         # x @ L', laid out [n, B, Cout]
    by_gather = RR.gather(dst, src, N, et, en, att, y)
    terms = RR.bins(dst, src, N, et, ena, att.abs(), xe.abs()).reshape(N, B * c_in) @ basis.abs().view(B * c_in, c_out)
    _close64(by_bins, by_gather, terms, "bins @ V against gather")
    _close64(by_bins, RR.rgcn_conv(x, ei, et, en, basis, att, None, None, p["flow"]), terms, "bins @ V against the layer")
    if x is None:                                                      # the featureless layer gathers basis in place
        _close64(RR.gather(dst, src, N, et, en, att, basis.permute(1, 0, 2)), by_gather, terms, "basis in place")
    dZ = torch.randn(N, B, c_in, generator=g, dtype=torch.float64)
    assert tuple(RR.att_grad(et, en, dst, src, dZ, xe, n_rel).shape) == (n_rel, B)
    if ei.shape[1] == 0:
        assert float(Z_.abs().sum()) == 0.0 and float(RR.att_grad(et, en, dst, src, dZ, xe, n_rel).abs().sum()) == 0.0


def test_assert_bound_compares_shapes_of_empty_tensors():
    for ref in (NR, RR):
        ref.assert_bound(torch.empty(0, 3), torch.empty(0, 3, dtype=torch.float64), torch.empty(0, 3), "empty")
        for got, want in ((torch.empty(0, 3), torch.empty(0, 4)), (torch.empty(0), torch.empty(0, 1)),
                          (torch.zeros(2, 1), torch.zeros(2, 3))):
            with pytest.raises(AssertionError, match="shapes"):
                ref.assert_bound(got, want.double(), want.double(), "mismatch")
        with pytest.raises(AssertionError, match="exceeds"):
            ref.assert_bound(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64),
                             torch.ones(1, dtype=torch.float64), "an unwritten entry")
