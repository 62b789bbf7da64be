"""Layer-level fuzzing of SplineConv, TopKPooling (topk / filter_adj) and
voxel-grid cluster pooling (voxel_grid, consecutive_cluster, max_pool / avg_pool,
their _x forms, pool_edge) on the engine: the sibling of test_gpu_fuzz_layers.py
for the three layer families added after it.

The inputs come from tests/_fuzz_cases.py (shared with the CPU test
tests/test_fuzz_cases_host.py); the references are the float64 / exact CPU
restatements tests/_spline_ref.py, tests/_pool_ref.py and tests/_cluster_ref.py.
Integer outputs (perm, inv, arg, relabelled edges, voxel keys), the max and the
gate are compared bit for bit; sums (spline output, means, attribute sums,
gradients) within the project's bound |err| <= 1e-5 * sum |terms|.

Every draw is valid by construction (no assume, no skip): the spline geometries
come from a table built once from mp_spline_ok, every batch holds a node.  The
top-k tests lower MP_TUNE_TOPK_WG_LIMIT (default 2048) for one example at a time,
which moves the boundary between the one-workgroup ranking and the sorted path
down to 64 or 100 nodes: the segmented and the single-graph sort, and a batch that
mixes them with the 256-thread workgroup form, are reached by batches of a few
hundred nodes.
"""
import contextlib
import itertools
import math

import pytest
import torch
from hypothesis import example, given, settings, strategies as st

from tests import _cluster_ref as C, _fuzz_cases as Z, _pool_ref as P, _spline_ref as S
from tests import test_gpu_cluster as TC
from tests.test_gpu_fuzz_layers import _N_EX, _SETTINGS
from tests.test_gpu_parity import _tuned
from tests.test_gpu_pool import RATIOS, _assert_bound as _pool_bound, _check_selection, _layer_perm_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_COSTLY = dict(_SETTINGS, max_examples=max(10, _N_EX // 2))
_COSTLIEST = dict(_SETTINGS, max_examples=max(10, _N_EX // 3))      # as test_fuzz_message_passing_node_dim
FLOWS = ("source_to_target", "target_to_source")


def _sizes_of(kind, seed, cap=None):
    """A batch_sizes kind, or the sizes themselves (the pinned examples)."""
    return Z.batch_sizes(kind, seed, cap) if isinstance(kind, str) else list(kind)


# --------------------------------------------------------------------------
# a. SplineConv
# --------------------------------------------------------------------------

def _spline_table():
    """(D, degree) -> [(kernel_size, is_open_spline)] of every combination with sizes
    in {2, 3, 5} and K <= 125 that mp_spline_ok accepts."""
    from mi355_mp import ops
    table = {}
    for D, M in itertools.product((1, 2, 3), (1, 2, 3)):
        rows = []
        for ks in itertools.product((2, 3, 5), repeat=D):
            if math.prod(ks) > 125:
                continue
            for op in itertools.product((0, 1), repeat=D):
                try:
                    ops._spline_geom(list(ks), list(op), M, D, 70)
                except NotImplementedError:
                    continue
                rows.append((list(ks), list(op)))
        assert rows, (D, M)
        table[(D, M)] = rows
    return table


SPLINE_TABLE = _spline_table()


@settings(**_COSTLIEST)
@given(N=st.integers(1, 80), deg=st.floats(0.0, 10.0), loops=st.sampled_from([0.0, 0.2]),
       f_in=st.sampled_from([1, 3, 8, 33, 70]), f_out=st.sampled_from([1, 4, 10, 70]), D=st.sampled_from([1, 2, 3]),
       M=st.sampled_from([1, 2, 3]), geo=st.integers(0, 1 << 16), aggr=st.sampled_from(["mean", "add"]),
       flow=st.sampled_from(FLOWS), root=st.booleans(), bias=st.booleans(),
       form=st.sampled_from(["bins", "gather", None]), seed=st.integers(0, 1 << 16))
@example(N=1, deg=0.0, loops=0.0, f_in=3, f_out=4, D=2, M=1, geo=0, aggr="mean", flow=FLOWS[0], root=True, bias=True,
         form=None, seed=1)
@example(N=1, deg=3.0, loops=1.0, f_in=8, f_out=10, D=2, M=2, geo=5, aggr="add", flow=FLOWS[0], root=True, bias=True,
         form="bins", seed=2)
@example(N=5, deg=0.0, loops=0.0, f_in=3, f_out=4, D=1, M=3, geo=1, aggr="mean", flow=FLOWS[1], root=True, bias=False,
         form="gather", seed=3)
@example(N=60, deg=4.0, loops=0.2, f_in=33, f_out=10, D=3, M=1, geo=7, aggr="mean", flow=FLOWS[0], root=False,
         bias=False, form="bins", seed=4)
@example(N=80, deg=6.0, loops=0.2, f_in=3, f_out=70, D=2, M=3, geo=11, aggr="add", flow=FLOWS[1], root=True, bias=True,
         form="gather", seed=5)
@example(N=100, deg=0.3, loops=0.0, f_in=70, f_out=4, D=3, M=2, geo=3, aggr="mean", flow=FLOWS[1], root=False,
         bias=True, form=None, seed=6)
def test_fuzz_splineconv_layer(N, deg, loops, f_in, f_out, D, M, geo, aggr, flow, root, bias, form, seed):
    """SplineConv(f_in, f_out, dim=D, kernel_size, is_open_spline, degree=M, aggr,
    flow, root_weight, bias)(x, edge_index, pseudo, form): the output and the
    gradients of x, weight, root and bias against the float64 restatement, each
    within 1e-5 * sum |terms|.  Pinned: N = 1 without edges and with self loops
    only, E = 0, no root and no bias, target_to_source through the gather form, a
    graph where most nodes have no incoming edge."""
    from torch_geometric.nn import SplineConv
    rows = SPLINE_TABLE[(D, M)]
    ks, op = rows[geo % len(rows)]
    torch.manual_seed(seed)
    ei, g = Z.graph(N, deg, loops, seed)
    E = ei.shape[1]
    u = Z.pseudo(E, D, ks, seed)
    x = torch.randn(N, f_in, generator=g)
    conv = SplineConv(f_in, f_out, dim=D, kernel_size=ks, is_open_spline=[bool(o) for o in op], degree=M, aggr=aggr,
                      flow=flow, root_weight=root, bias=bias).to(DEV)
    if bias:
        with torch.no_grad():
            conv.bias.copy_(torch.randn(f_out, generator=g))
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, ei.to(DEV), u.to(DEV), form=form)
    assert tuple(out.shape) == (N, f_out)
    gout = torch.randn(N, f_out, generator=g)
    (out * gout.to(DEV)).sum().backward()

    leaves = [t.detach().cpu().double().requires_grad_(True) if t is not None else None
              for t in (conv.weight, conv.root, conv.bias)]
    xr = x.double().requires_grad_(True)
    ref = S.spline_conv(xr, ei, u, leaves[0], leaves[1], leaves[2], ks, op, M, aggr, flow)
    scale = S.spline_conv(x, ei, u, leaves[0].detach(), None if leaves[1] is None else leaves[1].detach(),
                          None if leaves[2] is None else leaves[2].detach(), ks, op, M, aggr, flow, absolute=True)
    what = "N=%d E=%d %s %s D=%d M=%d ks=%s open=%s form=%s" % (N, E, aggr, flow, D, M, ks, op, form)
    S.assert_bound(out, ref, scale, "forward " + what)
    (ref * gout.double()).sum().backward()
    gscale = S.abs_grad_scale(conv.weight, conv.root, conv.bias, x, ei, u, ks, op, M, aggr, gout, flow)
    pairs = [("x", xd.grad, xr.grad), ("weight", conv.weight.grad, leaves[0].grad)]
    if root:
        pairs.append(("root", conv.root.grad, leaves[1].grad))
    if bias:
        pairs.append(("bias", conv.bias.grad, leaves[2].grad))
    assert set(gscale) == {name for name, _, _ in pairs}
    for name, got, want in pairs:
        assert got is not None and tuple(got.shape) == tuple(want.shape), name
        S.assert_bound(got, want, gscale[name], "grad %s %s" % (name, what))


# --------------------------------------------------------------------------
# b. top-k selection
# --------------------------------------------------------------------------

def _limit(limit):
    return contextlib.nullcontext() if limit is None else _tuned(topk_wg_limit=limit)


def _expected_path(n_g, limit):
    """0 = one wave, 1 = one workgroup, 2 = sorted, under the limit now in force."""
    return 0 if n_g <= 64 else (1 if n_g <= limit else 2)


@settings(**_SETTINGS)
@given(bkind=st.sampled_from(Z.BATCH_KINDS), skind=st.sampled_from(Z.SCORE_KINDS),
       ratio=st.one_of(st.sampled_from(RATIOS), st.floats(min_value=2.0 ** -10, max_value=1.0, width=32)),
       limit=st.sampled_from([64, 100, None]), single=st.booleans(), seed=st.integers(0, 1 << 16))
@example(bkind=(65,), skind="ties", ratio=0.5, limit=100, single=False, seed=1)
@example(bkind=(0, 0, 101, 0), skind="five", ratio=0.3, limit=100, single=False, seed=2)
@example(bkind=(130,), skind="ties", ratio=0.6, limit=64, single=True, seed=3)
@example(bkind=(0, 0, 0, 0, 3), skind="distinct", ratio=0.8, limit=None, single=False, seed=4)
@example(bkind="edge", skind="five", ratio=1.0, limit=100, single=False, seed=5)
@example(bkind=(100, 65, 101, 0, 130, 64, 1), skind="equal", ratio=0.5, limit=100, single=False, seed=6)
@example(bkind=(65, 130, 64, 101), skind="distinct", ratio=0.001, limit=64, single=False, seed=7)
def test_fuzz_topk_select(bkind, skind, ratio, limit, single, seed):
    """ops.topk_select and the public topk on random batches, scores with ties and
    special values, and a workgroup limit of 64, 100 or the default: perm,
    out_starts, K and inv bit for bit against the stable restatement.  At limit
    100 graphs of 65..100 nodes are ranked by the 256-thread workgroup form while
    graphs of 101 and 130 nodes of the same batch go through the segmented sort;
    at limit 64 everything above one wave is sorted; `single` ranks the batch as
    one graph (batch = None), which above the limit is the device-wide sort."""
    from mi355_mp import _lib, ops
    from torch_geometric.nn.pool import topk
    sizes = _sizes_of(bkind, seed)
    seen = [sum(sizes)] if single else Z.visible(sizes)
    n = sum(seen)
    s = Z.scores(skind, n, seed)
    batch = P.batch_of(seen)
    bd = None if single else batch.to(DEV)
    perm_ref, starts_ref = P.topk_stable(s, ratio, seen)
    with _limit(limit):
        in_force = int(_lib.load().mp_tune(_lib.MP_TUNE_TOPK_WG_LIMIT, -1))
        assert limit is None or in_force == limit
        for n_g in seen:
            assert ops.topk_path(n_g) == _expected_path(n_g, in_force)
        layout = ops.batch_layout(bd, n, DEV)          # fresh: a layout never crosses a change of the limit
        assert (layout.n_graphs, layout.max_n, layout.unsorted) == (len(seen), max(seen), 0)
        sel = ops.topk_select(s.to(DEV), ratio, layout)
        _check_selection(sel, perm_ref, starts_ref, n)
        assert torch.equal(topk(s.to(DEV), ratio, bd).cpu(), perm_ref)
        if skind == "distinct":
            m = float(s[seed % n])
            got = topk(s.to(DEV), None, bd, min_score=m)
            assert torch.equal(got.cpu(), P.topk_min_score(s, m, batch))


# --------------------------------------------------------------------------
# c. TopKPooling
# --------------------------------------------------------------------------

def _pool_edges(n, deg, g):
    """Edges over n nodes with duplicates and self loops."""
    E = int(deg * n)
    src = torch.randint(0, n, (E,), generator=g)
    dst = torch.randint(0, n, (E,), generator=g)
    dst[::9] = src[::9]
    ei = torch.stack([src, dst])
    if E:
        ei[:, 1::11] = ei[:, 0:1]
    return ei


def _offset_view(t):
    """t [n, F] as the column slice at offset 1 of an [n, F + 3] tensor: the same
    values, rows not 16-byte aligned."""
    big = torch.zeros(t.shape[0], t.shape[1] + 3, device=t.device)
    big[:, 1:t.shape[1] + 1] = t
    return big[:, 1:t.shape[1] + 1]


@settings(**_COSTLY)
@given(bkind=st.sampled_from(Z.BATCH_KINDS), F=st.sampled_from([1, 3, 4, 16, 130]),
       multiplier=st.sampled_from([1, 2.5]), ratio=st.sampled_from([0.5, 0.8, 1.0]), zero_rows=st.booleans(),
       own_attn=st.booleans(), attr_mode=st.sampled_from(["none", "vec", "mat"]), deg=st.sampled_from([0, 4]),
       seed=st.integers(0, 1 << 16))
@example(bkind=(1,), F=3, multiplier=1, ratio=0.5, zero_rows=False, own_attn=False, attr_mode="vec", deg=4, seed=1)
@example(bkind="edge", F=16, multiplier=2.5, ratio=1.0, zero_rows=True, own_attn=False, attr_mode="mat", deg=4, seed=2)
@example(bkind="random", F=130, multiplier=1, ratio=0.8, zero_rows=True, own_attn=True, attr_mode="mat", deg=0, seed=3)
@example(bkind="wave", F=4, multiplier=2.5, ratio=0.5, zero_rows=False, own_attn=False, attr_mode="none", deg=4, seed=4)
@example(bkind="tiny", F=1, multiplier=2.5, ratio=0.8, zero_rows=True, own_attn=True, attr_mode="vec", deg=0, seed=5)
def test_fuzz_topk_pooling_layer(bkind, F, multiplier, ratio, zero_rows, own_attn, attr_mode, deg, seed):
    """TopKPooling(F, ratio, multiplier)(x, edge_index, edge_attr, batch, attn): perm
    against the stable restatement of the score op's own output, the gate, the
    kept scores and batch bit for bit, filter_adj against its restatement, the
    gradients of x, attn, weight and edge_attr against the float64 restatement;
    and the same layer on x given as an offset column slice (rows not 16-byte
    aligned: the gate's scalar instantiation at F % 4 == 0) is bitwise the
    contiguous run.  Pinned: one 1-node graph, ratio 1.0 (nothing dropped), E =
    0 with an edge_attr, F = 4."""
    from torch_geometric.nn import TopKPooling
    seen = Z.visible(_sizes_of(bkind, seed, cap=600))
    batch = P.batch_of(seen)
    n = batch.numel()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g)
    if zero_rows:
        x[torch.randint(0, n, (max(n // 4, 1),), generator=g)] = 0.0
    fa = 7 if own_attn else F
    attn = torch.randn(n, fa, generator=g) if own_attn else None
    ei = _pool_edges(n, deg, g)
    E = ei.shape[1]
    attr = {"none": None, "vec": torch.randn(E, generator=g), "mat": torch.randn(E, 3, generator=g)}[attr_mode]
    torch.manual_seed(seed)
    pool = TopKPooling(fa, ratio=ratio, multiplier=multiplier).to(DEV)
    K = int(P.keep_counts(ratio, seen).sum())
    gy, gt = torch.randn(K, F, generator=g), torch.randn(K, generator=g)
    bd, eid = batch.to(DEV), ei.to(DEV)

    def run(xd):
        pool.zero_grad()
        ad = attn.to(DEV).requires_grad_(True) if own_attn else None
        ed = attr.to(DEV).requires_grad_(True) if attr is not None else None
        xo, eo, ao, bo, perm, so = pool(xd, eid, ed, bd, attn=ad)
        assert tuple(xo.shape) == (K, F) and perm.numel() == K
        loss = (xo * gy.to(DEV)).sum() + (so * gt.to(DEV)).sum()
        ga = None
        if attr is not None:
            ga = torch.randn(ao.shape, generator=torch.Generator().manual_seed(seed + 1))
            loss = loss + (ao * ga.to(DEV)).sum()
        loss.backward()
        return (xo, eo, ao, bo, perm, so), (xd.grad, None if ad is None else ad.grad, pool.weight.grad.clone(),
                                            None if ed is None else ed.grad), ad, ga

    xd = x.to(DEV).requires_grad_(True)
    (xo, eo, ao, bo, perm, so), (gx, gattn, gw, gattr), ad, ga = run(xd)

    # forward: exact given the scores
    s, perm_ref = _layer_perm_ref(pool, (ad if own_attn else xd).detach(), seen)
    assert torch.equal(perm.cpu(), perm_ref)
    want = xd.detach()[perm] * s[perm].view(-1, 1)
    if multiplier != 1:
        want = multiplier * want
    assert torch.equal(xo, want)
    assert torch.equal(so, s[perm]) and torch.equal(bo, bd[perm])
    re, ra, keep = P.filter_adj(ei, attr, perm_ref, n)
    assert torch.equal(eo.cpu(), re) and eo.is_contiguous() and tuple(eo.shape) == (2, re.shape[1])
    if attr is None:
        assert ao is None
    else:
        assert tuple(ao.shape) == tuple(ra.shape) and torch.equal(ao.cpu(), ra)
    if ratio == 1.0:
        assert K == n and re.shape[1] == E

    # gradients against the float64 restatement run with the device's perm
    p = perm.cpu()
    x64 = x.double().requires_grad_(True)
    a64 = attn.double().requires_grad_(True) if own_attn else None
    w64 = pool.weight.detach().cpu().double().requires_grad_(True)
    rxo, rso, _ = P.layer(x64, w64, p, attn=a64, multiplier=multiplier)
    ((rxo * gy.double()).sum() + (rso * gt.double()).sum()).backward()
    gate_abs, attn_abs, w_abs = P.layer_grad_scales(x64, a64 if own_attn else x64, w64, p, gy, gt, multiplier)
    if own_attn:
        _pool_bound(gx, x64.grad, gate_abs, "grad x")
        _pool_bound(gattn, a64.grad, attn_abs, "grad attn")
        dropped = torch.ones(n, dtype=torch.bool)
        dropped[p] = False
        assert float(gx.cpu()[dropped].abs().sum()) == 0.0                 # exact zeros from the gate
    else:
        _pool_bound(gx, x64.grad, gate_abs + attn_abs, "grad x (= attn)")
    _pool_bound(gw.view(-1), w64.grad.view(-1), w_abs, "grad weight")
    if attr is not None:
        want_ga = torch.zeros_like(attr)
        want_ga[keep] = ga
        assert torch.equal(gattr.cpu(), want_ga)                           # a copy forward, a scatter backward

    # the same through an offset column slice of x: bitwise
    xs = _offset_view(x.to(DEV)).detach().requires_grad_(True)
    assert xs.stride(0) == F + 3 and xs.data_ptr() % 16 != 0
    outs2, grads2, _, _ = run(xs)
    for a, b in zip((xo, eo, ao, bo, perm, so), outs2):
        assert (a is None and b is None) or torch.equal(a, b)
    for a, b in zip((gx, gattn, gw, gattr), grads2):
        assert (a is None and b is None) or torch.equal(a, b)


# --------------------------------------------------------------------------
# d. cluster pooling
# --------------------------------------------------------------------------

def _cluster_x(xkind, n, F, g):
    if xkind == "ints":
        return torch.randint(-2, 3, (n, F), generator=g).float() * 0.5           # tie-heavy
    if xkind == "all_masked":
        return torch.full((n, F), -20000.0)
    x = torch.randn(n, F, generator=g)
    x[torch.rand(n, F, generator=g) < 0.1] = -20000.0
    if n > 1:
        x[torch.randint(0, n, (2,), generator=g)] = -20000.0                      # whole rows: a masked singleton
    return x


def _graph_local_clusters(cluster, batch):
    """(ids in [0, G * size), size): every graph's clusters numbered from 0 in key
    order (the clusters of different graphs are disjoint)."""
    inv = torch.unique(cluster, sorted=True, return_inverse=True)[1]
    G = int(batch.max()) + 1
    first = torch.full((G,), inv.numel(), dtype=torch.int64).scatter_reduce_(0, batch, inv, "amin")
    local = inv - first[batch]
    size = int(local.max()) + 1
    return local + batch * size, size


@settings(**_COSTLY)
@given(bkind=st.sampled_from(Z.BATCH_KINDS), ckind=st.sampled_from(Z.CLUSTER_KINDS),
       ekind=st.sampled_from(Z.CLUSTER_EDGE_KINDS), F=st.sampled_from([1, 3, 33, 64, 130]),
       attr_mode=st.sampled_from(["none", "vec", "mat"]), reduce=st.sampled_from(["max", "mean"]),
       xkind=st.sampled_from(["ints", "masked"]), seed=st.integers(0, 1 << 16))
@example(bkind=(1,), ckind="voxel", ekind="random", F=3, attr_mode="vec", reduce="max", xkind="masked", seed=1)
@example(bkind="edge", ckind="one", ekind="random", F=33, attr_mode="mat", reduce="max", xkind="ints", seed=2)
@example(bkind="random", ckind="each", ekind="none", F=64, attr_mode="vec", reduce="mean", xkind="masked", seed=3)
@example(bkind="wave", ckind="wide", ekind="inside", F=130, attr_mode="mat", reduce="max", xkind="masked", seed=4)
@example(bkind="random", ckind="one", ekind="pairs", F=3, attr_mode="none", reduce="max", xkind="all_masked", seed=5)
@example(bkind="edge", ckind="wide", ekind="inside", F=1, attr_mode="vec", reduce="mean", xkind="ints", seed=6)
def test_fuzz_cluster_pooling(bkind, ckind, ekind, F, attr_mode, reduce, xkind, seed):
    """max_pool / avg_pool, the ops-level stage, max_pool_x / avg_pool_x (with and
    without size) and voxel_grid on batches of 1..250 nodes: voxel clusters, one
    cluster, one cluster per node and int64 keys of either sign spread over
    2^63; random edges, none, edges that all become loops (E > 0, E' = 0) and
    many duplicates of few pairs; x with ties or with entries (and whole
    clusters) below -10000.  Integer outputs and the max bit for bit, means and
    attribute sums within the bound, the gradients of x, pos and edge_attr
    against the float64 restatement (through the max: exact)."""
    from torch_geometric.nn import avg_pool, avg_pool_x, max_pool, max_pool_x, voxel_grid
    seen = Z.visible(_sizes_of(bkind, seed, cap=250))
    batch = P.batch_of(seen)
    n = batch.numel()
    assert 1 <= n <= 250
    cluster, pos, vsize = Z.clusters(ckind, n, batch, seed)
    ei = Z.cluster_edges(ekind, n, cluster, seed)
    E = ei.shape[1]
    g = torch.Generator().manual_seed(seed)
    x = _cluster_x(xkind, n, F, g)
    attr = {"none": None, "vec": torch.rand(E, generator=g) - 0.3, "mat": torch.rand(E, 2, generator=g) - 0.3}[attr_mode]
    ref = TC._ref(cluster, x, pos, batch, ei, attr, reduce)
    M, Ep = ref["perm"].numel(), ref["edge_index"].size(1)
    if ekind in ("none", "inside") or ckind == "one":
        assert Ep == 0
    cd, bd = cluster.to(DEV), batch.to(DEV)

    if ckind == "voxel":
        keys = voxel_grid(pos.to(DEV), bd, vsize, 0, Z.VOXEL_END)
        assert keys.dtype == torch.int64 and torch.equal(keys.cpu(), cluster)
        from torch_geometric.nn import consecutive_cluster
        inv_d, perm_d = consecutive_cluster(keys)
        assert torch.equal(inv_d.cpu(), ref["inv"]) and torch.equal(perm_d.cpu(), ref["perm"])

    # the ops-level stage (arg and edge_slot kept), then the layer
    got = TC._selection(cluster, x, pos, batch, ei, attr, reduce)
    assert got["perm"].numel() == M and got["edge_index"].shape[1] == Ep
    TC._check_stage(got, ref, x, pos, attr, reduce)
    d = TC._data(x, pos, batch, ei, attr)
    leaves_d = [d.x, d.pos] + ([d.edge_attr] if attr is not None else [])
    for t in leaves_d:
        t.requires_grad_(True)
    out = (max_pool if reduce == "max" else avg_pool)(cd, d)
    layer = {"inv": got["inv"], "perm": got["perm"], "x": out.x, "pos": out.pos, "batch": out.batch,
             "edge_index": out.edge_index, "edge_attr": out.edge_attr}
    TC._check_stage(layer, ref, x, pos, attr, reduce)
    assert tuple(out.x.shape) == (M, F) and out.x.is_contiguous() and out.edge_index.is_contiguous()
    if xkind == "all_masked" and reduce == "max":
        assert float(out.x.detach().abs().max()) == 0.0

    # gradients against the float64 form run with the reference's inv / arg / edge_slot
    wx, wp = torch.randn(M, F, generator=g), torch.randn(M, 2, generator=g)
    wa = None if attr is None else torch.randn((Ep,) + tuple(attr.shape[1:]), generator=g)
    loss = (out.x * wx.to(DEV)).sum() + (out.pos * wp.to(DEV)).sum()
    if attr is not None:
        loss = loss + (out.edge_attr * wa.to(DEV)).sum()
    loss.backward()

    def f64(leaves, ws):
        av = leaves[2] if attr is not None else None
        xo, po, ao = C.pool_f64(leaves[0], leaves[1], av, ref["inv"], ref["arg"], ref["edge_slot"], M, Ep, reduce)
        total = (xo * ws[0]).sum() + (po * ws[1]).sum()
        return total if attr is None else total + (ao * ws[2]).sum()

    srcs = [x, pos] + ([attr] if attr is not None else [])
    ws = [wx.double(), wp.double()] + ([wa.double()] if attr is not None else [])
    leaves = [t.double().requires_grad_(True) for t in srcs]
    f64(leaves, ws).backward()
    scales = [t.double().requires_grad_(True) for t in srcs]
    f64(scales, [w.abs() for w in ws]).backward()
    for name, t, want, sc in zip(("d x", "d pos", "d edge_attr"), leaves_d, leaves, scales):
        assert t.grad is not None and tuple(t.grad.shape) == tuple(want.shape), name
        want_g = want.grad if want.grad is not None else torch.zeros_like(want)
        sc_g = sc.grad.abs() if sc.grad is not None else torch.zeros_like(want)
        TC._assert_bound(t.grad, want_g, sc_g, "%s (%s)" % (name, reduce))
        if (name == "d x" and reduce == "max") or name == "d edge_attr":
            assert torch.equal(t.grad.cpu().double(), want_g), name              # a routing / a gather: exact

    # the _x forms without size: the same clusters
    fx = max_pool_x if reduce == "max" else avg_pool_x
    xo, bo = fx(cd, x.to(DEV), bd)
    assert torch.equal(bo.cpu(), ref["batch"]) and tuple(xo.shape) == (M, F)
    r64 = C.pool_f64(x.double(), None, None, ref["inv"], None, None, M, 0, "mean")[0]
    if reduce == "max":
        assert torch.equal(xo.cpu(), ref["x"])
    else:
        TC._assert_bound(xo, r64, TC._mean_scale(x, ref["inv"], M), "avg_pool_x")

    # with size: the voxel clusters relabelled into [0, G * size)
    if ckind == "voxel":
        sized, size = _graph_local_clusters(cluster, batch)
        G = int(batch.max()) + 1
        xo, bo = fx(sized.to(DEV), x.to(DEV), bd, size=size)
        assert bo is None and tuple(xo.shape) == (G * size, F)
        if reduce == "max":
            assert torch.equal(xo.cpu(), C.pool_x_sized(sized, x, batch, size, "max"))
        else:
            cnt = torch.bincount(sized, minlength=G * size).clamp(min=1).double().view(-1, 1)
            want = torch.zeros((G * size, F), dtype=torch.float64).index_add_(0, sized, x.double()) / cnt
            sc = torch.zeros((G * size, F), dtype=torch.float64).index_add_(0, sized, x.double().abs()) / cnt
            TC._assert_bound(xo, want, sc, "avg_pool_x(size)")
            fp32 = C.pool_x_sized(sized, x, batch, size, "mean")
            TC._assert_bound(xo, fp32.double(), sc, "avg_pool_x(size) against the fp32 restatement")


# --------------------------------------------------------------------------
# e. one stage's outputs as the next stage's inputs
# --------------------------------------------------------------------------

def _fresh(t):
    """A new tensor with the same values: no cached index range, graph count or
    batch layout is attached to it (a clone keeps the autograd link)."""
    return None if t is None else t.clone()


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), what


def _input_grad(outs, x_in, seed):
    """d <outs, R> / d x_in for the float outputs of a stage (the graph is kept)."""
    g = torch.Generator().manual_seed(seed)
    loss = 0
    for o in outs:
        if o is not None and o.is_floating_point() and o.requires_grad:
            loss = loss + (o * torch.randn(o.shape, generator=g).to(o.device)).sum()
    return torch.autograd.grad(loss, x_in, retain_graph=True)[0]


def _stage_twice(stage, prev, x_in, seed, what):
    """Run `stage` on the previous stage's outputs as returned and on fresh clones of
    them: outputs and the gradient reaching x_in must be bitwise equal.  Returns the
    outputs of the as-returned run."""
    a = stage(*prev)
    b = stage(*[_fresh(t) for t in prev])
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        _same(u, v, "%s: output %d" % (what, k))
    _same(_input_grad(a, x_in, seed), _input_grad(b, x_in, seed), "%s: d x" % what)
    return a


@settings(**_COSTLIEST)
@given(bkind=st.sampled_from(["edge", "random"]), F=st.sampled_from([4, 33]), seed=st.integers(0, 1 << 16))
@example(bkind=(1,), F=4, seed=1)
@example(bkind=(0, 130, 0, 65, 3), F=33, seed=2)
def test_fuzz_stage_outputs_feed_the_next_stage(bkind, F, seed):
    """What a pooling stage returns is sliced by counts read from the device and
    carries cached metadata (the noted graph count, a cached batch layout, a cached
    index range).  Each later stage of two pipelines --
      voxel_grid -> max_pool(Cartesian) -> SplineConv -> voxel_grid -> max_pool_x
      GraphConv -> TopKPooling -> GraphConv -> TopKPooling -> global_max_pool
    -- runs on the previous stage's outputs as returned and on clones of them,
    which carry none of that: outputs and the gradient at the pipeline's input
    x are bitwise equal (no tolerance: the cache must never disagree with the
    data)."""
    from torch_geometric.data import Batch
    from torch_geometric.nn import (GraphConv, SplineConv, TopKPooling, global_max_pool, max_pool, max_pool_x,
                                    voxel_grid)
    from torch_geometric.transforms import Cartesian
    seen = Z.visible(_sizes_of(bkind, seed, cap=250))
    batch = P.batch_of(seen)
    n = batch.numel()
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    pos = torch.rand(n, 2, generator=g) * 27.9
    ei = Z.cluster_edges("random", n, None, seed)
    x = torch.randn(n, F, generator=g).to(DEV).requires_grad_(True)
    bd, eid, pd = batch.to(DEV), ei.to(DEV), pos.to(DEV)

    # 1. cluster pooling feeding SplineConv and a second pooling
    conv = SplineConv(F, 8, dim=2, kernel_size=3).to(DEV)
    d1 = max_pool(voxel_grid(pd, bd, 5, 0, 28), Batch(batch=bd, x=x, pos=pd, edge_index=eid),
                  transform=Cartesian(cat=False))
    assert tuple(d1.edge_attr.shape) == (d1.edge_index.shape[1], 2) and not d1.edge_attr.requires_grad
    (h,) = _stage_twice(lambda xx, e, u: conv(xx, e, u), (d1.x, d1.edge_index, d1.edge_attr), x, seed, "SplineConv")

    def second_pool(hh, pp, bb):
        cl = voxel_grid(pp, bb, 14, 0, 27.99)
        a, _ = max_pool_x(cl, hh, bb, size=4)
        b, b_out = max_pool_x(cl, hh, bb)
        return cl, a, b, b_out
    cl, a, b, b_out = _stage_twice(second_pool, (h, d1.pos, d1.batch), x, seed, "voxel_grid -> max_pool_x")
    G = int(d1.batch.max()) + 1
    assert tuple(a.shape) == (G * 4, 8) and b.shape[0] == b_out.shape[0] == cl.unique().numel()

    # 2. GraphConv / TopKPooling chain
    gc1, gc2 = GraphConv(F, 8).to(DEV), GraphConv(8, 8).to(DEV)
    tp1, tp2 = TopKPooling(8, 0.6).to(DEV), TopKPooling(8, 0.6).to(DEV)
    h = torch.relu(gc1(x, eid))

    def pooled(tp):
        def stage(hh, e, bb):
            xo, eo, _, bo, perm, so = tp(hh, e, None, bb)
            return xo, eo, bo, perm, so
        return stage
    xo, eo, bo, perm, _ = _stage_twice(pooled(tp1), (h, eid, bd), x, seed, "TopKPooling 1")
    assert perm.numel() == int(P.keep_counts(0.6, seen).sum())
    (h2,) = _stage_twice(lambda hh, e: torch.relu(gc2(hh, e)), (xo, eo), x, seed, "GraphConv 2")
    xo2, eo2, bo2, perm2, _ = _stage_twice(pooled(tp2), (h2, eo, bo), x, seed, "TopKPooling 2")
    assert perm2.numel() == int(P.keep_counts(0.6, P.keep_counts(0.6, seen)).sum())
    (out,) = _stage_twice(lambda hh, bb: global_max_pool(hh, bb), (xo2, bo2), x, seed, "global_max_pool")
    assert tuple(out.shape) == (int(bo2.max()) + 1, 8)


# --------------------------------------------------------------------------
# non-contiguous inputs (the sibling of test_fuzz_layer_input_views)
# --------------------------------------------------------------------------

@settings(**_COSTLY)
@given(N=st.integers(1, 150), deg=st.floats(0.0, 8.0), F=st.sampled_from([1, 3, 8, 64, 100]),
       layer=st.sampled_from(["spline", "topk", "max_pool", "avg_pool"]),
       xview=st.sampled_from(["contiguous", "offset", "strided", "transposed"]), eiview=st.booleans(),
       seed=st.integers(0, 1 << 16))
@example(N=70, deg=3.0, F=8, layer="topk", xview="offset", eiview=True, seed=1)
@example(N=70, deg=3.0, F=64, layer="max_pool", xview="transposed", eiview=True, seed=2)
def test_fuzz_pool_layer_input_views(N, deg, F, layer, xview, eiview, seed):
    """SplineConv, TopKPooling, max_pool and avg_pool fed non-contiguous inputs -- x
    as a column slice at an odd offset, a strided column view, a transposed view,
    edge_index as the transposed view of an [E, 2] tensor, pos as an offset
    column slice -- give the same outputs and x gradient as on contiguous
    copies: bitwise for the pooling layers (the kernels see the same values in
    the same order), to the GEMM's rounding for SplineConv's x W."""
    from torch_geometric.data import Batch
    from torch_geometric.nn import SplineConv, TopKPooling, avg_pool, max_pool
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    E = int(N * deg)
    ei = torch.randint(N, (2, E), generator=g)
    base = torch.randn(N, F, generator=g)
    pos = torch.rand(N, 2, generator=g)
    u = torch.rand(E, 2, generator=g).to(DEV)
    cluster = (torch.randint(max(N // 3, 1), (N,), generator=g) * 5 - 3).to(DEV)
    mod = {"spline": lambda: SplineConv(F, 8, dim=2, kernel_size=3), "topk": lambda: TopKPooling(F, 0.5),
           "max_pool": lambda: None, "avg_pool": lambda: None}[layer]()
    mod = mod.to(DEV) if mod is not None else None

    def x_as(kind):
        b = base.to(DEV)
        if kind == "offset":
            v = _offset_view(b)
        elif kind == "strided":
            big = torch.zeros(N, 2 * F, device=DEV)
            big[:, ::2] = b
            v = big[:, ::2]
        elif kind == "transposed":
            v = b.t().contiguous().t()
        else:
            v = b.clone()
        return v.detach().requires_grad_()

    e_ref = ei.to(DEV)
    e_in = ei.t().contiguous().to(DEV).t() if eiview else e_ref.clone()
    p_ref = pos.to(DEV)
    p_in = _offset_view(p_ref) if xview != "contiguous" else p_ref.clone()

    def run(xx, e, p):
        if layer == "spline":
            return (mod(xx, e, u),)
        if layer == "topk":
            xo, eo, _, _, perm, so = mod(xx, e)
            return xo, eo, perm, so
        out = (max_pool if layer == "max_pool" else avg_pool)(cluster, Batch(x=xx, pos=p, edge_index=e))
        return out.x, out.pos, out.edge_index
    xa, xb = x_as("contiguous"), x_as(xview)
    oa, ob = run(xa, e_ref, p_ref), run(xb, e_in, p_in)
    grads = []
    for outs, xx in ((oa, xa), (ob, xb)):
        gg = torch.Generator().manual_seed(seed)
        loss = sum((o * torch.randn(o.shape, generator=gg).to(DEV)).sum() for o in outs if o.is_floating_point())
        loss.backward()
        grads.append(xx.grad)
    for a, b in list(zip(oa, ob)) + [tuple(grads)]:
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
        if layer == "spline":
            # x W: hipBLASLt picks its kernel by the operand layout, so the layer
            # agrees to the GEMM's rounding, not bitwise
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), float((a - b).abs().max())
        else:
            assert torch.equal(a, b)
