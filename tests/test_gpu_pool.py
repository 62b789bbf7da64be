"""TopKPooling on the GPU against the restatement tests/_pool_ref.py.

Selection is compared bit for bit (perm, out_starts, K, the inverse map): on
distinct scores against both restatement forms, on repeated scores against the
stable form, which fixes the tie rule.  The layer's perm is checked against the
stable form applied to the score vector the score op itself returns (the same
kernel, the same bits) -- a float64 ranking would differ at near-ties.  The
gate is one correctly rounded fp32 multiply per step, so it is compared with
torch.equal.  Floating-point results that are sums (score, gradients) use the
project's bound |err| <= 1e-5 * sum |terms|; the sums of magnitudes are written
out below next to each use.
"""
import importlib.util
import math
import os

import pytest
import torch

from tests import _pool_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOUND = 1e-5
RATIOS = [0.8, 0.5, 0.3, 0.6, 0.001, 1.0]
FIVE = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")])


def _wg_limit():
    """The largest graph ranked inside one workgroup, read through mp_topk_path."""
    from mi355_mp import ops
    lo, hi = 64, 1 << 20                                   # path(lo) <= 1 < path(hi)
    assert ops.topk_path(lo + 1) == 1 and ops.topk_path(hi) == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ops.topk_path(mid) == 2:
            hi = mid
        else:
            lo = mid
    return lo


@pytest.fixture(scope="module")
def select_case():
    """Graph sizes around every limit, the batch layout and three score vectors."""
    from mi355_mp import ops
    L = _wg_limit()
    sizes = [0, 1, 2, 25, 50, 63, 64, 65, 126, L - 1, L, L + 1, 3 * L + 7, 0, 5]
    assert {ops.topk_path(n) for n in sizes} == {0, 1, 2}          # all three paths are reached
    n = sum(sizes)
    assert n <= 20000
    g = torch.Generator().manual_seed(3)
    scores = {"distinct": R.distinct_scores(n, g), "five": FIVE[torch.randint(0, 5, (n,), generator=g)],
              "equal": torch.full((n,), 0.25)}
    batch = R.batch_of(sizes)
    layout = ops.batch_layout(batch.to(DEV), n)
    assert (layout.n_graphs, layout.max_n, layout.unsorted) == (len(sizes), 3 * L + 7, 0)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)])
    assert torch.equal(layout.starts.cpu(), starts)
    return sizes, batch, layout, scores


def _check_selection(sel, perm_ref, starts_ref, n):
    K = int(sel.counts[0])
    assert K == perm_ref.numel()
    assert torch.equal(sel.perm[:K].cpu(), perm_ref)
    assert torch.equal(sel.out_starts.cpu(), starts_ref)
    inv = torch.full((n,), -1, dtype=torch.int64)
    inv[perm_ref] = torch.arange(K)
    assert torch.equal(sel.inv.cpu(), inv)


# 1. select -------------------------------------------------------------------

@pytest.mark.parametrize("ratio", RATIOS)
def test_select_is_exact(select_case, ratio):
    from mi355_mp import ops
    sizes, batch, layout, scores = select_case
    n = sum(sizes)
    for name, s in scores.items():
        perm_ref, starts_ref = R.topk_stable(s, ratio, sizes)
        if name == "distinct":
            assert torch.equal(R.topk_dense(s, ratio, batch), perm_ref)
        sel = ops.topk_select(s.to(DEV), ratio, layout)
        _check_selection(sel, perm_ref, starts_ref, n)


def test_select_one_large_graph_and_public_topk(select_case):
    """batch = None on a graph above the workgroup limit (the device-wide sort),
    and torch_geometric.nn.pool.topk on the batch."""
    from mi355_mp import ops
    from torch_geometric.nn.pool import topk
    sizes, batch, layout, scores = select_case
    n = 3 * _wg_limit() + 7
    for name in ("five", "distinct"):
        s = scores[name][:n].contiguous()
        one = ops.batch_layout(None, n, DEV)
        assert ops.topk_path(one.max_n) == 2 and one.n_graphs == 1
        perm_ref, starts_ref = R.topk_stable(s, 0.3, [n])
        _check_selection(ops.topk_select(s.to(DEV), 0.3, one), perm_ref, starts_ref, n)
    s = scores["five"]
    assert torch.equal(topk(s.to(DEV), 0.6, batch.to(DEV)).cpu(), R.topk_stable(s, 0.6, sizes)[0])
    s = scores["distinct"]
    got = topk(s.to(DEV), None, batch.to(DEV), min_score=0.5)
    assert torch.equal(got.cpu(), R.topk_min_score(s, 0.5, batch))


def test_keep_counts_match_torch_for_every_size():
    from mi355_mp import ops
    sizes = torch.arange(4097)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(DEV)
    for ratio in RATIOS:
        out_starts, counts = ops.topk_counts(starts, ratio)
        k = R.keep_counts(ratio, sizes)
        assert torch.equal(out_starts.cpu().diff(), k), ratio
        assert int(counts[0]) == int(k.sum())


def test_understated_largest_graph_is_reported(select_case):
    from mi355_mp import ops
    sizes, batch, layout, scores = select_case
    low = ops.BatchLayout(layout.starts, layout.n_graphs, 64, 0, layout.n)
    sel = ops.topk_select(scores["equal"].to(DEV), 0.5, low)
    with pytest.raises(RuntimeError, match="max_n"):
        ops.pool_read_counts(sel, layout.n)


# 2. score --------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3, 33, 64, 128, 129, 300])
def test_score_within_the_bound(F):
    from mi355_mp import ops
    g = torch.Generator().manual_seed(F)
    n = 301
    big = torch.randn(n, F + 5, generator=g)
    attn = big[:, :F]                                              # row stride F + 5
    w = torch.randn(1, F, generator=g)
    a64, w64 = attn.double(), w.double()
    z = (a64 * w64).sum(-1)
    nrm = w64.norm()
    scale = ((a64 * w64).abs().sum(-1) / nrm).clamp(min=1.0)
    for kw, ref in ((dict(tanh=True), torch.tanh(z / nrm)), (dict(tanh=False), z / nrm)):
        got = ops.pool_score(big.to(DEV)[:, :F], w.to(DEV), **kw).cpu().double()
        ratio = float(((got - ref).abs() / scale).max())
        print("score F=%d %s: max |err| / scale = %.3g" % (F, kw, ratio))
        assert ratio <= BOUND
    raw = ops.pool_score(attn.contiguous().to(DEV), w.to(DEV), tanh=False, raw=True).cpu().double()
    assert float(((raw - z).abs() / (a64 * w64).abs().sum(-1).clamp(min=1.0)).max()) <= BOUND


# 3. gate, filter_adj, the layer ------------------------------------------------

SIZES = [0, 1, 2, 25, 50, 63, 64, 65, 126, 300, 0, 7]


def _layer_case(F, seed, zero_rows=True):
    """x with all-zero rows (equal scores, the common case after ReLU), edges with
    duplicates and self loops, a batch with empty graphs."""
    g = torch.Generator().manual_seed(seed)
    n = sum(SIZES)
    x = torch.randn(n, F, generator=g)
    if zero_rows:
        x[torch.randint(0, n, (n // 4,), generator=g)] = 0.0
    batch = R.batch_of(SIZES)
    E = 4 * n
    src = torch.randint(0, n, (E,), generator=g)
    dst = torch.randint(0, n, (E,), generator=g)
    dst[::9] = src[::9]                                            # self loops
    ei = torch.stack([src, dst])
    ei[:, 1::11] = ei[:, 0:1]                                      # duplicates of the first edge
    return x, batch, ei


def _layer_perm_ref(pool, attn, batch_sizes):
    from mi355_mp import ops
    s = ops.pool_score(attn, pool.weight.detach())
    return s, R.topk_stable(s.cpu(), pool.ratio, batch_sizes)[0]


@pytest.mark.parametrize("F,multiplier", [(3, 1), (128, 2.5), (130, 2.5), (128, 1), (1, 2.5)])
def test_layer_is_exact_given_the_scores(F, multiplier):
    from torch_geometric.nn import TopKPooling
    x, batch, ei = _layer_case(F, 10 + F)
    n = x.shape[0]
    attr = torch.randn(ei.shape[1], 3, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(F)
    pool = TopKPooling(F, ratio=0.6, multiplier=multiplier).to(DEV)
    xd, bd = x.to(DEV), batch.to(DEV)
    xo, eo, ao, bo, perm, so = pool(xd, ei.to(DEV), attr.to(DEV), bd)
    s, perm_ref = _layer_perm_ref(pool, xd, SIZES)
    assert torch.equal(perm.cpu(), perm_ref) and perm.numel() == int(R.keep_counts(0.6, SIZES).sum())
    want = xd[perm] * s[perm].view(-1, 1)
    if multiplier != 1:
        want = multiplier * want
    assert torch.equal(xo, want)
    assert torch.equal(so, s[perm]) and torch.equal(bo, bd[perm])
    re, ra, _ = R.filter_adj(ei, attr, perm_ref, n)
    assert torch.equal(eo.cpu(), re) and torch.equal(ao.cpu(), ra) and eo.is_contiguous()
    assert 0 < re.shape[1] < ei.shape[1]


def test_filter_adj_public_function_and_bad_edge():
    from torch_geometric.nn import TopKPooling
    from torch_geometric.nn.pool import filter_adj
    x, batch, ei = _layer_case(4, 2)
    n = x.shape[0]
    g = torch.Generator().manual_seed(4)
    perm = torch.randperm(n, generator=g)[: n // 2]
    ids = torch.arange(ei.shape[1]) * 3 - 7                        # int64 [E]
    eo, ao = filter_adj(ei.to(DEV), ids.to(DEV), perm.to(DEV), n)
    re, ra, _ = R.filter_adj(ei, ids, perm, n)
    assert torch.equal(eo.cpu(), re) and torch.equal(ao.cpu(), ra) and ao.dtype == torch.int64
    eo, ao = filter_adj(ei.to(DEV), None, perm.to(DEV), n)
    assert torch.equal(eo.cpu(), re) and ao is None
    half = torch.randn(ei.shape[1], 2, 2, generator=g).half()      # a trailing shape, 2-byte elements
    eo, ao = filter_adj(ei.to(DEV), half.to(DEV), perm.to(DEV), n)
    assert torch.equal(ao.cpu(), R.filter_adj(ei, half, perm, n)[1])
    bad = ei.clone()
    bad[1, 5] = n
    with pytest.raises(IndexError):
        filter_adj(bad.to(DEV), None, perm.to(DEV), n)
    with pytest.raises(IndexError):
        TopKPooling(4).to(DEV)(x.to(DEV), bad.to(DEV), None, batch.to(DEV))


def test_layer_modes_once_each():
    from mi355_mp import ops
    from torch_geometric.nn import TopKPooling
    from torch_geometric.utils import softmax
    F = 16
    x, batch, ei = _layer_case(F, 5)
    n = x.shape[0]
    xd, bd, ed = x.to(DEV), batch.to(DEV), ei.to(DEV)
    g = torch.Generator().manual_seed(6)
    torch.manual_seed(0)
    # batch = None: one graph
    pool = TopKPooling(F, ratio=0.3).to(DEV)
    xo, eo, _, bo, perm, so = pool(xd, ed)
    s, perm_ref = _layer_perm_ref(pool, xd, [n])
    assert torch.equal(perm.cpu(), perm_ref) and torch.equal(xo, xd[perm] * s[perm].view(-1, 1))
    assert torch.equal(bo.cpu(), torch.zeros(perm.numel(), dtype=torch.int64))
    assert torch.equal(eo.cpu(), R.filter_adj(ei, None, perm_ref, n)[0])
    # a 1-D attn (in_channels = 1) and attn != x
    a1 = torch.randn(n, generator=g).to(DEV)
    pool = TopKPooling(1, ratio=0.5).to(DEV)
    xo, _, _, _, perm, so = pool(xd, ed, None, bd, attn=a1)
    s, perm_ref = _layer_perm_ref(pool, a1.view(-1, 1), SIZES)
    assert torch.equal(perm.cpu(), perm_ref) and torch.equal(xo, xd[perm] * s[perm].view(-1, 1))
    a2 = torch.randn(n, 5, generator=g).to(DEV)
    pool = TopKPooling(5, ratio=0.5).to(DEV)
    xo, _, _, _, perm, so = pool(xd, ed, None, bd, attn=a2)
    s, perm_ref = _layer_perm_ref(pool, a2, SIZES)
    assert torch.equal(perm.cpu(), perm_ref) and torch.equal(xo, xd[perm] * s[perm].view(-1, 1))
    # a callable other than torch.tanh: applied in torch to the native projection
    pool = TopKPooling(F, ratio=0.5, nonlinearity=torch.sigmoid).to(DEV)
    xo, _, _, _, perm, so = pool(xd, ed, None, bd)
    s = torch.sigmoid(ops.pool_score(xd, pool.weight.detach(), tanh=False))
    assert torch.equal(perm.cpu(), R.topk_stable(s.cpu(), 0.5, SIZES)[0])
    assert torch.equal(xo, xd[perm] * s[perm].view(-1, 1)) and torch.equal(so, s[perm])
    # min_score: against the restatement on the device's own softmax scores
    dense = [5, 9, 0, 30, 64, 70]
    xs = torch.randn(sum(dense), F, generator=g).to(DEV)
    bs = R.batch_of(dense)
    es = torch.randint(0, sum(dense), (2, 500), generator=g)
    pool = TopKPooling(F, min_score=0.02, multiplier=2).to(DEV)
    xo, eo, _, bo, perm, so = pool(xs, es.to(DEV), None, bs.to(DEV))
    s = softmax(ops.pool_score(xs, pool.weight.detach(), tanh=False, raw=True), bs.to(DEV), len(dense))
    perm_ref = R.topk_min_score(s.cpu(), 0.02, bs)
    assert 0 < perm_ref.numel() < sum(dense) and torch.equal(perm.cpu(), perm_ref)
    assert torch.equal(xo, 2 * (xs[perm] * s[perm].view(-1, 1))) and torch.equal(bo.cpu(), bs[perm_ref])
    assert torch.equal(eo.cpu(), R.filter_adj(es, None, perm_ref, sum(dense))[0])


# 4. backward -----------------------------------------------------------------

def _assert_bound(got, ref, scale, what):
    err = (got.detach().cpu().double() - ref.detach()).abs()
    ratio = float((err / scale.clamp(min=1e-300)).max())
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert float((err - BOUND * scale).max()) <= 0.0, "%s: max ratio %.3g" % (what, ratio)


@pytest.mark.parametrize("own_attn,F,multiplier", [(False, 128, 1), (True, 33, 2.5), (False, 3, 2.5)])
def test_gradients_against_float64(own_attn, F, multiplier):
    """d x, d weight, d attn, d edge_attr and a loss on score[perm], against the
    float64 restatement run with the device's perm.

    sum |terms| of each gradient = the same computation on absolute values, with
    r = inv[n], m = multiplier, z_abs = sum_f |attn_f w_f| and
    s_abs = tanh(z_abs / ||w||) (the score of the absolute inputs):
      g_s[n]    : gs_abs = m * sum_f |g_y[r, f] x[n, f]| + |g_t[r]|     (0 when dropped)
      du_n      : du_abs = gs_abs * (1 + s_abs^2)     (tanh' is evaluated as 1 - s^2: terms 1 and s^2)
      gate g_x  : m * s_abs * |g_y[r, :]|
      g_attn    : du_abs / ||w|| * |w|
      g_w       : sum_n du_abs |attn_n| / ||w|| + (sum_n du_abs z_abs) |w| / ||w||^3
    (x's gradient is the sum of the gate and attn terms when attn is x.)"""
    from torch_geometric.nn import TopKPooling
    x, batch, ei = _layer_case(F, 20 + F, zero_rows=False)
    n = x.shape[0]
    g = torch.Generator().manual_seed(8)
    fa = 7 if own_attn else F
    attn = torch.randn(n, fa, generator=g) if own_attn else None
    attr = torch.randn(ei.shape[1], 2, generator=g)
    torch.manual_seed(3)
    pool = TopKPooling(fa, ratio=0.5, multiplier=multiplier).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    ad = attn.to(DEV).requires_grad_(True) if own_attn else None
    ed = attr.to(DEV).requires_grad_(True)
    xo, eo, ao, bo, perm, so = pool(xd, ei.to(DEV), ed, batch.to(DEV), attn=ad)
    K = perm.numel()
    gy, gt, ga = torch.randn(K, F, generator=g), torch.randn(K, generator=g), torch.randn(ao.shape, generator=g)
    ((xo * gy.to(DEV)).sum() + (so * gt.to(DEV)).sum() + (ao * ga.to(DEV)).sum()).backward()

    p = perm.cpu()
    x64 = x.double().requires_grad_(True)
    a64 = attn.double().requires_grad_(True) if own_attn else None
    w64 = pool.weight.detach().cpu().double().requires_grad_(True)
    rxo, rso, s = R.layer(x64, w64, p, attn=a64, multiplier=multiplier)
    ((rxo * gy.double()).sum() + (rso * gt.double()).sum()).backward()

    gate_abs, attn_abs, w_abs = R.layer_grad_scales(x64, a64 if own_attn else x64, w64, p, gy, gt, multiplier)
    if own_attn:
        _assert_bound(xd.grad, x64.grad, gate_abs, "grad x")
        _assert_bound(ad.grad, a64.grad, attn_abs, "grad attn")
        dropped = torch.ones(n, dtype=torch.bool)
        dropped[p] = False
        assert dropped.any() and float(xd.grad.cpu()[dropped].abs().max()) == 0.0   # exact zeros from the gate
    else:
        _assert_bound(xd.grad, x64.grad, gate_abs + attn_abs, "grad x (= attn)")
    _assert_bound(pool.weight.grad.view(-1), w64.grad.view(-1), w_abs, "grad weight")
    # edge_attr: a copy forward, a scatter by out_pos backward -- exact
    keep = R.filter_adj(ei, None, p, n)[2]
    want = torch.zeros_like(attr)
    want[keep] = ga
    assert torch.equal(ed.grad.cpu(), want)


def test_raw_score_gradients():
    """The min_score path's projection <attn, w> (no norm): d attn = du * w,
    d w = sum_n du_n attn_n; sum |terms| = the same on absolute values."""
    from mi355_mp import ops
    g = torch.Generator().manual_seed(12)
    n, F = 777, 19
    attn, w, gs = torch.randn(n, F, generator=g), torch.randn(1, F, generator=g), torch.randn(n, generator=g)
    ad, wd = attn.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    (ops.pool_score(ad, wd, tanh=False, raw=True) * gs.to(DEV)).sum().backward()
    a64, w64, g64 = attn.double(), w.double(), gs.double()
    _assert_bound(ad.grad, g64.view(-1, 1) * w64, (g64.view(-1, 1) * w64).abs(), "raw grad attn")
    _assert_bound(wd.grad, (g64.view(-1, 1) * a64).sum(0, keepdim=True),
                  (g64.view(-1, 1) * a64).abs().sum(0, keepdim=True), "raw grad weight")


# 5. determinism ----------------------------------------------------------------

def test_two_runs_are_bitwise_equal():
    from torch_geometric.nn import TopKPooling
    x, batch, ei = _layer_case(128, 30)
    attr = torch.randn(ei.shape[1], 3, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(1)
    pool = TopKPooling(128, ratio=0.8, multiplier=1.5).to(DEV)
    runs = []
    for _ in range(2):
        pool.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        ed = attr.to(DEV).requires_grad_(True)
        out = pool(xd, ei.to(DEV), ed, batch.to(DEV))
        (out[0].square().sum() + out[5].sum() + out[2].square().sum()).backward()
        runs.append([t.detach().clone() for t in out] + [xd.grad.clone(), ed.grad.clone(), pool.weight.grad.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# 6. the reference's model and example --------------------------------------------

def _example():
    spec = importlib.util.spec_from_file_location("example_enzymes_topk_pool",
                                                  os.path.join(ROOT, "examples", "enzymes_topk_pool.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_three_stage_model_shapes_follow_the_keep_rule():
    from torch_geometric.data import Batch
    mod = _example()
    torch.manual_seed(0)
    data = Batch.from_data_list(mod.enzymes_like(60, 3)).to(DEV)
    model = mod.Net().to(DEV)
    model.train()
    x, ei, batch = data.x, data.edge_index, data.batch
    sizes = torch.bincount(batch.cpu(), minlength=60)
    for conv, pool in ((model.conv1, model.pool1), (model.conv2, model.pool2), (model.conv3, model.pool3)):
        x = torch.relu(conv(x, ei))
        x, ei, _, batch, perm, score = pool(x, ei, None, batch)
        sizes = R.keep_counts(0.8, sizes)
        assert torch.equal(torch.bincount(batch.cpu(), minlength=60), sizes)
        assert x.shape == (int(sizes.sum()), 128) and perm.shape == score.shape == (int(sizes.sum()),)
        assert int(ei.max()) < x.shape[0] and torch.isfinite(x).all()
    out = model(data)
    assert out.shape == (60, mod.NUM_CLASSES) and torch.isfinite(out).all()
    torch.nn.functional.nll_loss(out, data.y).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_example_enzymes_topk_pool():
    torch.manual_seed(0)
    losses = _example().main(["--epochs", "4", "--graphs", "240", "--lr", "0.005"])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


# 7. refusals -------------------------------------------------------------------

def test_debug_mode_raises_on_an_unsorted_batch():
    import torch_geometric
    from torch_geometric.nn import TopKPooling
    from torch_geometric.nn.pool import topk
    batch = torch.tensor([0, 0, 1, 0, 2], device=DEV)
    x = torch.randn(5, 4, device=DEV)
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with torch_geometric.debug():
        with pytest.raises(ValueError, match="non-decreasing"):
            TopKPooling(4).to(DEV)(x, ei, None, batch)
        with pytest.raises(ValueError, match="non-decreasing"):
            topk(x[:, 0].contiguous(), 0.5, batch)
    with pytest.raises(ValueError, match="ratio"):
        topk(x[:, 0].contiguous(), 1.5, batch)
