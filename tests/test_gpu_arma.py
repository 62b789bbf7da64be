"""ARMAConv on the GPU against the float64 restatement tests/_arma_ref.py, every comparison at
|err| <= 1e-5 * sum |terms|.  The graph: 257 nodes, ~3000 directed edges with duplicates, node 5 with
700 edges at `row` (split over tasks, finished in the fix-up), nodes 200.. never at `row`, nodes 230..
isolated, edge weights in [0.5, 1.5)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _arma_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 257
# (K, C, T, shared, F): the example's shape; a stack boundary inside a lane's vector with
# distinct weights per step; no mean and no in-kernel transform; K * C = 256
CASES = [(3, 16, 2, True, 33), (3, 7, 3, False, 16), (1, 64, 1, False, 5), (8, 32, 2, True, 9)]


@functools.lru_cache(maxsize=None)
def _graph():
    g = torch.Generator().manual_seed(1)
    row = torch.randint(0, 200, (2300,), generator=g)
    col = torch.randint(0, 230, (2300,), generator=g)
    ei = torch.stack([row, col])
    hub = torch.stack([torch.full((700,), 5, dtype=torch.int64), torch.randint(0, 230, (700,), generator=g)])
    ei = torch.cat([ei, ei[:, :40], hub], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    assert int(torch.bincount(ei[0], minlength=N)[5]) >= 700 and int(ei[0].max()) < 200 and int(ei.max()) < 230
    return ei, torch.rand(ei.shape[1], generator=g) + 0.5


@functools.lru_cache(maxsize=None)
def _case(case, act, weighted=True):
    """Inputs, the layer on the GPU and the reference's answers for one case, computed once."""
    from torch_geometric.nn import ARMAConv
    K, C, T, shared, Fin = case
    ei, ew = _graph()
    ew = ew if weighted else None
    g = torch.Generator().manual_seed(K * 1000 + C * 10 + T)
    x = torch.randn(N, Fin, generator=g)
    layer = ARMAConv(Fin, C, K, T, shared_weights=shared, act=F.relu if act == "relu" else act)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    ws, vs, bias = [p.detach().clone() for p in layer.ws], [p.detach().clone() for p in layer.vs], \
        [p.detach().clone() for p in layer.bias]
    args = (x, ei, ew, ws, vs, bias, T, shared)
    ref, absv = R.forward(*args, act), R.forward(*args, act, absolute=True)
    return dict(x=x, ei=ei, ew=ew, args=args, ref=ref, abs=absv, gout=torch.randn(N, C, generator=g),
                layer=layer.to(DEV))


def _k(h, K, C):
    """A stacked [N, P] operand as the reference's float64 [K, N, C]."""
    return h[:, :K * C].reshape(-1, K, C).permute(1, 0, 2).cpu().double()


def _stacked(h, K, C):
    """_k of a kernel's output, whose padding columns must be zeros."""
    assert float(h[:, K * C:].abs().sum()) == 0.0
    return _k(h, K, C)


def _nan_rows(K, C, fill=False, n=N):
    """A NaN-filled [n, P] buffer (an unwritten element fails every comparison); fill: random valid columns."""
    from mi355_mp import ops
    t = torch.full((n, ops.arma_width(K, C)), float("nan"), device=DEV)
    if fill:
        t[:, :K * C] = torch.randn(n, K * C, device=DEV)
    return t


def check_forward_steps(edges, graph, lap, K, C, act, w_nexts=(None,), lap64=None, what=""):
    """Single forward steps (ops.arma_step) into NaN-filled outputs against the reference's aggregation, one per
    entry of w_nexts: a [K, C, C] next transform (the result is Y_{t+1}) or None (the last step: the mean over
    the stacks).  edges: the CPU edge_index; graph: keyed on edges[0]; lap: fp32 [E] on the device in edge
    order; lap64: the reference's weights (default: lap itself).  Returns the largest |err| / sum |terms|."""
    from mi355_mp import ops
    n = graph.n_dst
    lap64 = lap.cpu().double() if lap64 is None else lap64
    Y, S = _nan_rows(K, C, True, n), _nan_rows(K, C, True, n)
    pre = R.aggregate(edges, lap64, _k(Y, K, C)) + _k(S, K, C)
    pre_abs = R.aggregate(edges, lap64, _k(Y, K, C).abs()) + _k(S, K, C).abs()
    h_ref = pre.clamp(min=0) if act else pre
    worst = 0.0
    for w in w_nexts:
        o, h = ops.arma_step(graph.dst, graph.dst.to_csr_order(lap), Y, S, K, C, act is not None, w,
                             out=_nan_rows(K, C, n=n)[:, :C].contiguous() if w is None else _nan_rows(K, C, n=n),
                             hidden=_nan_rows(K, C, n=n))
        worst = max(worst, R.assert_bound(_stacked(h, K, C), h_ref, pre_abs, "step H %s" % (what,)))
        if w is None:
            worst = max(worst, R.assert_bound(o, h_ref.mean(0), pre_abs.mean(0), "step out %s" % (what,)))
        else:
            w64 = w.cpu().double()
            worst = max(worst, R.assert_bound(_stacked(o, K, C), h_ref @ w64, pre_abs @ w64.abs(),
                                              "step Y %s" % (what,)))
    return worst


def check_backward_step(edges, graph, lap, K, C, act, w=None, h=None, lap64=None, what=""):
    """One backward step (ops.arma_step_backward) into NaN-filled outputs against the reference's transposed
    aggregation; w [K, C, C]: the step's transform (dPre of the step before is checked too), h: with act and
    w, the stacked hidden state whose sign is the mask.  Returns the largest |err| / sum |terms|."""
    from mi355_mp import ops
    n = graph.n_src
    lap64 = lap.cpu().double() if lap64 is None else lap64
    masked = bool(act) and w is not None and h is not None
    dpre = _nan_rows(K, C, True, n)
    dy, prev = ops.arma_step_backward(graph.src, graph.src.to_csr_order(lap), dpre, K, C,
                                      None if w is None else w.transpose(1, 2), h if masked else None,
                                      dy=_nan_rows(K, C, n=n), out=None if w is None else _nan_rows(K, C, n=n))
    dy_ref = R.aggregate(edges, lap64, _k(dpre, K, C), True)
    dy_abs = R.aggregate(edges, lap64, _k(dpre, K, C).abs(), True)
    worst = R.assert_bound(_stacked(dy, K, C), dy_ref, dy_abs, "step dY %s" % (what,))
    if w is not None:
        wt, m = w.cpu().double().transpose(1, 2), ((_k(h, K, C) > 0) if masked else 1)
        worst = max(worst, R.assert_bound(_stacked(prev, K, C), (dy_ref @ wt) * m, (dy_abs @ wt.abs()) * m,
                                          "step dPre %s" % (what,)))
    return worst


def _gpu_masks(Hs, pres, abs_pres, K, C):
    """The GPU's ReLU masks, for the reference's backward (the gradient jumps at the kink): the reference's own
    wherever its pre-activation is clear of zero by the bound, and at most 0.5 % of its elements are not clear."""
    masks = [_stacked(h, K, C) > 0 for h in Hs]
    close = 0
    for m, pre, a in zip(masks, pres, abs_pres):
        clear = pre.abs() > R.BOUND * a
        assert torch.equal(m[clear], (pre > 0)[clear])
        close += int((~clear).sum())
    assert close <= 0.005 * sum(m.numel() for m in masks), "%d pre-activations within the bound of zero" % close
    return masks


def _propagate(c, case, act, want_hidden=True):
    from mi355_mp import ops
    from mi355_mp.graph import graph_for
    K, C, T, shared, _ = case
    layer, ei = c["layer"], c["ei"].to(DEV)
    graph = graph_for(ei, N, N, "target_to_source")
    lap = ops.arma_laplacian(graph, None if c["ew"] is None else c["ew"].to(DEV))
    return ops.arma_propagate(graph, c["x"].to(DEV), list(layer.ws), list(layer.vs), list(layer.bias), K, C, T, shared,
                              act is not None, 0.0, False, want_hidden=want_hidden, lap=lap), graph, lap


@pytest.mark.parametrize("act", ["relu", None])
@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_reference(case, act):
    K, C, T, shared, _ = case
    c = _case(case, act)
    (out, Hs), graph, lap = _propagate(c, case, act)
    (r_out, r_H, _), (a_out, a_H, _) = c["ref"], c["abs"]
    R.assert_bound(out, r_out, a_out, "out %s" % (case,))
    for t in range(T):
        R.assert_bound(_stacked(Hs[t], K, C), r_H[t], a_H[t], "H_%d %s" % (t + 1, case))
    (out2, Hs2), _, _ = _propagate(c, case, act)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(Hs, Hs2))
    assert torch.equal(c["layer"](c["x"].to(DEV), c["ei"].to(DEV), c["ew"].to(DEV), form="fused"), out)
    # single steps into NaN-filled outputs: the last step and, with T > 1, one with the in-kernel transform
    check_forward_steps(c["ei"], graph, lap, K, C, act, [c["layer"].ws[1].detach(), None] if T > 1 else [None],
                        lap64=R.laplacian(c["ei"], N, c["ew"]), what=case)


@pytest.mark.parametrize("act", ["relu", None])
@pytest.mark.parametrize("case", CASES)
def test_backward_matches_the_reference(case, act):
    K, C, T, shared, _ = case
    c = _case(case, act)
    layer = c["layer"]
    layer.zero_grad()
    x = c["x"].to(DEV).requires_grad_(True)
    (_, Hs), graph, lap = _propagate(c, case, act)
    layer(x, c["ei"].to(DEV), c["ew"].to(DEV), form="fused").backward(c["gout"].to(DEV))
    # one backward step into NaN-filled outputs against the reference's transposed aggregation
    check_backward_step(c["ei"], graph, lap, K, C, act, layer.ws[1].detach() if T > 1 else None, Hs[0],
                        lap64=R.laplacian(c["ei"], N, c["ew"]), what=case)
    masks = _gpu_masks(Hs, c["ref"][2], c["abs"][2], K, C) if act == "relu" else None
    args = c["args"] + (c["gout"],)
    ref = R.gradients(*args, act=act, masks=masks)
    absv = R.gradients(*args, act=act, masks=masks, absolute=True)
    R.assert_bound(x.grad, ref[0], absv[0], "d x %s" % (case,))
    for name, params, i in (("ws", layer.ws, 1), ("vs", layer.vs, 2), ("bias", layer.bias, 3)):
        for j, p in enumerate(params):
            R.assert_bound(p.grad, ref[i][j], absv[i][j], "d %s[%d] %s" % (name, j, case))


def test_dropout_draws_the_masks_of_the_recipe(monkeypatch):
    from mi355_mp import ops
    from mi355_mp.graph import graph_for
    case = CASES[0]
    K, C, T, shared, Fin = case
    c = _case(case, "relu")
    layer, x, ei, ew = c["layer"], c["x"].to(DEV), c["ei"].to(DEV), c["ew"].to(DEV)
    monkeypatch.setattr(layer, "dropout", 0.25)
    layer.train()
    torch.manual_seed(7)
    drops = [F.dropout(torch.ones(N, Fin, device=DEV), 0.25, True).cpu() for _ in range(T)]
    got = {}
    for form in ("fused", "unfused"):
        layer.zero_grad()
        xg = x.clone().requires_grad_(True)
        torch.manual_seed(7)
        out = layer(xg, ei, ew, form=form)
        out.backward(c["gout"].to(DEV))
        got[form] = [out, xg.grad] + [p.grad.clone() for p in layer.parameters()]
    r_out, _, r_pre = R.forward(*c["args"], drops=drops)
    a_out, _, a_pre = R.forward(*c["args"], drops=drops, absolute=True)
    torch.manual_seed(7)
    masks = _gpu_masks(ops.arma_propagate(graph_for(ei, N, N, "target_to_source"), x, list(layer.ws),
                                          list(layer.vs), list(layer.bias), K, C, T, shared, True, 0.25, True,
                                          want_hidden=True, edge_weight=ew)[1], r_pre, a_pre, K, C)
    args = c["args"] + (c["gout"],)
    ref = R.gradients(*args, masks=masks, drops=drops)
    absv = R.gradients(*args, masks=masks, drops=drops, absolute=True)
    flat = lambda r: [r[0]] + list(r[1]) + list(r[2]) + list(r[3])  # noqa: E731  (the order of parameters())
    for form in ("fused", "unfused"):
        R.assert_bound(got[form][0], r_out, a_out, "dropout out %s" % form)
        for i, (gr, rr, ar) in enumerate(zip(got[form][1:], flat(ref), flat(absv))):
            R.assert_bound(gr, rr, ar, "dropout grad %d %s" % (i, form))
    layer.eval()                                                      # eval mode: bitwise the p = 0 result
    e = layer(x, ei, ew, form="fused")
    layer.dropout = 0.0
    assert torch.equal(e, layer(x, ei, ew, form="fused"))


@pytest.mark.parametrize("K,C,act", [(4, 64, "relu"), (3, 16, torch.tanh)])
def test_shapes_and_activations_outside_the_fused_path_take_the_recipe(K, C, act):
    from mi355_mp import ops
    c = _case((K, C, 2, True, 6), act)
    layer, x, ei, ew = c["layer"], c["x"].to(DEV), c["ei"].to(DEV), c["ew"].to(DEV)
    assert ops.arma_ok(K, C) == (act != "relu") and not layer.fused(x, ew)
    R.assert_bound(layer(x, ei, ew), c["ref"][0], c["abs"][0], "recipe K=%d C=%d" % (K, C))
    with pytest.raises(ValueError):
        layer(x, ei, ew, form="fused")


def test_unweighted_edges_and_an_edge_weight_that_needs_a_gradient():
    u = _case(CASES[1], "relu", False)                                # edge_weight None: the degree by counting
    R.assert_bound(u["layer"](u["x"].to(DEV), u["ei"].to(DEV), form="fused"), u["ref"][0], u["abs"][0], "unweighted")
    c = _case(CASES[0], "relu")
    layer, x, ei = c["layer"], c["x"].to(DEV), c["ei"].to(DEV)
    ew = c["ew"].to(DEV).requires_grad_(True)
    assert layer.fused(x, ew.detach()) and not layer.fused(x, ew)
    with pytest.raises(ValueError):
        layer(x, ei, ew, form="fused")
    layer(x, ei, ew).sum().backward()
    assert ew.grad is not None and bool(torch.isfinite(ew.grad).all())
