"""ARMAConv (PyG 1.4.3 nn.conv.arma_conv) restated in float64 on the CPU: the contract the layer
and csrc/mp_arma.hip are checked against.  absolute=True runs the same computation on |x|, |w|,
|v|, |b| (every term non-negative, the activation the identity): the sum of |terms| of the bound
|err| <= 1e-5 * sum |terms|.  masks= replaces `pre > 0`, forward and (through autograd) backward,
by given 0 / 1 tensors [K, N, C] per step.
"""
import torch

BOUND = 1e-5


def laplacian(edge_index, n, edge_weight=None):
    row, col = edge_index
    w = torch.ones(row.numel(), dtype=torch.float64) if edge_weight is None else edge_weight.double()
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, row, w)
    dinv = deg.pow(-0.5)
    dinv[dinv == float("inf")] = 0
    return dinv[row] * w * dinv[col]


def aggregate(edge_index, lap, y, transpose=False):
    """For y [K, N, C]: the sum at row of lap * y[:, col] (transpose: at col of lap * y[:, row])."""
    dst, src = (edge_index[1], edge_index[0]) if transpose else (edge_index[0], edge_index[1])
    return torch.zeros_like(y).index_add_(1, dst, y[:, src] * lap.view(1, -1, 1))


def forward(x, edge_index, edge_weight, ws, vs, bias, T, shared, act="relu", absolute=False, masks=None, drops=None):
    """(result [N, C], [H_1 .. H_T] each [K, N, C], [pre_0 .. pre_{T-1}]).  act: "relu", None or a callable;
    drops: per step, the factor F.dropout applied to x ([N, F]: 0 or 1 / (1 - p)), or None."""
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    x = f(x)
    lap = laplacian(edge_index, x.shape[0], edge_weight)
    out = x.unsqueeze(0)
    Hs, pres = [], []
    for t in range(T):
        out = torch.matmul(out, f(ws[min(t, 1) if shared else t]))
        out = aggregate(edge_index, lap, out)
        skip = x if drops is None else x * drops[t].double()
        out = out + torch.matmul(skip.unsqueeze(0), f(vs[0 if shared else t]))
        if bias is not None:
            out = out + f(bias[0 if shared else t])
        pres.append(out)
        if masks is not None:
            out = out * masks[t].double()
        elif not absolute and act is not None:
            out = out.clamp(min=0) if act == "relu" else act(out)
        Hs.append(out)
    return out.mean(dim=0), Hs, pres


def gradients(x, edge_index, edge_weight, ws, vs, bias, T, shared, g, act="relu", absolute=False, masks=None,
              drops=None):
    """d (x, ws, vs, bias) of sum(result * g) by autograd over forward() (absolute: on |values| and |g|)."""
    leaf = lambda t: (t.double().abs() if absolute else t.double()).requires_grad_(True)  # noqa: E731
    xl, wl, vl = leaf(x), [leaf(w) for w in ws], [leaf(v) for v in vs]
    bl = None if bias is None else [leaf(b) for b in bias]
    res, _, _ = forward(xl, edge_index, edge_weight, wl, vl, bl, T, shared, act, absolute, masks, drops)
    (res * (g.double().abs() if absolute else g.double())).sum().backward()
    return xl.grad, [w.grad for w in wl], [v.grad for v in vl], None if bl is None else [b.grad for b in bl]


def assert_bound(got, ref, scale, what):
    """|got - ref| <= 1e-5 * scale elementwise (scale = sum |terms|); prints and returns the largest ratio
    |err| / sum |terms| (0.0 for an empty tensor)."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(scale.shape), "%s: shapes %s / %s / %s" % (
        what, tuple(got.shape), tuple(ref.shape), tuple(scale.shape))
    assert bool(torch.isfinite(got.detach()).all()), "%s: non-finite entries" % what
    if got.numel() == 0:
        return 0.0
    err = (got.detach().cpu().double() - ref.detach()).abs()
    lim = BOUND * scale.detach()
    worst = float((err - lim).max())
    ratio = float((err / scale.detach().clamp(min=1e-300)).max())
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert worst <= 0.0, "%s: |err| exceeds 1e-5 * sum|terms| by %.3g (max ratio %.3g)" % (what, worst, ratio)
    return ratio
