"""SplineConv restated per edge in torch float64 (the checker of the spline tests).

Per edge e = (j -> i) with pseudo-coordinates u[e, 0..D) in [0, 1], kernel sizes
ks[d], open flags op[d], degree M and S = (M+1)^D:

    for s in 0..S:  k = s; b = 1; wi = 0; off = 1
      for d in 0..D:
        km = k % (M+1); k //= (M+1)
        v  = u[e,d] * float(ks[d] - M*op[d])        # ONE fp32 multiply
        wi += ((int(floor(v)) + km) % ks[d]) * off;  off *= ks[d]
        f  = v - floor(v);  b *= B_M(f, km)
      basis[e,s] = b; weight_index[e,s] = wi

    m_e   = sum_s basis[e,s] * x_j W[weight_index[e,s]]          W [K, Fin, Fout]
    out_i = AGGR_e m_e (mean: / max(deg, 1)) + x_i root + bias

v and floor(v) are computed in float32 exactly as above, so weight_index is
comparable exactly; f and the basis are float64 from that v.  Everything is
differentiable in x, W, root and bias.  Each function also has an `abs` form
(the same computation on |x|, |W|, ...; the basis is >= 0 for degrees 1..3)
giving sum |terms|, the scale of the project's error bound
|err| <= 1e-5 * sum |terms|.
"""
import torch


def _bspline(f, k, M):
    if M == 1:
        return 1 - f - k + 2 * f * k
    if M == 2:
        return (0.5 * f * f - f + 0.5, -f * f + f + 0.5, 0.5 * f * f)[k]
    return ((1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6,
            f ** 3 / 6)[k]


def basis(pseudo, kernel_size, is_open_spline, degree):
    """(basis [E, S] float64, weight_index [E, S] int64) of float32 pseudo [E, D] (CPU)."""
    pseudo = pseudo.detach().cpu().to(torch.float32)
    pseudo = pseudo.view(-1, 1) if pseudo.dim() == 1 else pseudo
    E, D = pseudo.shape
    M = int(degree)
    ks = [int(k) for k in kernel_size]
    op = [int(bool(o)) for o in is_open_spline]
    S = (M + 1) ** D
    span = torch.tensor([float(ks[d] - M * op[d]) for d in range(D)], dtype=torch.float32)
    v = pseudo * span                               # one fp32 multiply per entry
    fl = torch.floor(v)
    f = v.double() - fl.double()
    fi = fl.to(torch.int64)
    b = torch.ones(E, S, dtype=torch.float64)
    wi = torch.zeros(E, S, dtype=torch.int64)
    for s in range(S):
        k, off = s, 1
        for d in range(D):
            km = k % (M + 1)
            k //= M + 1
            wi[:, s] += ((fi[:, d] + km) % ks[d]) * off
            off *= ks[d]
            b[:, s] = b[:, s] * _bspline(f[:, d], km, M)
    return b, wi


def bins(edge_dst, edge_src, n_rows, b, wi, K, x, row_scale=None):
    """A[i, k*F + f] = scale[i] * sum_e sum_{s: wi = k} b[e,s] * x[j, f] (float64)."""
    x = x.double()
    F = x.shape[1]
    A = torch.zeros(n_rows * K, F, dtype=torch.float64)
    for s in range(b.shape[1]):
        A = A.index_add(0, edge_dst * K + wi[:, s], b[:, s:s + 1] * x[edge_src])
    A = A.view(n_rows, K * F)
    if row_scale is not None:
        A = A * row_scale.double().view(-1, 1)
    return A


def gather(edge_dst, edge_src, n_rows, b, wi, K, xk, F, row_scale=None, bias=None):
    """out[i, f] = scale[i] * sum_e sum_s b[e,s] * xk[j, wi[e,s]*F + f] (+ bias) (float64)."""
    xk = xk.double().view(xk.shape[0], K, F)
    out = torch.zeros(n_rows, F, dtype=torch.float64)
    for s in range(b.shape[1]):
        out = out.index_add(0, edge_dst, b[:, s:s + 1] * xk[edge_src, wi[:, s]])
    if row_scale is not None:
        out = out * row_scale.double().view(-1, 1)
    if bias is not None:
        out = out + bias.double()
    return out


def spline_conv(x, edge_index, pseudo, weight, root, bias, kernel_size, is_open_spline, degree, aggr="mean",
                flow="source_to_target", absolute=False):
    """The layer in float64 (CPU tensors; x / weight / root / bias may require
    grad).  absolute: the same on |x|, |W|, |root|, |bias|: sum |terms|."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    conv = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    x = conv(x)
    x = x.view(-1, 1) if x.dim() == 1 else x
    weight = conv(weight)
    n = x.shape[0]
    b, wi = basis(pseudo, kernel_size, is_open_spline, degree)
    dst, src = edge_index[i], edge_index[j]
    K, f_in, f_out = weight.shape
    xw = torch.einsum("nf,kfo->nko", x, weight)                 # [n, K, Fout]
    out = torch.zeros(n, f_out, dtype=torch.float64)
    for s in range(b.shape[1]):
        out = out.index_add(0, dst, b[:, s:s + 1] * xw[src, wi[:, s]])
    if aggr == "mean":
        deg = torch.bincount(dst, minlength=n).clamp(min=1).double()
        out = out / deg.view(-1, 1)
    if root is not None:
        out = out + x @ conv(root)
    if bias is not None:
        out = out + conv(bias)
    return out


BOUND = 1e-5


def assert_bound(got, ref, scale, what):
    """|got - ref| <= 1e-5 * scale elementwise (scale = sum |terms|); prints the largest ratio."""
    err = (got.detach().cpu().double() - ref.detach()).abs()
    if not err.numel():
        return
    lim = BOUND * scale.detach()
    worst = float((err - lim).max())
    ratio = float((err / scale.detach().clamp(min=1e-300)).max())
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert worst <= 0.0, "%s: |err| exceeds 1e-5 * sum|terms| by %.3g (max ratio %.3g)" % (what, worst, ratio)


def abs_grad_scale(weight, root, bias, x, ei, u, ks, op, M, aggr, gout, flow="source_to_target"):
    """sum |terms| of every gradient, {"x", "weight", "root", "bias"} (root / bias
    when given): the float64 autograd of the restatement on absolute inputs with
    |grad_out| (all terms >= 0, so the gradient of the absolute computation is
    the sum of the terms' magnitudes)."""
    leaves = {"x": x, "weight": weight, "root": root, "bias": bias}
    leaves = {k: v.detach().cpu().abs().double().clone().requires_grad_(True) for k, v in leaves.items()
              if v is not None}
    out = spline_conv(leaves["x"], ei, u, leaves["weight"], leaves.get("root"), leaves.get("bias"), ks, op, M, aggr,
                      flow)
    (out * gout.double().abs()).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
