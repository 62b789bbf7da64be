"""GMMConv restated in torch float64 (the checker of the GMMConv tests).

PyG 1.4.3 nn.conv.GMMConv.  With Cin, M = Cout, D = dim, K = kernel_size and
EPS = 1e-15, per edge e = (j -> i) with pseudo-coordinates p_e in R^D:

shared Gaussians (mu, sigma [K, D]; g [Cin, K*M], column index k*M + m)
    w[e, k] = exp(sum_d -0.5 (p[e, d] - mu[k, d])^2 / (EPS + sigma[k, d]^2))
    m_e     = sum_k w[e, k] * (x_j @ g)[k*M : (k+1)*M]
separate Gaussians (mu, sigma [Cin, M, K, D]; g [Cin, M*K], column index m*K + k)
    w[e, c, m, k] as above,  W_e[c, m] = sum_k g[c, m*K + k] * w[e, c, m, k],  m_e = x_j @ W_e
    out_i = AGGR_e m_e (add; mean: / max(deg, 1); max: 0 for empty rows)  + x_i @ root + bias

gmm_conv is that, vectorised over the edges; gmm_conv_loop is the literal loop.
The kernel contracts are restated next to it (iv = 1 / (EPS + sigma^2)):

    bins        Z[r, k*Cin + c] = scale[r] * sum_{e -> r} w[e, k] * x[j_e, c]
    gather      out[r, f]       = scale[r] * sum_{e -> r} sum_k w[e, k] * y[j_e, k*F + f] (+ bias[f])
    param_grad  dw[e, k] = sum_c dz[i_e, k*Cin + c] * x[j_e, c],  t = dw * w
                dmu[k, d]     = sum_e t (p_d - mu_kd) iv_kd
                dsigma[k, d]  = sum_e t ((p_d - mu_kd)^2 iv_kd) (sigma_kd iv_kd)
                dpseudo[e, d] = -sum_k t (p_d - mu_kd) iv_kd
                (an (edge, k) with w == 0 contributes exactly zero)

and mix_matrix builds G' [K*Cin, M] with G'[k*Cin + c, m] = g[c, k*M + m], so
that sum_e m_e = Z @ G'.  Each function takes absolute inputs for sum |terms|,
the scale of the project's bound |err| <= 1e-5 * sum |terms|.
"""
import torch

BOUND = 1e-5
EPS = 1e-15


def _cols(t):
    return t.view(-1, 1) if t.dim() == 1 else t


def weights(pseudo, mu, sigma):
    """w [E, K] (shared: mu [K, D]) or [E, Cin, M, K] (separate: mu [Cin, M, K, D]) in float64."""
    p = _cols(pseudo).double()
    mu, sigma = mu.double(), sigma.double()
    p = p.view((p.shape[0],) + (1,) * (mu.dim() - 1) + (p.shape[1],))
    q = -0.5 * (p - mu.unsqueeze(0)).pow(2) / (EPS + sigma.unsqueeze(0).pow(2))
    return torch.exp(q.sum(dim=-1))


def mix_matrix(g, K, c_in, c_out):
    """G' [K*Cin, M] with G'[k*Cin + c, m] = g[c, k*M + m]."""
    return g.double().view(c_in, K, c_out).permute(1, 0, 2).reshape(K * c_in, c_out)


def bins(edge_dst, edge_src, n_rows, pseudo, mu, sigma, x, row_scale=None, absolute=False):
    w, x = weights(pseudo, mu, sigma), _cols(x).double()
    if absolute:
        x = x.abs()
    terms = w[:, :, None] * x[edge_src][:, None, :]                    # [E, K, Cin]
    Z = torch.zeros(n_rows, terms.shape[1] * terms.shape[2], dtype=torch.float64)
    Z = Z.index_add(0, edge_dst, terms.reshape(terms.shape[0], Z.shape[1]))
    if row_scale is None:
        return Z
    return Z * (row_scale.double().abs() if absolute else row_scale.double()).view(-1, 1)


def gather(edge_dst, edge_src, n_rows, pseudo, mu, sigma, y, F, row_scale=None, bias=None, absolute=False):
    w = weights(pseudo, mu, sigma)
    conv = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    y = conv(y).view(y.shape[0], w.shape[1], F)
    out = torch.zeros(n_rows, F, dtype=torch.float64)
    out = out.index_add(0, edge_dst, torch.einsum("ek,ekf->ef", w, y[edge_src]))
    if row_scale is not None:
        out = out * conv(row_scale).view(-1, 1)
    if bias is not None:
        out = out + conv(bias)
    return out


def param_grad(edge_dst, edge_src, pseudo, mu, sigma, dz, x, absolute=False):
    """(dmu, dsigma, dpseudo) by the closed forms above, float64; absolute: sum |terms|."""
    p, mu, sigma = _cols(pseudo).double(), mu.double(), sigma.double()
    x = _cols(x).double()
    K, D = mu.shape
    w = weights(p, mu, sigma)                                           # [E, K]
    dzr = dz.double().view(dz.shape[0], K, x.shape[1])[edge_dst]       # [E, K, Cin]
    if absolute:
        dw = torch.einsum("ekc,ec->ek", dzr.abs(), x[edge_src].abs())
    else:
        dw = torch.einsum("ekc,ec->ek", dzr, x[edge_src])
    t = dw * w
    iv = 1.0 / (EPS + sigma.pow(2))
    df = p[:, None, :] - mu[None]                                       # [E, K, D]
    a = df * iv[None]
    live = (w != 0)[:, :, None]
    tm = torch.where(live, t[:, :, None] * a, torch.zeros_like(a))
    ts = torch.where(live, t[:, :, None] * (df * a) * (sigma * iv)[None], torch.zeros_like(a))
    if absolute:
        return tm.abs().sum(0), ts.abs().sum(0), tm.abs().sum(1)
    return tm.sum(0), ts.sum(0), -tm.sum(1)


def _aggregate(msg, dst, n, aggr):
    if aggr == "max":
        out = torch.full((n, msg.shape[1]), float("-inf"), dtype=torch.float64)
        out = out.scatter_reduce(0, dst.view(-1, 1).expand_as(msg), msg, "amax", include_self=True)
        return torch.where(out < -10000, torch.zeros_like(out), out)
    out = torch.zeros(n, msg.shape[1], dtype=torch.float64).index_add(0, dst, msg)
    if aggr == "mean":
        out = out / torch.bincount(dst, minlength=n).clamp(min=1).double().view(-1, 1)
    return out


def gmm_conv(x, edge_index, pseudo, g, mu, sigma, K, root=None, bias=None, aggr="mean", flow="source_to_target",
             absolute=False):
    """The layer in float64 (CPU; every tensor argument may require grad).  mu of
    2 dims: shared Gaussians, of 4: separate.  absolute: the same on absolute
    values of x, g, root and bias (add / mean): sum |terms|."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    conv = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    x = conv(_cols(x))
    dst, src = edge_index[i], edge_index[j]
    c_in = x.shape[1]
    c_out = g.shape[1] // K
    w = weights(pseudo, mu, sigma)
    if mu.dim() == 2:
        Y = (x @ conv(g)).view(-1, K, c_out)
        msg = (w[:, :, None] * Y[src]).sum(dim=1)
    else:
        W = (w * conv(g).view(1, c_in, c_out, K)).sum(dim=-1)           # [E, Cin, M]
        msg = torch.matmul(x[src].unsqueeze(1), W).squeeze(1)
    out = _aggregate(msg, dst, x.shape[0], aggr)
    if root is not None:
        out = out + x @ conv(root)
    if bias is not None:
        out = out + conv(bias)
    return out


def gmm_conv_loop(x, edge_index, pseudo, g, mu, sigma, K, root=None, bias=None, aggr="mean",
                  flow="source_to_target"):
    """gmm_conv as the literal loop over the edges (no autograd use)."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    x, p = _cols(x).double(), _cols(pseudo).double()
    g, mu, sigma = g.double(), mu.double(), sigma.double()
    n, c_in = x.shape
    c_out = g.shape[1] // K
    D = p.shape[1]
    out = torch.zeros(n, c_out, dtype=torch.float64)
    seen = torch.zeros(n, dtype=torch.int64)
    for e in range(edge_index.shape[1]):
        r, c = int(edge_index[i, e]), int(edge_index[j, e])
        m = torch.zeros(c_out, dtype=torch.float64)
        if mu.dim() == 2:
            y = x[c] @ g
            for k in range(K):
                q = sum(-0.5 * (p[e, d] - mu[k, d]) ** 2 / (EPS + sigma[k, d] ** 2) for d in range(D))
                m = m + torch.exp(q) * y[k * c_out:(k + 1) * c_out]
        else:
            for ci in range(c_in):
                for mo in range(c_out):
                    s = 0.0
                    for k in range(K):
                        q = sum(-0.5 * (p[e, d] - mu[ci, mo, k, d]) ** 2 / (EPS + sigma[ci, mo, k, d] ** 2)
                                for d in range(D))
                        s = s + g[ci, mo * K + k] * torch.exp(q)
                    m[mo] = m[mo] + x[c, ci] * s
        if aggr == "max":
            out[r] = m if seen[r] == 0 else torch.maximum(out[r], m)
        else:
            out[r] += m
        seen[r] += 1
    if aggr == "mean":
        out = out / seen.clamp(min=1).double().view(-1, 1)
    if aggr == "max":
        out = torch.where(out < -10000, torch.zeros_like(out), out)
    if root is not None:
        out = out + x @ root.double()
    if bias is not None:
        out = out + bias.double()
    return out


def gmm_form(K, D, c_in, c_out, E, N):
    """The floats each form moves, restated: ('bins' | 'gather', bins count, gather count)."""
    b = E * (D + c_in) + 2 * N * K * c_in
    g = E * (D + K * c_out) + N * K * c_out
    return ("bins" if b <= g else "gather"), b, g


def assert_bound(got, ref, scale, what):
    """|got - ref| <= 1e-5 * scale elementwise (scale = sum |terms|); prints the largest ratio."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(scale.shape), "%s: shapes %s / %s / %s" % (
        what, tuple(got.shape), tuple(ref.shape), tuple(scale.shape))
    err = (got.detach().cpu().double() - ref.detach()).abs()
    if not err.numel():
        return
    assert bool(torch.isfinite(got.detach()).all()), "%s: non-finite entries" % what
    lim = BOUND * scale.detach()
    worst = float((err - lim).max())
    ratio = float((err / scale.detach().clamp(min=1e-300)).max())
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert worst <= 0.0, "%s: |err| exceeds 1e-5 * sum|terms| by %.3g (max ratio %.3g)" % (what, worst, ratio)
