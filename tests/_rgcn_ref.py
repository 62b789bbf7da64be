"""RGCNConv restated per edge in torch float64 (the checker of the RGCN tests).

Per edge e = (j -> i) of relation t_e with norm n_e (None: 1), basis [B, Cin,
Cout] and att [R, B]:

    W_r   = sum_b att[r, b] basis[b]                                materialised
    m_e   = n_e x_j @ W_{t_e}        (x = None: row j of W_{t_e}, Cin = N)
    out_i = sum_e m_e + x_i @ root (x = None: + root) + bias

rgcn_conv is that, vectorised over the edges; rgcn_conv_loop is the literal
loop.  The kernel contracts are restated next to it, with a_e = n_e att[t_e, :]:

    bins      Z[r, b, c]  = sum_{e -> r} a_e[b] * x[j_e, c]
    gather    out[r, f]   = sum_{e -> r} sum_b a_e[b] * y[j_e, b, f] (+ bias[f])
    att_grad  datt[r, b]  = sum_{e: t_e = r} n_e * sum_c P[rows_e, b, c] * Q[cols_e, c]

Z, y and P are [n, B, C] here; the tests lay them out node-major ([n, B*C]) or
block-major ([B, n, C]) for the kernels.  Each function takes absolute inputs
for sum |terms|, the scale of the project's bound |err| <= 1e-5 * sum |terms|.
"""
import torch

BOUND = 1e-5


def _coef(edge_type, edge_norm, att):
    a = att.double()[edge_type]                                        # [E, B]
    return a if edge_norm is None else a * edge_norm.double().view(-1, 1)


def bins(edge_dst, edge_src, n_rows, edge_type, edge_norm, att, x):
    """Z [n_rows, B, C]."""
    a, x = _coef(edge_type, edge_norm, att), x.double()
    terms = a[:, :, None] * x[edge_src][:, None, :]
    return torch.zeros(n_rows, a.shape[1], x.shape[1], dtype=torch.float64).index_add(0, edge_dst, terms)


def gather(edge_dst, edge_src, n_rows, edge_type, edge_norm, att, y, bias=None):
    """out [n_rows, F] of y [n, B, F]."""
    a = _coef(edge_type, edge_norm, att)
    out = torch.zeros(n_rows, y.shape[2], dtype=torch.float64)
    out = out.index_add(0, edge_dst, torch.einsum("eb,ebf->ef", a, y.double()[edge_src]))
    return out if bias is None else out + bias.double()


def att_grad(edge_type, edge_norm, rows, cols, P, Q, R):
    """datt [R, B] of P [n, B, C] and Q [m, C]."""
    per_edge = torch.einsum("ebc,ec->eb", P.double()[rows], Q.double()[cols])
    if edge_norm is not None:
        per_edge = per_edge * edge_norm.double().view(-1, 1)
    return torch.zeros(R, P.shape[1], dtype=torch.float64).index_add(0, edge_type, per_edge)


def rgcn_conv(x, edge_index, edge_type, edge_norm, basis, att, root=None, bias=None, flow="source_to_target",
              absolute=False):
    """The layer in float64 (CPU; every float argument may require grad).  x None:
    the featureless layer.  absolute: the same on absolute values: sum |terms|."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    conv = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    dst, src = edge_index[i], edge_index[j]
    basis, att = conv(basis), conv(att)
    B, c_in, c_out = basis.shape
    W = (att @ basis.view(B, -1)).view(-1, c_in, c_out)                 # materialised [R, Cin, Cout]
    if x is None:
        n = c_in
        msg = W[edge_type, src]
    else:
        x = conv(x)
        n = x.shape[0]
        msg = torch.matmul(x[src].unsqueeze(1), W[edge_type]).squeeze(1)
    if edge_norm is not None:
        msg = msg * conv(edge_norm).view(-1, 1)
    out = torch.zeros(n, c_out, dtype=torch.float64).index_add(0, dst, msg)
    if root is not None:
        out = out + (conv(root) if x is None else x @ conv(root))
    if bias is not None:
        out = out + conv(bias)
    return out


def rgcn_conv_loop(x, edge_index, edge_type, edge_norm, basis, att, root=None, bias=None, flow="source_to_target"):
    """rgcn_conv as the literal loop over the edges (no autograd use)."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    basis, att = basis.double(), att.double()
    B, c_in, c_out = basis.shape
    n = c_in if x is None else x.shape[0]
    out = torch.zeros(n, c_out, dtype=torch.float64)
    for e in range(edge_index.shape[1]):
        r, c, t = int(edge_index[i, e]), int(edge_index[j, e]), int(edge_type[e])
        W = torch.zeros(c_in, c_out, dtype=torch.float64)
        for b in range(B):
            W += att[t, b] * basis[b]
        m = W[c] if x is None else x[c].double() @ W
        out[r] += m if edge_norm is None else m * float(edge_norm[e])
    if root is not None:
        out = out + (root.double() if x is None else x.double() @ root.double())
    if bias is not None:
        out = out + bias.double()
    return out


def assert_bound(got, ref, scale, what):
    """|got - ref| <= 1e-5 * scale elementwise (scale = sum |terms|); prints the largest ratio."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(scale.shape), "%s: shapes %s / %s / %s" % (
        what, tuple(got.shape), tuple(ref.shape), tuple(scale.shape))
    err = (got.detach().cpu().double() - ref.detach()).abs()
    if not err.numel():
        return
    lim = BOUND * scale.detach()
    worst = float((err - lim).max())
    ratio = float((err / scale.detach().clamp(min=1e-300)).max())
    print("%s: max |err| / sum|terms| = %.3g" % (what, ratio))
    assert worst <= 0.0, "%s: |err| exceeds 1e-5 * sum|terms| by %.3g (max ratio %.3g)" % (what, worst, ratio)
