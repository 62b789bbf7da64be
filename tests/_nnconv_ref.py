"""NNConv restated per edge in torch float64 (the checker of the NNConv tests).

Per edge e = (j -> i) with h_e = trunk(edge_attr_e) in R^H, the input of the
edge network's last Linear (head: weight [Cin*Cout, H], bias [Cin*Cout] or None):

    W_e   = reshape(head.weight @ h_e + head.bias, [Cin, Cout])     materialised
    m_e   = x_j @ W_e                                               one mat-vec
    out_i = AGGR_e m_e  (add; mean: / max(deg, 1); max: 0 for empty rows and
            for values < -10000)  + x_i @ root + bias

nn_conv is that, vectorised over the edges; nn_conv_loop is the literal loop.
The kernel contracts are restated next to it: with ht_e = [h_e, 1] in R^(H+1)

    bins      Z[r, h*Cin + c] = scale[r] * sum_{e -> r} ht_e[h] * x[j_e, c]
    gather    out[r, f]       = scale[r] * sum_{e -> r} sum_h ht_e[h] * y[j_e, h*F + f] (+ bias[f])
    edge_grad dh[e, h]        = sum_c dz[i_e, h*Cin + c] * x[j_e, c]          for h < H

and head_matrix builds L [(H+1)*Cin, Cout] with L[h*Cin + c, o] =
head.weight[c*Cout + o, h] and the rows h = H holding head.bias, so that
sum_e m_e = Z @ L.  Each function takes absolute inputs for sum |terms|, the
scale of the project's bound |err| <= 1e-5 * sum |terms|.
"""
import torch

BOUND = 1e-5


def _cols(t):
    return t.view(-1, 1) if t.dim() == 1 else t


def head_matrix(head_w, head_b, c_in, c_out):
    """L [(H+1)*Cin, Cout] of head.weight [Cin*Cout, H] and head.bias (None: a zero row block)."""
    H = head_w.shape[1]
    top = head_w.double().view(c_in, c_out, H).permute(2, 0, 1).reshape(H * c_in, c_out)
    last = torch.zeros(c_in, c_out, dtype=torch.float64) if head_b is None else head_b.double().view(c_in, c_out)
    return torch.cat([top, last], dim=0)


def gather_matrix(L, H, c_in, c_out):
    """L' [Cin, (H+1)*Cout] with L'[c, h*Cout + o] = L[h*Cin + c, o]."""
    return L.view(H + 1, c_in, c_out).permute(1, 0, 2).reshape(c_in, (H + 1) * c_out)


def _ht(h):
    h = _cols(h).double()
    return torch.cat([h, torch.ones(h.shape[0], 1, dtype=torch.float64)], dim=1)


def bins(edge_dst, edge_src, n_rows, h, x, row_scale=None):
    ht, x = _ht(h), _cols(x).double()
    terms = ht[:, :, None] * x[edge_src][:, None, :]                   # [E, H+1, Cin]
    Z = torch.zeros(n_rows, terms.shape[1] * terms.shape[2], dtype=torch.float64)
    Z = Z.index_add(0, edge_dst, terms.reshape(terms.shape[0], Z.shape[1]))
    return Z if row_scale is None else Z * row_scale.double().view(-1, 1)


def gather(edge_dst, edge_src, n_rows, h, y, F, row_scale=None, bias=None):
    ht = _ht(h)
    y = y.double().view(y.shape[0], ht.shape[1], F)
    out = torch.zeros(n_rows, F, dtype=torch.float64)
    out = out.index_add(0, edge_dst, torch.einsum("eh,ehf->ef", ht, y[edge_src]))
    if row_scale is not None:
        out = out * row_scale.double().view(-1, 1)
    if bias is not None:
        out = out + bias.double()
    return out


def edge_grad(edge_dst, edge_src, dz, x, H):
    x = _cols(x).double()
    dz = dz.double().view(dz.shape[0], -1, x.shape[1])[:, :H]          # [n, H, Cin]
    return torch.einsum("ehc,ec->eh", dz[edge_dst], x[edge_src])


def _aggregate(msg, dst, n, aggr):
    if aggr == "max":
        out = torch.full((n, msg.shape[1]), float("-inf"), dtype=torch.float64)
        out = out.scatter_reduce(0, dst.view(-1, 1).expand_as(msg), msg, "amax", include_self=True)
        return torch.where(out < -10000, torch.zeros_like(out), out)
    out = torch.zeros(n, msg.shape[1], dtype=torch.float64).index_add(0, dst, msg)
    if aggr == "mean":
        out = out / torch.bincount(dst, minlength=n).clamp(min=1).double().view(-1, 1)
    return out


def nn_conv(x, edge_index, h, head_w, head_b, c_in, c_out, root=None, bias=None, aggr="add",
            flow="source_to_target", absolute=False):
    """The layer in float64 (CPU; every tensor argument may require grad).  h [E, H]
    is the head's input; a head-less edge network passes its output as
    head_w = None, h = nn(edge_attr) [E, Cin*Cout].  absolute: the same on
    absolute values (add / mean): sum |terms|."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    conv = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    x, h = conv(_cols(x)), conv(_cols(h))
    dst, src = edge_index[i], edge_index[j]
    if head_w is None:
        W = h
    else:
        W = h @ conv(head_w).t()
        if head_b is not None:
            W = W + conv(head_b)
    W = W.view(-1, c_in, c_out)                                         # materialised [E, Cin, Cout]
    msg = torch.matmul(x[src].unsqueeze(1), W).squeeze(1)
    out = _aggregate(msg, dst, x.shape[0], aggr)
    if root is not None:
        out = out + x @ conv(root)
    if bias is not None:
        out = out + conv(bias)
    return out


def nn_conv_loop(x, edge_index, h, head_w, head_b, c_in, c_out, root=None, bias=None, aggr="add",
                 flow="source_to_target"):
    """nn_conv as the literal loop over the edges (no autograd use)."""
    i, j = (1, 0) if flow == "source_to_target" else (0, 1)
    x, h = _cols(x).double(), _cols(h).double()
    n = x.shape[0]
    out = torch.zeros(n, c_out, dtype=torch.float64)
    seen = torch.zeros(n, dtype=torch.int64)
    for e in range(edge_index.shape[1]):
        r, c = int(edge_index[i, e]), int(edge_index[j, e])
        w = head_w.double() @ h[e]
        if head_b is not None:
            w = w + head_b.double()
        m = x[c] @ w.view(c_in, c_out)
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
