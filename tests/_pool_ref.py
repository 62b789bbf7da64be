"""CPU restatement of TopKPooling (PyG 1.4.3 nn.pool.topk_pool [U]) that the
pooling tests check the kernels against.  Three pieces:

  * topk_dense: the upstream recipe as it stands -- a dense [G, max_nodes] copy
    of the scores padded with the lowest float, one descending sort per row, and
    the first k_g columns of every row.  Its order among equal scores is
    whatever torch.sort gives, i.e. unspecified.
  * topk_stable: the same selection per graph through
    torch.sort(descending=True, stable=True): among equal scores the lower node
    index first.  This fixes the project's tie rule.
  * layer: the layer's arithmetic in float64, differentiable, with perm given.

k_g = ceil(fl32(ratio) * fl32(n_g)) in float32, as upstream's
(ratio * num_nodes.to(torch.float)).ceil().
"""
import torch


def keep_counts(ratio, sizes):
    """k_g of every graph size: one float32 multiply, then ceil."""
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    return (ratio * sizes.to(torch.float)).ceil().to(torch.int64)


def batch_of(sizes):
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(len(sizes)), sizes)


def topk_dense(score, ratio, batch):
    """The dense-sort recipe on CPU tensors (batch non-decreasing, every id used
    or not: an unused id is an empty row)."""
    G = int(batch.max()) + 1 if batch.numel() else 0
    if G == 0:
        return torch.empty(0, dtype=torch.int64)
    sizes = torch.bincount(batch, minlength=G)
    width = int(sizes.max())
    first = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]])
    slot = torch.arange(batch.numel()) - first[batch] + batch * width
    dense = score.new_full((G * width,), torch.finfo(score.dtype).min)
    dense[slot] = score
    order = dense.view(G, width).sort(dim=-1, descending=True)[1] + first.view(-1, 1)
    order = order.view(-1)
    k = keep_counts(ratio, sizes)
    take = torch.cat([torch.arange(int(k[g])) + g * width for g in range(G)])
    return order[take]


def topk_stable(score, ratio, sizes):
    """(perm, out_starts): per graph a stable descending sort, first k_g kept."""
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    k = keep_counts(ratio, sizes)
    parts, s0 = [], 0
    for n_g, k_g in zip(sizes.tolist(), k.tolist()):
        order = torch.sort(score[s0:s0 + n_g], descending=True, stable=True)[1]
        parts.append(order[:k_g] + s0)
        s0 += n_g
    perm = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64)
    return perm, torch.cat([k.new_zeros(1), k.cumsum(0)])


def topk_min_score(score, min_score, batch, tol=1e-7):
    """nonzero(score > min(max_g(score) - tol, min_score)), ascending."""
    G = int(batch.max()) + 1
    mx = torch.full((G,), -float("inf"), dtype=score.dtype)
    for g in range(G):
        seg = score[batch == g]
        if seg.numel():
            mx[g] = seg.max()
    thr = (mx[batch] - tol).clamp(max=min_score)
    return (score > thr).nonzero().view(-1)


def filter_adj(edge_index, edge_attr, perm, num_nodes):
    """Edges between kept nodes in original order, relabelled by position in perm."""
    inv = torch.full((num_nodes,), -1, dtype=torch.int64)
    inv[perm] = torch.arange(perm.numel())
    row, col = inv[edge_index[0]], inv[edge_index[1]]
    keep = (row >= 0) & (col >= 0)
    out = torch.stack([row[keep], col[keep]])
    return out, (None if edge_attr is None else edge_attr[keep]), keep.nonzero().view(-1)


def segment_softmax(z, batch):
    G = int(batch.max()) + 1
    out = torch.empty_like(z)
    for g in range(G):
        m = batch == g
        if m.any():
            e = (z[m] - z[m].max()).exp()
            out[m] = e / (e.sum() + 1e-16)
    return out


def score(attn, weight, nonlinearity=torch.tanh, min_score=None, batch=None):
    """The full score vector in the dtype of its inputs (float64 in the tests)."""
    attn = attn.unsqueeze(-1) if attn.dim() == 1 else attn
    z = (attn * weight).sum(-1)
    if min_score is None:
        return nonlinearity(z / weight.norm(p=2, dim=-1))
    return segment_softmax(z, batch)


def layer(x, weight, perm, attn=None, multiplier=1, nonlinearity=torch.tanh, min_score=None, batch=None):
    """(x_out, score[perm], score) with perm given; differentiable."""
    s = score(x if attn is None else attn, weight, nonlinearity, min_score, batch)
    x_out = x[perm] * s[perm].view(-1, 1)
    if multiplier != 1:
        x_out = multiplier * x_out
    return x_out, s[perm], s


def distinct_scores(m, generator):
    """m distinct float32 values in (-1, 1): tanh(randn) repeats values in fp32."""
    return ((torch.randperm(m, generator=generator).float() + 0.5) / m * 2 - 1)


def layer_grad_scales(x, attn, weight, perm, gy, gt, multiplier):
    """sum |terms| of the layer's gradients for the loss <x_out, gy> + <score[perm], gt>:
    (gate_abs [n, F], attn_abs [n, Fa], w_abs [Fa]), the same computation on absolute
    values.  x [n, F], attn [n, Fa] (x itself when the layer scores x) and weight are
    float64; with r = inv[n], m = multiplier, z_abs = sum_f |attn_f w_f| and
    s_abs = tanh(z_abs / ||w||) (the score of the absolute inputs):
      g_s[n]    : gs_abs = m * sum_f |g_y[r, f] x[n, f]| + |g_t[r]|     (0 when dropped)
      du_n      : du_abs = gs_abs * (1 + s_abs^2)     (tanh' is evaluated as 1 - s^2: terms 1 and s^2)
      gate g_x  : m * s_abs * |g_y[r, :]|
      g_attn    : du_abs / ||w|| * |w|
      g_w       : sum_n du_abs |attn_n| / ||w|| + (sum_n du_abs z_abs) |w| / ||w||^3
    (x's gradient is the sum of the gate and attn terms when attn is x.)"""
    with torch.no_grad():
        n, F = x.shape
        m = float(multiplier)
        att = attn.detach()
        w = weight.detach().view(-1)
        nrm = w.norm()
        gy_n = torch.zeros(n, F, dtype=torch.float64)
        gy_n[perm] = gy.double().abs()
        gt_n = torch.zeros(n, dtype=torch.float64)
        gt_n[perm] = gt.double().abs()
        z_abs = (att * w).abs().sum(-1)
        s_abs = torch.tanh(z_abs / nrm)
        gs_abs = m * (gy_n * x.detach().abs()).sum(-1) + gt_n
        du_abs = gs_abs * (1 + s_abs ** 2)
        gate_abs = m * s_abs.view(-1, 1) * gy_n
        attn_abs = du_abs.view(-1, 1) / nrm * w.abs().view(1, -1)
        w_abs = (du_abs.view(-1, 1) * att.abs()).sum(0) / nrm + (du_abs * z_abs).sum() * w.abs() / nrm ** 3
    return gate_abs, attn_abs, w_abs
