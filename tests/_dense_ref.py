"""Float64 restatement of the dense family (PyG 1.4.3 nn.dense.dense_diff_pool,
nn.dense.DenseSAGEConv, utils.to_dense_batch / to_dense_adj), the checker of the
GPU tests.

    P = softmax(s, -1) * mask        T = adj P        V = adj^T P
    out = P^T (x * mask)             out_adj = P^T adj P
    q_b = sum_ij (adj_ij - p_i . p_j)^2     h_b = sum_ic -p log(p + 1e-15)
    link = sqrt(sum_b q_b) / (B N N)        ent = sum_b h_b / (B N)

`diff_pool` is vectorised and differentiable, `diff_pool_loop` is the literal
per-graph, per-entry loop it is tested against, `diff_pool_recipe` is upstream's
chain of tensor ops in whatever dtype it is given (the fp32 recipe the loss
bound is measured from), and `diff_pool_backward` states the fused backward's
formulas, which the host tests hold against float64 autograd."""
import torch

EPS = 1e-15


def _mask(mask, B, N):
    if mask is None:
        return torch.ones((B, N), dtype=torch.float64)
    return mask.reshape(B, N).double()


def _3d(t):
    return t.unsqueeze(0) if t.dim() == 2 else t


def diff_pool(x, adj, s, mask=None):
    """dict(out, out_adj, link, ent, P, T, V, q, h) in float64; differentiable."""
    x, adj, s = _3d(x).double(), _3d(adj).double(), _3d(s).double()
    B, N, _ = x.shape
    m = _mask(mask, B, N).unsqueeze(-1)
    P = torch.softmax(s, dim=-1) * m
    xm = x * m
    T = adj @ P
    V = adj.transpose(1, 2) @ P
    out = P.transpose(1, 2) @ xm
    out_adj = P.transpose(1, 2) @ T
    q = ((adj - P @ P.transpose(1, 2)) ** 2).sum(dim=(1, 2))
    h = (-P * torch.log(P + EPS)).sum(dim=(1, 2))
    link = torch.sqrt(q.sum()) / (B * N * N)
    ent = h.sum() / (B * N)
    return {"out": out, "out_adj": out_adj, "link": link, "ent": ent, "P": P, "T": T, "V": V, "q": q, "h": h}


def diff_pool_loop(x, adj, s, mask=None):
    """The same, graph by graph and entry by entry, in Python floats."""
    import math
    x, adj, s = _3d(x).double(), _3d(adj).double(), _3d(s).double()
    B, N, F = x.shape
    C = s.shape[2]
    m = _mask(mask, B, N)
    r = {k: torch.zeros(shape, dtype=torch.float64) for k, shape in
         (("out", (B, C, F)), ("out_adj", (B, C, C)), ("P", (B, N, C)), ("T", (B, N, C)), ("V", (B, N, C)),
          ("q", (B,)), ("h", (B,)))}
    for b in range(B):
        for i in range(N):
            mx = max(float(s[b, i, c]) for c in range(C))
            e = [math.exp(float(s[b, i, c]) - mx) for c in range(C)]
            den = sum(e)
            for c in range(C):
                r["P"][b, i, c] = e[c] / den * float(m[b, i])
        P = r["P"][b]
        for i in range(N):
            for c in range(C):
                r["T"][b, i, c] = sum(float(adj[b, i, j]) * float(P[j, c]) for j in range(N))
                r["V"][b, i, c] = sum(float(adj[b, j, i]) * float(P[j, c]) for j in range(N))
                r["h"][b] += -float(P[i, c]) * math.log(float(P[i, c]) + EPS)
            for j in range(N):
                d = sum(float(P[i, c]) * float(P[j, c]) for c in range(C))
                r["q"][b] += (float(adj[b, i, j]) - d) ** 2
        for c in range(C):
            for f in range(F):
                r["out"][b, c, f] = sum(float(P[n, c]) * float(x[b, n, f]) * float(m[b, n]) for n in range(N))
            for c2 in range(C):
                r["out_adj"][b, c, c2] = sum(float(P[n, c]) * float(r["T"][b, n, c2]) for n in range(N))
    r["link"] = torch.sqrt(r["q"].sum()) / (B * N * N)
    r["ent"] = r["h"].sum() / (B * N)
    return r


def diff_pool_recipe(x, adj, s, mask=None):
    """Upstream's dense_diff_pool, op for op, in the dtype of its inputs:
    (out, out_adj, link_loss, ent_loss)."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    s = s.unsqueeze(0) if s.dim() == 2 else s
    batch_size, num_nodes, _ = x.size()
    s = torch.softmax(s, dim=-1)
    if mask is not None:
        mask = mask.view(batch_size, num_nodes, 1).to(x.dtype)
        x, s = x * mask, s * mask
    out = torch.matmul(s.transpose(1, 2), x)
    out_adj = torch.matmul(torch.matmul(s.transpose(1, 2), adj), s)
    link_loss = adj - torch.matmul(s, s.transpose(1, 2))
    link_loss = torch.norm(link_loss, p=2)
    link_loss = link_loss / adj.numel()
    ent_loss = (-s * torch.log(s + EPS)).sum(dim=-1).mean()
    return out, out_adj, link_loss, ent_loss


def diff_pool_grads(x, adj, s, mask, g_out, g_oa, gl, ge, adj_grad=False):
    """dict(dx, ds[, dadj]) of sum(out * g_out) + sum(out_adj * g_oa) + gl * link +
    ge * ent, float64 autograd through diff_pool."""
    xr = _3d(x).double().clone().requires_grad_(True)
    sr = _3d(s).double().clone().requires_grad_(True)
    ar = _3d(adj).double().clone().requires_grad_(adj_grad)
    r = diff_pool(xr, ar, sr, mask)
    obj = (r["out"] * g_out.double()).sum() + (r["out_adj"] * g_oa.double()).sum() + ge * r["ent"]
    if gl:                                   # sqrt has no derivative at 0: gl = 0 leaves the link term out entirely
        obj = obj + gl * r["link"]
    obj.backward()
    res = {"dx": xr.grad if xr.grad is not None else torch.zeros_like(xr),
           "ds": sr.grad if sr.grad is not None else torch.zeros_like(sr)}
    if adj_grad:
        res["dadj"] = ar.grad
    return res


def diff_pool_backward(x, mask, P, T, V, q_sum, g_out, g_oa, gl, ge):
    """(dx, ds) by the fused backward's formulas, from what the forward saves."""
    x, P, T, V, g_out, g_oa = (t.double() for t in (_3d(x), P, T, V, g_out, g_oa))
    B, N, _ = x.shape
    m = _mask(mask, B, N).unsqueeze(-1)
    q_sum = float(q_sum)
    k = gl / (q_sum ** 0.5 * B * N * N) if q_sum > 0 else 0.0
    G = P.transpose(1, 2) @ P
    dP = (x * m) @ g_out.transpose(1, 2) + T @ g_oa.transpose(1, 2) + V @ g_oa - k * (T + V - 2 * P @ G) \
        - (ge / (B * N)) * (torch.log(P + EPS) + P / (P + EPS))
    ds = P * (dP - (dP * P).sum(-1, keepdim=True))
    dx = m * (P @ g_out)
    return dx, ds


def mean_agg(x, adj, add_loop=True):
    """(agg, deg): agg[b, i] = sum_j A^_ij x_j / max(sum_j A^_ij, 1), A^ = adj with
    its diagonal set to 1 when add_loop.  float64, differentiable in x."""
    x, adj = _3d(x).double(), _3d(adj).double()
    B, N, _ = adj.shape
    if add_loop:
        eye = torch.eye(N, dtype=torch.float64).unsqueeze(0)
        adj = adj * (1 - eye) + eye
    deg = adj.sum(-1)
    return (adj @ x) / deg.clamp(min=1).unsqueeze(-1), deg


def mean_agg_loop(x, adj, add_loop=True):
    x, adj = _3d(x).double(), _3d(adj).double()
    B, N, F = x.shape
    agg = torch.zeros((B, N, F), dtype=torch.float64)
    deg = torch.zeros((B, N), dtype=torch.float64)
    for b in range(B):
        for i in range(N):
            row = [1.0 if (add_loop and i == j) else float(adj[b, i, j]) for j in range(N)]
            deg[b, i] = sum(row)
            for f in range(F):
                agg[b, i, f] = sum(row[j] * float(x[b, j, f]) for j in range(N)) / max(float(deg[b, i]), 1.0)
    return agg, deg


def dense_sage(x, adj, weight, bias=None, mask=None, add_loop=True, normalize=False):
    """DenseSAGEConv.forward in float64: mean_agg @ W + b, normalised, masked."""
    out = mean_agg(x, adj, add_loop)[0] @ weight.double()
    if bias is not None:
        out = out + bias.double()
    if normalize:
        out = torch.nn.functional.normalize(out, p=2, dim=-1)
    if mask is not None:
        out = out * mask.reshape(out.shape[0], out.shape[1], 1).double()
    return out


def to_dense_batch(x, starts, fill_value=0.0, max_n=None):
    """(dense [B, Nmax, ...], mask [B, Nmax] bool) of rows grouped by segment starts."""
    starts = [int(v) for v in starts]
    B = len(starts) - 1
    sizes = [starts[g + 1] - starts[g] for g in range(B)]
    Nmax = max(sizes + [0]) if max_n is None else max_n
    dense = torch.full((B, Nmax) + tuple(x.shape[1:]), fill_value, dtype=x.dtype)
    mask = torch.zeros((B, Nmax), dtype=torch.bool)
    for g in range(B):
        for i in range(sizes[g]):
            dense[g, i] = x[starts[g] + i]
            mask[g, i] = True
    return dense, mask


def to_dense_adj(edge_index, starts, batch=None, edge_attr=None, max_n=None):
    """[B, Nmax, Nmax] (ones) or [B, Nmax, Nmax, D]; the last edge of a cell wins."""
    starts = [int(v) for v in starts]
    B = len(starts) - 1
    sizes = [starts[g + 1] - starts[g] for g in range(B)]
    Nmax = max(sizes + [0]) if max_n is None else max_n
    tail = () if edge_attr is None else tuple(edge_attr.reshape(edge_attr.shape[0], -1).shape[1:])
    out = torch.zeros((B, Nmax, Nmax) + tail, dtype=torch.float32 if edge_attr is None else edge_attr.dtype)
    for e in range(edge_index.shape[1]):
        r, c = int(edge_index[0, e]), int(edge_index[1, e])
        g = 0 if batch is None else int(batch[r])
        out[g, r - starts[g], c - starts[g]] = 1.0 if edge_attr is None else edge_attr.reshape(
            edge_attr.shape[0], -1)[e]
    return out
