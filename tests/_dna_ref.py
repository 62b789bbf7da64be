"""Float64 restatement of DNAConv (PyG 1.4.3 nn.conv.dna_conv [U]) for the tests.

Per edge e = (j -> i) and head h (a d = C / H wide slice of the channels):

    q   = lin_q(x_i[T-1])[h]        k_t = lin_k(x_j[t])[h]       v_t = lin_v(x_j[t])[h]
    s_t = q . k_t / sqrt(d)
    m   = max(0, max_t s_t);  a_t = exp(s_t - m) / (sum_u exp(s_u - m) + exp(-m))
    a~_t = keep_t a_t / (1 - p)                                   (attention dropout)
    msg_e[h] = norm_e sum_t a~_t v_t;    out_i = sum_{e -> i} msg_e

Four forms of it:
  dna_conv_recipe   upstream's order: gather x_i, x_j per edge, project per edge
                    with the grouped Linears, the clamp form of the softmax
  dna_conv          the factored form the fused path computes: Q, K, V once per
                    node, then `attention` (the softmax as the ordinary one over
                    {0, s_1 .. s_T} with its first entry dropped)
  dna_conv_loop     a literal loop over edges, heads and t
  attention_backward  the backward the kernels implement, written out

and the `absolute` mode: sum |terms| of out, d Q, d K, d V -- every product by
its magnitude, a_t itself (a positive weight computed from the signed scores)
kept, |ds_t| taken as a_t (|d alpha_t| + sum_u a_u |d alpha_u|) -- carried through
absolute-valued grouped GEMMs to the scales of d x, d weight and d bias
(`layer`).  The GPU tests bound |err| by 1e-5 * that.
"""
import math

import torch

BOUND = 1e-5
F64 = torch.float64


def gcn_norm(edge_index, n, edge_weight=None, absolute=False):
    """GCNConv.norm: add_remaining_self_loops (kept edges in order, then the loops
    0..n-1; a node's loop keeps the weight of its LAST existing loop, else 1),
    deg over row, norm = deg^-1/2[row] w deg^-1/2[col].  Differentiable in
    edge_weight.  Returns (edge_index', norm).  absolute: the same values, with a
    backward that adds the magnitudes of its terms (deg^-1/2 is replaced by 2 c -
    deg^-1/2, c its own value as a constant: the same number, the derivative with
    the opposite sign, so that no two terms of d edge_weight cancel)."""
    row, col = edge_index[0], edge_index[1]
    E = row.numel()
    w = torch.ones(E, dtype=F64) if edge_weight is None else edge_weight.to(F64)
    keep = row != col
    lpos = torch.full((n,), -1, dtype=torch.int64)
    for e in torch.nonzero(~keep).flatten().tolist():
        lpos[int(row[e])] = e
    loop_w = torch.where(lpos >= 0, w[lpos.clamp(min=0)] if E else torch.ones(n, dtype=F64), torch.ones(n, dtype=F64))
    ar = torch.arange(n, dtype=edge_index.dtype)
    ei = torch.cat([edge_index[:, keep], torch.stack([ar, ar])], dim=1)
    w2 = torch.cat([w[keep], loop_w])
    deg = torch.zeros(n, dtype=F64).index_add(0, ei[0], w2)
    dinv = deg.pow(-0.5)
    if absolute:
        dinv = 2.0 * dinv.detach() - dinv
    dinv = dinv.masked_fill(deg == 0, 0)
    return ei, dinv[ei[0]] * w2 * dinv[ei[1]]


def linear(src, weight, bias):
    """The grouped Linear: output group g = src[..., g * in/G:(g + 1) * in/G] @ weight[g], + bias."""
    G, cin, cout = weight.shape
    lead = src.shape[:-1]
    s = src.reshape(-1, G, cin)
    out = torch.einsum("ngi,gio->ngo", s, weight).reshape(*lead, G * cout)
    return out if bias is None else out + bias


def softmax_clamp(s):
    """restricted_softmax(s, dim=-1, margin=0) as upstream writes it."""
    m = torch.clamp(s.max(dim=-1, keepdim=True)[0], min=0)
    out = (s - m).exp()
    return out / (out.sum(dim=-1, keepdim=True) + (0 - m).exp())


def softmax_extended(s):
    """The same: the ordinary softmax over {0, s_1 .. s_T} without its first entry."""
    z = torch.zeros(s.shape[:-1] + (1,), dtype=s.dtype)
    return torch.softmax(torch.cat([z, s], dim=-1), dim=-1)[..., 1:]


def _ends(edge_index, flow):
    """(dst, src) of every edge."""
    return (edge_index[1], edge_index[0]) if flow == "source_to_target" else (edge_index[0], edge_index[1])


def _heads(t, idx, heads):
    """[n, T, C] (or [n, C]) gathered at idx as [E, H, T, d] (or [E, H, 1, d])."""
    t = t[idx]
    if t.dim() == 2:
        t = t.unsqueeze(1)
    E, T, C = t.shape
    return t.reshape(E, T, heads, C // heads).transpose(1, 2)


def _keep_scale(keep, p):
    return 1.0 if keep is None else keep.to(F64) / (1.0 - p)


def scores(q, k, dst, src, heads):
    """s [E, H, T] of the signed q [n, C], k [n, T, C]."""
    d = q.shape[1] // heads
    return (_heads(q, dst, heads) * _heads(k, src, heads)).sum(-1) / math.sqrt(d)


def attention(q, k, v, norm, dst, src, n, heads, keep=None, p=0.0, a=None):
    """The kernel contract of the forward: q [n, C], k, v [n, T, C], norm [E],
    keep None or bool [E, H, T] -> out [n, C].  a: the coefficients to use
    (the absolute mode passes those of the signed scores)."""
    q, k, v, norm = q.to(F64), k.to(F64), v.to(F64), norm.to(F64)
    if a is None:
        a = softmax_extended(scores(q, k, dst, src, heads))
    at = a * _keep_scale(keep, p)
    msg = (at.unsqueeze(-1) * _heads(v, src, heads)).sum(2)           # [E, H, d]
    msg = msg.reshape(msg.shape[0], -1) * norm.view(-1, 1)
    return torch.zeros(n, q.shape[1], dtype=F64).index_add(0, dst, msg)


def attention_backward(q, k, v, norm, dst, src, n, heads, g, keep=None, p=0.0, absolute=False, mags=None):
    """(d Q, d K, d V) of sum(out * g), as the kernels compute them: do = norm_e g_i,
    d v_t += a~_t do, d alpha_t = keep_t scale <do, v_t>, ds_t = a_t (d alpha_t - sum_u a_u
    d alpha_u), d q += ds_t k_t / sqrt(d), d k_t += ds_t q / sqrt(d).  absolute: sum |terms|
    (a from the signed q, k; mags = the magnitudes (|q|, |k|, |v|) to use, default the
    operands' own)."""
    q, k, v, norm, g = q.to(F64), k.to(F64), v.to(F64), norm.to(F64), g.to(F64)
    T, C = k.shape[1], k.shape[2]
    d = C // heads
    a = softmax_extended(scores(q, k, dst, src, heads))
    if absolute:
        q, k, v = (q.abs(), k.abs(), v.abs()) if mags is None else [t.to(F64) for t in mags]
        norm, g = norm.abs(), g.abs()
    ks = _keep_scale(keep, p)
    do = _heads(g, dst, heads) * norm.view(-1, 1, 1, 1)              # [E, H, 1, d]
    dv_e = (a * ks).unsqueeze(-1) * do                               # [E, H, T, d]
    dal = ks * (do * _heads(v, src, heads)).sum(-1)                  # [E, H, T]
    tot = (a * dal).sum(-1, keepdim=True)
    ds = a * (dal + tot) if absolute else a * (dal - tot)
    dq_e = (ds.unsqueeze(-1) * _heads(k, src, heads)).sum(2) / math.sqrt(d)      # [E, H, d]
    dk_e = ds.unsqueeze(-1) * _heads(q, dst, heads) / math.sqrt(d)               # [E, H, T, d]
    E = dst.numel()
    dQ = torch.zeros(n, C, dtype=F64).index_add(0, dst, dq_e.reshape(E, C))
    dK = torch.zeros(n, T, C, dtype=F64).index_add(0, src, dk_e.transpose(1, 2).reshape(E, T, C))
    dV = torch.zeros(n, T, C, dtype=F64).index_add(0, src, dv_e.transpose(1, 2).reshape(E, T, C))
    return dQ, dK, dV


def attention_abs(q, k, v, norm, dst, src, n, heads, keep=None, p=0.0, v_mag=None):
    """sum |terms| of attention's out: sum_e |norm_e| sum_t a~_t |v_t|."""
    a = softmax_extended(scores(q.to(F64), k.to(F64), dst, src, heads))
    vm = v.to(F64).abs() if v_mag is None else v_mag.to(F64)
    return attention(q, k, vm, norm.to(F64).abs(), dst, src, n, heads, keep, p, a=a)


def project(x, params):
    """(Q [n, C], K, V [n, T, C]) of x [n, T, C]; params: wq, bq, wk, bk, wv, bv (biases may be None)."""
    return (linear(x[:, -1], params["wq"], params.get("bq")), linear(x, params["wk"], params.get("bk")),
            linear(x, params["wv"], params.get("bv")))


def dna_conv(x, edge_index, norm, params, heads, flow="source_to_target", keep=None, p=0.0):
    """The factored form: node-level projections, then the attention."""
    dst, src = _ends(edge_index, flow)
    q, k, v = project(x.to(F64), {n: (None if t is None else t.to(F64)) for n, t in params.items()})
    return attention(q, k, v, norm, dst, src, x.shape[0], heads, keep, p)


def dna_conv_recipe(x, edge_index, norm, params, heads, flow="source_to_target", keep=None, p=0.0):
    """Upstream's message and aggregation, step by step: x_i[:, -1:] and x_j
    gathered per edge, projected per edge, the clamp form of the softmax."""
    prm = {n: (None if t is None else t.to(F64)) for n, t in params.items()}
    x = x.to(F64)
    dst, src = _ends(edge_index, flow)
    x_i, x_j = x[dst][:, -1:], x[src]                                 # [E, 1, C], [E, T, C]
    query, key, value = (linear(x_i, prm["wq"], prm.get("bq")), linear(x_j, prm["wk"], prm.get("bk")),
                         linear(x_j, prm["wv"], prm.get("bv")))
    E, T, C = key.shape
    d = C // heads
    query = query.view(E, 1, heads, d).transpose(-2, -3)
    key = key.view(E, T, heads, d).transpose(-2, -3)
    value = value.view(E, T, heads, d).transpose(-2, -3)
    score = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(d)     # [E, H, 1, T]
    score = softmax_clamp(score)
    if keep is not None:
        score = score * (keep.to(F64) / (1.0 - p)).unsqueeze(2)
    out = torch.matmul(score, value).transpose(-3, -2).contiguous().view(E, C)
    return torch.zeros(x.shape[0], C, dtype=F64).index_add(0, dst, norm.to(F64).view(-1, 1) * out)


def dna_conv_loop(x, edge_index, norm, params, heads, flow="source_to_target", keep=None, p=0.0):
    """A literal loop over edges, heads and t."""
    prm = {n: (None if t is None else t.to(F64)) for n, t in params.items()}
    x = x.to(F64)
    n, T, C = x.shape
    d = C // heads
    dst, src = _ends(edge_index, flow)
    out = torch.zeros(n, C, dtype=F64)
    for e in range(dst.numel()):
        i, j = int(dst[e]), int(src[e])
        q = linear(x[i, T - 1], prm["wq"], prm.get("bq"))
        kk = [linear(x[j, t], prm["wk"], prm.get("bk")) for t in range(T)]
        vv = [linear(x[j, t], prm["wv"], prm.get("bv")) for t in range(T)]
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = [float(q[sl] @ kk[t][sl]) / math.sqrt(d) for t in range(T)]
            m = max(0.0, max(s))
            den = sum(math.exp(v - m) for v in s) + math.exp(-m)
            for t in range(T):
                a = math.exp(s[t] - m) / den
                if keep is not None:
                    a = a / (1.0 - p) if bool(keep[e, h, t]) else 0.0
                out[i, sl] += float(norm[e]) * a * vv[t][sl]
    return out


PARAMS = ("wq", "bq", "wk", "bk", "wv", "bv")


def layer(x, edge_index, norm, params, heads, flow="source_to_target", keep=None, p=0.0, gout=None, absolute=False):
    """(out, grads or None) of the layer on float64 copies; grads (with gout): d x and
    d of every entry of params that is not None, of sum(out * gout).  absolute: the
    sum |terms| scales instead -- attention_abs / attention_backward(absolute) on
    the magnitudes Q~ = |x| |W_q| + |b_q| (K~, V~ alike) with a from the signed
    projections, then the absolute-valued grouped GEMMs' backward."""
    dst, src = _ends(edge_index, flow)
    n = x.shape[0]
    cvt = (lambda t: t.detach().to(F64).abs()) if absolute else (lambda t: t.detach().to(F64))
    leaves = {k: cvt(v).requires_grad_(True) for k, v in params.items() if v is not None}
    leaves["x"] = cvt(x).requires_grad_(True)
    q, k, v = project(leaves["x"], leaves)
    nrm = norm.detach().to(F64)
    if not absolute:
        out = attention(q, k, v, nrm, dst, src, n, heads, keep, p)
        if gout is None:
            return out.detach(), None
        (out * gout.to(F64)).sum().backward()
    else:
        sq, sk, sv = project(x.detach().to(F64), {k_: (None if t is None else t.detach().to(F64))
                                                  for k_, t in params.items()})
        out = attention_abs(sq, sk, sv, nrm, dst, src, n, heads, keep, p, v_mag=v.detach())
        if gout is None:
            return out.detach(), None
        dq, dk, dv = attention_backward(sq, sk, sv, nrm, dst, src, n, heads, gout, keep, p, absolute=True,
                                        mags=(q.detach(), k.detach(), v.detach()))
        ((q * dq).sum() + (k * dk).sum() + (v * dv).sum()).backward()
    return out.detach(), {k_: t.grad for k_, t in leaves.items()}


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
