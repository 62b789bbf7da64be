"""Float64 restatement of the attention readout and the two layers built on it
(PyG 1.4.3 nn.glob.Set2Set / GlobalAttention), the checker of the GPU tests.

    e_n = x_n . q[g(n)]  or  score[n]
    m_g = max e_n, den_g = sum exp(e_n - m_g), a_n = exp(e_n - m_g) / den_g
    r_g = sum a_n x_n            (a graph without nodes: r = 0, m = den = 0)

Graphs are segment starts [G + 1].  `readout` is vectorised, `readout_loop` is
the literal per-graph loop it is tested against; gradients come from float64
autograd through `readout`."""
import torch


def _batch_of(starts):
    starts = torch.as_tensor(starts, dtype=torch.int64)
    counts = starts[1:] - starts[:-1]
    return torch.repeat_interleave(torch.arange(counts.numel()), counts), counts


def readout(x, starts, q=None, score=None):
    """(r [G, C], e [N], m [G], den [G], a [N]) in float64; differentiable."""
    assert (q is None) != (score is None)
    x = x.double()
    batch, counts = _batch_of(starts)
    G = counts.numel()
    n0 = int(torch.as_tensor(starts)[0])
    xs = x[n0:n0 + batch.numel()]
    if q is not None:
        e = (xs * q.double()[batch]).sum(-1)
    else:
        e = score.double().reshape(-1)[n0:n0 + batch.numel()]
    m = torch.full((G,), -float("inf"), dtype=torch.float64)
    m = m.scatter_reduce(0, batch, e.detach(), "amax", include_self=True)
    m = torch.where(counts > 0, m, torch.zeros_like(m))
    p = (e - m[batch]).exp()
    den = torch.zeros(G, dtype=torch.float64).index_add(0, batch, p)
    a = p / den[batch]
    r = torch.zeros((G, x.shape[1]), dtype=torch.float64).index_add(0, batch, a[:, None] * xs)
    return r, e, m, den, a


def readout_loop(x, starts, q=None, score=None):
    """The same five, graph by graph and node by node."""
    x = x.double()
    starts = [int(s) for s in starts]
    G, C = len(starts) - 1, x.shape[1]
    r = torch.zeros((G, C), dtype=torch.float64)
    m = torch.zeros(G, dtype=torch.float64)
    den = torch.zeros(G, dtype=torch.float64)
    e = torch.zeros(starts[-1] - starts[0], dtype=torch.float64)
    a = torch.zeros_like(e)
    for g in range(G):
        b, t = starts[g], starts[g + 1]
        if b == t:
            continue
        for n in range(b, t):
            if q is not None:
                e[n - starts[0]] = sum(float(x[n, c]) * float(q[g, c]) for c in range(C))
            else:
                e[n - starts[0]] = float(score.reshape(-1)[n])
        eg = e[b - starts[0]:t - starts[0]]
        m[g] = eg.max()
        p = (eg - m[g]).exp()
        den[g] = p.sum()
        a[b - starts[0]:t - starts[0]] = p / den[g]
        for n in range(b, t):
            r[g] += a[n - starts[0]] * x[n]
    return r, e, m, den, a


def readout_grads(x, starts, dr, q=None, score=None):
    """dict(dx, dq | dscore) of sum(r * dr), float64 autograd through readout."""
    xr = x.double().clone().requires_grad_(True)
    qr = None if q is None else q.double().clone().requires_grad_(True)
    sr = None if score is None else score.double().clone().requires_grad_(True)
    r = readout(xr, starts, qr, sr)[0]
    (r * dr.double()).sum().backward()
    out = {"dx": xr.grad}
    if qr is not None:
        out["dq"] = qr.grad if qr.grad is not None else torch.zeros_like(qr)
    else:
        out["dscore"] = sr.grad.reshape(-1) if sr.grad is not None else torch.zeros_like(sr).reshape(-1)
    return out


def _softmax(e, batch, size):
    """torch_geometric.utils.softmax as upstream writes it (the 1e-16 included)."""
    m = torch.zeros((size,) + e.shape[1:], dtype=e.dtype)
    m = m.scatter_reduce(0, batch.view(-1, *[1] * (e.dim() - 1)).expand_as(e), e.detach(), "amax", include_self=False)
    out = (e - m[batch]).exp()
    den = torch.zeros((size,) + e.shape[1:], dtype=e.dtype).index_add(0, batch, out)
    return out / (den[batch] + 1e-16)


def _scatter_add(src, batch, size):
    return torch.zeros((size,) + src.shape[1:], dtype=src.dtype).index_add(0, batch, src)


def lstm64(lstm):
    """A float64 copy (CPU) of a torch.nn.LSTM with the same weights."""
    ref = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, lstm.num_layers).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in lstm.state_dict().items()})
    return ref


def set2set(x, batch, lstm, steps):
    """Set2Set.forward from upstream's recipe; lstm: a float64 torch.nn.LSTM
    (lstm64).  Any batch order."""
    x = x.double()
    B = int(batch.max()) + 1 if batch.numel() else 0
    C = x.shape[1]
    h = (torch.zeros((lstm.num_layers, B, C), dtype=torch.float64),
         torch.zeros((lstm.num_layers, B, C), dtype=torch.float64))
    q_star = torch.zeros((B, 2 * C), dtype=torch.float64)
    for _ in range(steps):
        q, h = lstm(q_star.unsqueeze(0), h)
        q = q.view(B, C)
        e = (x * q[batch]).sum(dim=-1, keepdim=True)
        a = _softmax(e, batch, B)
        r = _scatter_add(a * x, batch, B)
        q_star = torch.cat([q, r], dim=-1)
    return q_star


def global_attention(x, batch, size, gate_nn, nn=None):
    """GlobalAttention.forward from upstream's recipe; gate_nn / nn: float64 callables."""
    x = x.double()
    x = x.unsqueeze(-1) if x.dim() == 1 else x
    size = int(batch[-1]) + 1 if size is None else size
    gate = gate_nn(x).view(-1, 1)
    x = nn(x) if nn is not None else x
    gate = _softmax(gate, batch, size)
    return _scatter_add(gate * x, batch, size)
