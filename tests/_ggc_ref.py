"""GatedGraphConv restated in float64 on the CPU: the GRU cell of csrc/mp_gru.hip with the repository's
error bound propagated through it, and the layer (upstream's loop with index_add_).

Bound.  A pre-activation computed in fp32 is off by at most 1e-5 * sum |terms| (tests/_arma_ref.py).
With |sigmoid'| <= 1/4, |tanh'| <= 1 and |r|, |z|, |n| <= 1 that propagates to
    |dh'| <= |dz_pre| |n - h| / 4 + |dn_pre| + |hn| |dr_pre| / 4 + |dhn| + 8 eps_fp32
the last term for evaluating sigmoid and tanh themselves.
"""
import torch

BOUND = 1e-5
EPS = float(torch.finfo(torch.float32).eps)


def cell(a, h, wc, wh, b_ih=None, b_hh=None):
    """(h', bound on |h' error|, (n, r, z, hn)) for a, h [N, C] and wc, wh [C, 3C] in GRUCell's gate order."""
    a, h, wc, wh = a.double(), h.double(), wc.double(), wh.double()
    C = h.shape[1]
    zero = torch.zeros(3 * C, dtype=torch.float64)
    bi, bh = (zero if b is None else b.double() for b in (b_ih, b_hh))
    gi, gh = a @ wc + bi, h @ wh + bh
    si, sh = a.abs() @ wc.abs() + bi.abs(), h.abs() @ wh.abs() + bh.abs()
    r = torch.sigmoid(gi[:, :C] + gh[:, :C])
    z = torch.sigmoid(gi[:, C:2 * C] + gh[:, C:2 * C])
    hn = gh[:, 2 * C:]
    n = torch.tanh(gi[:, 2 * C:] + r * hn)
    d_r, d_z = (BOUND * (si[:, s] + sh[:, s]) for s in (slice(0, C), slice(C, 2 * C)))
    d_hn = BOUND * sh[:, 2 * C:]
    d_n = BOUND * (si[:, 2 * C:] + (r * hn).abs())
    bound = d_z * (n - h).abs() / 4 + d_n + hn.abs() * d_r / 4 + d_hn + 8 * EPS
    return (1 - z) * n + z * h, bound, (n, r, z, hn)


def cell_backward(dh, h, gates):
    """fp64 autograd of h' = (1 - z) n + z h through the pre-activations recovered from the given gates
    (n, r, z, hn): ([dn_pre, dr_pre, dz_pre, dhn_pre], dh_dir) and, in the same order, the sums of |terms|."""
    dh, h = dh.double(), h.double()
    n, r, z, hn = (g.double() for g in gates)
    hl, hnl = h.clone().requires_grad_(True), hn.clone().requires_grad_(True)
    rp, zp = torch.logit(r).requires_grad_(True), torch.logit(z).requires_grad_(True)
    np_ = (torch.atanh(n) - r * hn).requires_grad_(True)      # a Wc_n + b_in
    rr, zz = torch.sigmoid(rp), torch.sigmoid(zp)
    out = (1 - zz) * torch.tanh(np_ + rr * hnl) + zz * hl
    grads = torch.autograd.grad((out * dh).sum(), [np_, rp, zp, hnl, hl])
    dn_s = dh.abs() * (1 + z) * (1 + n * n)
    scales = [dn_s, dn_s * hn.abs() * r * (1 + r), dh.abs() * (h.abs() + n.abs()) * z * (1 + z), dn_s * r,
              dh.abs() * z]
    return list(grads[:4]), grads[4], scales


def layer(x, edge_index, edge_weight, weight, rnn, aggr="add", dtype=torch.float64):
    """Upstream's forward: h = x zero-padded; per step m = AGGR_{edge_index[1]} w_e (h W_l)[edge_index[0]], h = GRU(m, h)."""
    weight = weight.to(dtype)
    w_ih, w_hh = rnn["weight_ih"].to(dtype), rnn["weight_hh"].to(dtype)
    C = weight.shape[1]
    b_ih, b_hh = (rnn[k].to(dtype) if k in rnn else torch.zeros(3 * C, dtype=dtype) for k in ("bias_ih", "bias_hh"))
    h = torch.nn.functional.pad(x.to(dtype), (0, C - x.shape[1]))
    src, dst = edge_index
    for l in range(weight.shape[0]):
        msg = (h @ weight[l])[src]
        if edge_weight is not None:
            msg = msg * edge_weight.to(dtype).view(-1, 1)
        m = torch.zeros_like(h).index_add_(0, dst, msg)
        if aggr == "mean":
            m = m / torch.bincount(dst, minlength=h.shape[0]).clamp(min=1).to(dtype).view(-1, 1)
        gi, gh = m @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :C] + gh[:, :C])
        z = torch.sigmoid(gi[:, C:2 * C] + gh[:, C:2 * C])
        h = (1 - z) * torch.tanh(gi[:, 2 * C:] + r * gh[:, 2 * C:]) + z * h
    return h
