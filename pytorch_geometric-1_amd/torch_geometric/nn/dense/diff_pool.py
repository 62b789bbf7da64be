from mi355_mp import ops as _ops

from . import _dense


def dense_diff_pool(x, adj, s, mask=None):
    r"""Differentiable pooling (PyG 1.4.3 nn.dense.dense_diff_pool): with the
    assignment P = softmax(s, -1) (times the mask),

        out = P^T x,   out_adj = P^T adj P,
        link_loss = ||adj - P P^T||_F / numel(adj),
        ent_loss = mean over nodes of sum_c -P log(P + 1e-15).

    x [B, N, F], adj [B, N, N], s [B, N, C] (2-D inputs are one graph), mask [B,
    N].  Returns (out, out_adj, link_loss, ent_loss).  Float32 inputs on the GPU
    with an adjacency that needs no gradient and graphs that fit the
    one-workgroup form (nn/dense/_dense.py pool_fused) run as one fused native
    call that never forms an [B, N, N] array; an adjacency that requires a
    gradient (the pooled one of an earlier level) runs the upstream recipe in
    torch ops, so that gradient exists, and so do graphs beyond that form."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    s = s.unsqueeze(0) if s.dim() == 2 else s
    if _dense.pool_fused(x, adj, s):
        return _ops.dense_diff_pool(x, adj, s, mask)
    return _dense.diff_pool_recipe(x, adj, s, mask)
