"""knn_interpolate (PyG 1.4.3 nn.unpool.knn_interpolate [U]): PointNet++'s feature
propagation, on the native engine (csrc/mp_knn.hip).

    out[j] = (sum_t w_t x[i_t]) / (sum_t w_t),   w_t = 1 / max(d2(pos_x[i_t], pos_y[j]), 1e-16)

over the k nearest points i_0 .. i_{c-1} of pos_y[j] in pos_x, in knn order
(distance, then index), both sums accumulated in fp32 in that order.  The
neighbours are never written out as an edge list: the interpolation runs from
the search's slab, so the forward makes no device-to-host read.  There is no CPU
path.
"""
from mi355_mp import _lib, ops


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3):
    r"""float32 [M, C]: x [N, C] interpolated from pos_x [N, D] onto pos_y [M, D].

    A y whose graph holds no x gets a row of zeros.  Gradients flow to x only
    (upstream computes the weights under no_grad): d x[i] is the deterministic sum
    of (w_ji / W_j) g[j] over the pairs of i, grouped by source.  1 <= k <= 64;
    ValueError as for knn."""
    _lib.require_device(x, pos_x, pos_y, batch_x, batch_y)
    return ops.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k)
