"""fps (PyG 1.4.3 nn.fps over torch_cluster 1.5 [U]) on the native engine
(csrc/mp_point.hip): farthest point sampling, per graph.

Upstream leaves ties and rounding to the hardware; here the sampler is a pure
function of the points and of each graph's first point.  Graph g keeps
k_g = ceil(fl32(ratio * fl32(n_g))) points (TopKPooling's count).  With m[i] the
smallest squared distance (fp32, include/mi355_mp.h "Point sets") from point i to
the points chosen so far, updated as m[i] = d < m[i] ? d : m[i] from +inf, the
next point is the argmax of m, equal values to the lower index.  A graph with
fewer distinct points than k_g therefore selects points twice, as upstream.
The output is grouped by graph in ascending order, within a graph in selection
order.  There is no CPU path.
"""
from mi355_mp import _lib, ops


def fps(x, batch=None, ratio=0.5, random_start=True):
    r"""Indices int64 [K] of the sampled rows of x ([N, D] float32, D <= 8).

    batch: sorted int64 [N] or None.  random_start=False starts every graph at its
    first point; True draws the in-graph offset floor(u * n_g) (clamped to
    n_g - 1) with torch's generator of the device, and the kernel is deterministic
    given that draw.  ValueError for an unsorted batch, more than 8 columns or a
    ratio outside (0, 1].

    Host synchronisation: one device-to-host read (K), beyond the batch layout,
    which is read once per batch tensor and cached.
    """
    _lib.require_device(x, batch)
    start = None
    if random_start:
        xr = x.view(-1, 1) if x.dim() == 1 else x
        layout = ops._sorted_layout(batch, xr.shape[0], x.device, "batch")
        start = ops.fps_random_start(layout)
    return ops.fps(x, batch, ratio, start)
