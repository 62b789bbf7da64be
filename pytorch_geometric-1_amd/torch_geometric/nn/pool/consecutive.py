"""consecutive_cluster (PyG 1.4.3 nn.pool.consecutive [U]) on the native engine
(csrc/mp_cluster.hip, mp_cluster_build)."""
from mi355_mp import ops


def consecutive_cluster(src):
    """(inv, perm) of any int64 cluster vector src [N]: inv =
    torch.unique(src, sorted=True, return_inverse=True)[1] (keys ordered as signed
    int64), perm[c] = the largest node index i with inv[i] == c (what upstream's
    CPU scatter_ leaves; its GPU winner is unspecified).  One stable sort, one
    host read (the number of clusters)."""
    sel = ops.cluster_build(src)
    M = ops.cluster_read_counts(sel)[0]
    return sel.inv, sel.perm[:M]
