"""avg_pool / avg_pool_x (PyG 1.4.3 nn.pool.avg_pool [U]): max_pool with
scatter_mean on x -- every kernel but the reducer is shared (max_pool.py)."""
from .max_pool import _pool, _pool_x


def avg_pool(cluster, data, transform=None):
    """max_pool with the node features averaged over every cluster (the float32
    sum in ascending node order over the member count).  One host read."""
    return _pool(cluster, data, transform, "mean")


def avg_pool_x(cluster, x, batch, size=None):
    """max_pool_x with the mean: with `size`, scatter_('mean', x, cluster,
    dim_size=(batch.max() + 1) * size)."""
    return _pool_x(cluster, x, batch, size, "mean")
