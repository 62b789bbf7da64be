"""negative_sampling / structured_negative_sampling (PyG 1.4.x [U]) on the native
sampler (mi355_mp.ops.negative_sample -> mp_neg_sample).

Upstream copies the edge keys to the host, draws with random.sample and rejects
through np.isin in a retry loop.  Here a draw is the r-th key that is not in the
edge list's sorted key table (cached per edge_index tensor): one binary search
on the device, no retry, no host read.  Differences, on purpose:
  * sampling is WITH replacement (upstream's first round is without): a pair can
    come back twice; every returned pair is a non-edge;
  * force_undirected draws from the strict upper triangle (upstream's includes
    the diagonal) and returns each pair with its mirror, [i | j ; j | i];
  * structured_negative_sampling gives -1 to the edges of a node that is linked
    to every node, where upstream's loop never ends.
The draws follow the device generator's seed (torch.cuda.manual_seed repeats them).
"""
from mi355_mp import ops as _ops

from .num_nodes import maybe_num_nodes


def negative_sampling(edge_index, num_nodes=None, num_neg_samples=None, force_undirected=False):
    """[2, min(num_neg_samples or E, N^2 - E)] pairs that are not in edge_index."""
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    return _ops.negative_sample(edge_index, num_nodes, num_neg_samples, force_undirected)


def structured_negative_sampling(edge_index, num_nodes=None):
    """(i, j, k): for every edge (i, j) a node k such that (i, k) is not an edge."""
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    k = _ops.structured_negative_sample(edge_index, num_nodes)
    return edge_index[0], edge_index[1], k
