"""graclus (PyG 1.4.3 nn.pool.graclus over torch_cluster 1.5 graclus_cluster [U]) on the
native engine (csrc/mp_graclus.hip): a greedy matching of every node with at most
one neighbour, the pair of largest edge weight first.

Upstream walks the nodes in a random order (CPU) or in random propose / respond
colourings (GPU), so its clusters change from call to call.  Here the matching is
a pure function of the graph.  Every edge (row, col) with row != col is an entry
of the unordered pair (a, b) = (min, max); its priority is the tuple

    (wkey, h, a, b),   wkey = the order-preserving uint32 image of the float32 weight
                              (0 without weights),
                       h    = the upper 32 bits of mix64(mix64(seed) ^ (a << 32 | b)),

compared lexicographically (include/mi355_mp.h "Graclus" has the bit formulas).
Walk the entries in descending priority and match (a, b) when both ends are
unmatched: cluster[a] = cluster[b] = a, and cluster[i] = i for everybody else.
The result does not depend on the order or the direction of the edges: an edge
present one way only still joins its pair, duplicates of a pair count with their
largest weight, loops are ignored.  The hash breaks weight ties (all of them
without weights); another `seed` gives another, equally valid matching.

The kernels reach the same matching in parallel rounds of mutual pointers;
hashed priorities take O(log N) of them in expectation, a path whose weights
increase strictly along it takes one per matched pair.  There is no CPU path.
"""
import torch

from mi355_mp import _lib, ops

from ...debug import is_debug_enabled
from ...utils.num_nodes import maybe_num_nodes


def graclus(edge_index, weight=None, num_nodes=None, *, seed=0):
    r"""The cluster vector [N] (int64) of the greedy matching described above:
    the smaller node index of a matched pair, the node's own index otherwise.

    edge_index: int64 [2, E]; weight: float32 [E] or None (any other dtype raises
    TypeError); num_nodes: None means edge_index.max() + 1; seed: keyword only,
    an addition to upstream's signature.  An edge end outside [0, N) raises
    IndexError.  NaN weights are out of scope (debug mode raises ValueError).

    Host synchronisation: one device-to-host read per ops.GRACLUS_ROUNDS_PER_READ
    rounds (the index check of the incidence build rides on the first), plus
    edge_index.max() when num_nodes is None.
    """
    _lib.require_device(edge_index, weight)
    if weight is not None:
        if weight.dtype != torch.float32:
            raise TypeError("graclus: weight must be float32 (got %s)" % weight.dtype)
        if is_debug_enabled() and bool(torch.isnan(weight).any()):
            raise ValueError("graclus: weight must not hold NaN")
    n = maybe_num_nodes(edge_index, num_nodes)
    return ops.graclus_match(edge_index, weight, n, seed=seed).cluster
