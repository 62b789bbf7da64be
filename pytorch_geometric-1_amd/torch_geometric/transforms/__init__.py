"""torch_geometric.transforms (PyG 1.4.3): the transforms the example models
need: Cartesian (SplineConv's pseudo-coordinates), Distance (the QM9 NNConv
example's edge attribute), ToDense (the DiffPool example's dense graphs) and
Compose."""
import torch


class Cartesian(object):
    r"""Saves the relative Cartesian coordinates of linked nodes in its edge
    attributes: ``pos[col] - pos[row]`` per edge.

    Args:
        norm (bool): map the result to [0, 1]: divide by ``2 * max_value`` and
            add 0.5. (default: True)
        max_value (float, optional): the normaliser; None takes the largest
            absolute coordinate difference of the graph. (default: None)
        cat (bool): concatenate to an existing ``edge_attr`` instead of
            replacing it. (default: True)
    """

    def __init__(self, norm=True, max_value=None, cat=True):
        self.norm = norm
        self.max = max_value
        self.cat = cat

    def __call__(self, data):
        (row, col), pos, pseudo = data.edge_index, data.pos, data.edge_attr
        cart = pos[col] - pos[row]
        cart = cart.view(-1, 1) if cart.dim() == 1 else cart
        if self.norm and cart.numel() > 0:
            max_value = cart.abs().max() if self.max is None else self.max
            cart = cart / (2 * max_value) + 0.5
        if pseudo is not None and self.cat:
            pseudo = pseudo.view(-1, 1) if pseudo.dim() == 1 else pseudo
            data.edge_attr = torch.cat([pseudo, cart.type_as(pseudo)], dim=-1)
        else:
            data.edge_attr = cart
        return data

    def __repr__(self):
        return "{}(norm={}, max_value={})".format(self.__class__.__name__, self.norm, self.max)


class Distance(object):
    r"""Saves the Euclidean distance of linked nodes in its edge attributes:
    ``||pos[col] - pos[row]||_2`` per edge, as a column.

    Args:
        norm (bool): divide by the largest distance of the graph, or by
            ``max_value``. (default: True)
        max_value (float, optional): the normaliser. (default: None)
        cat (bool): concatenate to an existing ``edge_attr`` instead of
            replacing it. (default: True)
    """

    def __init__(self, norm=True, max_value=None, cat=True):
        self.norm = norm
        self.max = max_value
        self.cat = cat

    def __call__(self, data):
        (row, col), pos, pseudo = data.edge_index, data.pos, data.edge_attr
        dist = torch.norm(pos[col] - pos[row], p=2, dim=-1).view(-1, 1)
        if self.norm and dist.numel() > 0:
            dist = dist / (dist.max() if self.max is None else self.max)
        if pseudo is not None and self.cat:
            pseudo = pseudo.view(-1, 1) if pseudo.dim() == 1 else pseudo
            data.edge_attr = torch.cat([pseudo, dist.type_as(pseudo)], dim=-1)
        else:
            data.edge_attr = dist
        return data

    def __repr__(self):
        return "{}(norm={}, max_value={})".format(self.__class__.__name__, self.norm, self.max)


class Compose(object):
    """Composes several transforms: each is applied to the result of the one
    before it."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data

    def __repr__(self):
        args = ["    {},".format(t) for t in self.transforms]
        return "{}([\n{}\n])".format(self.__class__.__name__, "\n".join(args))


class ToDense(object):
    r"""Converts a sparse graph to a dense one: ``data.adj`` [n, n] (or [n, n, D]
    from ``edge_attr``) replaces ``edge_index`` and ``edge_attr``, ``data.mask``
    (bool [n]) marks the graph's own nodes, and ``x``, ``pos`` and a node-level
    ``y`` are padded with zeros to ``num_nodes`` rows.

    Args:
        num_nodes (int, optional): the padded node count; None keeps the
            graph's own. (default: None)
    """

    def __init__(self, num_nodes=None):
        self.num_nodes = num_nodes

    def __call__(self, data):
        assert data.edge_index is not None
        orig_num_nodes = data.num_nodes
        if self.num_nodes is None:
            num_nodes = orig_num_nodes
        else:
            assert orig_num_nodes <= self.num_nodes
            num_nodes = self.num_nodes
        edge_attr = data.edge_attr
        if edge_attr is None:
            edge_attr = torch.ones(data.edge_index.size(1), dtype=torch.float)
        adj = torch.zeros((num_nodes, num_nodes) + tuple(edge_attr.shape[1:]), dtype=edge_attr.dtype)
        adj[data.edge_index[0], data.edge_index[1]] = edge_attr
        data.adj = adj
        data.edge_index = None
        data.edge_attr = None
        data.mask = torch.zeros(num_nodes, dtype=torch.bool)
        data.mask[:orig_num_nodes] = True

        def pad(t):
            size = [num_nodes - t.size(0)] + list(t.size())[1:]
            return torch.cat([t, t.new_zeros(size)], dim=0)
        if data.x is not None:
            data.x = pad(data.x)
        if data.pos is not None:
            data.pos = pad(data.pos)
        if data.y is not None and torch.is_tensor(data.y) and data.y.dim() >= 1 and data.y.size(0) == orig_num_nodes:
            data.y = pad(data.y)
        return data

    def __repr__(self):
        if self.num_nodes is None:
            return "{}()".format(self.__class__.__name__)
        return "{}(num_nodes={})".format(self.__class__.__name__, self.num_nodes)


__all__ = ["Cartesian", "Distance", "ToDense", "Compose"]
