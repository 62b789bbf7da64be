"""torch_geometric.transforms (PyG 1.4.3): the transforms the example models
need: Cartesian (SplineConv's pseudo-coordinates), Distance (the QM9 NNConv
example's edge attribute) and Compose."""
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


__all__ = ["Cartesian", "Distance", "Compose"]
