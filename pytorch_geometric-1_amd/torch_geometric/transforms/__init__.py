"""torch_geometric.transforms (PyG 1.4.3): the transform SplineConv's models
need to turn node positions into pseudo-coordinates."""
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


__all__ = ["Cartesian"]
