"""torch_geometric.utils.repeat (PyG 1.4.3): a per-dimension argument given as
one number or as a short / long list."""
import numbers
import itertools


def repeat(src, length):
    """``src`` as a list of ``length`` entries: a number is broadcast, a short
    list is padded with its last entry, a long one truncated; None stays None."""
    if src is None:
        return None
    if isinstance(src, numbers.Number):
        return list(itertools.repeat(src, length))
    src = list(src)
    if len(src) > length:
        return src[:length]
    if len(src) < length:
        return src + list(itertools.repeat(src[-1], length - len(src)))
    return src
