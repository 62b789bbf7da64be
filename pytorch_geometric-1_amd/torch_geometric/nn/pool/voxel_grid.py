"""voxel_grid (PyG 1.4.3 nn.pool.voxel_grid over torch_cluster 1.5 grid_cluster [U]) on the
native engine (csrc/mp_cluster.hip, mp_voxel_keys_f32).

A batch column is appended to the positions (size 1, start 0, end batch.max()),
and per column d, in float32 with IEEE subtraction and division,

    c_d = trunc((pos_d - start_d) / size_d),  m_d = trunc((end_d - start_d) / size_d) + 1,
    key = sum_d c_d * prod_{j<d} m_j           (int64).

Positions outside [start, end] follow the same arithmetic: keys may then collide
or be negative, as upstream.  Non-finite positions are out of scope (debug mode
raises ValueError).  There is no CPU path.
"""
import torch

from mi355_mp import _lib, ops

from ...debug import is_debug_enabled
from ...utils.repeat import repeat

_geometry = {}


def _column(v, D, pos, last):
    """v (a number, a list or a tensor) repeated to D entries, then `last`, as a
    float32 device tensor.  Host-known values are uploaded once and kept."""
    if torch.is_tensor(v) or torch.is_tensor(last):
        if torch.is_tensor(v):
            v = v.detach().reshape(-1).to(device=pos.device, dtype=pos.dtype)
            v = v[:D] if v.numel() >= D else torch.cat([v, v[-1:].expand(D - v.numel())])
        else:
            v = torch.tensor([float(t) for t in repeat(v, D)], dtype=pos.dtype, device=pos.device)
        if not torch.is_tensor(last):
            last = torch.tensor([float(last)], device=pos.device)
        return torch.cat([v, last.detach().to(device=pos.device, dtype=pos.dtype).view(1)])
    vals = [float(t) for t in repeat(v, D)]
    key = (tuple(vals), float(last), str(pos.device))
    hit = _geometry.get(key)
    if hit is None:
        if len(_geometry) > 256:
            _geometry.clear()
        hit = _geometry[key] = torch.tensor(vals + [float(last)], dtype=pos.dtype, device=pos.device)
    return hit


def voxel_grid(pos, batch, size, start=None, end=None):
    r"""The voxel key [N] (int64) of every node: a regular grid of cell `size`
    laid over [start, end] in every position column, one grid per graph.

    pos: [N] or [N, D] float32, D <= 8; batch: [N] int64; size, start, end: a
    number, a list or a tensor each (repeated to D entries); a None start / end
    is the per-column minimum / maximum of the positions, reduced on the device.

    Host synchronisation: none of its own.  The number of graphs comes from the
    batch layout when the engine already knows it for this batch tensor
    (ops.known_num_graphs), else from a device-side batch.max().
    """
    _lib.require_device(pos, batch)
    pos2 = pos.detach()
    pos2 = pos2.unsqueeze(-1) if pos2.dim() == 1 else pos2
    if pos2.dtype != torch.float32:
        raise TypeError("voxel_grid: positions must be float32 (got %s)" % pos2.dtype)
    if is_debug_enabled() and not bool(torch.isfinite(pos2).all()):
        raise ValueError("voxel_grid: positions must be finite")
    D = pos2.size(1)
    G = ops.known_num_graphs(batch)
    b_max = batch.max() if G is None else float(G - 1)
    size_t = _column(size, D, pos2, 1.0)
    if start is None:
        start_t = torch.cat([pos2.min(dim=0)[0], batch.min().to(pos2.dtype).view(1)])
    else:
        start_t = _column(start, D, pos2, 0.0)
    if end is None:
        b_end = b_max if torch.is_tensor(b_max) else torch.tensor([b_max], dtype=pos2.dtype, device=pos2.device)
        end_t = torch.cat([pos2.max(dim=0)[0], b_end.to(pos2.dtype).view(1)])
    else:
        end_t = _column(end, D, pos2, b_max)
    return ops.voxel_keys(pos2, batch, size_t, start_t, end_t)
