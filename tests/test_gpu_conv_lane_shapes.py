"""The NNConv and RGCNConv kernels at the lane mappings, tile counts and kernel
boundaries the fixed graphs of test_gpu_nnconv.py / test_gpu_rgcn.py never
reach, on one tiny graph (tests/_conv_lane_cases.py: 70 nodes, 203 edges, rows
60.. without in-edges, one hub row, duplicates, self loops, shuffled), so that
every float64 restatement takes milliseconds.

The checks are the helpers of the two modules (the same assertions as their
own kernel tests): every output is written into a NaN-filled tensor and
compared whole under |err| <= 1e-5 * sum |terms|, rows without slots and the
relation without edges are exactly zero, the strided forms are bitwise the
plain ones.

NNConv (Cin = F, H): the lane-group widths 2..32 of gather and of the grouped
edge gradient, flat bins rows of 3..8 entries, Cin = 31 / 32 / 33; the wave
edge gradient's partial tiles at both widths (one tile below the width, a
partial tile after full ones, several c per lane).  RGCN (B, C = F): the att
gradient's lane-group widths 2, 4, 16, a second and third tile of 64 values of
b and their partial last tile, with 16-byte (C = 4) and scalar (C = 3) row
loads; flat bins rows of 2..4 entries; B * C on both sides of 64, 128, 256
and 512 (entries per lane); columns bins with one, two and five tiles of 16
values of b; the gather widths.
"""
import pytest
import torch

from tests import _conv_lane_cases as K
from tests import test_gpu_nnconv as TN, test_gpu_rgcn as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _edge_grad_reach():
    from mi355_mp import ops
    return K.edge_grad_reach(ops.nnconv_edge_grad_width, K.NNCONV_WIDTHS + K.NNCONV_EDGE_GRAD)


assert _edge_grad_reach() >= K.EDGE_GRAD_REACHED, sorted(K.EDGE_GRAD_REACHED - _edge_grad_reach())


@pytest.fixture(scope="module")
def edges():
    return K.tiny_graph()                                             # asserts the graph's properties


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    return Graph(edges.to(DEV), K.N_NODES, K.N_NODES)


@pytest.fixture(scope="module")
def types():
    return {n_rel: K.tiny_relations(n_rel) for n_rel in (1, 3)}


@pytest.fixture(scope="module")
def norm():
    return torch.rand(K.N_EDGES, generator=torch.Generator().manual_seed(3)) + 0.5


@pytest.mark.parametrize("C,H", K.NNCONV_WIDTHS)
def test_nnconv_lane_group_widths(edges, graph, C, H):
    """bins with and without row_scale, gather with and without row_scale and
    bias, edge_grad."""
    TN.check_aggregates(edges, graph.dst, K.N_NODES, C, H, K.N_DST)
    TN.check_edge_grad(edges, K.N_NODES, C, H)


@pytest.mark.parametrize("C,H", K.NNCONV_EDGE_GRAD)
def test_nnconv_edge_grad_partial_tiles(edges, C, H):
    from mi355_mp import ops
    assert ops.nnconv_edge_grad_width(H, C) in (32, 64)
    TN.check_edge_grad(edges, K.N_NODES, C, H)


@pytest.mark.parametrize("B,C", K.RGCN_CASES)
def test_rgcn_lane_shapes(edges, graph, types, norm, B, C):
    """bins node-major and block-major, gather from both layouts and with bias,
    att_grad in both roles, with and without edge_norm, att with ld_att = B + 2,
    R in {1, 3} (relation 1 of 3 without edges: an exact zero row)."""
    TR.check_kernels(edges, graph.dst, K.N_NODES, types, norm, C, B, K.N_DST)
