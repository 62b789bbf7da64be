"""A lane-shape sweep of the GMMConv kernels: every tile shape of the flat and
column bins mappings, every lane-group width of the gather kernel (its scalar
and shuffled hand-over, one and eight loads in flight), and every way the
parameter-gradient kernel spreads (edge, k) pairs over a wave -- on the
257-node graph of tests/test_gpu_gmm.py and on a three-node graph smaller than
any tile, with the checks of that file (float64 restatement, the project's
bound, NaN-filled outputs, bitwise-equal reruns)."""
import pytest
import torch

from tests.test_gpu_gmm import DEV, N, _graph_edges, check_aggregates, check_param_grad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def edges():
    return _graph_edges()


@pytest.fixture(scope="module")
def graph(edges):
    from mi355_mp.graph import Graph
    return Graph(edges.to(DEV), N, N)


# (C, K, D): bins at Cin = C and gather at F = C
AGGREGATE_SHAPES = [
    (1, 1, 1),      # flat: one lane per row, 64 rows per wave; gather: a lane per row, one load in flight
    (2, 1, 2),      # groups of two lanes
    (3, 2, 1),      # gather groups of four with a dead lane; flat rows of 6 in groups of 8
    (8, 2, 2),      # gather groups of eight: the shuffled hand-over, eight loads in flight
    (9, 7, 2),      # flat rows of 63 entries: one row per wave, one dead lane; gather groups of 16
    (2, 40, 1),     # flat rows of 80 entries: two tiles over blockIdx.y, the second partial
    (17, 5, 3),     # gather groups of 32: two rows per wave
    (31, 3, 2),     # the last flat shape below the columns threshold
    (32, 16, 2),    # columns: exactly one tile of k, half of the lanes beyond Cin
    (32, 17, 1),    # columns: a second tile holding one k
    (33, 33, 2),    # columns: three tiles of k; gather: one row per wave, the scalar hand-over
    (64, 2, 3),     # every lane busy, a batch of four slots holding 8 live weights
    (65, 3, 2),     # two column tiles, the second with one lane; gather: two tiles of f
    (130, 1, 1),    # three column tiles
]


@pytest.mark.parametrize("shape", AGGREGATE_SHAPES)
def test_aggregate_lane_shapes(edges, graph, shape):
    C, K, D = shape
    check_aggregates(edges, graph.dst, N, C, K, D, 200)


# (C, K, D): how the parameter gradient spreads (edge, k) over a wave
PARAM_GRAD_SHAPES = [
    (3, 1, 1),      # 64 edges per wave step, one lane each
    (3, 1, 8),      # one lane per edge walks all 8 dims of dpseudo
    (5, 2, 3),      # 32 edges per wave step
    (2, 7, 40),     # K * D = 280: the accumulator sets bound the step to 3 edges (9 would fit the lanes)
    (4, 40, 25),    # K * D = 1000: one edge per step
    (2, 63, 2),     # one edge per step, one dead lane
    (2, 64, 2),     # one edge per step, every lane busy
    (2, 65, 2),     # k strided over the lanes: lane 0 owns k = 0 and 64
    (33, 25, 3),    # the large benchmark's table at a ragged Cin
]


@pytest.mark.parametrize("shape", PARAM_GRAD_SHAPES)
def test_param_grad_lane_shapes(edges, shape):
    C, K, D = shape
    check_param_grad(edges, N, C, K, D)


def test_a_graph_smaller_than_any_tile():
    """Three nodes, five edges, node 2 without in-edges: fewer rows than one
    wave's row groups and fewer edges than one parameter-gradient step."""
    from mi355_mp.graph import Graph
    ei = torch.tensor([[0, 1, 2, 2, 1], [1, 0, 0, 1, 1]])
    g = Graph(ei.to(DEV), 3, 3)
    for C, K, D in ((1, 1, 1), (5, 3, 2), (33, 17, 2), (64, 25, 3)):
        check_aggregates(ei, g.dst, 3, C, K, D, 2)
        check_param_grad(ei, 3, C, K, D, sizes=(1, 4, 5))
