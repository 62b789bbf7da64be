"""The ARMA step and the GRU cell at the template instantiations and grid shapes the fixed graphs of
test_gpu_arma.py / test_gpu_ggc.py never reach (the AGNN widths of the same kind extend test_gpu_agnn.py's
own parametrisation).  The shapes and the dispatch rules they follow: tests/_recurrent_lane_cases.py.

ARMA (csrc/mp_arma.hip): every task width L = 4 .. 64 of k_arma_main, forward and backward, with the vector
and the scalar transform and with full and partly inactive lane groups, on the 70-node tiny graph (a hub row in
either CSR, 22 consecutive rows without slots, an empty tail) under three schedules: the default one, chunk
16 with split rows (continuation / head slab slots and k_arma_fixup at every L) and one task that owns every
row (the rowptr window of an L = 4 task reloads 23 times).  The checks are test_gpu_arma.py's single-step
helpers: NaN-filled outputs, padding columns exactly zero, |err| <= 1e-5 * sum |terms|.

GRU (csrc/mp_gru.hip): every P / 16 of gru_cell's switch at one row, half a tile and a tile plus a row; and
grids past the cap of CUs * kPerCu workgroups, where a workgroup walks two or three tiles through the
double-buffered prefetch and k_gru_cell_bwd strides.  The checks are test_gpu_ggc.check_cell.

With -s every case prints its lane mapping and its largest err / bound.
"""
import pytest
import torch

from tests import _arma_ref as AR
from tests import _recurrent_lane_cases as K
from tests import test_gpu_arma as TA, test_gpu_ggc as TG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEDULES = {"default": None, "chunk16": 16, "one_task": 1024}


@pytest.fixture(scope="module")
def edges():
    return K.tiny_graph().flip(0).contiguous()      # keyed on edge_index[0]: HUB_IN's 50 edges arrive at its row


@pytest.fixture(scope="module")
def graphs(edges):
    """schedule -> (Graph keyed on edges[0], lap on the device in edge order), and the reference's float64 lap."""
    from mi355_mp import ops
    from mi355_mp.graph import MIN_CHUNK, Graph
    assert MIN_CHUNK == SCHEDULES["chunk16"]
    ew = torch.rand(edges.shape[1], generator=torch.Generator().manual_seed(5)) + 0.5
    out = {}
    for name, chunk in SCHEDULES.items():
        graph = Graph(edges.to(DEV), K.N_NODES, K.N_NODES, "target_to_source", chunk=chunk)
        for csr in (graph.dst, graph.src):
            if name == "chunk16":
                assert csr.chunk == 16 and csr.n_split >= 1, (csr.chunk, csr.n_split)
            if name == "one_task":
                assert csr.n_waves == 1 and csr.n_split == 0, (csr.n_waves, csr.n_split)
        out[name] = (graph, ops.arma_laplacian(graph, ew.to(DEV)))
    return out, AR.laplacian(edges, K.N_NODES, ew)


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("K_,C", K.ARMA_CASES)
def test_arma_step_lane_shapes(edges, graphs, K_, C, schedule):
    """Per case and schedule: the forward step with a next transform and as the last step, the backward step
    without a transform, with one, and with one and the mask; ReLU and the identity."""
    from mi355_mp import ops
    assert ops.arma_ok(K_, C) and ops.arma_width(K_, C) == K.arma_width(K_, C)
    (graph, lap), lap64 = graphs[0][schedule], graphs[1]
    torch.manual_seed(1000 * K_ + C)
    w = torch.randn(K_, C, C, device=DEV) * 0.5
    h = TA._nan_rows(K_, C, True, K.N_NODES)
    worst = 0.0
    for act in ("relu", None):
        what = "(%d, %d) %s %s" % (K_, C, schedule, act)
        worst = max(worst, TA.check_forward_steps(edges, graph, lap, K_, C, act, [w, None], lap64=lap64, what=what))
        for wt, hh in ((None, None), (w, None), (w, h)):
            if act is None and hh is not None:
                continue                                      # (the identity has no mask)
            worst = max(worst, TA.check_backward_step(edges, graph, lap, K_, C, act, wt, hh, lap64=lap64, what=what))
    print("ARMA (K, C) = (%d, %d): P = %d, L = %d, %s transform, %s: max err / bound %.3g"
          % (K_, C, K.arma_width(K_, C), K.arma_lanes(K_, C), "vector" if C % 4 == 0 else "scalar", schedule,
             worst / AR.BOUND))


@pytest.mark.parametrize("N", [1, 33, 65])
@pytest.mark.parametrize("C", K.GRU_WIDTHS)
def test_gru_cell_widths(C, N):
    from mi355_mp import ops
    assert ops.gru_ok(C) and ops.gru_width(C) == K.gru_width(C)
    worst = TG.check_cell(N, C, True)
    print("GRU C = %d: P = %d, N = %d: max err / bound %.3g" % (C, K.gru_width(C), N, worst))


@pytest.mark.parametrize("P", K.GRU_MANY_TILES)
def test_gru_cell_many_tiles(P):
    """More tiles than the grid's cap of CUs * kPerCu workgroups: with N = (2 cap + 1) BM + 1 the first two
    workgroups take three tiles and the others two, each prefetching its next tile into the other LDS buffer,
    and the last tile holds one row; at P = 128 N also exceeds the backward kernel's CUs * 16 * 256 threads.
    check_cell compares every row, requires zero padding columns and runs both kernels twice, bitwise equal."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = K.GruShape(P)
    N = K.gru_many_tiles_rows(P, cus)
    cap, tiles = cus * s.per_cu, -(-N // s.bm)
    assert tiles >= 2 * cap + 2 and tiles % cap == 2 and N % s.bm == 1
    if P == 128:
        assert N * P // 4 > cus * K.GRU_BWD_BLOCKS_PER_CU * K.GRU_BWD_BLOCK
    C = P if P in (64, 128) else P - 3
    assert K.gru_width(C) == P
    worst = TG.check_cell(N, C, True)
    print("GRU many tiles P = %d (C = %d): %d CUs, cap %d workgroups x %d slice(s), %d tiles of %d rows, N = %d: "
          "max err / bound %.3g" % (P, C, cus, cap, s.slices, tiles, s.bm, N, worst))
