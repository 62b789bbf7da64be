"""The shapes of tests/test_gpu_recurrent_lane_shapes.py (and of the AGNN sweep in
tests/test_gpu_agnn.py) with the tiny graph they run on, importable without a GPU:
tests/test_recurrent_cases_host.py checks on the CPU that each list reaches every
template instantiation it claims.

The reach functions restate the dispatch rules of csrc/mp_arma.hip (arma_run),
csrc/mp_gru.hip (gru_cell, GruShape) and csrc/mp_agnn.hip (agnn_launch, agnn_with).
"""
import torch

N_NODES = 70
HUB_IN, HUB_OUT = 7, 55     # 50 extra edges arrive at HUB_IN, 50 extra leave HUB_OUT
EMPTY_RUN = (30, 52)        # nodes 30..51: on no edge (22 consecutive rows without slots in either CSR)
N_ACTIVE = 62               # nodes 62..69: on no edge either (the tail)
N_EDGES = 203               # not a multiple of 8

# ---- ARMA step (K, C): P = arma_width(K, C), L = max(4, next_pow2(P / 4)) lanes per task ---------------------
ARMA_CASES = (
    # L = 4: one padded vector (K * C < 4), one vector, three of four lanes, the full group in both transforms
    (1, 1), (2, 2), (1, 4), (1, 12), (3, 5), (4, 4),
    # L = 8: P = 20 is the first width; a stack boundary inside a vector; the full group in both transforms
    (5, 4), (3, 7), (1, 32), (2, 15),
    # L = 16: P = 36 the first width; the scalar transform partial and full; K = 1 at the limit of C
    (9, 4), (5, 12), (3, 15), (7, 9), (1, 64),
    # L = 32: P = 68 the first width; K * C * C = 8192 at C = 64
    (17, 4), (5, 13), (3, 24), (2, 64),
    # L = 64: P = 132 the first width; 255 columns and one padding float; C = 1; K * C * C = 8192 at K * C = 256
    (33, 4), (17, 15), (64, 4), (256, 1), (8, 32),
)
ARMA_OUTSIDE = (4, 64)      # K * C * C = 16384: outside arma_ok, the layer takes the recipe
ARMA_MAX_C, ARMA_MAX_WIDTH, ARMA_MAX_W = 64, 256, 8192
ARMA_LANES = (4, 8, 16, 32, 64)

# ---- GRU cell C: P = gru_width(C) = C rounded up to 16, one instantiation per P / 16 ------------------------
# one C per P (16, 32, .. 128), padding inside the first column block of the second slice (P - 15 at 96 and 112), C = 1
GRU_WIDTHS = (12, 32, 44, 64, 72, 96, 112, 128, 81, 97, 1)
GRU_MANY_TILES = (16, 64, 80, 128)       # P of the many-tiles test: 1, 4, 4 + 1 and 4 + 4 waves, both row-tile heights
GRU_MAX_C = 128
GRU_BWD_BLOCKS_PER_CU, GRU_BWD_BLOCK = 16, 256

# ---- AGNN F -------------------------------------------------------------------------------------------------
# the seven of test_gpu_agnn.py before this list; (4, 3); (1, 4); (1, 16); groups of 2, 8, 2 (W = 4), 16 and 16 lanes
AGNN_WIDTHS = (1, 3, 16, 18, 256, 260, 1024, 516, 768, 70, 255, 257, 1023, 2, 7, 8, 13, 36)
AGNN_MAPPINGS = frozenset([(4, 1), (4, 2), (4, 3), (4, 4), (1, 1), (1, 4), (1, 16)])


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def arma_ok(K, C):
    return K >= 1 and 1 <= C <= ARMA_MAX_C and K * C <= ARMA_MAX_WIDTH and K * C * C <= ARMA_MAX_W


def arma_width(K, C):
    return (K * C + 3) & ~3


def arma_lanes(K, C):
    return max(4, next_pow2(arma_width(K, C) // 4))


def arma_reach(cases):
    """{(L, transform, group)}: transform "vector" (C % 4 == 0) or "scalar"; group "full" when the row's
    P / 4 vectors fill the L lanes of a task, "partial" when some lanes stay inactive."""
    seen = set()
    for K, C in cases:
        L = arma_lanes(K, C)
        assert arma_width(K, C) <= 4 * L and L in ARMA_LANES, (K, C, L)
        seen.add((L, "vector" if C % 4 == 0 else "scalar", "full" if arma_width(K, C) == 4 * L else "partial"))
    return seen


def gru_width(C):
    return (C + 15) & ~15


class GruShape(object):
    """GruShape<P> of csrc/mp_gru.hip: the row-tile height, waves per workgroup, workgroups per CU, grid slices."""

    def __init__(self, P):
        assert P % 16 == 0 and 16 <= P <= 128, P
        self.P, self.nkb = P, P // 16
        self.waves = min(self.nkb, 4)
        self.bm = 32 if P > 64 else 64
        self.per_cu = 4 // self.waves
        self.slices = 2 if self.nkb > 4 else 1


def gru_reach(widths):
    """{P / 16} of the widths: the case labels of gru_cell's switch."""
    return {gru_width(C) // 16 for C in widths}


def gru_many_tiles_rows(P, cus):
    """N of the many-tiles test: with cap = cus * kPerCu workgroups, (m * cap + 1) * BM + 1 rows are m * cap + 2
    tiles -- the first two workgroups take m + 1 tiles, the others m, and the last tile holds one row.  m = 2,
    but at P = 128 the smallest m >= 2 at which N * P / 4 exceeds the backward kernel's cus * 16 * 256 threads."""
    s = GruShape(P)
    cap = cus * s.per_cu
    m = 2
    rows = lambda m: (m * cap + 1) * s.bm + 1  # noqa: E731
    if P == 128:
        while rows(m) * P // 4 <= cus * GRU_BWD_BLOCKS_PER_CU * GRU_BWD_BLOCK:
            m += 1
    return rows(m)


def group_lanes(elems):
    g = 1
    while g < 64 and g < elems:
        g <<= 1
    return g


def agnn_mapping(F):
    """(W, NV, lanes per group) of agnn_launch for contiguous 16-byte aligned operands."""
    W = 4 if F % 4 == 0 else 1
    elems = F // W
    nv = -(-elems // 64)
    if W == 1 and nv > 1:
        nv = 4 if nv <= 4 else 16
    return W, nv, group_lanes(elems)


def agnn_reach(widths):
    """({(W, NV)}, {lanes per group}) of the widths."""
    maps = [agnn_mapping(F) for F in widths]
    return {(w, nv) for w, nv, _ in maps}, {g for _, _, g in maps}


def tiny_graph():
    """edge_index int64 [2, 203] over 70 nodes, fixed and shuffled: both ends in [0, 30) + [52, 62), so nodes
    30..51 (a run of 22 in the middle) and 62..69 (the tail) have no slot in either CSR; 50 extra edges into
    HUB_IN and 50 out of HUB_OUT (a hub row whichever end keys the CSR); eight repeated pairs; five self loops."""
    g = torch.Generator().manual_seed(21)
    active = torch.cat([torch.arange(0, EMPTY_RUN[0]), torch.arange(EMPTY_RUN[1], N_ACTIVE)])
    pick = lambda n: active[torch.randint(0, active.numel(), (n,), generator=g)]  # noqa: E731
    ei = torch.stack([pick(90), pick(90)])
    dup = ei[:, :8]
    loops = pick(5).repeat(2, 1)
    hub_in = torch.stack([pick(50), torch.full((50,), HUB_IN, dtype=torch.int64)])
    hub_out = torch.stack([torch.full((50,), HUB_OUT, dtype=torch.int64), pick(50)])
    ei = torch.cat([ei, dup, loops, hub_in, hub_out], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    assert tuple(ei.shape) == (2, N_EDGES) and N_EDGES % 8
    for end, hub in ((1, HUB_IN), (0, HUB_OUT)):
        deg = torch.bincount(ei[end], minlength=N_NODES)
        assert 50 <= int(deg[hub]) <= 62 and int(deg.max()) == int(deg[hub])
        assert int(deg[EMPTY_RUN[0]:EMPTY_RUN[1]].sum()) == 0 and EMPTY_RUN[1] - EMPTY_RUN[0] >= 20
        assert int(deg[N_ACTIVE:].sum()) == 0 and int(deg[EMPTY_RUN[1]:N_ACTIVE].sum()) > 0
    assert int((ei[0] == ei[1]).sum()) >= 5
    assert torch.unique(ei[0] * N_NODES + ei[1]).numel() <= N_EDGES - 8           # duplicate edges
    assert not torch.equal(ei[1], ei[1].sort().values) and not torch.equal(ei[0], ei[0].sort().values)
    return ei
