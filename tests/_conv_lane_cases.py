"""The shapes of tests/test_gpu_conv_lane_shapes.py and the tiny graph they run
on, importable without a GPU: tests/test_nnconv_host.py checks on the CPU that
the NNConv list reaches every edge-gradient kernel and tile shape it claims.

The lists follow the dispatch code of csrc/mp_nnconv.hip and csrc/mp_rgcn.hip:
every lane-group width 1 << glog of the aggregate kernels, both sides of each
threshold between two kernels or tile counts, and the partial tiles.
"""
import torch

N_NODES = 70            # rows 60.. have no in-edge
N_DST = 60
N_EDGES = 203           # not a multiple of 8
HUB = 7                 # the row with about 50 in-edges

# NNConv (Cin = F, H): the lane-group widths 2, 4, 8, 16, 32 of gather and of the grouped edge gradient (Cin
# of 2, 3..4, 5..8, 9..16, 17..32), (H + 1) * Cin of 3..8 and above for flat bins, the boundaries Cin = 31 / 32
# (flat against columns bins) and 32 / 33 (grouped against wave edge gradient)
NNCONV_WIDTHS = tuple((c, h) for c in (2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33) for h in (1, 3))
# NNConv edge gradient above 32 columns (Cin, H): the partial tiles of both widths
NNCONV_EDGE_GRAD = ((33, 40), (64, 63), (64, 100), (70, 40), (64, 65), (128, 33), (130, 5))

# RGCN (B, C = F)
RGCN_ATT_GRAD = tuple((b, c) for b in (2, 3, 4, 9, 16, 17, 64, 65, 130) for c in (3, 4))
RGCN_FLAT_BINS = ((2, 1), (1, 3), (4, 1), (2, 2))
RGCN_T_BOUNDARIES = ((4, 16), (5, 13), (8, 16), (43, 3), (16, 16), (257, 1), (32, 16), (27, 19))
RGCN_COLUMNS_BINS = ((16, 32), (17, 32), (65, 33))
RGCN_GATHER = tuple((b, f) for f in (2, 3, 4, 9, 17, 31, 32) for b in (7, 8, 9))
RGCN_CASES = tuple(dict.fromkeys(RGCN_ATT_GRAD + RGCN_FLAT_BINS + RGCN_T_BOUNDARIES + RGCN_COLUMNS_BINS + RGCN_GATHER))

EDGE_GRAD_REACHED = frozenset([
    "grouped", "w32 full tile", "w64 full tile", "w32 partial tile after a full one",
    "w64 partial tile after a full one", "w64 single partial tile", "w32 several c per lane",
    "w64 several c per lane"])


def edge_grad_reach(width, cases):
    """What the (Cin, H) pairs reach in the edge gradient, by the library's own
    choice width(H, Cin) in {0, 32, 64}: the names of EDGE_GRAD_REACHED (and
    'w32 single partial tile')."""
    seen = set()
    for c_in, H in cases:
        w = width(H, c_in)
        assert w in (0, 32, 64) and (w == 0) == (c_in <= 32), (c_in, H, w)
        if w == 0:
            seen.add("grouped")
            continue
        tiles, last = -(-H // w), H - (-(-H // w) - 1) * w
        if H >= w:
            seen.add("w%d full tile" % w)
        if last < w:
            seen.add("w%d %s" % (w, "partial tile after a full one" if tiles > 1 else "single partial tile"))
        if c_in > w:
            seen.add("w%d several c per lane" % w)
    return seen


def tiny_graph():
    """edge_index int64 [2, 203] over 70 nodes, fixed: destinations in [0, 60), row
    HUB with 50 extra in-edges, eight repeated (j, i) pairs, five self loops, in
    shuffled order."""
    g = torch.Generator().manual_seed(12)
    ei = torch.stack([torch.randint(0, N_NODES, (140,), generator=g), torch.randint(0, N_DST, (140,), generator=g)])
    dup = ei[:, :8]
    loops = torch.randint(0, N_DST, (5,), generator=g).repeat(2, 1)
    hub = torch.stack([torch.randint(0, N_NODES, (50,), generator=g), torch.full((50,), HUB, dtype=torch.int64)])
    ei = torch.cat([ei, dup, loops, hub], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    deg = torch.bincount(ei[1], minlength=N_NODES)
    assert tuple(ei.shape) == (2, N_EDGES) and N_EDGES % 8
    assert int(deg[N_DST:].sum()) == 0 and 50 <= int(deg[HUB]) <= 60 and int(deg.max()) == int(deg[HUB])
    assert int((ei[0] == ei[1]).sum()) >= 5
    assert torch.unique(ei[0] * N_NODES + ei[1]).numel() <= N_EDGES - 8           # duplicate edges
    assert not torch.equal(ei[1], ei[1].sort().values)                               # not in row order
    return ei


def tiny_relations(n_rel):
    """int64 [203]: zeros for one relation; for three, relations 0 and 2 only
    (relation 1 has no edge)."""
    if n_rel == 1:
        return torch.zeros(N_EDGES, dtype=torch.int64)
    assert n_rel == 3
    et = torch.randint(0, 2, (N_EDGES,), generator=torch.Generator().manual_seed(3)) * 2
    assert torch.bincount(et, minlength=3).tolist()[1] == 0 and int(torch.bincount(et, minlength=3).min()) == 0
    return et
