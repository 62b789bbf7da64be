"""CPU tests of the shape lists of tests/_recurrent_lane_cases.py and of the pinned examples of
tests/test_gpu_fuzz_recurrent_layers.py: the lists reach every template instantiation they claim by the
restated dispatch rules, the restated widths and limits agree with the library's, the tiny graph has the
properties the sweep relies on, and the float64 restatements accept every pinned example.  (The forced
schedule's chunk and split rows are asserted where the schedule is built, on the GPU:
tests/test_gpu_recurrent_lane_shapes.py.)"""
import pytest
import torch

from tests import _arma_ref as AR, _fuzz_cases as Z, _ggc_ref as GR, _recurrent_lane_cases as K


def test_arma_cases_reach_every_task_width_in_both_transforms():
    reach = K.arma_reach(K.ARMA_CASES)
    for L in K.ARMA_LANES:
        assert {t for (l, t, _) in reach if l == L} == {"vector", "scalar"}, L
        assert {g for (l, _, g) in reach if l == L} == {"full", "partial"}, L
    required = [(1, 1), (2, 2), (1, 4), (1, 12), (3, 5), (4, 4), (5, 4), (3, 7), (1, 32), (9, 4), (5, 12), (1, 64),
                (17, 4), (5, 13), (3, 24), (2, 64), (33, 4), (17, 15), (64, 4), (256, 1), (8, 32)]
    assert set(required) <= set(K.ARMA_CASES) and len(set(K.ARMA_CASES)) == len(K.ARMA_CASES)
    lanes = {kc: K.arma_lanes(*kc) for kc in K.ARMA_CASES}
    assert [lanes[kc] for kc in required] == [4] * 6 + [8] * 3 + [16] * 3 + [32] * 4 + [64] * 5
    assert (K.arma_width(5, 4), K.arma_width(9, 4), K.arma_width(17, 4), K.arma_width(33, 4)) == (20, 36, 68, 132)
    assert K.arma_lanes(4, 4) == 4 and K.arma_lanes(16, 4) == 16 and K.arma_lanes(32, 4) == 32   # the last widths
    assert any(k * c < 4 for k, c in K.ARMA_CASES) and any(c == 1 for _, c in K.ARMA_CASES)
    assert any(k == 1 and c > 1 for k, c in K.ARMA_CASES)
    assert sum(k * c * c == K.ARMA_MAX_W for k, c in K.ARMA_CASES) >= 2


def test_arma_restatement_agrees_with_the_library():
    from mi355_mp import ops
    for k, c in K.ARMA_CASES:
        assert ops.arma_ok(k, c) and K.arma_ok(k, c), (k, c)
        assert ops.arma_width(k, c) == K.arma_width(k, c), (k, c)
    assert not ops.arma_ok(*K.ARMA_OUTSIDE) and not K.arma_ok(*K.ARMA_OUTSIDE)
    for k in (1, 2, 3, 8, 33, 64, 128, 256, 257):
        for c in (1, 3, 4, 31, 32, 33, 64, 65):
            assert ops.arma_ok(k, c) == K.arma_ok(k, c), (k, c)


def test_gru_widths_reach_every_instantiation():
    from mi355_mp import ops
    assert K.gru_reach(K.GRU_WIDTHS) == set(range(1, 9))
    assert {81, 97, 1} <= set(K.GRU_WIDTHS) and K.gru_width(81) == 96 and K.gru_width(97) == 112
    for c in list(K.GRU_WIDTHS) + [15, 16, 17, 127]:
        assert ops.gru_ok(c) and ops.gru_width(c) == K.gru_width(c), c
    assert not ops.gru_ok(K.GRU_MAX_C + 1) and ops.gru_ok(K.GRU_MAX_C)
    shapes = {P: K.GruShape(P) for P in range(16, 129, 16)}
    assert [(s.waves, s.per_cu, s.bm, s.slices) for s in shapes.values()] == [
        (1, 4, 64, 1), (2, 2, 64, 1), (3, 1, 64, 1), (4, 1, 64, 1)] + [(4, 1, 32, 2)] * 4
    for P in K.GRU_MANY_TILES:
        for cus in (256, 304, 8):
            s, n = shapes[P], K.gru_many_tiles_rows(P, cus)
            tiles, cap = -(-n // s.bm), cus * s.per_cu
            assert n % s.bm == 1 and tiles % cap == 2 and tiles // cap >= 2
            assert P != 128 or n * P // 4 > cus * K.GRU_BWD_BLOCKS_PER_CU * K.GRU_BWD_BLOCK
    assert K.gru_many_tiles_rows(128, 256) * 128 * 4 <= 20e6                 # the largest [N, P] operand, in bytes


def test_agnn_widths_reach_every_mapping_and_group_width():
    maps, groups = K.agnn_reach(K.AGNN_WIDTHS)
    assert maps == K.AGNN_MAPPINGS and groups == {1, 2, 4, 8, 16, 32, 64}
    assert K.AGNN_WIDTHS[:7] == (1, 3, 16, 18, 256, 260, 1024)
    first, _ = K.agnn_reach(K.AGNN_WIDTHS[:7])
    assert first == {(4, 1), (4, 2), (4, 4), (1, 1)}                          # what the seven reached before
    want = {516: (4, 3, 64), 768: (4, 3, 64), 70: (1, 4, 64), 255: (1, 4, 64), 257: (1, 16, 64), 1023: (1, 16, 64),
            2: (1, 1, 2), 7: (1, 1, 8), 8: (4, 1, 2), 13: (1, 1, 16), 36: (4, 1, 16)}
    for F, m in want.items():
        assert K.agnn_mapping(F) == m, F
    from mi355_mp import ops
    assert all(ops.agnn_ok(F) for F in K.AGNN_WIDTHS) and not ops.agnn_ok(1025)


def test_tiny_graph_is_what_it_claims():
    ei = K.tiny_graph()                                                       # asserts its own properties
    assert torch.equal(ei, K.tiny_graph()) and ei.dtype == torch.int64
    lo, hi = K.EMPTY_RUN
    touched = torch.bincount(ei.reshape(-1), minlength=K.N_NODES)
    assert int(touched[lo:hi].sum()) == 0 and hi - lo == 22 and int(touched[K.N_ACTIVE:].sum()) == 0
    assert int(touched[:lo].min()) >= 0 and int(touched[hi:K.N_ACTIVE].sum()) > 0
    # three rows of an L = 4 task's rowptr window: the run of empty rows spans several reloads
    assert (hi - lo) // 3 >= 7
    from mi355_mp.graph import MIN_CHUNK, auto_chunk
    assert MIN_CHUNK == 16 == auto_chunk(K.N_NODES, K.N_EDGES)


def _arma_reference(p):
    ei, ew, x, ws, vs, bias, gout = Z.arma_inputs(p)
    act = p["act"]
    args = (x, ei, ew, ws, vs, bias, p["T"], p["shared"])
    return args, gout, AR.forward(*args, act), AR.forward(*args, act, absolute=True)


def test_pinned_recurrent_examples_are_what_their_comments_say():
    ar = [(p, Z.arma_inputs(p)) for p in Z.ARMA_PINNED]
    gg = [(p, Z.ggc_inputs(p)) for p in Z.GGC_PINNED]
    for p, (ei, ew, x, ws, vs, bias, gout) in ar:
        (k, c), T, shared = p["kc"], p["T"], p["shared"]
        assert p["kc"] in K.ARMA_CASES + (K.ARMA_OUTSIDE,) and p["act"] in ("relu", None)
        assert ei.shape[1] == int(p["N"] * p["deg"]) and tuple(x.shape) == (p["N"], p["F_in"])
        assert (ew is None) == (not p["weighted"]) and (bias is None) == (not p["bias"])
        assert len(ws) == 1 + (min(1, T - 1) if shared else T - 1) and len(vs) == (1 if shared else T)
        assert tuple(ws[0].shape) == (k, p["F_in"], c) and all(tuple(w.shape) == (k, c, c) for w in ws[1:])
        assert bias is None or all(float(b.abs().min()) > 0 for b in bias)
        assert p["form"] in (None, "fused") and (K.arma_ok(k, c) or p["form"] is None)
        if p["loops"] == 1.0:
            assert bool((ei[0] == ei[1]).all())
    shapes = [(p["N"], i[0].shape[1]) for p, i in ar]
    assert (1, 0) in shapes and (5, 0) in shapes
    assert any(p["N"] == 1 and i[0].shape[1] > 0 for p, i in ar)
    assert any(p["loops"] == 1.0 and i[0].shape[1] > 10 for p, i in ar)
    assert any(p["deg"] == 0.3 and int((torch.bincount(i[0].reshape(-1), minlength=p["N"]) == 0).sum()) > 5
               for p, i in ar)
    assert {K.arma_lanes(*p["kc"]) for p, i in ar if K.arma_ok(*p["kc"]) and i[0].shape[1] > 10} == set(K.ARMA_LANES)
    assert any(p["T"] == 3 and p["kc"][0] == 1 for p, _ in ar) and any(p["kc"][1] == 1 for p, _ in ar)
    assert any(not K.arma_ok(*p["kc"]) for p, _ in ar)
    for p, (ei, ew, x, gout) in gg:
        assert ei.shape[1] == int(p["N"] * p["deg"]) and (ew is None) == (not p["weighted"])
        assert x.shape[0] == p["N"] and (x.dim() == 1) == (p["xcols"] == 0)
        assert x.dim() == 1 or x.shape[1] == min(p["xcols"], p["C"])
        assert ew is None or not ew.numel() or (0.25 <= float(ew.min()) and float(ew.max()) < 1.25)
    assert any(p["N"] == 1 and i[2].dim() == 1 for p, i in gg) and any(i[0].shape[1] == 0 and p["N"] > 1 for p, i in gg)
    assert any(p["C"] == 1 for p, _ in gg) and any(p["C"] == 128 and tuple(i[2].shape) == (p["N"], 128) for p, i in gg)
    assert any(not p["bias"] and p["aggr"] == "mean" for p, _ in gg)
    assert {p["flow"] for p, _ in gg} == set(Z.FLOWS)


@pytest.mark.parametrize("k", range(len(Z.ARMA_PINNED)))
def test_arma_reference_alone_meets_the_mask_cap_on_the_pinned_examples(k):
    """At most 0.5 % of the reference's pre-activations lie within the bound of zero (the cap of
    test_gpu_arma._gpu_masks: elsewhere the GPU's ReLU mask must be the reference's own); the output has the
    layer's shape and the gradients those of their parameters."""
    p = Z.ARMA_PINNED[k]
    args, gout, (out, Hs, pres), (a_out, _, a_pres) = _arma_reference(p)
    assert tuple(out.shape) == (p["N"], p["kc"][1]) and len(pres) == p["T"]
    assert bool((a_out >= out.abs() - 1e-12).all())
    close = sum(int((pre.abs() <= AR.BOUND * a).sum()) for pre, a in zip(pres, a_pres))
    total = sum(pre.numel() for pre in pres)
    assert close <= 0.005 * total, "%d of %d pre-activations within the bound of zero" % (close, total)
    grads = AR.gradients(*args, gout, act=p["act"])
    assert grads[0].shape == args[0].shape and [g.shape for g in grads[1]] == [w.shape for w in args[3]]
    assert (grads[3] is None) == (not p["bias"])


@pytest.mark.parametrize("k", range(len(Z.GGC_PINNED)))
def test_ggc_reference_accepts_the_pinned_examples(k):
    p = Z.GGC_PINNED[k]
    ei, ew, x, gout = Z.ggc_inputs(p)
    C, g = p["C"], torch.Generator().manual_seed(p["seed"])
    weight = torch.randn(p["L"], C, C, generator=g, dtype=torch.float64) / max(1.0, C ** 0.5)
    rnn = {"weight_ih": torch.randn(3 * C, C, generator=g, dtype=torch.float64) / max(1.0, C ** 0.5),
           "weight_hh": torch.randn(3 * C, C, generator=g, dtype=torch.float64) / max(1.0, C ** 0.5)}
    if p["bias"]:
        rnn.update(bias_ih=torch.randn(3 * C, generator=g, dtype=torch.float64),
                   bias_hh=torch.randn(3 * C, generator=g, dtype=torch.float64))
    x2 = x if x.dim() == 2 else x.unsqueeze(-1)
    ends = ei if p["flow"] == Z.FLOWS[0] else ei.flip(0)
    out = GR.layer(x2, ends, ew, weight, rnn, p["aggr"])
    assert tuple(out.shape) == (p["N"], C) and out.dtype == torch.float64 and bool(torch.isfinite(out).all())
    if ei.shape[1] == 0:                                   # no edge: every node is the cell on m = 0
        zero = torch.zeros(p["N"], C, dtype=torch.float64)
        h = torch.nn.functional.pad(x2.double(), (0, C - x2.shape[1]))
        for _ in range(p["L"]):
            h, _, _ = GR.cell(zero, h, torch.zeros(C, 3 * C, dtype=torch.float64), rnn["weight_hh"].t(),
                              rnn.get("bias_ih"), rnn.get("bias_hh"))
        assert float((h - out).abs().max()) <= 1e-12
