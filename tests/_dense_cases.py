"""The shapes and inputs the dense family's tests share (tests/test_dense_host.py
measures the fp32 recipe on them, tests/test_gpu_dense.py runs the kernels on
them), and the bounds both hold them to."""
import torch

# |got - want| <= ARRAY_TOL * max(1, |want|) entrywise: the project's bound for softmax layers
ARRAY_TOL = 1e-4
# The two scalar losses, relative: four times the worst relative error of the fp32
# upstream recipe on the CPU against float64 over diff_pool_cases() (measured:
# 7.9e-7, tests/test_dense_host.py::test_fp32_recipe_sets_the_loss_bound), four
# times because the kernels sum in another order than the recipe and both are
# honest fp32; never more than 1e-4.
RECIPE_LOSS_ERR = 7.9e-7
LOSS_RTOL = min(4 * RECIPE_LOSS_ERR, 1e-4)
# With one cluster P is 1 and the entropy is -log(1 + 1e-15): about -1e-15, which
# the float64 restatement itself only knows to 11 % (it returns -1.11e-15) and
# fp32 rounds to 0.  A relative figure measures nothing there, so the entropy's
# error is taken relative to max(|want|, ENT_FLOOR); every case with C > 1 has an
# entropy above 0.3, far from the floor, and the link loss has no floor.
ENT_FLOOR = 1e-6


def loss_err(got, want, floor=0.0):
    """|got - want| / max(|want|, floor); 0 when both are 0."""
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    assert got == got and abs(got) != float("inf"), "a non-finite loss"
    den = max(abs(want), floor)
    return 0.0 if got == want else abs(got - want) / den if den > 0 else float("inf")


ADJ_KINDS = ("01", "01loop", "real")
MASK_KINDS = (None, "part", "empty_graph")


def path_twin(N, C, F):
    """mp_diff_pool_path restated (csrc/mp_dense.hip dp_path), so that collecting
    the GPU tests needs no library; tests/test_dense_host.py holds it to the native one."""
    np_, cp = N | 1, C | 1
    rows = min(N, max(1, 4096 // np_))
    return 0 if N <= 128 and (3 * N * cp + rows * np_) * 4 <= 60 * 1024 else 1


def boundaries(path_fn, C):
    """N = t - 1, t, t + 1 around every N at which the path query changes for this C."""
    out = []
    prev = path_fn(1, C, 1)
    for n in range(2, 4096):
        p = path_fn(n, C, 1)
        if p != prev:
            out += [n - 2, n - 1, n]
        prev = p
    return [n for n in out if n >= 1]


def diff_pool_cases(path_fn):
    """[(B, N, C, F, adj kind, mask kind)]: N in {1, 2, 63, 64, 65, 100} and around
    every path boundary, C in {1, 3, 10, 33, 64, 65}, F in {1, 3, 64, 65, 192}, B in
    {1, 3, 20}, every adjacency and mask kind."""
    shapes = [(1, 1, 1, 1), (3, 2, 3, 3), (20, 63, 10, 64), (1, 64, 33, 65), (3, 65, 64, 192), (20, 100, 10, 192),
              (3, 100, 65, 1), (3, 64, 1, 3), (1, 100, 3, 65)]
    for C in (1, 10, 33, 64):
        shapes += [(3, n, C, 3) for n in boundaries(path_fn, C)]
    return [(B, N, C, F, ADJ_KINDS[i % 3], MASK_KINDS[(i // 3 + i) % 3]) for i, (B, N, C, F) in enumerate(shapes)]


def make_mask(kind, B, N):
    if kind is None:
        return None
    m = torch.ones((B, N), dtype=torch.bool)
    if kind == "part":
        for b in range(1, B):                # graph 0 stays full
            m[b, N - min(N, 1 + (7 * b) % max(N, 1)):] = False
    else:
        m[0] = False                         # every node of graph 0 is masked
        if B > 1 and N > 1:
            m[1, N // 2:] = False
    return m


def make_adj(kind, B, N, g):
    a = torch.randn(B, N, N, generator=g)
    if kind == "real":
        return a                             # asymmetric, real-valued: the pooled level
    a = (a > 0.5).float()                    # asymmetric 0/1
    eye = torch.eye(N).unsqueeze(0)
    return a * (1 - eye) + (eye if kind == "01loop" else 0)


def diff_pool_inputs(case, seed=0):
    """dict(x, adj, s, mask, g_out, g_oa, gl, ge): float32 randn at unit scale."""
    B, N, C, F, adj_kind, mask_kind = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * N + 17 * C + F)
    return {"x": torch.randn(B, N, F, generator=g), "adj": make_adj(adj_kind, B, N, g),
            "s": torch.randn(B, N, C, generator=g), "mask": make_mask(mask_kind, B, N),
            "g_out": torch.randn(B, C, F, generator=g), "g_oa": torch.randn(B, C, C, generator=g),
            "gl": float(torch.randn((), generator=g)) * 50.0, "ge": float(torch.randn((), generator=g))}


def close(got, want, tol=ARRAY_TOL):
    """the worst |got - want| / max(1, |want|), which the array bound caps"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "a non-finite entry survived"
    return float(((got - want).abs() / want.abs().clamp(min=1)).max())
