"""CPU tests of the host side: the C-ABI library loads and exports every
symbol include/mi355_mp.h declares (no compute call without a GPU), the
ctypes signatures mirror the header, and the pure-host logic of the Python
API (MessagePassing argument plumbing, torch_scatter index handling, graph
generators, no-CPU-fallback guard)."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_mp.h")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")])
    from mi355_mp import _lib
    return _lib.load()


def test_library_exports_every_declared_symbol(lib):
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), n


def test_ctypes_signatures_cover_the_header():
    from mi355_mp import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_abi_version_and_error_string(lib):
    import re
    from mi355_mp import _lib
    assert lib.mp_abi_version() == 7
    assert isinstance(lib.mp_last_error(), bytes)
    # the header, the bindings and __graft_entry__.build()'s check agree (round 6:
    # build() still asserted ABI 6 after the bump)
    hdr = open(os.path.join(ROOT, "include", "mi355_mp.h")).read()
    assert int(re.search(r"#define MP_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == lib.mp_abi_version()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.ABI_VERSION" in entry and "mp_abi_version() == 6" not in entry


def test_library_is_bound_to_its_sources(lib, monkeypatch):
    """The library carries the hash of the sources it was compiled from
    (Makefile -> mp_source_hash), equal to the tree's (_lib.source_hash: same
    scheme); a library built from other sources is refused, whatever its
    timestamp says."""
    from mi355_mp import _lib
    assert _lib.library_hash(_lib.DEFAULT_LIB_PATH) == _lib.source_hash()
    assert lib.mp_source_hash().decode() == _lib.source_hash()
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc"), "hash"],
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == _lib.source_hash()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "source_hash", lambda: "0123456789abcdef")
    with pytest.raises(_lib.NativeLibraryStale, match="0123456789abcdef"):
        _lib.load()


def test_tuning_knob_set_query_restore(lib):
    from mi355_mp import _lib
    k = _lib.MP_TUNE_FLAT_VEC1_MIN_BYTES
    default = lib.mp_tune(k, -1)
    assert default == 0
    assert lib.mp_tune(k, 123) == default
    assert lib.mp_tune(k, -1) == 123
    assert lib.mp_tune(k, default) == 123
    assert lib.mp_tune(99, 5) == -1


def test_host_side_sizes_without_gpu(lib):
    # pure host arithmetic of the C-ABI (no device calls)
    assert lib.mp_schedule_n_waves(100, 1000, 256) == 5
    assert lib.mp_schedule_n_waves(0, 0, 256) == 1
    from mi355_mp import _lib
    g = _lib.MpCsr(None, None, None, None, None, None, 1000, 5000, 256, 24, 3, 0, 0)
    assert lib.mp_aggregate_slab_bytes(g, 256, 0) >= 2 * 24 * 256 * 4
    assert lib.mp_aggregate_slab_bytes(g, 256, 2) >= 2 * 2 * 24 * 256 * 4


def test_argument_errors_are_reported(lib):
    from mi355_mp import _lib
    g = _lib.MpCsr(None, None, None, None, None, None, 10, 10, 256, 1, 0, 0, 0)
    rc = lib.mp_aggregate_f32(g, None, None, 0, 4, 0, 0, None, None, 4, None, None, 0, 3, None)
    assert rc == 1 and b"null" in lib.mp_last_error()
    rc = lib.mp_schedule_build(None, 0, 0, 100, 10, None, None, None, None, None, 0, None)
    assert rc == 1 and b"chunk" in lib.mp_last_error()



# ABI 6: every entry point that writes (or reads) a caller-allocated partial,
# workspace or per-edge array whose size the call's own row / edge counts do not
# fix takes the array's extent in bytes and rejects a short one before any
# launch.  (Round 4's sharded GAT backward sized att_part for the rank's own rows
# while the finish pass covers own + halo rows: a device write past the end.)
# Each case: (entry point, argument builder(extent) -> args, the exact extent
# the call needs, the buffer name the error names).
def _extent_cases():
    from mi355_mp import _lib
    lib = _lib.load()
    D = 0x7F0000000000            # fake device pointer: never dereferenced, the check fails first
    n_own, n, H, C = 1000, 1700, 8, 32
    F = H * C
    blocks = int(lib.mp_gat_bwd_blocks(n))
    gt = _lib.MpCsr(D, D, D, D, D, D, n, 9000, 256, int(lib.mp_schedule_n_waves(n, 9000, 256)), 0, n_own, 0)
    slab = lib.mp_gat_slab_bytes(gt, H, C)
    Cw = 36
    Fw = H * Cw
    wslab = lib.mp_gat_train_slab_bytes(gt, H, Cw)
    E, R, Fa = 5000, 300, 200
    W = int(lib.mp_arg_mask_words(Fa))
    ga = _lib.MpCsr(D, D, D, D, D, D, 400, E, 256, int(lib.mp_schedule_n_waves(400, E, 256)), 0, R, 0)
    return [
        ("mp_gat_backward_finish_f32", lambda b: (None, D, D, D, D, n, H, C, D, b, None),
         blocks * 2 * F * 4, "att_part"),
        ("mp_gat_backward_prep_f32", lambda b: (D, F, D, F, None, D, D, n, H, C, D, b, None, 0, None), n * H * 16, "pack"),
        ("mp_gat_backward_prep_f32", lambda b: (D, F, D, F, None, D, D, n, H, C, D, n * H * 16, D, b, None),
         blocks * F * 4, "gsum_part"),
        ("mp_gat_backward_prep_train_f32", lambda b: (D, F, D, F, None, D, D, D, D, n, H, C, D, b, None, 0, D, None),
         n * H * 16, "pack"),
        ("mp_gat_backward_prep_train_f32",
         lambda b: (D, F, D, F, None, D, D, D, D, n, H, C, D, n * H * 16, D, b, D, None),
         blocks * F * 4, "gsum_part"),
        ("mp_gat_backward_prep_wide_f32", lambda b: (D, Fw, D, Fw, None, D, D, D, D, n, H, Cw, D, b, D, None),
         n * H * 16, "pack"),
        ("mp_col_sums_f32", lambda b: (D, F, n, F, D, b, None), blocks * F * 4, "part"),
        ("mp_gat_backward_f32", lambda b: (gt, D, F, D, D, D, D, H, C, 0.2, D, D, D, b, D, slab, 7, None),
         9000 * H * 4, "de"),
        ("mp_gat_backward_wide_f32", lambda b: (gt, D, Fw, D, D, H, Cw, 0.2, 0, 0.0, None, D, D, b, D, n * H * 4, D, wslab,
                                                7, None), n * Fw * 4, "acc2"),
        ("mp_gat_backward_wide_f32", lambda b: (gt, D, Fw, D, D, H, Cw, 0.2, 0, 0.0, None, D, D, n * Fw * 4, D, b, D, wslab,
                                                7, None), n * H * 4, "sc"),
        ("mp_arg_winner_mask", lambda b: (D, R, Fa, E, D, D, b, None), E * W * 4, "mask"),
        ("mp_scatter_arg_backward_csr_f32", lambda b: (ga, D, b, D, Fa, Fa, None, D, Fa, None), E * W * 4, "mask"),
        ("mp_scatter_arg_grad_w_f32", lambda b: (D, D, E, D, D, b, Fa, D, Fa, D, Fa, D, None), E * W * 4, "mask"),
        # ABI 7: the GAT merge list's pieces (PPI conv3's 6 x 124 heads)
        ("mp_gat_merge_partials_f32", lambda b: (n, 6, 124, D, D, 300, D, b, 744, D, 300 * 6 * 8, None, D, 744, D,
                                                 None, None, None), 300 * 744 * 4, "part_out"),
        ("mp_gat_merge_partials_f32", lambda b: (n, 6, 124, D, D, 300, D, 300 * 744 * 4, 744, D, b, None, D, 744, D,
                                                 None, None, None), 300 * 6 * 8, "part_stats"),
    ]


def test_every_partial_array_carries_its_extent(lib):
    """One rejection test per ABI-6 extent: a buffer one byte (or, for
    att_part, the round-4 rank's own rows) short is MP_ERR_ARG with the
    buffer's name in the error text; checked on the host before any HIP call
    (this container has no GPU, so an accepted call would fail later with
    MP_ERR_HIP -- the harness under ASAN checks that side,
    test_abi_rejections_under_asan)."""
    cases = _extent_cases()
    assert {c[0] for c in cases} >= {"mp_gat_backward_finish_f32", "mp_gat_backward_prep_f32",
                                     "mp_gat_backward_prep_train_f32", "mp_gat_backward_prep_wide_f32",
                                     "mp_col_sums_f32", "mp_gat_backward_f32", "mp_gat_backward_wide_f32",
                                     "mp_arg_winner_mask", "mp_scatter_arg_backward_csr_f32",
                                     "mp_scatter_arg_grad_w_f32", "mp_gat_merge_partials_f32"}
    for name, args, need, what in cases:
        for short in (need - 1, 0):
            rc = getattr(lib, name)(*args(short))
            err = lib.mp_last_error().decode()
            assert rc == 1 and what in err and str(need) in err, (name, short, rc, err)
    # the round-4 sizing: att_part for the rank's own rows, the pass over own + halo rows
    blocks_own = int(lib.mp_gat_bwd_blocks(1000))
    rc = lib.mp_gat_backward_finish_f32(None, 1 << 40, 1 << 40, 1 << 40, 1 << 40, 1700, 8, 32, 1 << 40,
                                        blocks_own * 2 * 256 * 4, None)
    assert rc == 1 and b"att_part" in lib.mp_last_error()


def test_workspace_one_byte_short_is_rejected(lib):
    """Every entry point that carves a caller-allocated workspace rejects one of
    mp_*_workspace() - 1 bytes before any launch: the size function and the
    entry point read one layout (csrc/mp_workspace.h), so an array added to one
    cannot be forgotten in the other."""
    D = 0x7F0000000000            # fake device pointer: never dereferenced, the check fails first
    N, E, F = 1000, 3000, 33
    nw = lib.mp_schedule_n_waves(N, E, 256)
    cases = [
        ("mp_csr_build", lib.mp_csr_build_workspace(E, N), lambda b: (D, D, E, N, N, D, D, D, D, D, b, None)),
        ("mp_schedule_build", lib.mp_schedule_workspace(nw), lambda b: (D, N, E, 256, 24, D, D, D, D, D, b, None)),
        ("mp_self_loops", lib.mp_self_loops_workspace(E, N), lambda b: (D, D, E, N, 2, E - 5, D, D, D, D, b, None)),
        ("mp_shard_plan", lib.mp_shard_plan_workspace(E, N),
         lambda b: (D, D, E, N, D, 2, 0, 0, N // 2, D, D, D, D, D, D, b, None)),
        ("mp_pool_score_bwd_f32", lib.mp_pool_score_bwd_workspace(N, F),
         lambda b: (D, F, N, F, D, 1, D, D, D, F, D, F * 4, D, b, None)),
        ("mp_topk_select_f32", lib.mp_topk_workspace(N, 7, 64),
         lambda b: (D, N, D, 7, 64, 0.5, D, N * 8, D, 64, D, N * 8, D, D, b, None)),
        ("mp_pool_compact", lib.mp_pool_compact_workspace(N), lambda b: (D, N, D, N * 8, D, D, b, None)),
        ("mp_pool_filter_adj", lib.mp_pool_filter_workspace(E), lambda b: (D, D, E, D, N, D, D, D, E * 8, D, D, b, None)),
        ("mp_cluster_build", lib.mp_cluster_build_workspace(N),
         lambda b: (D, N, D, N * 8, D, (N + 1) * 4, D, N * 4, D, N * 8, D, D, b, None)),
        ("mp_cluster_edges", lib.mp_cluster_edges_workspace(E, N),
         lambda b: (D, D, E, D, N, D, D, D, D, E * 8, D, (E + 1) * 4, D, E * 4, D, b, None)),
    ]
    assert cases[5][1] == 256                                      # the on-chip select paths
    for graphs in (1, 3):                                          # the sorted path: one graph, several
        need = lib.mp_topk_workspace(10000, graphs, 10000)
        assert need > 2 * 10000 * 8
        cases.append(("mp_topk_select_f32", need,
                      lambda b, g=graphs: (D, 10000, D, g, 10000, 0.5, D, 80000, D, (g + 1) * 8, D, 80000, D, D, b, None)))
    assert len({c[0] for c in cases}) == 10 and len(cases) == 12
    for name, need, args in cases:
        assert need >= 256, name
        rc = getattr(lib, name)(*args(need - 1))
        err = lib.mp_last_error().decode()
        assert rc == 1 and name in err, (name, need, rc, err)
        assert "workspace too small" in err or "ws holds %d bytes, the call needs %d" % (need - 1, need) in err, err


def test_extent_arguments_in_the_header():
    """Every ABI-6 extent is declared next to its array in include/mi355_mp.h and
    in the ctypes signatures (size_t after the pointer)."""
    from mi355_mp import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    want = {"mp_gat_backward_finish_f32": ["att_part"], "mp_gat_backward_prep_f32": ["pack", "gsum_part"],
            "mp_gat_backward_prep_train_f32": ["pack", "gsum_part"], "mp_gat_backward_prep_wide_f32": ["pack"],
            "mp_col_sums_f32": ["part"], "mp_gat_backward_f32": ["de"], "mp_gat_backward_wide_f32": ["acc2", "sc"],
            "mp_arg_winner_mask": ["mask"], "mp_scatter_arg_backward_csr_f32": ["mask"],
            "mp_scatter_arg_grad_w_f32": ["mask"], "mp_gat_merge_partials_f32": ["part_out", "part_stats"]}
    for fn, arrays in want.items():
        decl = re.search(r"\b%s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        for a in arrays:
            i = next(k for k, p in enumerate(params) if re.search(r"\*\s*%s$" % a, p))
            assert params[i + 1] == "size_t %s_bytes" % a, (fn, a, params[i + 1])
            assert _lib.SIGNATURES[fn][1][i + 1] is _lib.sz, (fn, a)


def test_abi_rejections_under_asan():
    """The host-side AddressSanitizer build of the library (make asan: device
    code as usual, host code under -fsanitize=address) and the C harness
    tests/abi/abi_reject.c: every entry point's argument checks -- null
    pointers, bad sizes and shapes, short workspaces and ABI-6 extents (each
    also at its exact extent, which must pass the checks) -- run without a
    host memory error, each rejection naming its argument."""
    csrc = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
    subprocess.check_call(["make", "-s", "-j8", "-C", csrc, "asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    env.pop("LD_PRELOAD", None) if "asan" in env.get("LD_PRELOAD", "") else None
    r = subprocess.run([os.path.join(csrc, "build", "asan", "abi_reject")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    m = re.match(r"abi_reject: (\d+) cases, 0 failures", last)
    assert m and int(m.group(1)) >= 100, last
    # every extent rejection and the matching exact-extent acceptance ran
    assert r.stdout.count("holds") >= 19
    assert "att_part holds 512000 bytes" in r.stdout       # the round-4 own-rows sizing, rejected


def test_column_array_requires_n_cols(lib):
    """A graph with a gather column but n_cols = 0 (e.g. a C caller that left the
    last mp_csr field zero) is rejected before anything is launched: n_cols bounds
    the 32-bit buffer offsets and selects the kernel shape."""
    from mi355_mp import _lib
    fake = 0x1000  # never dereferenced: the argument check fails first
    g = _lib.MpCsr(fake, fake, fake, fake, fake, None, 10, 40, 256, 1, 0, 0, 0)
    rc = lib.mp_aggregate_f32(g, None, fake, 4, 4, 0, 0, None, fake, 4, None, fake, 1 << 20, 3, None)
    assert rc == 1 and b"n_cols" in lib.mp_last_error()
    buf = __import__("ctypes").create_string_buffer(256)
    rc = lib.mp_aggregate_kernel_name(g, None, fake, 4, 4, 0, None, fake, 4, buf, 256, None)
    assert rc == 1 and b"n_cols" in lib.mp_last_error()
    # identity gather (col = NULL) needs no n_cols
    g2 = _lib.MpCsr(fake, None, fake, fake, fake, None, 10, 40, 256, 1, 0, 0, 0)
    rc = lib.mp_aggregate_f32(g2, None, fake, 4, 4, 0, 0, None, fake, 4, None, None, 0, 3, None)
    assert rc == 1 and b"slab" in lib.mp_last_error()


def test_tune_table_keys(lib):
    from mi355_mp import _lib
    for key in (_lib.MP_TUNE_FLAT_VEC1_MIN_BYTES, _lib.MP_TUNE_FLAT_SMEM, _lib.MP_TUNE_FLAT_MIN_F,
                _lib.MP_TUNE_FLAT_MIN_F_ARG, _lib.MP_TUNE_FLAT_NARROW_VEC1, _lib.MP_TUNE_FLAT_VEC,
                _lib.MP_TUNE_FLAT_VEC_ARG, _lib.MP_TUNE_FLAT_SEQ_TILES, _lib.MP_TUNE_FLAT_FAR_MIN_BYTES,
                _lib.MP_TUNE_GAT_BWD_VEC):
        v = lib.mp_tune(key, -1)
        assert v >= 0
        assert lib.mp_tune(key, v) == v
    assert lib.mp_tune(_lib.MP_TUNE_FLAT_MIN_F, -1) == 64
    assert lib.mp_tune(_lib.MP_TUNE_FLAT_MIN_F_ARG, -1) == 64
    assert lib.mp_tune(_lib.MP_TUNE_FLAT_NARROW_VEC1, -1) == 64
    assert lib.mp_tune(_lib.MP_TUNE_FLAT_SEQ_TILES, -1) == 0
    assert lib.mp_tune(_lib.MP_TUNE_GAT_BWD_VEC, -1) == 4           # 256-feature tiles (A/B default)
    assert lib.mp_tune(_lib.MP_TUNE_GAT_BWD_VEC, 3) == -1           # 1, 2 or 4 only
    assert lib.mp_tune(99, 1) == -1


def test_no_cpu_fallback_guard():
    import torch_scatter
    from mi355_mp import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch_scatter.scatter_add(torch.ones(3, 2), torch.tensor([0, 1, 0]), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_reduce(torch.ones(3, 2), torch.tensor([0, 1, 0]), 2)


def test_torch_scatter_index_broadcast_logic():
    from torch_scatter import _index_1d
    src = torch.zeros(5, 3)
    idx = torch.tensor([0, 2, 1, 0, 2])
    assert torch.equal(_index_1d(src, idx, 0), idx)
    assert torch.equal(_index_1d(src, idx.view(-1, 1).expand(5, 3), 0), idx)
    assert torch.equal(_index_1d(src, idx.view(-1, 1).repeat(1, 3), 0), idx)
    assert _index_1d(src, torch.arange(15).view(5, 3) % 3, 0) is None     # element-wise: general path
    with pytest.raises(ValueError):
        _index_1d(src, torch.tensor([0, 1]), 0)


def test_message_passing_collect_and_distribute_on_host():
    from torch_geometric.nn import MessagePassing

    class M(MessagePassing):
        def __init__(self):
            super(M, self).__init__(aggr="add")

        def message(self, x_i, x_j, edge_index_i, size_j, norm):
            return x_j

        def update(self, aggr_out, x):
            return aggr_out

    m = M()
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    x = torch.arange(12.).view(3, 4)
    kw = m.__collect__(ei, [None, None], {"x": x, "norm": torch.ones(3)})
    assert torch.equal(kw["x_j"], x[ei[0]]) and torch.equal(kw["x_i"], x[ei[1]])
    assert kw["size"] == [3, 3] and kw["size_j"] == 3 and torch.equal(kw["index"], ei[1])
    msg = m.__distribute__(m.__msg_params__, kw)
    assert sorted(msg) == ["edge_index_i", "norm", "size_j", "x_i", "x_j"]
    # bipartite tuple input sets both sizes; a size mismatch raises
    kw = m.__collect__(ei, [None, None], {"x": (x, x[:3]), "norm": None})
    assert kw["size"] == [3, 3]
    with pytest.raises(ValueError):
        m.__collect__(ei, [5, None], {"x": x, "norm": None})
    with pytest.raises(TypeError):
        m.__distribute__(m.__msg_params__, {k: v for k, v in kw.items() if k != "norm"} |
                         {"norm": __import__("inspect").Parameter.empty})


def test_flow_target_to_source_swaps_roles():
    from torch_geometric.nn import MessagePassing
    m = MessagePassing(flow="target_to_source")
    ei = torch.tensor([[0, 1], [2, 3]])
    x = torch.arange(4.).view(4, 1)
    kw = m.__collect__(ei, [None, None], {"x": x})
    assert torch.equal(kw["x_j"], x[ei[1]]) and torch.equal(kw["index"], ei[0])


def test_graph_generators_deterministic_and_shaped():
    from mi355_mp.graphgen import rmat_edge_index, powerlaw_edge_index, cora_like
    a = rmat_edge_index(scale=10, n_samples=5000, seed=3)
    b = rmat_edge_index(scale=10, n_samples=5000, seed=3)
    assert torch.equal(a, b) and a.shape == (2, 10000) and int(a.max()) < 1024
    # symmetric: (u,v) present iff (v,u) present
    assert torch.equal(a[0, :5000], a[1, 5000:])
    p = powerlaw_edge_index(1000, 4000, seed=1)
    assert p.shape == (2, 4000) and int(p.max()) < 1000
    deg = torch.bincount(p[1], minlength=1000)
    assert int(deg.max()) > 8 * float(deg.float().mean())   # power law: hubs
    d = cora_like()
    assert d["x"].shape == (2708, 1433) and d["edge_index"].shape == (2, 10556)
    assert torch.allclose(d["x"].sum(1), torch.ones(2708))
    assert int(d["train_mask"].sum()) == 140


def test_loop_utilities_host_tensors_match_oracle():
    """utils.loop on host tensors (CPU preprocessing, e.g. a dataset transform)
    takes the torch form of the rewrite: order, loop weights (last duplicate
    loop wins) and fills equal to the oracle's sequential restatement.  Device
    tensors run mp_self_loops (GPU parity: test_gpu_parity.py
    test_self_loop_utilities_bit_exact); the aggregation itself still has no CPU
    path (test_no_cpu_fallback)."""
    from torch_geometric.utils import add_remaining_self_loops, add_self_loops, remove_self_loops
    from oracle import pyg_ref as P
    ei = torch.tensor([[0, 1, 1, 2, 2, 1], [1, 1, 2, 0, 2, 1]])
    w = torch.tensor([1., 2., 3., 4., 5., 6.])
    r_ei, r_w = P.add_remaining_self_loops(ei, w, 2, 4)
    assert r_w.tolist()[-4:] == [2., 6., 5., 2.]
    assert r_ei[:, :3].tolist() == [[0, 1, 2], [1, 2, 0]]
    g = torch.Generator().manual_seed(3)
    for ei_, w_ in ((ei, w), (torch.randint(40, (2, 500), generator=g), torch.rand(500, generator=g))):
        N = int(ei_.max()) + 3
        for fill in (1, 2):
            a = add_remaining_self_loops(ei_, w_, fill, N)
            b = P.add_remaining_self_loops(ei_, w_, fill, N)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = add_self_loops(ei_, w_, 3.0, N)
        b = P.add_self_loops(ei_, w_, 3.0, N)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = remove_self_loops(ei_, w_)
        b = P.remove_self_loops(ei_, w_)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(IndexError):
        add_remaining_self_loops(torch.tensor([[0, 7], [1, 7]]), num_nodes=3)


def test_data_batch_semantics():
    from torch_geometric.data import Data, Batch, DataLoader, DataListLoader
    d1 = Data(x=torch.randn(3, 4), edge_index=torch.tensor([[0, 1, 2], [1, 2, 0]]), y=torch.tensor([1]),
              mask=torch.tensor([True, False, True]))
    d2 = Data(x=torch.randn(2, 4), edge_index=torch.tensor([[0], [1]]), y=torch.tensor([0]),
              mask=torch.tensor([False, True]))
    assert d1.num_nodes == 3 and d1.num_edges == 3 and d1.num_node_features == 4
    assert Data(edge_index=torch.tensor([[0, 5], [1, 2]])).num_nodes == 6
    assert Data(edge_index=torch.tensor([[0], [1]]), num_nodes=10).num_nodes == 10
    b = Batch.from_data_list([d1, d2], follow_batch=["x"])
    # edge_index offset by the running node count, concatenated along the last dim
    assert b.edge_index.tolist() == [[0, 1, 2, 3], [1, 2, 0, 4]]
    assert b.batch.tolist() == [0, 0, 0, 1, 1] and b.num_graphs == 2
    assert torch.equal(b.x, torch.cat([d1.x, d2.x])) and b.y.tolist() == [1, 0]
    assert b.mask.tolist() == [True, False, True, False, True]        # bool: never offset
    assert b.x_batch.tolist() == [0, 0, 0, 1, 1]
    assert d1.contains_self_loops() is False and d1.is_undirected() is False
    lists = list(DataListLoader([d1, d2, d1], batch_size=2))
    assert isinstance(lists[0], list) and len(lists[0]) == 2 and len(lists[1]) == 1
    batches = list(DataLoader([d1, d2, d1], batch_size=3))
    assert isinstance(batches[0], Batch) and batches[0].num_graphs == 3


def test_data_parallel_split_points():
    from torch_geometric.nn.data_parallel import split_points
    assert split_points([10, 10, 10, 10], 2) == [0, 2, 4]
    assert split_points([100, 1, 1, 1], 2) == [0, 1, 4]
    assert split_points([5, 5, 5], 8) == [0, 1, 2, 3]                  # at most one chunk per graph
    s = split_points([3, 9, 1, 7, 7, 2, 8, 4], 4)
    assert s[0] == 0 and s[-1] == 8 and all(a <= b for a, b in zip(s, s[1:]))


def test_torch_scatter_dispatcher_ops_registered():
    import torch_scatter  # noqa: F401  (registers torch.ops.torch_scatter.*)
    names = ["scatter_max", "scatter_min", "segment_sum_csr", "segment_mean_csr", "segment_min_csr",
             "segment_max_csr", "gather_csr", "segment_sum_coo", "segment_mean_coo", "segment_min_coo",
             "segment_max_coo", "gather_coo"]
    for n in names:
        assert hasattr(torch.ops.torch_scatter, n), n
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.torch_scatter.segment_sum_csr(torch.ones(3, 2), torch.tensor([0, 2, 3]), None)



def _bench(args, env_extra, timeout=240):
    import sys
    env = dict(os.environ, MP_BENCH_LAUNCH_PROBE="1", MASTER_ADDR="127.0.0.1", **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` with no launcher (RANK unset) starts N rank
    processes itself (a torch.distributed.run child) and every rank sees a world
    of N -- the driver's plain `--gpus 8` call must never silently run one
    GPU.  MP_BENCH_LAUNCH_PROBE stops the ranks right after the process group
    is up (gloo, no GPU touched)."""
    import json
    r = _bench(["bench.py", "--gpus", "3", "--steps", "1"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    # the JSON line alone on stdout: gloo's connection lines (and RCCL's banner on
    # a node) go to stderr (bench.claim_stdout)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    assert d["gpus"] == 3
    assert sorted(p["rank"] for p in d["launch_probe"]) == [0, 1, 2]
    assert all(p["world"] == 3 for p in d["launch_probe"])
    assert "starting 3 ranks" in r.stderr


def test_bench_config4_workload_is_one_gpu():
    """--workload reddit (BASELINE config 4, a one-GPU configuration) with
    --gpus 2 exits non-zero before launching ranks or touching a GPU."""
    r = _bench(["bench.py", "--gpus", "2", "--workload", "reddit"], {})
    assert r.returncode == 2, r.stderr[-2000:]
    assert "one-GPU configuration" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_refuses_a_world_that_differs_from_gpus():
    """Launched by torch.distributed.run with 2 ranks but --gpus 3: every rank
    exits non-zero before any work (no line claiming n_gpus it did not use)."""
    port = __import__("socket").socket()
    port.bind(("127.0.0.1", 0))
    p = port.getsockname()[1]
    port.close()
    r = _bench(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(p), "bench.py", "--gpus", "3"], {})
    assert r.returncode != 0
    assert "the job has 2 ranks but --gpus 3" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_arg_backward_has_no_atomic_form(lib):
    """ABI 5: mp_scatter_arg_backward_f32 is the plain-store form only (message
    row e belongs to one output row); the float-atomic src_map / grad_w form of
    ABI <= 4 -- non-deterministic, unused -- is gone from the header, the
    ctypes signature and the kernel."""
    from mi355_mp import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int mp_scatter_arg_backward_f32\((.*?)\);", text, flags=re.S).group(1)
    assert "src_map" not in decl and "grad_w" not in decl and decl.count(",") == 7
    assert len(_lib.SIGNATURES["mp_scatter_arg_backward_f32"][1]) == 8
    src = open(os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc", "mp_misc.hip")).read()
    body = src[src.index("void k_scatter_arg_backward"):]
    body = body[:body.index("\n}\n")]
    assert "atomic" not in body


def test_loop_utilities_host_no_edges_with_weights():
    """add_self_loops / add_remaining_self_loops on host tensors with E == 0
    edges and an empty weight vector: the N loops with the fill value, as
    upstream's concatenation gives (no gather from the empty weights)."""
    from torch_geometric.utils import add_remaining_self_loops, add_self_loops, remove_self_loops
    from oracle import pyg_ref as P
    ei = torch.zeros((2, 0), dtype=torch.long)
    w = torch.zeros(0)
    for fn, ref in ((add_self_loops, P.add_self_loops), (add_remaining_self_loops, P.add_remaining_self_loops)):
        a = fn(ei, w, 2.0, 4)
        b = ref(ei, w, 2.0, 4)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[0].tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]] and a[1].tolist() == [2.0] * 4
    a = remove_self_loops(ei, w)
    assert a[0].shape == (2, 0) and a[1].numel() == 0
    # the weight gradient still flows through the host rewrite
    wr = torch.rand(3, requires_grad=True)
    _, ww = add_remaining_self_loops(torch.tensor([[0, 1, 1], [1, 1, 0]]), wr, 1.0, 3)
    ww.sum().backward()
    assert wr.grad.tolist() == [1.0, 1.0, 1.0]


def test_torch_scatter_dispatcher_ops_under_fake_tensors():
    """Every torch.ops.torch_scatter.* op propagates shapes under FakeTensorMode
    (register_fake kernels: no data_ptr, no launch) -- static sizes where
    dim_size / out / the index length fix them, data-dependent ones (like
    nonzero's) under a ShapeEnv; each op also has a registered backward."""
    import torch_scatter  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    ops = torch.ops.torch_scatter
    with FakeTensorMode(shape_env=ShapeEnv()) as m:
        src = m.from_tensor(torch.randn(6, 3, 2))
        idx = m.from_tensor(torch.tensor([0, 0, 1, 2, 2, 2]))
        ptr = m.from_tensor(torch.tensor([0, 2, 3, 6]))
        o, a = ops.scatter_max(src, idx, 0, None, 5)
        assert o.shape == (5, 3, 2) and a.shape == (5, 3, 2) and a.dtype == torch.int64
        o, a = ops.scatter_min(src, m.from_tensor(torch.zeros(2, dtype=torch.long)), 2, None, 4)
        assert o.shape == (6, 3, 4) and a.dtype == torch.int64
        o, _ = ops.scatter_max(src, idx, 0, m.from_tensor(torch.zeros(7, 3, 2)), None)
        assert o.shape == (7, 3, 2)
        for n in ("segment_sum_csr", "segment_mean_csr"):
            assert getattr(ops, n)(src, ptr, None).shape == (3, 3, 2)
        for n in ("segment_min_csr", "segment_max_csr"):
            o, a = getattr(ops, n)(src, ptr, None)
            assert o.shape == (3, 3, 2) and a.dtype == torch.int64
        for n in ("segment_sum_coo", "segment_mean_coo"):
            assert getattr(ops, n)(src, idx, None, 4).shape == (4, 3, 2)
        for n in ("segment_min_coo", "segment_max_coo"):
            o, a = getattr(ops, n)(src, idx, None, 4)
            assert o.shape == (4, 3, 2) and a.dtype == torch.int64
        assert ops.gather_coo(m.from_tensor(torch.randn(3, 5)), idx, None).shape == (6, 5)
        # data-dependent row counts become unbacked symbolic sizes
        g = ops.gather_csr(m.from_tensor(torch.randn(3, 5)), ptr, None)
        assert isinstance(g.shape[0], torch.SymInt) and g.shape[1] == 5
        s = ops.segment_sum_coo(src, idx, None, None)
        assert isinstance(s.shape[0], torch.SymInt)
    for n in ("scatter_max", "scatter_min", "segment_sum_csr", "segment_mean_csr", "segment_min_csr",
              "segment_max_csr", "gather_csr", "segment_sum_coo", "segment_mean_coo", "segment_min_coo",
              "segment_max_coo", "gather_coo"):
        op = getattr(ops, n).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), n
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "Autograd"), n


def test_bench_verify_max_matches_the_serial_loop():
    """bench.py's chunked max + first-index argmax verifier (the config-4
    workload's --verify) agrees with the oracle's serial scatter_max loop on a
    tie-heavy graph with empty rows, and rejects a moved argmax."""
    import bench
    from oracle import scatter_ref as S
    g = torch.Generator().manual_seed(13)
    N, E, F = 300, 5000, 9
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, N - 20, (E,), generator=g)         # the last 20 rows stay empty
    x = torch.randint(-3, 4, (N, F), generator=g).float()
    out, arg = S.scatter_loop(x[src], dst, N, "max")
    out = torch.where(out < -10000, torch.zeros_like(out), out)
    v = bench.verify_max(out, arg, x, src, dst, step=777)
    assert v["values_bitwise_equal"] and v["args_bitwise_equal"], v
    bad = arg.clone()
    r = int(dst[0])
    bad[r, 0] = E - 1 if bad[r, 0] != E - 1 else 0
    assert not bench.verify_max(out, bad, x, src, dst)["args_bitwise_equal"]


def test_bench_dump_outputs_and_full_option(tmp_path):
    """bench.py --dump-outputs: every array as DIR/<name>.npy (N>1: one file per
    rank), float32 (integer arrays float64, exact), at most DUMP_ROWS rows in
    all -- of a larger output the same seeded rows in every run and for every
    array of a step; --full is off unless asked for."""
    import numpy as np
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs == "" and a.steps == 3
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    n = bench.DUMP_ROWS + 1001
    out = torch.arange(n, dtype=torch.float32).view(-1, 1) * torch.ones(1, 3)
    arg = torch.arange(n, dtype=torch.int64).view(-1, 1) + (1 << 40) * torch.ones(1, 3, dtype=torch.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out": out, "arg": arg}, 0, 1, False)
    o, g = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "a" / "arg.npy")
    assert o.dtype == np.float32 and g.dtype == np.float64
    assert o.shape == g.shape == (bench.DUMP_ROWS // 2, 3)
    assert o.nbytes + g.nbytes <= 64 << 20
    rows = o[:, 0].astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows.max() < n           # distinct rows of the output, in order
    assert np.array_equal(g[:, 0], rows + float(1 << 40))          # the same rows, integers exact
    assert np.array_equal(o, np.load(tmp_path / "b" / "out.npy"))
    small = torch.randn(5, 4, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "c"), {"out": small}, 1, 2, True)
    s = np.load(tmp_path / "c" / "out_rank1.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())


def test_halo_tile_widths():
    """Feature tilings of the sharded step: uniform widths (the last tile takes
    the rest) or an explicit list that must cover F exactly."""
    from mi355_mp import dist as mdist
    assert mdist.tile_widths(256, 128) == [128, 128]
    assert mdist.tile_widths(200, 128) == [128, 72]
    assert mdist.tile_widths(256, [64, 128, 64]) == [64, 128, 64]
    for bad in ([64, 64], [0, 256], [128, 129]):
        with pytest.raises(ValueError):
            mdist.tile_widths(256, bad)


def test_hidden_fraction_is_null_when_pieces_are_not_comparable():
    """The step decomposition's hidden_frac: the r05 P = 2
    gloo rehearsal's sample -- exchange alone 230 ms, longer than the whole
    serial step of 212 ms -- gives None with the reason; a ratio outside
    [-1, 1] and an empty exchange give None too; a node-like sample keeps its
    number."""
    from mi355_mp.dist import hidden_fraction
    gloo = {"exchange_only_ms": 230.4, "compute_only_ms": 4.3, "serial_step_ms": 212.0, "overlapped_step_ms": 215.1}
    h = hidden_fraction(gloo)
    assert h["hidden_frac"] is None and not h["hidden_frac_valid"] and "exceeds the serial step" in h["hidden_frac_note"]
    odd = {"exchange_only_ms": 2.0, "compute_only_ms": 1.0, "serial_step_ms": 3.1, "overlapped_step_ms": 0.5}
    assert hidden_fraction(odd)["hidden_frac"] is None          # (2 + 1 - 0.5) / 1 = 2.5
    one_rank = {"exchange_only_ms": 0.0, "compute_only_ms": 6.6, "serial_step_ms": 6.6, "overlapped_step_ms": 6.6}
    assert hidden_fraction(one_rank)["hidden_frac"] is None
    staged = hidden_fraction({"exchange_only_ms": 100.0, "compute_only_ms": 4.3, "serial_step_ms": 120.0,
                              "overlapped_step_ms": 101.0}, staged=True)
    assert staged["hidden_frac"] is None and "gloo" in staged["hidden_frac_note"]
    node = {"exchange_only_ms": 0.30, "compute_only_ms": 0.91, "serial_step_ms": 1.20, "overlapped_step_ms": 1.04}
    h = hidden_fraction(node)
    assert h["hidden_frac_valid"] and abs(h["hidden_frac"] - (0.30 + 0.91 - 1.04) / 0.30) < 1e-12
