"""The dispatch table of the plain aggregation, pinned.

mp_aggregate_kernel_name answers "which main kernel would mp_aggregate_f32 run
for these arguments" without dereferencing anything, so every case below is a
name lookup on fake addresses and a hand-built MpCsr: no kernel, no allocation.
tests/golden/agg_dispatch.json holds the names recorded before the dispatch
became a value (choose() -> AggLaunch); the choice must not move.

The grid reaches every arm of the choice: reduce x weights x row width x
operand layout, x sizes below / above the Infinity Cache / above 4 GiB, the
identity gather, and each mp_tune dispatch key once away from its default."""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_dispatch.json")

REDUCES = ("sum", "mean", "max", "min")
WIDTHS = (1, 2, 4, 8, 9, 16, 32, 63, 64, 65, 66, 128, 130, 200, 256, 260, 512)
LAYOUTS = ("aligned", "ldx+1", "ldx+2", "ldx+4", "x+4", "x+8", "out+4", "bias+4")
ROWS_FIT, ROWS_FAR, ROWS_4G = 1000, 300000, 4400000   # x at F = 256: 1 MB, 307 MB (> 256 MiB), 4.5 GB (> 4 GiB)
TUNES = ("FLAT_SMEM=0", "FLAT_VEC=4", "FLAT_VEC_ARG=1", "FLAT_VEC_ARG=4", "FLAT_MIN_F=128", "FLAT_MIN_F_ARG=128",
         "FLAT_NARROW_VEC1=0", "FLAT_VEC1_MIN_BYTES=%d" % (1 << 40), "FLAT_FAR_MIN_BYTES=1",
         # beyond every width of the grid: the only way to k_agg_main at 32 and (VEC = 4) 64 lanes
         "FLAT_MIN_F=%d" % (1 << 20), "FLAT_MIN_F_ARG=%d" % (1 << 20))
TUNE_LAYOUTS = ("aligned", "ldx+2")

# fake addresses, 256-byte aligned; nothing is read through them
ARR, W, BIAS, X, OUT = 0x1000, 0x2000, 0x3000, 0x10000000000, 0x20000000000


def _cases():
    """(reduce, weighted, F, layout, rows of x, has a column array, tune) in recording order."""
    cases = [(r, w, F, lay, ROWS_FIT, 1, "") for r in REDUCES for w in (0, 1) for F in WIDTHS for lay in LAYOUTS]
    cases += [(r, w, 256, "aligned", rows, 1, "") for r in REDUCES for w in (0, 1) for rows in (ROWS_FAR, ROWS_4G)]
    cases += [(r, w, F, "aligned", ROWS_FIT, 0, "") for r in REDUCES for w in (0, 1) for F in WIDTHS]
    cases += [(r, w, F, lay, ROWS_FIT, 1, t) for t in TUNES for r in REDUCES for w in (0, 1) for F in WIDTHS
              for lay in TUNE_LAYOUTS]
    return cases


def _kernel_name(lib, case):
    from mi355_mp import _lib
    reduce, weighted, F, layout, rows, has_col, tune = case
    at = {"x": X, "out": OUT, "bias": BIAS, "ldx": F}
    if layout != "aligned":
        which, off = layout.split("+")   # "ldx+2": two floats of padding; "x+4": the base 4 bytes on
        at[which] += int(off)
    x, out, bias, ldx = at["x"], at["out"], at["bias"], at["ldx"]
    g = _lib.MpCsr(ARR, ARR if has_col else None, ARR, ARR, ARR, None, 10, 40, 256, 1, 0, rows, 0)
    buf = ctypes.create_string_buffer(512)
    key = prev = None
    if tune:
        k, v = tune.split("=")
        key = getattr(_lib, "MP_TUNE_" + k)
        prev = lib.mp_tune(key, int(v))
        assert prev >= 0, tune
    try:
        rc = lib.mp_aggregate_kernel_name(g, W if weighted else None, x, ldx, F, _lib.MP_REDUCE[reduce], bias, out, F,
                                          buf, 512, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mp_aggregate_kernel_name %r" % (case,), lib)
    finally:
        if tune:
            lib.mp_tune(key, prev)
    return buf.value.decode()


def _template_args(name):
    """('k_agg_flat', ['mp::SumRed<1, true, false>', '1', '16', '64', ...]) of a demangled kernel name."""
    head, rest = name.split("<", 1)
    inner = rest[:rest.rindex(">(")]
    args, depth, cur = [], 0, ""
    for ch in inner:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    args.append(cur.strip())
    return head.split("::")[-1], args


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    return doc["names"], [(tuple(c[:-1]), c[-1]) for c in doc["cases"]]


def test_recorded_grid_is_the_grid(golden):
    names, rows = golden
    assert [c for c, _ in rows] == _cases()
    assert all(0 <= i < len(names) for _, i in rows)


def test_recorded_grid_reaches_every_kernel_family(golden):
    """The names the table pins are not a corner of the dispatch: each family of
    main kernels -- lane tasks at both vector widths, k_agg_main at every task
    width, k_agg_flat through the slot window and through scalar batches (at
    both in-flight depths) and at every vector width -- is in it."""
    names, rows = golden
    used = [_template_args(names[i]) for i in sorted({i for _, i in rows})]
    lane = [a for k, a in used if k == "k_agg_lane"]      # <Red, VEC, NV, U>
    main = [a for k, a in used if k == "k_agg_main"]      # <Red, VEC, U, L>
    flat = [a for k, a in used if k == "k_agg_flat"]      # <Red, VEC, U, L, GA, SM, XM, TM>
    assert len(lane) + len(main) + len(flat) == len(used)
    assert any(a[1:3] == ["4", "1"] for a in lane) and any(a[1:3] == ["1", "8"] for a in lane)
    assert {a[3] for a in main} >= {"4", "8", "16", "32", "64"}
    assert any(a[5] == "false" for a in flat)
    assert any(a[5] == "true" for a in flat)
    assert any(a[5] == "true" and a[1:3] == ["1", "8"] for a in flat)   # kU_Vec1Far
    assert {a[1] for a in flat} >= {"1", "2", "4"}
    assert {a[3] for a in flat} == {"64"}


def test_dispatch_table_is_unchanged(golden):
    from mi355_mp import _lib
    lib = _lib.load()
    names, rows = golden
    moved = []
    for case, i in rows:
        got = _kernel_name(lib, case)
        if got != names[i]:
            moved.append((case, names[i], got))
    assert not moved, "%d of %d cases chose another kernel; first: %r" % (len(moved), len(rows), moved[:3])
