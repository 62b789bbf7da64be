"""CPU tests of the two views of the native library -- _lib.load() returns
status codes, _lib.native() raises on them.  Every native call here is
rejected or answered on the host, before any device call."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_geometric-1_amd", "csrc")
LIB = os.path.join(ROOT, "pytorch_geometric-1_amd", "mi355_mp", "libmi355_mp.so")

D = 0x7f0000000000          # fake device pointer: never dereferenced, the checks fail first


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    from mi355_mp import _lib
    return _lib.load()


def _rejected_calls(lib):
    """(symbol, arguments, needle of the error text): one per native unit."""
    n, F, E = 1000, 33, 3000
    ks = (ctypes.c_int32 * 2)(5, 5)
    op = (ctypes.c_int32 * 2)(1, 1)
    score_ws = lib.mp_pool_score_bwd_workspace(n, F)
    build_ws = lib.mp_cluster_build_workspace(n)
    big = 1 << 40
    return [
        # a NULL key with edges to sort
        ("mp_csr_build", (None, D, 5, 4, 4, D, D, D, D, D, lib.mp_csr_build_workspace(5, 4), None), "null"),
        # each of these one byte short of the extent the call needs
        ("mp_spline_basis_f32", (D, E, 2, ks, op, 1, D, E * 4 * 4 - 1, D, E * 4 * 8, None), "basis"),
        ("mp_pool_score_bwd_f32", (D, F, n, F, D, 1, D, D, D, F, D, F * 4, D, score_ws - 1, None),
         "ws holds %d" % (score_ws - 1)),
        ("mp_cluster_build", (D, n, D, big, D, big, D, big, D, big, D, D, build_ws - 1, None),
         "ws holds %d" % (build_ws - 1)),
    ]


def test_plain_view_returns_the_code_and_raising_view_raises(lib):
    from mi355_mp import _lib
    nat = _lib.native()
    for name, args, needle in _rejected_calls(lib):
        assert getattr(lib, name)(*args) == 1, name          # no exception: bench.py and the host tests rely on it
        text = lib.mp_last_error().decode()
        assert needle in text, (name, text)
        with pytest.raises(RuntimeError) as e:
            getattr(nat, name)(*args)
        assert str(e.value) == "%s failed (code 1): %s" % (name, text)
        assert getattr(lib, name)(*args) == 1, name          # and the plain view still does not raise afterwards


def test_check_keeps_its_format(lib):
    from mi355_mp import _lib
    name, args, _ = _rejected_calls(lib)[0]
    with pytest.raises(RuntimeError) as e:
        _lib.check(getattr(lib, name)(*args), name)
    assert str(e.value) == "%s failed (code 1): %s" % (name, lib.mp_last_error().decode())


def test_value_returning_symbols_are_never_checked(lib):
    from mi355_mp import _lib
    nat = _lib.native()
    assert len(set(_lib.VALUE_RETURNING)) == len(_lib.VALUE_RETURNING) == 11
    for name in _lib.VALUE_RETURNING:
        res, _ = _lib.SIGNATURES[name]
        assert res in (ctypes.c_int, ctypes.c_int32), name
        fn = getattr(nat, name)
        assert fn is getattr(lib, name) and fn.errcheck is None, name
    # nonzero answers come back as they are
    assert nat.mp_abi_version() == 7
    assert nat.mp_cluster_max_blocks() > 0
    assert nat.mp_gat_wide_ok(8, 32) == 1
    assert nat.mp_gat_train_ok(8, 32) != 0 and nat.mp_gat_two_pass_ok(8, 32) != 0
    assert nat.mp_schedule_n_waves(100, 1000, 256) == 5
    assert nat.mp_gat_bwd_blocks(1700) > 0 and nat.mp_arg_mask_words(200) > 0
    assert nat.mp_pool_score_bwd_parts(1000) > 0 and nat.mp_topk_path(65) == 1
    ks = (ctypes.c_int32 * 2)(5, 5)
    op = (ctypes.c_int32 * 2)(1, 1)
    assert nat.mp_spline_ok(2, 1, ks, op, 32) != 0


def test_every_status_symbol_raises_and_nothing_else_does(lib):
    from mi355_mp import _lib
    nat = _lib.native()
    assert sorted(vars(nat)) == sorted(_lib.SIGNATURES)
    status = [n for n, (res, _) in _lib.SIGNATURES.items()
              if res in (ctypes.c_int, ctypes.c_int32) and n not in _lib.VALUE_RETURNING]
    assert sorted(status) == sorted(_lib.STATUS_RETURNING) and len(status) == 72
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(nat, name)
        assert fn.__name__ == name and fn.restype is res and list(fn.argtypes) == list(args), name
        if name in status:
            assert fn.errcheck is not None and fn is not getattr(lib, name), name
            assert args[-1] is ctypes.c_void_p, name          # a status comes from a call that takes a stream
            assert getattr(lib, name).errcheck is None, name
        else:
            assert fn is getattr(lib, name) and fn.errcheck is None, name


def test_native_of_an_explicit_path_is_that_library(lib):
    from mi355_mp import _lib
    assert _lib.native() is _lib.native() is lib.raising
    other = _lib.load(LIB)
    assert other is not lib and _lib.native(LIB) is not lib.raising
    name, args, _ = _rejected_calls(other)[0]
    assert getattr(other, name)(*args) == 1
    with pytest.raises(RuntimeError, match=name + r" failed \(code 1\): "):
        getattr(other.raising, name)(*args)


def test_no_unchecked_status_call_in_the_package():
    """The package reaches the library through native() alone: no check()
    wrapper to forget, no load() whose status results would go unread."""
    pkg = os.path.join(ROOT, "pytorch_geometric-1_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert "_lib.check(" not in text, os.path.join(dirpath, f)
