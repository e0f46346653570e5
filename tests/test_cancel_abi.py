"""CPU: the cancellation surface (kabc_ctx_cancel, kabc_ctx_clear_cancel, kabc_ctx_cancel_on_sigint,
KABC_ERR_CANCELLED = 7) is declared in include/kabc.h, exported by the library and mirrored in the
ctypes binding and the Julia shim; a status of 7 raises Cancelled.  What a cancelled call leaves behind
is checked on the GPU (tests/test_gpu_cancel.py)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kabc_ctx_cancel", "kabc_ctx_clear_cancel", "kabc_ctx_cancel_on_sigint")


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kabc.h")).read(), flags=re.S)


def test_header_declares_the_cancel_surface():
    h = _header()
    assert re.search(r"KABC_ERR_CANCELLED\s*=\s*7\b", h)
    # appended: every earlier status keeps its value
    assert re.search(r"KABC_ERR_NAN_COST\s*=\s*6\s*,", h)
    assert re.search(r"kabc_status_t\s+kabc_ctx_cancel\s*\(\s*kabc_ctx_t\s*\*\s*ctx\s*\)\s*;", h)
    assert re.search(r"kabc_status_t\s+kabc_ctx_clear_cancel\s*\(\s*kabc_ctx_t\s*\*\s*ctx\s*\)\s*;", h)
    assert re.search(r"kabc_status_t\s+kabc_ctx_cancel_on_sigint\s*\(\s*kabc_ctx_t\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", h)
    assert re.search(r"#define KABC_VERSION 321\b", h)


def test_library_exports_and_ctypes_mirror(k):
    import ctypes as C
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    assert cd.KABC_ERR_CANCELLED == 7
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in cd.PROTOTYPES, n
    assert cd.PROTOTYPES["kabc_ctx_cancel"] == (C.c_int, [C.c_void_p])
    assert cd.PROTOTYPES["kabc_ctx_clear_cancel"] == (C.c_int, [C.c_void_p])
    assert cd.PROTOTYPES["kabc_ctx_cancel_on_sigint"] == (C.c_int, [C.c_void_p, C.c_int32])
    # NULL contexts are refused without touching a device
    assert lib.kabc_ctx_cancel(None) == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_ctx_clear_cancel(None) == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_ctx_cancel_on_sigint(None, 1) == cd.KABC_ERR_INVALID_ARG


def test_status_7_raises_cancelled(k):
    from kissabc_jl_amd import _lib
    with pytest.raises(_lib.Cancelled) as ei:
        _lib.check(7)
    assert ei.value.status == 7
    assert isinstance(ei.value, k.KabcError)
    assert k.Cancelled is _lib.Cancelled
    with pytest.raises(k.KabcError) as e2:
        _lib.check(6)
    assert not isinstance(e2.value, _lib.Cancelled)
    assert hasattr(k.Context, "cancel") and hasattr(k.Context, "clear_cancel")


def test_julia_shim_binds_cancel():
    src = open(os.path.join(ROOT, "kissabc.jl_amd", "julia", "KissABCHip.jl")).read()
    assert re.search(r"ccall\(\(:kabc_ctx_cancel, libkabc\), Cint, \(Ptr\{Cvoid\},\)", src)
    assert re.search(r"ccall\(\(:kabc_ctx_clear_cancel, libkabc\), Cint, \(Ptr\{Cvoid\},\)", src)
    assert re.search(r"const KABC_ERR_CANCELLED = Cint\(7\)", src)
    assert "throw(InterruptException())" in src
    assert re.search(r"^export cancel!, clear_cancel!", src, flags=re.M)
