"""CPU: the C-ABI shared library loads and exports every symbol include/kabc.h
declares (no compute calls: there is no GPU here), struct layouts match, and the
product refuses to run without a device instead of falling back."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "kabc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kabc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(k):
    from kissabc_jl_amd import _cdefs, _lib
    lib = _lib.load()
    names = _declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/kabc.h but not exported"
    assert sorted(_cdefs.PROTOTYPES) == names, "ctypes prototypes out of sync with kabc.h"
    assert lib.kabc_version() == _cdefs.KABC_VERSION == 321


def test_struct_layouts(k):
    from kissabc_jl_amd import _cdefs as cd, _lib
    # the hand-written ctypes mirrors against the library's own sizeof (kabc_abi_sizeof): the
    # same self-check julia/KissABCHip.jl runs in __init__
    lib = _lib.load()
    mirrors = [cd.Prior, cd.Cost, cd.Model, cd.Stats, cd.SmcOpts, cd.SmcIter, cd.SmcResult,
               cd.AbcdeOpts, cd.AbcdeResult, cd.PfilterOpts, cd.PfilterResult]
    assert [lib.kabc_abi_sizeof(i) for i in range(len(mirrors))] == [C.sizeof(m) for m in mirrors]
    assert lib.kabc_abi_sizeof(len(mirrors)) == -1
    assert C.sizeof(cd.Prior) == 40
    assert C.sizeof(cd.Cost) == 32
    assert C.sizeof(cd.Model) == 24 + 32
    assert C.sizeof(cd.Stats) == 24
    assert C.sizeof(cd.SmcOpts) == 80
    assert C.sizeof(cd.SmcIter) == 40
    assert C.sizeof(cd.SmcResult) == 96


def test_smc_default_opts_match_reference_defaults(k):
    # src/smc.jl:95-105
    import math
    from kissabc_jl_amd import _cdefs as cd, _lib
    o = cd.SmcOpts()
    _lib.load().kabc_smc_default_opts(C.byref(o))
    assert (o.nparticles, o.alpha, o.mcmc_retrys, o.mcmc_tol, o.epstol, o.max_stretch) == \
        (100, 0.95, 0, 0.015, 0.0, 2.0)
    assert math.isnan(o.r_epstol) and math.isnan(o.min_r_ess) and o.verbose == 0


def test_no_device_no_fallback(k):
    """On a box without a GPU the product path must fail loudly."""
    from kissabc_jl_amd import _lib
    if _lib.load().kabc_device_count() > 0:
        pytest.skip("a GPU is visible: covered by the -m gpu tests")
    with pytest.raises(k.KabcError) as e:
        k.Context(0)
    assert "no CPU fallback" in str(e.value)
    model = k.ApproxKernelizedPosterior(k.Factored(k.Normal(0, 1), k.Normal(0, 1)),
                                        k.costs.GaussDist([0, 0]), 0.1)
    with pytest.raises(k.KabcError):
        k.sample(model, k.AIS(16), 10)


def test_product_never_touches_the_oracle():
    """No file of the product package mentions the oracle."""
    pkg = os.path.join(ROOT, "kissabc.jl_amd")
    for dp, _, fns in os.walk(pkg):
        if os.path.basename(dp) in ("build", "lib", "__pycache__"):
            continue
        for fn in fns:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp", ".jl")) or fn == "Makefile":
                txt = open(os.path.join(dp, fn), errors="replace").read()
                for needle in ("import oracle", "from oracle", "kabc_oracle", "libkabc_oracle",
                               "orc_", "oracle.oracle", "oracle/_build", "oracle/_ref"):
                    assert needle not in txt, f"{fn} references the oracle ({needle})"


def test_host_closure_is_rejected(k):
    with pytest.raises(TypeError):
        k.ApproxKernelizedPosterior(k.Normal(0, 1), lambda x: abs(x - 1.5), 0.01)


def test_poison_probe_prototype_and_arguments(k):
    """kabc_poison_probe (verification only): declared, bound, and refusing bad arguments before it touches a
    device; the Python mirror of the KABC_POISON_ALLOC byte rule (csrc/host_common.hpp poison_byte)"""
    from kissabc_jl_amd import _cdefs as cd, _lib
    lib = _lib.load()
    res, args = cd.PROTOTYPES["kabc_poison_probe"]
    u8 = C.POINTER(C.c_uint8)
    assert res is C.c_int and args == [cd.VP, C.c_int64, u8, u8, u8, C.POINTER(C.c_int32)]
    buf, info = (C.c_uint8 * 16)(), (C.c_int32 * 2)()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(4096)))   # (the checks come before any look at the context)
    for ctx, n, a, b, c, i in [(None, 16, buf, buf, buf, info), (fake, 16, None, buf, buf, info),
                               (fake, 16, buf, None, buf, info), (fake, 16, buf, buf, None, info),
                               (fake, 16, buf, buf, buf, None), (fake, 0, buf, buf, buf, info),
                               (fake, -1, buf, buf, buf, info), (fake, (1 << 24) + 1, buf, buf, buf, info)]:
        assert lib.kabc_poison_probe(ctx, n, a, b, c, i) == cd.KABC_ERR_INVALID_ARG, (n, a, b, c, i)
        assert b"kabc_poison_probe" in lib.kabc_last_error()
    rule = _lib.poison_byte_rule
    assert [rule(v) for v in ("", "0", "00", "1", "yes", "0xff", "0XA5", "0x0", "0x3c", "0x100", "0xzz", "0x")] == \
        [None, None, None, 0xA5, 0xA5, 0xFF, 0xA5, 0, 0x3C, 0xA5, 0xA5, 0xA5]
