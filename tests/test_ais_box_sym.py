"""CPU: the symmetric-box flag an AIS handle hands its half-generation kernels (csrc/ais_kernels.hpp
box_is_symmetric, through kabc_ais_box_sym -- no device needed).  Set exactly when every component is
a continuous Uniform(-a_k, a_k) and 2 <= D <= 8: only then is |y_k| <= a_k the kernel's support test."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib(k):
    from kissabc_jl_amd import _lib
    return _lib.load()


def _flag(lib, cd, comps):
    arr = (cd.Prior * len(comps))()
    for q, (kind, p) in zip(arr, comps):
        q.kind = kind
        for j, v in enumerate(p):
            q.p[j] = v
    sym = C.c_int32(-1)
    assert lib.kabc_ais_box_sym(arr, len(comps), C.byref(sym)) == 0, lib.kabc_last_error()
    return sym.value


def _u(cd, a, b):
    return (cd.PRIOR_UNIFORM, (a, b))


def test_symmetric_boxes_of_two_to_eight(k, lib):
    from kissabc_jl_amd import _cdefs as cd
    for D in range(2, 9):
        assert _flag(lib, cd, [_u(cd, -5.0, 5.0)] * D) == 1, D
        # a width of its own per component, and one that is not a binary fraction
        assert _flag(lib, cd, [_u(cd, -(0.1 + j), 0.1 + j) for j in range(D)]) == 1, D


def test_dimension_outside_two_to_eight(k, lib):
    from kissabc_jl_amd import _cdefs as cd
    for D in (1, 9, 12, 16):
        assert _flag(lib, cd, [_u(cd, -5.0, 5.0)] * D) == 0, D


def test_one_asymmetric_component_clears_it(k, lib):
    from kissabc_jl_amd import _cdefs as cd
    for D in (2, 5, 8):
        for j in range(D):
            for a, b in ((-0.5, 0.75), (0.0, 1.0), (-0.5, 0.5000000000000001), (-1.0, 3.0)):
                comps = [_u(cd, -0.5, 0.5)] * D
                comps[j] = _u(cd, a, b)
                assert _flag(lib, cd, comps) == 0, (D, j, a, b)


def test_discrete_or_other_family_clears_it(k, lib):
    from kissabc_jl_amd import _cdefs as cd
    u = _u(cd, -3.0, 3.0)
    assert _flag(lib, cd, [u, (cd.PRIOR_DISCRETE_UNIFORM, (-3.0, 3.0)), u]) == 0
    assert _flag(lib, cd, [(cd.PRIOR_DISCRETE_UNIFORM, (-3.0, 3.0))] * 2) == 0
    assert _flag(lib, cd, [u, (cd.PRIOR_NORMAL, (0.0, 1.0))]) == 0
    assert _flag(lib, cd, [u, (cd.PRIOR_TRUNCNORMAL, (0.0, 1.0, -3.0, 3.0))]) == 0


def test_bad_arguments(k, lib):
    from kissabc_jl_amd import _cdefs as cd
    arr = (cd.Prior * 2)()
    for q in arr:
        q.kind, q.p[0], q.p[1] = cd.PRIOR_UNIFORM, -1.0, 1.0
    sym = C.c_int32(0)
    assert lib.kabc_ais_box_sym(arr, 2, None) == cd.KABC_ERR_INVALID_ARG
    assert lib.kabc_ais_box_sym(arr, 0, C.byref(sym)) == cd.KABC_ERR_INVALID_ARG
    assert b"kabc_ais_box_sym" in lib.kabc_last_error()
    arr[1].p[1] = -2.0   # an empty interval: not a valid prior
    assert lib.kabc_ais_box_sym(arr, 2, C.byref(sym)) == cd.KABC_ERR_INVALID_ARG
