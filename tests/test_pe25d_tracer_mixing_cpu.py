"""CPU tests of the implicit vertical mixing of the tracers of GCM_PE25D (gcm_set_tracer_mixing): the declarations, the
binding and the refusals that need no device, the coefficient routine gcm_tracer_mixing_coeffs against the NumPy
restatement bit for bit, and the properties of the restatement the GPU tests compare the kernel with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pe25d_tracer_mixing_ref import coeffs, column_sum_drift, dsig_nonuniform, mix, profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
LEVELS = [1, 2, 3, 9, 24]


def test_header_declares_the_three_functions():
    with open(os.path.join(ROOT, "include", "gcmcore.h")) as f:
        h = re.sub(r"\s+", " ", f.read())
    assert "int gcm_set_tracer_mixing(gcm_handle *h, int tracer, const double *k, int nk);" in h
    assert "int gcm_tracer_mixed(const gcm_handle *h, int tracer);" in h
    assert ("int gcm_tracer_mixing_coeffs(int L, const double *dsig, const double *k, double dtd, "
            "double *lo, double *w, double *g);") in h


def test_symbols_are_bound():
    from gcmiipy_amd import _lib
    dp = C.POINTER(C.c_double)
    assert _lib.SYMBOLS["gcm_set_tracer_mixing"] == (C.c_int, [_lib._H, C.c_int, dp, C.c_int])
    assert _lib.SYMBOLS["gcm_tracer_mixed"] == (C.c_int, [_lib._H, C.c_int])
    assert _lib.SYMBOLS["gcm_tracer_mixing_coeffs"] == (C.c_int, [C.c_int, dp, dp, C.c_double, dp, dp, dp])
    assert _lib.lib.gcm_set_tracer_mixing.restype is C.c_int


def test_null_handle_is_an_argument_error():
    from gcmiipy_amd import _lib
    k = (C.c_double * 2)(1e-5, 1e-5)
    assert _lib.lib.gcm_set_tracer_mixing(None, 0, k, 2) == _lib.ERR_ARG
    assert _lib.lib.gcm_set_tracer_mixing(None, -1, None, 0) == _lib.ERR_ARG
    assert _lib.lib.gcm_tracer_mixed(None, 0) == _lib.ERR_ARG


def test_core_checks_the_shape_before_the_library():
    """ValueError for a wrong shape comes from Core itself: no handle is needed to see it"""
    from gcmiipy_amd.core import Core
    c = Core.__new__(Core)
    c.L, c.H, c.W, c._h, c._mixing = 5, 4, 6, None, {}
    for bad in (np.zeros(5), np.zeros(3), np.zeros((4, 1)), 1e-5):
        with pytest.raises(ValueError, match="k has shape"):
            c.set_tracer_mixing(0, bad)
    assert c._mixing == {}


# ---------------------------------------------------------------- the coefficient routine
def _lib_coeffs(L, dsig, k, dtd):
    from gcmiipy_amd import _lib
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    out = [np.full(max(L, 1), -7.0) for _ in range(3)]
    rc = _lib.lib.gcm_tracer_mixing_coeffs(L, dp(dsig), dp(k), dtd, *[dp(a) for a in out])
    return rc, out


@pytest.mark.parametrize("dt", [900.0, 1.0 / 3.0])
@pytest.mark.parametrize("L", [2, 3, 9, 24, 41])
def test_coefficients_equal_the_restatement_bit_for_bit(L, dt):
    """non-uniform dsig, one interior interface with K = 0 (L >= 3; at L = 2 the only interface keeps its K)"""
    from gcmiipy_amd import _lib
    dsig = dsig_nonuniform(L)
    k = profile(L, seed=L, zero_at=(L - 1) // 2 if L >= 3 else None)
    rc, got = _lib_coeffs(L, dsig, k, dt)
    assert rc == _lib.OK
    want = coeffs(dsig, k, dt)
    for name, a, b in zip(("lo", "w", "g"), got, want):
        assert a.tobytes() == b.tobytes(), (L, dt, name)
    lo, w, g = got
    assert lo[0] == 0.0 and g[L - 1] == 0.0 and np.all(lo >= 0) and np.all(g >= 0) and np.all(w > 0) and np.all(w <= 1)
    if L >= 3:
        m = (L - 1) // 2
        assert g[m] == 0.0 and lo[m + 1] == 0.0                   # no exchange across the interface with K = 0
    # the same profile as float32 handles take it: dt as the type holds it
    dt32 = float(np.float32(dt))
    rc, got = _lib_coeffs(L, dsig, k, dt32)
    assert rc == _lib.OK and all(a.tobytes() == b.tobytes() for a, b in zip(got, coeffs(dsig, k, dt32)))


def test_coefficient_routine_refusals():
    from gcmiipy_amd import _lib
    lib = _lib.lib
    dsig, k = dsig_nonuniform(4), profile(4)
    for L, ds, kk in ((1, dsig_nonuniform(1), np.zeros(1)), (0, dsig, k), (4, None, k), (4, dsig, None)):
        rc, out = _lib_coeffs(L, ds, kk, 900.0)
        assert rc == _lib.ERR_ARG, (L, ds is None, kk is None)
        assert all(np.all(a == -7.0) for a in out)                # nothing written
        assert b"gcm_tracer_mixing_coeffs" in lib.gcm_last_error(None)
    for bad in (np.nan, np.inf, -1e-12):
        kk = k.copy()
        kk[1] = bad
        rc, out = _lib_coeffs(4, dsig, kk, 900.0)
        assert rc == _lib.ERR_ARG and all(np.all(a == -7.0) for a in out), bad
        assert b"finite" in lib.gcm_last_error(None)
    dp = dsig.ctypes.data_as(C.POINTER(C.c_double))
    kp = k.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.gcm_tracer_mixing_coeffs(4, dp, kp, 900.0, None, dp, dp) == _lib.ERR_ARG


# ---------------------------------------------------------------- the restatement
def _columns(L, dtype, seed=3):
    """(L, 5, 7) columns >= 0: random, with a surface-heavy one, a zero one and a spike"""
    c = np.random.default_rng(seed).random((L, 5, 7))
    c[:, 0, 0] = np.exp(-np.arange(L)[::-1] / 2.0)
    c[:, 0, 1] = 0.0
    c[:, 0, 2] = 0.0
    c[L - 1, 0, 2] = 1.0e3
    return c.astype(dtype)


def _k(L, zero=True):
    if L == 1:
        return np.zeros(0)
    return profile(L, seed=L, zero_at=(L - 1) // 2 if (zero and L >= 3) else None)


def _mix(c, dt, k, dsig, dtype):
    # (L = 1: no interface, no exchange -- the library refuses the registration, the restatement is the identity)
    return np.asarray(c, dtype=dtype).copy() if c.shape[0] == 1 else mix(c, dt, k, dsig, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LEVELS)
def test_zero_k_returns_the_field(L, dtype):
    c = _columns(L, dtype) - dtype(0.25)                          # both signs
    got = _mix(c, 900.0, np.zeros(max(L - 1, 0)), dsig_nonuniform(L), dtype)
    assert got.dtype == dtype and np.array_equal(got, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LEVELS)
def test_a_uniform_column_stays_within_4_ulp(L, dtype):
    dsig = dsig_nonuniform(L)
    for value in (1.0, 2.5, 3.0e-6, 417.3):
        c = np.full((L, 2, 2), value, dtype=dtype)
        for dt in (900.0, 1.0 / 3.0):
            x = _mix(c, dt, _k(L), dsig, dtype)
            assert np.max(np.abs(x - c)) <= 4 * np.spacing(dtype(value)), (L, value, dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", LEVELS)
def test_positivity_extrema_and_the_column_sum(L, dtype):
    """ten steps of dt = 900 s, an interface with K = 0: the result of a column >= 0 is >= 0 exactly (a zero column
    stays zero), no column's maximum rises and none's minimum falls by more than 4 ulp of the value, and the column
    sum sum_k c dsig drifts by rounding only.  The bound on the drift: a solve is 5 L rounded operations on a column,
    and its tables are 3 L rounded entries, each a relative perturbation of eps of terms no larger than the column's
    sum of c dsig when c >= 0 (every intermediate is a non-negative combination of the inputs): 8 L eps a step.  The
    GPU mass test takes the same figure, measured on its own columns"""
    dsig = dsig_nonuniform(L)
    c = _columns(L, dtype)
    steps, eps = 10, float(np.finfo(dtype).eps)
    x = c
    for _ in range(steps):
        x_new = _mix(x, 900.0, _k(L), dsig, dtype)
        assert np.all(x_new >= 0)
        assert np.all(x_new.max(axis=0) <= x.max(axis=0) + 4 * np.spacing(x.max(axis=0)))
        assert np.all(x_new.min(axis=0) >= x.min(axis=0) - 4 * np.spacing(x.min(axis=0)))
        x = x_new
    assert not x[:, 0, 1].any()
    if L > 1:
        assert not np.array_equal(x, c)
        drift = column_sum_drift(np.delete(c.reshape(L, -1), 1, axis=1), 900.0, _k(L), dsig, dtype, steps)
        print("L = %d, %s: largest relative drift of a column sum over %d steps %.3e (bound %.3e)"
              % (L, np.dtype(dtype).name, steps, drift, steps * 8 * L * eps))
        assert drift <= steps * 8 * L * eps
