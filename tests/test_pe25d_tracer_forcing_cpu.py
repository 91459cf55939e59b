"""CPU tests of the tracer forcing of GCM_PE25D (gcm_set_tracer_forcing): the declaration, the binding and the
refusals that need no device, and the properties of the NumPy restatement the GPU tests compare the kernel with."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from pe25d_tracer_forcing_ref import force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gcmcore.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_both_functions():
    h = re.sub(r"\s+", " ", _header())
    assert "typedef struct gcm_tracer_forcing { double source, decay, pin_value;" in h
    assert "const double *emission;" in h and "const unsigned char *pin_mask;" in h
    assert "int gcm_set_tracer_forcing(gcm_handle *h, int tracer, const gcm_tracer_forcing *f);" in h
    assert "int gcm_tracer_forced(const gcm_handle *h, int tracer);" in h


def test_symbols_are_bound():
    from gcmiipy_amd import _lib
    assert _lib.SYMBOLS["gcm_set_tracer_forcing"] == (C.c_int, [_lib._H, C.c_int, C.POINTER(_lib.TracerForcing)])
    assert _lib.SYMBOLS["gcm_tracer_forced"] == (C.c_int, [_lib._H, C.c_int])
    assert _lib.lib.gcm_set_tracer_forcing.restype is C.c_int


def test_null_handle_is_an_argument_error():
    from gcmiipy_amd import _lib
    rec = _lib.TracerForcing(1.0, 0.0, 0.0, None, None)
    assert _lib.lib.gcm_set_tracer_forcing(None, 0, C.byref(rec)) == _lib.ERR_ARG
    assert _lib.lib.gcm_set_tracer_forcing(None, -1, None) == _lib.ERR_ARG
    assert _lib.lib.gcm_tracer_forced(None, 0) == _lib.ERR_ARG


def test_ctypes_layout_of_the_struct():
    from gcmiipy_amd import _lib
    S = _lib.TracerForcing
    assert [f[0] for f in S._fields_] == ["source", "decay", "pin_value", "emission", "pin_mask"]
    assert (S.source.offset, S.decay.offset, S.pin_value.offset, S.emission.offset, S.pin_mask.offset) == (0, 8, 16, 24, 32)
    assert C.sizeof(S) == 40


def test_core_checks_shapes_before_the_library():
    """ValueError for a wrong shape or mask type comes from Core itself: no handle is needed to see it"""
    from gcmiipy_amd.core import Core
    c = Core.__new__(Core)
    c.L, c.H, c.W, c._h, c._forcing = 3, 4, 5, None, {}
    with pytest.raises(ValueError, match="emission"):
        c.set_tracer_forcing(0, emission=np.zeros((3, 4, 6)))
    with pytest.raises(ValueError, match="pin_mask"):
        c.set_tracer_forcing(0, pin_mask=np.zeros((3, 5, 4), dtype=bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        c.set_tracer_forcing(0, pin_mask=np.zeros((3, 4, 5)))
    assert c._forcing == {}
    c._h = None


# ---------------------------------------------------------------- the restatement
def _field(dtype, seed=3):
    return (1.0 + np.random.default_rng(seed).random((3, 5, 7))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_source_only_adds_n_dt(dtype):
    """a source S alone: c + n S dt after n applications, up to the n roundings of the sums"""
    c0, n, dt, S = _field(dtype), 7, 60.0, 0.5
    c = c0
    for _ in range(n):
        c = force(c, dt, dict(source=S), dtype)
    assert c.dtype == dtype
    exact = c0.astype(np.float64) + n * S * dt
    assert np.max(np.abs(c - exact)) <= n * np.finfo(dtype).eps * np.max(np.abs(exact))
    # with values that are exact in the type: no rounding at all
    c = np.full((2, 2, 2), 8.0, dtype=dtype)
    for _ in range(n):
        c = force(c, dt, dict(source=S), dtype)
    assert np.array_equal(c, np.full((2, 2, 2), 8.0 + n * S * dt))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_decay_only_multiplies_by_fac_to_the_n(dtype):
    c0, n, dt, lam = _field(dtype), 6, 120.0, 3.0e-4
    fac = dtype(math.exp(-lam * dt))
    c, want = c0, c0
    for _ in range(n):
        c = force(c, dt, dict(decay=lam), dtype)
        want = want * fac
    assert np.array_equal(c, want) and c.dtype == dtype
    exact = c0.astype(np.float64) * math.exp(-lam * dt * n)
    assert np.max(np.abs(c / exact - 1)) <= 2 * n * np.finfo(dtype).eps


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_pin_wins_over_source_and_decay(dtype):
    c0 = _field(dtype)
    mask = np.zeros(c0.shape, dtype=np.uint8)
    mask[0] = 1
    mask[2, 1, 3] = 255
    rec = dict(source=2.0, decay=1e-3, pin_mask=mask, pin_value=-4.5, emission=np.ones(c0.shape))
    got = force(c0, 30.0, rec, dtype)
    free = force(c0, 30.0, dict(rec, pin_mask=None), dtype)
    assert np.all(got[mask != 0] == dtype(-4.5))
    assert np.array_equal(got[mask == 0], free[mask == 0]) and not np.any(free == dtype(-4.5))
    nan = c0.copy()
    nan[0, 0, 0] = np.nan                                         # a pinned cell is set whatever it held
    assert force(nan, 30.0, rec, dtype)[0, 0, 0] == dtype(-4.5)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_decay_and_no_source_return_the_field(dtype):
    c0 = _field(dtype) - dtype(1.5)                               # both signs
    got = force(c0, 60.0, dict(source=0.0, decay=0.0), dtype)
    assert got.tobytes() == c0.tobytes()
    assert force(c0, 60.0, dict(), dtype).tobytes() == c0.tobytes()
