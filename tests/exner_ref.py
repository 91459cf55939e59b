"""(p/P0)**kappa three ways, shared by the host test of the algorithm (test_math_cpu.py) and the GPU
test of the device function (test_operator_dropins_gpu.py): the library's table, a float64 emulation
of gcm_math.h's exner() operation for operation, and the x87 extended-precision yardstick."""
import ctypes as C

import numpy as np

KAPPA = 287.0 / 1004.0

# what test_math_cpu.py asserts of the emulation against extended precision (measured 2.9e-16 .. 5.3e-16)
ERR_BOUND = 6e-16
# ... and at the mantissa-interval boundaries and powers of two
EDGE_ERR_BOUND = 5e-16


def table():
    from gcmiipy_amd import _lib
    tab = np.empty(256)
    assert _lib.lib.gcm_exner_table(tab.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return tab


def exner_emulated(p, tab):
    bits = p.view(np.int64)
    hi = (bits >> 32).astype(np.int64)
    e = ((hi >> 20) & 0x7ff) - 1023
    idx = (hi >> 14) & 63
    m = ((bits & 0x000fffffffffffff) | 0x3ff0000000000000).view(np.float64)
    E = tab[np.clip(e, -64, 63) + 64]
    rc, ck = tab[128 + 2 * idx], tab[129 + 2 * idx]
    # t = fma(m, rc, -1): exact product minus one; emulate with extended precision
    t = (np.longdouble(m) * np.longdouble(rc) - 1).astype(np.float64)
    b = [KAPPA]
    for n in range(2, 8):
        b.append(b[-1] * (KAPPA - (n - 1)) / n)
    t2 = t * t
    t4 = t2 * t2
    q12 = t * b[1] + b[0]
    q34 = t * b[3] + b[2]
    q56 = t * b[5] + b[4]
    hi3 = t4 * b[6] + (t2 * q56 + q34)
    poly = (t * t2) * hi3 + (t * q12 + 1.0)
    return E * ck * poly


def exner_extended(p):
    """the yardstick: exp(kappa log(p / P0)) in extended precision"""
    return np.exp(np.longdouble(KAPPA) * np.log(np.longdouble(p) / np.longdouble(1e5)))


def max_rel_err(x, ref):
    return float(np.max(np.abs((x - ref) / ref)))
