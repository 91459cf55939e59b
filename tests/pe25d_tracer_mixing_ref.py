"""The NumPy restatement of the implicit vertical mixing of the tracers of GCM_PE25D (gcm_set_tracer_mixing in
include/gcmcore.h), written from the equations there: the float64 coefficient routine (gcm_tracer_mixing_coeffs) and the
column solve in the handle's real type.  Shared by tests/test_pe25d_tracer_mixing_cpu.py and
tests/test_pe25d_tracer_mixing_gpu.py, with the profiles and set-ups those tests use.  TEST INFRASTRUCTURE, no test in
here."""
import numpy as np

DTYPES = {"f64": np.float64, "f32": np.float32}


def _type(dtype):
    return np.dtype(DTYPES.get(dtype, dtype)).type


def coeffs(dsig, k, dtd):
    """-> (lo, w, g), float64 [L]: every operation a float64 operation of its own, in the header's order
        a[-1] = a[L-1] = 0;   a[m] = dtd * K[m] / (0.5 * (dsig[m] + dsig[m+1]))
        lo[k] = a[k-1] / dsig[k];   up[k] = a[k] / dsig[k];   d = 1.0 + lo[k] + up[k]
        w[0]  = 1.0 / d;            w[k] = 1.0 / (d - lo[k] * g[k-1]);      g[k] = up[k] * w[k]"""
    dsig = [float(x) for x in np.asarray(dsig, dtype=np.float64).reshape(-1)]
    k = [float(x) for x in np.asarray(k, dtype=np.float64).reshape(-1)]
    dtd = float(dtd)
    L = len(dsig)
    assert L >= 2 and len(k) == L - 1
    a = [(dtd * k[m]) / (0.5 * (dsig[m] + dsig[m + 1])) for m in range(L - 1)]
    lo, w, g = np.empty(L), np.empty(L), np.empty(L)
    for i in range(L):
        lo_k = (a[i - 1] if i >= 1 else 0.0) / dsig[i]
        up_k = (a[i] if i < L - 1 else 0.0) / dsig[i]
        d = (1.0 + lo_k) + up_k
        w_k = 1.0 / d if i == 0 else 1.0 / (d - lo_k * float(g[i - 1]))
        lo[i], w[i], g[i] = lo_k, w_k, up_k * w_k
    return lo, w, g


def tables(dsig, k, dt, dtype):
    """the kernel's tables: the coefficients for dt as the type holds it, rounded to the type"""
    T = _type(dtype)
    return tuple(x.astype(T) for x in coeffs(dsig, k, float(T(dt))))


def mix(c, dt, k, dsig, dtype):
    """one solve of every column of c (L, ...) in the real type `dtype`, every operation rounded on its own:
        y[0] = c[0] * w[0];   y[k] = (c[k] + lo[k] * y[k-1]) * w[k];   x[L-1] = y[L-1];   x[k] = y[k] + g[k] * x[k+1]
    -> a new array of that type"""
    T = _type(dtype)
    c = np.asarray(c, dtype=T)
    lo, w, g = tables(dsig, k, dt, dtype)
    L = c.shape[0]
    y = np.empty_like(c)
    y[0] = c[0] * w[0]
    for i in range(1, L):
        y[i] = (c[i] + lo[i] * y[i - 1]) * w[i]
    x = np.empty_like(c)
    x[L - 1] = y[L - 1]
    for i in range(L - 2, -1, -1):
        x[i] = y[i] + g[i] * x[i + 1]
    assert x.dtype == np.dtype(T)
    return x


def column_sum_drift(c, dt, k, dsig, dtype, steps=10):
    """the largest relative change of a column's sum_k c dsig over `steps` solves of c (L, ...) >= 0, the sums taken
    in float64 from the exactly widened values"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(c) - 1))
    x = np.asarray(c, dtype=_type(dtype))
    s0 = np.sum(x.astype(np.float64) * dsig, axis=0)
    worst = 0.0
    for _ in range(steps):
        x = mix(x, dt, k, dsig.reshape(-1), dtype)
        s = np.sum(x.astype(np.float64) * dsig, axis=0)
        worst = max(worst, float(np.max(np.abs(s - s0) / np.abs(s0))))
    return worst


# ---------------------------------------------------------------- what the tests register
def profile(L, seed=5, zero_at=None):
    """K [L - 1] in sigma^2 / s: with dt = 120 s and dsig ~ 1 / L the off-diagonal entries are of order one.  zero_at:
    an interface without exchange"""
    k = (0.2 + np.random.default_rng(seed).random(L - 1)) * 1.0e-2 / L ** 2
    if zero_at is not None:
        k[zero_at] = 0.0
    return k


def dsig_nonuniform(L, seed=9):
    """a non-uniform dsig [L] that sums to one"""
    d = 0.5 + np.random.default_rng(seed).random(L)
    return d / d.sum()
