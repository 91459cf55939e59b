"""The NumPy restatement of the tracer forcing of GCM_PE25D (gcm_set_tracer_forcing in include/gcmcore.h), shared by
tests/test_pe25d_tracer_forcing_cpu.py and tests/test_pe25d_tracer_forcing_gpu.py, and the forcing records those tests
register.  TEST INFRASTRUCTURE, no test in here."""
import math

import numpy as np

DTYPES = {"f64": np.float64, "f32": np.float32}


def force(c, dt, rec, dtype):
    """one application of the forcing `rec` = dict(source, decay, emission, pin_mask, pin_value) to the field c, in
    the real type `dtype` ("f64" / "f32" or a NumPy type), every operation rounded on its own:
        c1 = c + dt * (source + e);  c2 = c1 * fac;  c = pinned ? pin_value : c2
    fac = T(exp(-decay * dt)) with dt as T holds it and the exponential of the C library in double (math.exp, which
    calls it; np.exp is NumPy's own).  -> a new array of that type"""
    T = np.dtype(DTYPES.get(dtype, dtype)).type
    c = np.asarray(c, dtype=T)
    dt = T(dt)
    emission, mask = rec.get("emission"), rec.get("pin_mask")
    e = T(0) if emission is None else np.asarray(emission, dtype=T)
    fac = T(math.exp(-float(rec.get("decay", 0.0)) * float(dt)))
    c1 = c + dt * (T(rec.get("source", 0.0)) + e)
    c2 = c1 * fac
    if mask is not None:
        c2 = np.where(np.asarray(mask) != 0, T(rec.get("pin_value", 0.0)), c2)
    assert c2.dtype == np.dtype(T)
    return c2


def records(L, H, W, k_surface, seed=21):
    """the forcing of the GPU tests' four tracers: 0 unforced, 1 source + decay, 2 an emission on the lowest level +
    decay, 3 an age-of-air clock (source 1, pinned to 0 on the lowest level)"""
    rng = np.random.default_rng(seed)
    emission = np.zeros((L, H, W))
    emission[k_surface] = 1e-3 * rng.random((H, W))
    mask = np.zeros((L, H, W), dtype=bool)
    mask[k_surface] = True
    return {1: dict(source=0.25, decay=1.0e-4),
            2: dict(emission=emission, decay=2.1e-6),
            3: dict(source=1.0, pin_mask=mask, pin_value=0.0)}
