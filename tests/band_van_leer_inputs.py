"""Inputs shared by tests/test_pe25d_band_van_leer_cpu.py and tests/test_pe25d_band_van_leer_gpu.py: the seeded state and
tracers of the band parity runs, so that the CPU test can show on the very same numbers that a one-row message could
not have produced the single domain's bits.  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

STATE_SEED, TRACER_SEED = 12, 15
# the 8-band split of the 64-row grid (test 1 of the GPU file)
EIGHT = dict(H=64, W=1440, L=24, nb=8, dt=60.0, steps=3, ntr=3)


def state(H, W, L, sig, ptop, seed=STATE_SEED):
    """(p, u, v, t, q): noise around a resting atmosphere; v of the global last row is zero (the pole boundary)"""
    rng = np.random.default_rng(seed)
    p = 1e5 + 10 * rng.standard_normal((H, W))
    u, v = rng.standard_normal((L, H, W)), rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    t = (300 + rng.standard_normal((L, H, W))) * ((1e5 / (p * sig + ptop)) ** (287.0 / 1004.0))
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    return p, u, v, t, q


def tracers(H, W, L, n, seed=TRACER_SEED):
    """n >= 2 tracers in turn: random positive, a latitude step function (0 / 1: the field on which a limited scheme
    must create no new extrema), a constant; beyond three: other offsets, steps at other latitudes"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 3
        if kind == 0:
            out.append(1.0 + k + rng.random((L, H, W)))
        elif kind == 1:
            c = np.zeros((L, H, W))
            c[:, H // 3 + k // 3: 2 * H // 3 - k // 3, :] = 1.0
            out.append(c)
        else:
            out.append(np.full((L, H, W), 2.5 + k))
    return np.ascontiguousarray(np.stack(out))


def rows(a, sl):
    """rows `sl` of a (..., H, W) array"""
    return np.ascontiguousarray(a[..., sl, :])


def halo_bytes(W, L, esz, ntr, R):
    """the formula include/gcmcore.h documents for gcm_halo_bytes (one side)"""
    return esz * 2 * W * (1 + 4 * L) + 8 * 2 * W + ntr * esz * R * L * W
