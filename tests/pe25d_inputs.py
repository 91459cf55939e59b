"""Seeded inputs of the GCM_PE25D tests, NumPy only (no torch, no device, no library): the "resting atmosphere plus
noise" state, the two tracer recipes, the ground temperature, the rows of a band and the halo message's size.  The CPU
tests show on these very numbers what the GPU tests then check on the device, and tolerances in the suite were
measured on them: seeds, the order of the generator's draws and the arithmetic stay as they are.  `geom` is the
product's geometry or the oracle's (height, width, layers, sig, ptop).  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

STATE_SEED, TRACER_SEED, GROUND_SEED = 12, 15, 13
UTC0 = 5 * 3600.0
# the 8-band split of the 64-row grid (test 1 of tests/test_pe25d_band_van_leer_gpu.py)
EIGHT = dict(H=64, W=1440, L=24, nb=8, dt=60.0, steps=3, ntr=3)


def state(geom, seed=STATE_SEED):
    """(p, u, v, t, q): noise around a resting atmosphere; v of the global last row is zero (the pole boundary).
    seed: a seed, or a np.random.Generator the caller has drawn from already and goes on drawing from"""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    H, W, L = geom.height, geom.width, geom.layers
    p = 1e5 + 10 * rng.standard_normal((H, W))
    u, v = rng.standard_normal((L, H, W)), rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    t = (300 + rng.standard_normal((L, H, W))) * ((1e5 / (p * np.asarray(geom.sig) + geom.ptop)) ** (287.0 / 1004.0))
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    return p, u, v, t, q


def state_of(geom, dtype="f64", wind=8.0):
    """the seeded state with winds of several m/s, p about 1e5 - ptop and a meridional theta gradient; f32: rounded to
    float32 (what the handle holds)"""
    p, u, v, t, q = state(geom)
    p = p - geom.ptop
    t = t * (1.0 + 0.05 * np.sin(np.arange(geom.height) * 0.7)[None, :, None])
    st = [p, wind * u, wind * v, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


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


def tracers_from_q(q, n, seed=14):
    """n tracers: the first a copy of q, the others positive noise of other magnitudes"""
    rng = np.random.default_rng(seed)
    c = [q] + [(k + 1.0) * (1 + 0.5 * rng.random(q.shape)) for k in range(n - 1)]
    return np.ascontiguousarray(np.stack(c)[:n])


def ground(H, W):
    return 288.0 + np.random.default_rng(GROUND_SEED).standard_normal((H, W))


def rows(a, sl):
    """rows `sl` of a (..., H, W) array"""
    return np.ascontiguousarray(a[..., sl, :])


def halo_bytes(W, L, esz, ntr, R):
    """the formula include/gcmcore.h documents for gcm_halo_bytes (one side)"""
    return esz * 2 * W * (1 + 4 * L) + 8 * 2 * W + ntr * esz * R * L * W
