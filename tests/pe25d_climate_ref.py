"""NumPy restatement of the zonal-mean climatology of GCM_PE25D (gcm_set_climate, include/gcmcore.h): the moments in
float64 with the documented per-row reduction order, the sums accumulated over the samples in sample order.  T comes
from np.power, where the device takes its own Exner routine.  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

P0 = 1e5
KAPPA = 287.0 / 1004.0
WORDS3 = ("u", "v", "theta", "T", "uu", "vv", "TT", "uv", "vT", "vtheta")
WORDS2 = ("p", "pp")
EXNER_WORDS = (3, 6, 8)          # the words that carry the device's Exner routine
LANES, WAVE = 256, 64


def row_sum(x):
    """the sum over the last axis in the device's order: the row padded with zeros to a multiple of 256, the 256-column
    chunks added one after the other onto 0.0, the xor butterfly 32 .. 1 within each 64, the four results in order"""
    x = np.asarray(x, dtype=np.float64)
    W = x.shape[-1]
    n = -(-W // LANES)
    pad = np.zeros(x.shape[:-1] + (n * LANES,))
    pad[..., :W] = x
    chunks = pad.reshape(x.shape[:-1] + (n, LANES))
    acc = np.zeros(x.shape[:-1] + (LANES,))
    for c in range(n):
        acc = acc + chunks[..., c, :]
    a = acc.reshape(x.shape[:-1] + (LANES // WAVE, WAVE))
    lane = np.arange(WAVE)
    d = WAVE // 2
    while d >= 1:
        a = a + a[..., lane ^ d]
        d //= 2
    r = a[..., 0, 0]
    for w in range(1, LANES // WAVE):
        r = r + a[..., w, 0]
    return r


def terms(p, u, v, t, sig, ptop, v_north=None):
    """-> (the ten (L, H, W) terms of m3, the two (H, W) terms of m2) of one state; v_north (L, W): row -1 of v where
    it is not row H - 1 (a band's north ghost row)"""
    p, u, v, t = (np.asarray(a, dtype=np.float64) for a in (p, u, v, t))
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    vm = np.roll(v, 1, axis=1)
    if v_north is not None:
        vm[:, 0, :] = v_north
    uc = 0.5 * (u + np.roll(u, 1, axis=2))
    vc = 0.5 * (v + vm)
    pl = sig[:, None, None] * p[None] + ptop
    T = t * np.power(pl / P0, KAPPA)
    return [u, v, t, T, u * u, v * v, T * T, uc * vc, vc * T, vc * t], [p, p * p]


def sample(p, u, v, t, sig, ptop, v_north=None):
    """-> (m3 (10, L, H), m2 (2, H)): one sample's zonal sums"""
    t3, t2 = terms(p, u, v, t, sig, ptop, v_north)
    return np.stack([row_sum(x) for x in t3]), np.stack([row_sum(x) for x in t2])


def bound(p, u, v, t, sig, ptop, v_north=None):
    """-> (10, L, H): sum_i |term|, what the parity bound of a word's sum is relative to"""
    t3, _ = terms(p, u, v, t, sig, ptop, v_north)
    return np.stack([np.sum(np.abs(x), axis=-1) for x in t3])


def accumulate(states, sig, ptop):
    """-> (n, m3, m2): the sums over the samples `states` (each (p, u, v, t, ...)) in sample order"""
    m3 = m2 = None
    for st in states:
        a, b = sample(st[0], st[1], st[2], st[3], sig, ptop)
        m3 = a if m3 is None else m3 + a
        m2 = b if m2 is None else m2 + b
    return len(states), m3, m2
