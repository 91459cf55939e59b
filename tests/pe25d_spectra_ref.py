"""NumPy restatement of the zonal wavenumber spectra of GCM_PE25D (gcm_set_spectra, include/gcmcore.h): the four real
rows uc, vc, theta and T of every (level, row) as tests/pe25d_climate_ref.py forms them (T from np.power, where the
device takes its own Exner routine), np.fft.fft in float64 along i, the six raw products at the wavenumbers
0 .. mmax, and the unit the parity bound of a word is relative to.  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

import pe25d_climate_ref as clim

WORDS = ("uu", "vv", "TT", "uv", "vT", "vtheta")
EXNER_FACTORS = (0, 0, 2, 0, 1, 0)      # the T factors of each word: each carries the Exner routine's 1e-10 once
CLIMATE_WORD = {2: 6, 3: 7, 4: 8, 5: 9}  # word of the spectra -> the climatology's word it splits by wavenumber
EPS = 2.0 ** -53
FFT_CONSTANT = 8.0


def rows(p, u, v, t, sig, ptop, v_north=None):
    """-> (uc, vc, theta, T), each (L, H, W) float64: the rows the device transforms; v_north (L, W): row -1 of v where
    it is not row H - 1 (a band's north ghost row)"""
    t3, _ = clim.terms(p, u, v, t, sig, ptop, v_north)
    u, v, t = (np.asarray(a, dtype=np.float64) for a in (u, v, t))
    vm = np.roll(v, 1, axis=1)
    if v_north is not None:
        vm[:, 0, :] = v_north
    uc = 0.5 * (u + np.roll(u, 1, axis=2))
    vc = 0.5 * (v + vm)
    return uc, vc, t, t3[3]


def pairs(uc, vc, th, T):
    """the two factors of each word, in word order"""
    return ((uc, uc), (vc, vc), (T, T), (uc, vc), (vc, T), (vc, th))


def products(uc, vc, th, T, mmax):
    """-> (6, L, H, mmax + 1): Re(X_m conj Y_m) of each word's two rows, X = fft(x) along i"""
    M = mmax + 1
    F = {id(a): np.fft.fft(a, axis=-1)[..., :M] for a in (uc, vc, th, T)}
    out = []
    for x, y in pairs(uc, vc, th, T):
        X, Y = F[id(x)], F[id(y)]
        out.append(X.real * Y.real + X.imag * Y.imag)
    return np.stack(out)


def unit(uc, vc, th, T):
    """-> (6, L, H): B_x B_y with B_x = sqrt(W sum_i x_i^2) >= |X_m| for every m"""
    W = uc.shape[-1]
    B = {id(a): np.sqrt(W * np.sum(a * a, axis=-1)) for a in (uc, vc, th, T)}
    return np.stack([B[id(x)] * B[id(y)] for x, y in pairs(uc, vc, th, T)])


def sample(p, u, v, t, sig, ptop, mmax, v_north=None):
    """-> (s (6, L, H, mmax + 1), unit (6, L, H)): one sample's products and their parity unit"""
    r = rows(p, u, v, t, sig, ptop, v_north)
    return products(*r, mmax), unit(*r)


def bound_factor(W, exner=True):
    """-> (6,): what multiplies the unit in |device - restatement| <= factor unit, per sample.  A float64 FFT of length
    W errs per coefficient by at most a small constant times eps log2(W) B_x, a product by that times B_y once for each
    side, on the device and in the restatement: 8 eps log2 W; each T factor adds the 1e-10 of the device's Exner
    routine against pow (exner=False: both sides hold the device's T)"""
    f = FFT_CONSTANT * EPS * np.log2(W)
    return np.array([f + (e * 1e-10 if exner else 0.0) for e in EXNER_FACTORS])


def weights(M, W):
    """the one-sided weights: 1 for m = 0 and m = W / 2 (even W), 2 otherwise"""
    w = np.full(M, 2.0)
    w[0] = 1.0
    if W % 2 == 0 and W // 2 < M:
        w[W // 2] = 1.0
    return w


def accumulate(states, sig, ptop, mmax):
    """-> (n, s, unit): the sums over the samples `states` (each (p, u, v, t, ...)) in sample order, and the sum of
    their units"""
    s = b = None
    for st in states:
        a, c = sample(st[0], st[1], st[2], st[3], sig, ptop, mmax)
        s = a if s is None else s + a
        b = c if b is None else b + c
    return len(states), s, b
