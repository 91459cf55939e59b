"""NumPy restatement of the geopotential height on pressure levels and of the time-mean maps of GCM_PE25D
(gcm_plev_height_columns, gcm_plev_height, gcm_set_plev_maps, include/gcmcore.h): the model's mid-level geopotential in
its summation order, continued inside the bracketing layer linearly in the Exner function, in float64 with every
operation rounded on its own; Pi from np.power, where the device and the host build take the library's own Exner
routine.  The pressure-level quantities of the maps (T, uc, vc, q) are tests/pe25d_plev_ref.py's.  Arrays are
(L, H, W), level 0 the bottom.  TEST INFRASTRUCTURE, no test in here."""
import numpy as np

import pe25d_plev_ref as pref

P0, KAPPA = pref.P0, pref.KAPPA
RD, CP, G = 287.0, 1004.0, 9.8
WORDS = ("count", "Z", "ZZ", "T", "TT", "uc", "vc", "ucuc", "vcvc", "ucvc", "vcT", "q", "vcq")
EXACT_WORDS = (0, 5, 6, 7, 8, 9, 11, 12)        # no Exner routine in them: bit for bit the restatement's
EXNER_WORDS = (1, 2, 3, 4, 10)


def level_arrays(geom):
    """sig, dsig, sigt of a geometry (the product's or the oracle's) as float64 (L,)"""
    return tuple(np.asarray(getattr(geom, k), dtype=np.float64).reshape(-1) for k in ("sig", "dsig", "sigt"))


def geopotential(p, t, sig, dsig, sigt, ptop, hm):
    """-> (pl, Pi, stp, phi), each (L, H, W): the model's mid-level geopotential.  hm (H, W): the heightmap in m"""
    p, t, hm = (np.asarray(a, dtype=np.float64) for a in (p, t, hm))
    sig, dsig, sigt = (np.asarray(a, dtype=np.float64).reshape(-1)[:, None, None] for a in (sig, dsig, sigt))
    L = t.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        pl = sig * p[None] + ptop
        Pi = np.power(pl / P0, KAPPA)
        rho = pl / (RD * (t * Pi))
        s1 = ((sig * p[None]) / rho) * dsig
        stp = (CP * (0.5 * (t + np.roll(t, -1, axis=0)))) * (Pi - np.roll(Pi, -1, axis=0))
        s2 = sigt * stp
        acc = np.zeros(p.shape)
        for k in range(L):
            acc = acc + (s1[k] - s2[k])
        phi = [acc + hm * G]
        for k in range(1, L):
            phi.append(phi[-1] + stp[k - 1])
    return pl, Pi, stp, np.stack(phi)


def heights(p, t, sig, dsig, sigt, ptop, hm, P):
    """-> (Z (N, H, W), valid (N, H, W) bool): gcm_plev_height, NaN where a target is invalid"""
    pl, Pi, _, phi = geopotential(p, t, sig, dsig, sigt, ptop, hm)
    t = np.asarray(t, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64).reshape(-1)
    L = pl.shape[0]
    tup = np.roll(t, -1, axis=0)
    Z = np.full((P.size,) + pl.shape[1:], np.nan)
    valid = np.zeros((P.size,) + pl.shape[1:], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, Pn in enumerate(P):
            valid[n] = (pl[L - 1] < pl[0]) & (pl[L - 1] <= Pn) & (Pn <= pl[0])
            ge = pl[:L - 1] >= Pn
            k = np.where(ge.any(axis=0), L - 2 - np.argmax(ge[::-1], axis=0), 0)[None]
            take = lambda x: np.take_along_axis(x, k, 0)[0]                              # noqa: E731
            plk = take(pl)
            # (Pi of the target through the same np.power call as the levels': a target on pl[k] gives a difference of 0.0)
            piP = np.power(np.where(plk == Pn, plk, Pn) / P0, KAPPA)
            layer = CP * (0.5 * (take(t) + take(tup)))
            Z[n] = np.where(valid[n], (take(phi) + layer * (take(Pi) - piP)) / G, np.nan)
    return Z, valid


def terms(p, u, v, t, q, sig, dsig, sigt, ptop, hm, P, v_north=None):
    """-> (the thirteen (N, H, W) terms of one sample, 0.0 where the target is invalid in the column; [p, p p])"""
    Z, valid = heights(p, t, sig, dsig, sigt, ptop, hm, P)
    out, v2 = pref.fields(p, u, v, t, q, sig, ptop, P, v_north)
    assert np.array_equal(valid, v2)
    uc, vc, _, T, qq = out
    raw = [np.ones(valid.shape), Z, Z * Z, T, T * T, uc, vc, uc * uc, vc * vc, uc * vc, vc * T, qq, vc * qq]
    p = np.asarray(p, dtype=np.float64)
    return [np.where(valid, x, 0.0) for x in raw], [p, p * p]


def accumulate(states, sig, dsig, sigt, ptop, hm, P):
    """-> (n, s (13, N, H, W), s2 (2, H, W), bound (13, N, H, W)): the sums over the samples `states` (each (p, u, v, t,
    q)) in sample order, and sum |term|, what the parity bound of a word's sum is relative to"""
    s = s2 = b = None
    for st in states:
        a, a2 = terms(st[0], st[1], st[2], st[3], st[4], sig, dsig, sigt, ptop, hm, P)
        a, a2 = np.stack(a), np.stack(a2)
        s, s2, b = (a, a2, np.abs(a)) if s is None else (s + a, s2 + a2, b + np.abs(a))
    return len(states), s, s2, b
