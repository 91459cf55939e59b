"""The grey radiation of GCM_PE25D restated in NumPy (grey_solar.py:323-333, 358-563; no_limits_2_5d.py:66-75) with the
parameters, the clock and the arithmetic type open, the comparison rule the radiation tests share, and the same
computation with one planted fault.  With real = float64 the restatement is oracle.physics bit for bit
(test_pe25d_radiation_cpu.py asserts it), so it is the oracle with its terms visible, not a second opinion;
real = longdouble is the high-precision side.  TEST INFRASTRUCTURE, NumPy only, no test in here."""
import collections
import math

import numpy as np

from oracle.constants import Cp, G, P0, kappa
from oracle.physics import Cg, sb_constant, solar_constant

TOL64 = 1e-10                    # the project's parity bound
U32, H32 = 2.0 ** -23, 2.0 ** -24   # one and half a unit in the last place of a float32

Rad = collections.namedtuple("Rad", "dTdt dt_ground em lwa lwb U_n S_n factor sza tt tp")

FAULTS = ("albedo_default", "tables_stale", "lwb_shift", "down_from_below_top", "no_clamp", "hour_sign", "lon_next",
          "lat_own_row", "sigk_of_k1")


def _col(a, real):
    return np.asarray(a, dtype=real).reshape(-1, 1, 1)


def tables(dsig, sig, t_lw, t_sw, real=np.float64):
    """-> tlw, tsw, csw_top, clw_b_div, swfac, sigk, each of the shape of dsig: the level tables of the radiation in the
    expression order of oracle/physics.py (grey_solar.py:323-333, 377-385, 541)"""
    dsig, sig = np.asarray(dsig, dtype=real), np.asarray(sig, dtype=real)
    e_n = 1 - real(t_lw) ** dsig
    e_n_sw = 1 - real(t_sw) ** dsig
    tlw, tsw = 1 - e_n, 1 - e_n_sw
    csw_top = np.cumprod(tsw[::-1], axis=0)[::-1]
    clw_b_div = np.cumprod(tlw, axis=0) / tlw
    swfac = (1 - tsw) * csw_top / tsw
    return tlw, tsw, csw_top, clw_b_div, swfac, sig ** real(kappa)


def _radiation(p, t, gt, geom, utc, t_lw, t_sw, albedo, real, row0, lev_real, fault, stale):
    L, (H, W) = geom.layers, np.shape(p)
    p, t, gt = (np.asarray(a, dtype=real) for a in (p, t, gt))
    sig, dsig = _col(geom.sig, real), _col(geom.dsig, real)
    if fault == "albedo_default":
        albedo = 0.3
    if fault == "tables_stale":
        t_lw, t_sw = stale
    lw, sw, csw_top, clw_b_div, swfac, _ = tables(dsig, sig, t_lw, t_sw, real)
    if lev_real is not None:
        # what the kernel reads from a handle's own level tables (a float32 handle keeps them in float32); the
        # transmissivities above come from the host's float64 dsig on either handle
        sig, dsig = _col(_col(sig, lev_real), real), _col(_col(dsig, lev_real), real)
    sig_t = np.concatenate([sig[1:], sig[-1:]]) if fault == "sigk_of_k1" else sig
    tp = p * sig_t + real(geom.ptop)
    tt = t / ((real(P0) / tp) ** real(kappa))
    emission = (1 - lw) * real(sb_constant) * tt ** 4
    B = np.sum(emission * clw_b_div, axis=0)
    # zenith_angle, grey_solar.py:39-65 (declination 0)
    hour_angle = real(utc) / (-24 * 3600.0) * 360 * (math.pi / 180)
    if fault == "hour_sign":
        hour_angle = -hour_angle
    longs = np.asarray(geom.long, dtype=real).reshape(-1)
    if fault == "lon_next":
        longs = np.roll(longs, -1)
    lat_all = np.asarray(geom.lat, dtype=real).reshape(-1, 1)
    lats = lat_all[0:H] if fault == "lat_own_row" else lat_all[row0:row0 + H]
    point_angle = np.tile(longs, (H, 1)) + hour_angle
    declination = real(0 * (math.pi / 180))
    cosz = np.sin(lats) * np.sin(declination) + np.cos(lats) * np.cos(declination) * np.cos(point_angle)
    sza = cosz if fault == "no_clamp" else np.maximum(cosz, 0)
    Sc = real(solar_constant) * sza
    S = (1 - real(albedo)) * Sc * csw_top[0]
    U_s = 1 * real(sb_constant) * gt ** 4
    dt_ground = (B + S - U_s) / real(Cg) / real(.1)
    upwelling = np.zeros((L + 1, H, W), dtype=real)
    downwelling = np.zeros((L + 1, H, W), dtype=real)
    lwa = np.zeros(tt.shape, dtype=real)
    lwb = np.zeros(tt.shape, dtype=real)
    for i in reversed(range(L - 1 if fault == "down_from_below_top" else L)):
        lwa[i] = downwelling[i + 1] * (1 - lw[i])
        downwelling[i] = downwelling[i + 1] * lw[i] + emission[i]
    for i in range(L):
        lwb[i] = upwelling[i] * (1 - lw[i])
        upwelling[i + 1] = upwelling[i] * lw[i] + emission[i]
    if fault == "lwb_shift":
        lwb = np.concatenate([np.zeros((1, H, W), dtype=real), lwb[:-1]])
    U_n = clw_b_div * U_s * (1 - lw)
    S_n = swfac * Sc
    factor = real(G) / (real(Cp) * p * dsig)
    dTdt = (U_n + S_n - 2 * emission + lwa + lwb) * factor
    return Rad(dTdt, dt_ground, emission, lwa, lwb, U_n, S_n, factor, sza, tt, tp)


def radiation(p, t, gt, geom, utc, t_lw=0.1, t_sw=0.9, albedo=0.3, real=np.float64, row0=0, lev_real=None):
    """basic_grey_radiation of the state (p [H, W], theta t [L, H, W]) and the ground temperature gt on geom's levels,
    rows row0 ... of its latitudes (a band) -> Rad: dTdt, dt_ground, the terms of dTdt (emission, the absorbed
    downwelling and upwelling long wave, the ground's and the sun's share), factor = G / (Cp p dsig), the clamped
    zenith cosine, the true temperature and the level pressure.  lev_real: the type of the handle's own sig and dsig"""
    return _radiation(p, t, gt, geom, utc, t_lw, t_sw, albedo, real, row0, lev_real, None, None)


def faulty(name, p, t, gt, geom, utc, t_lw=0.1, t_sw=0.9, albedo=0.3, real=np.float64, row0=0, stale=(0.1, 0.9)):
    """radiation() with the planted fault `name` (FAULTS); stale: the (t_lw, t_sw) whose tables "tables_stale" kept"""
    assert name in FAULTS, name
    return _radiation(p, t, gt, geom, utc, t_lw, t_sw, albedo, real, row0, None, name, stale)


def advance(p, t, gt, rec, dt, real=np.float64):
    """the three lines of solar_timestep behind the radiation record rec -> theta_n, gt_n"""
    gt_n = np.asarray(gt, dtype=real) + rec.dt_ground * real(dt)
    tt_n = rec.tt + rec.dTdt * real(dt)
    return tt_n * ((real(P0) / rec.tp) ** real(kappa)), gt_n


def solar_step(p, t, gt, geom, utc, t_lw, t_sw, albedo, dt, real=np.float64, row0=0, lev_real=None):
    """no_limits_2_5d.solar_timestep with the parameters open -> theta_n, gt_n"""
    rec = radiation(p, t, gt, geom, utc, t_lw, t_sw, albedo, real, row0, lev_real)
    return advance(p, t, gt, rec, dt, real)


# ---------------------------------------------------------------- the comparison rule
def level_scale(want):
    """the maximum of |want| over (j, i), per level for a 3-D field"""
    want = np.abs(np.asarray(want, dtype=np.float64))
    return np.max(want, axis=(-2, -1), keepdims=True)


def bounds(rec, theta_n, gt_n, dt, f32):
    """the allowed |got - want| per element of (dTdt, dt_ground, theta_n, gt_n), from the float64 record rec.  fp64: 1e-10
    of the scale (the level's maximum of |dTdt|, the field's maximum of the others).  fp32, float64 arithmetic on
    float32 storage, adds: for dTdt 2^-23 |want| (the stored rounding), 4 kappa 2^-24 (2 em + lwa + lwb) factor (every
    Exner argument formed from a float32 sig is off by at most half a float32 ulp, which enters T as kappa and the
    emission as 4 kappa) and 2^-24 |want| (the float32 dsig in factor); for dt_ground 2^-23 |want| (stored as
    float32); for theta 2^-23 |theta| and dt times dTdt's bound over the Exner factor.  The ground temperature is
    float64 on either handle"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    dT, dg, th, g_n = f(rec.dTdt), f(rec.dt_ground), f(theta_n), f(gt_n)
    b_dT = TOL64 * level_scale(dT)
    b_dg = TOL64 * np.max(np.abs(dg)) + 0 * dg
    b_th = TOL64 * np.max(np.abs(th)) + 0 * th
    b_g = TOL64 * np.max(np.abs(g_n)) + 0 * g_n
    if f32:
        b_dT = b_dT + U32 * np.abs(dT) + 4 * kappa * H32 * (2 * f(rec.em) + f(rec.lwa) + f(rec.lwb)) * f(rec.factor) \
            + H32 * np.abs(dT)
        b_dg = b_dg + U32 * np.abs(dg)
        exner = (f(rec.tp) / P0) ** kappa
        b_th = b_th + U32 * np.abs(th) + dt * b_dT / exner
    return b_dT + 0 * dT, b_dg, b_th, b_g


NAMES = ("dTdt", "dt_ground", "theta", "gt")


def judge(got, want, bnds, what, names=NAMES, dark=None, out=None):
    """every figure printed, then asserted: the worst |got - want| over its bound, per field.  dark: a [H, W] mask of
    the columns whose dTdt (the first field) is exactly 0 by construction: there the device's must be exactly 0.
    out: a dict that collects the worst share per field.  -> the shares"""
    shares = []
    for name, x, y, b in zip(names, got, want, bnds):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert x.shape == y.shape == np.shape(b), (what, name, x.shape, y.shape, np.shape(b))
        err = np.abs(x - y)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0, 0.0, err / b)
        share = np.where(np.isfinite(x), share, np.inf)
        shares.append(float(np.max(share)))
        if out is not None:
            out[name] = max(out.get(name, 0.0), shares[-1])
    print("radiation", what, " ".join("%s %.3g" % kv for kv in zip(names, shares)))
    if dark is not None:
        x, y = np.asarray(got[0]), np.asarray(want[0])
        assert np.any(dark) and np.all(y[:, dark] == 0), (what, "the reference's dark columns are not exactly 0")
        assert np.all(x[:, dark] == 0), (what, "dTdt of a dark column is not exactly 0")
    for name, s in zip(names, shares):
        assert s <= 1.0, (what, name, "error / bound = %.3g" % s)
    return shares


def accepts(got, want, bnds, dark=None):
    """the rule as a predicate (what judge asserts), for the planted faults"""
    for x, y, b in zip(got, want, bnds):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if not np.all(np.isfinite(x)) or np.any(np.abs(x - y) > b):
            return False
    if dark is not None and not np.all(np.asarray(got[0])[:, dark] == 0):
        return False
    return True
