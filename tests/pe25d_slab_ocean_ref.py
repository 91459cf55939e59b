"""The slab mixed-layer ocean of GCM_PE25D restated in NumPy: the flux words the radiation stores while the slab is
registered (built on pe25d_radiation_ref.tables: the level tables in the oracle's expression order, and the scans in the
kernel's), the words of the boundary layer (pe25d_boundary_layer_ref: the increments of shf and evap), the cell rule with
its sums in the order include/gcmcore.h states, and the energy the radiation leaves in the column.  Every operation is
float64 and rounded on its own, as on the device.  TEST INFRASTRUCTURE, NumPy only, no test in here."""
import math

import numpy as np

import pe25d_boundary_layer_ref as bref
import pe25d_radiation_ref as rad
from oracle.constants import Cp, G, P0, kappa
from oracle.physics import sb_constant, solar_constant

WORDS = ("SC", "SW_SFC", "LW_DOWN", "LW_UP", "OLR", "SH_J", "EVAP_KG")
SC, SW_SFC, LW_DOWN, LW_UP, OLR, SH_J, EVAP_KG = range(7)
NWORDS, NSUMS = 7, 10
DEFAULTS = dict(heat_capacity=1.0e7, Lv=2.5e6)
# (H, W, L): a partial wave; two 64-lane tiles with a tail inside one 128-thread radiation tile; L = 30, the 40-level
# instantiation; 300 columns (five 64-lane tiles, three 128-thread ones, both ragged) at L = 42, the LDS-parked form
SHAPES = ((6, 10, 3), (24, 36, 9), (4, 70, 30), (5, 300, 42))
PTOPS = (0.0, 1000.0)


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update({k: float(v) for k, v in over.items()})
    return out


def radiation_words(p, t, gt, geom, utc, t_lw=0.1, t_sw=0.9, albedo=0.3, row0=0):
    """SC, SW_SFC, LW_DOWN, LW_UP, OLR (5, H, W) of the state (p [H, W], theta t [L, H, W]) and the ground temperature
    gt: the kernel's statements in the kernel's order -- U_s from (gt gt)(gt gt), B and `up` level by level from the
    bottom, OLR = up + U_s (clw_b_div[L-1] tlw[L-1]) -- with NumPy's Exner factor, which is why every word but LW_UP is
    held to 1e-10 and not to the bit"""
    p, t, gt = (np.asarray(a, dtype=np.float64) for a in (p, t, gt))
    L, (H, W) = geom.layers, p.shape
    sig, dsig = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (geom.sig, geom.dsig))
    tlw, _, csw_top, clw_b_div, _, _ = rad.tables(dsig, sig, t_lw, t_sw)
    hour_angle = utc / (-24 * 3600.0) * 360 * (math.pi / 180)
    lats = np.asarray(geom.lat, dtype=np.float64).reshape(-1, 1)[row0:row0 + H]
    pa = np.asarray(geom.long, dtype=np.float64).reshape(1, -1) + hour_angle
    sza = np.maximum(np.sin(lats) * 0.0 + np.cos(lats) * 1.0 * np.cos(pa), 0.0)
    Sc = (solar_constant * sza) + np.zeros((H, W))
    S = (1 - albedo) * Sc * csw_top[0]
    g2 = gt * gt
    U_s = 1 * sb_constant * (g2 * g2)
    B, up = np.zeros((H, W)), np.zeros((H, W))
    for k in range(L):
        tt = t[k] / ((P0 / (p * sig[k] + geom.ptop)) ** kappa)
        t2 = tt * tt
        em = (1 - tlw[k]) * sb_constant * (t2 * t2)
        B = B + em * clw_b_div[k]
        up = up * tlw[k] + em
    tcol = clw_b_div[L - 1] * tlw[L - 1]
    return np.stack([Sc, S, B, U_s, up + U_s * tcol])


def boundary_words(p, u, v, t, q, gt, geom, dt, par, dtype="f64"):
    """SH_J, EVAP_KG (2, H, W): what one application of the boundary layer adds to shf and evap"""
    out = bref.boundary_layer_step(p, u, v, t, q, gt, geom.sig, geom.dsig, geom.ptop, dt, par, dtype)
    return np.stack([out[4], out[5]])


def cells(gt, words, dt, C=DEFAULTS["heat_capacity"], Lv=DEFAULTS["Lv"], Q=0.0):
    """the cell rule -> (gt', E4); words (7, ...), C and Q scalars or fields"""
    gt, w = np.asarray(gt, dtype=np.float64), np.asarray(words, dtype=np.float64)
    C, Q = np.asarray(C, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        R = (w[SW_SFC] + w[LW_DOWN]) - w[LW_UP]
        E1 = dt * R
        E2 = E1 - w[SH_J]
        E3 = E2 - Lv * w[EVAP_KG]
        E4 = E3 + dt * Q
        return gt + E4 / C, E4 + 0 * gt


def terms(words, dt, Lv, Q, gt1):
    """what one application adds to the ten sums (10, ...), in their order"""
    w = np.asarray(words, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64) + 0 * gt1
    return np.stack([dt * w[SC], dt * w[SW_SFC], dt * w[LW_DOWN], dt * w[LW_UP], dt * w[OLR], w[SH_J] + 0 * gt1,
                     Lv * w[EVAP_KG], dt * Q, dt * gt1, dt * (gt1 * gt1)])


def apply(gt, words, dt, sums=None, C=DEFAULTS["heat_capacity"], Lv=DEFAULTS["Lv"], Q=0.0):
    """one launch: -> (gt', sums + terms); sums None: zero"""
    gt1, _ = cells(gt, words, dt, C, Lv, Q)
    add = terms(words, dt, Lv, Q, gt1)
    return gt1, (add if sums is None else np.asarray(sums, dtype=np.float64) + add)


def column_heating(dTdt, p, geom):
    """(sum_k dTdt_k Cp p dsig_k / G, sum_k |...|) (H, W): W / m^2 the radiation leaves in the column"""
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(-1, 1, 1)
    x = np.asarray(dTdt, dtype=np.float64) * Cp * np.asarray(p, dtype=np.float64) * dsig / G
    return np.sum(x, axis=0), np.sum(np.abs(x), axis=0)


def ulps(a, b):
    """the largest distance of a from b in units of b's last place"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.abs(b))))
