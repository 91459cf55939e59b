"""The grey radiation of GCM_PE25D that absorbs by water vapour and CO2, restated in NumPy statement by statement from
the reference's grey_radiation (grey_solar.py:192-320) with clouds off (c = 0: every cloud term is an exact zero and is
left out), the parameters, the insolation, the arithmetic type and a band's first row open; the comparison rule the gas
radiation tests share; and the same computation with one planted fault.  With real = float64 and the reference's
weights the restatement is golden g15 bit for bit (test_pe25d_gas_radiation_cpu.py asserts it), so it is the reference
with its terms visible, not a second opinion; real = longdouble is the high-precision side.
TEST INFRASTRUCTURE, NumPy only, no test in here."""
import collections
import math

import numpy as np

from oracle.constants import Cp, G, P0, Rd, kappa
from oracle.physics import Cg, sb_constant

TOL64 = 1e-10                    # the project's parity bound
CLOSURE = 1e-12                  # the project's closure bound, of SC
U32 = 2.0 ** -23                 # one unit in the last place of a float32
M_CO2, Md = 44.010 * 1e-3, 28.97 * 1e-3      # constants.py:68,13 as the unit bookkeeping holds them, kg / mol

DEFAULTS = collections.OrderedDict(k_h2o_lw=0.125, k_co2_lw=1.0, k_h2o_sw=0.125, k_co2_sw=1.0, co2_vmr=300 / 1e6,
                                   ground_albedo=0.1, solar_constant=2 * 41840 * 60.0 ** -1, declination=0.0,
                                   insolation="uniform")

Gas = collections.namedtuple("Gas", "dt_ground dt_air olr SC sw_sfc lw_down lw_up swd0 heat tt tp")
WORDS = ("SC", "sw_sfc", "lw_down", "lw_up", "olr")      # the five budget words, in the order of GCM_SLAB_SC .. GCM_SLAB_OLR

FAULTS = ("q_no_clamp", "weights_swapped", "up_from_zero", "abs_of_k1", "albedo_on_lw", "decl_sign", "lat_own_row",
          "olr_below_top")


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = collections.OrderedDict(DEFAULTS)
    out.update(over)
    return out


def _col(a, real):
    return np.asarray(a, dtype=real).reshape(-1, 1, 1)


def insolation(par, lat, lon, utc, H, row0=0, real=np.float64, fault=None):
    """SC [H, W] of rows row0 ... of the latitudes lat (all global rows) and the longitudes lon"""
    S0, decl = real(par["solar_constant"]), real(par["declination"])
    if fault == "decl_sign":
        decl = -decl
    lon = np.asarray(lon, dtype=real).reshape(-1)
    lat_all = np.asarray(lat, dtype=real).reshape(-1, 1)
    lats = lat_all[0:H] if fault == "lat_own_row" else lat_all[row0:row0 + H]
    kind = par["insolation"]
    if kind == "uniform":
        irradiance = S0
        irradiance = irradiance * real(0.5 * 0.5)                 # grey_solar.py:208-209
        return np.full((H, lon.size), irradiance, dtype=real)
    if kind == "zenith":
        hour_angle = real(utc) / (-24 * 3600.0) * 360 * (math.pi / 180)      # grey_solar.py:51
        point_angle = np.tile(lon, (H, 1)) + hour_angle
        cosz = np.sin(lats) * np.sin(decl) + np.cos(lats) * np.cos(decl) * np.cos(point_angle)
        return S0 * np.maximum(cosz, 0)
    assert kind == "daily", kind
    # daily_average_irradiance, grey_solar.py:32-36, the arccos argument kept inside [-1, 1]
    dH = np.arccos(np.clip(-np.tan(lats) * np.tan(decl), -1, 1))
    day = S0 / (real(math.pi) * 1.0) * (dH * np.sin(lats) * np.sin(decl) + np.cos(lats) * np.cos(decl) * np.sin(dH))
    return np.tile(day, (1, lon.size))


def _columns(p, tt, q, gt, sig, dsig, ptop, SC, par, real, fault):
    L, (H, W) = np.shape(tt)[0], np.shape(p)
    p, tt, q, gt = (np.asarray(a, dtype=real) for a in (p, tt, q, gt))
    SC = np.broadcast_to(np.asarray(SC, dtype=real), (H, W))
    sig, dsig = _col(sig, real), _col(dsig, real)
    lw = (real(par["k_h2o_lw"]), real(par["k_co2_lw"]))
    sw = (real(par["k_h2o_sw"]), real(par["k_co2_sw"]))
    if fault == "weights_swapped":
        lw, sw = sw, lw
    co2_mmr = real(par["co2_vmr"]) * real(M_CO2) / real(Md)       # mmr_from_vmr
    a_g = real(par["ground_albedo"])
    qc = q if fault == "q_no_clamp" else np.maximum(q, 0)
    tp = p * sig + real(ptop)
    rho = tp / (real(Rd) * tt)
    dp = p * dsig
    depth = dp / (rho * real(G))

    def absorbance(weights):
        a = np.zeros(rho.shape, dtype=real)
        for gas, k in zip((qc, co2_mmr), weights):
            a += gas * rho * depth * k
        return a
    sw_transmittance = real(10) ** -absorbance(sw)
    lw_emissivity = 1 - real(10) ** -absorbance(lw)
    emittance = real(sb_constant) * tt ** 4 * lw_emissivity
    ground_emittance = real(sb_constant) * gt ** 4
    swd = np.zeros((L + 1, H, W), dtype=real)
    lwd = np.zeros((L + 1, H, W), dtype=real)
    lwu = np.zeros((L + 1, H, W), dtype=real)
    swd[-1] = SC
    absorbed = np.zeros(tt.shape, dtype=real)
    for k in reversed(range(L)):
        previous = swd[k + 1]
        total = previous * (1 - sw_transmittance[k])
        swd[k] = previous - total
        absorbed[k] += total
        previous = lwd[k + 1]
        total = previous * lw_emissivity[k]
        absorbed[k] += total
        lwd[k] = previous - total + emittance[k]
    if fault == "albedo_on_lw":
        gain = (1 - a_g) * swd[0] + (1 - a_g) * lwd[0]
    else:
        gain = (1 - a_g) * swd[0] + lwd[0]
    lwu[0] = 0 if fault == "up_from_zero" else ground_emittance
    for k in range(L):
        previous = lwu[k]
        total = previous * lw_emissivity[k]
        absorbed[k] += total
        lwu[k + 1] = previous - total + emittance[k]
    if fault == "abs_of_k1":
        absorbed = np.concatenate([absorbed[1:], absorbed[-1:]])
    dt_ground = (gain - ground_emittance) / real(Cg) / real(.1)
    heat = real(Cp) * rho * depth
    dt_air = (absorbed - 2 * emittance) / heat
    olr = lwu[-2] if fault == "olr_below_top" else lwu[-1]
    return Gas(dt_ground, dt_air, olr, SC + 0, (1 - a_g) * swd[0], lwd[0] + 0, ground_emittance, swd[0] + 0, heat, tt, tp)


def columns(p, tt, q, gt, sig, dsig, ptop, SC, par=DEFAULTS, real=np.float64):
    """grey_radiation, c = 0, of the columns (p, gt [H, W]; the true temperature tt and q [L, H, W]) under the insolation
    SC (a scalar or [H, W]) -> Gas: the three results, the budget words, SWd[0], Cp rho depth, tt and tp"""
    return _columns(p, tt, q, gt, sig, dsig, ptop, SC, par, real, None)


def true_temp(p, t, geom, real=np.float64):
    """temperature.to_true_temp on geom's levels -> tt"""
    tp = np.asarray(p, dtype=real) * _col(geom.sig, real) + real(geom.ptop)
    return np.asarray(t, dtype=real) / ((real(P0) / tp) ** real(kappa))


def radiation(p, t, q, gt, geom, utc, par=DEFAULTS, real=np.float64, row0=0, fault=None):
    """the diagnostic form on the state (p [H, W], theta t and q [L, H, W]) and the ground temperature gt on geom's
    levels, rows row0 ... of its latitudes (a band) -> Gas.  fault: one of FAULTS, planted"""
    assert fault is None or fault in FAULTS, fault
    H = np.shape(p)[0]
    SC = insolation(par, geom.lat, geom.long, utc, H, row0, real, fault)
    return _columns(p, true_temp(p, t, geom, real), q, gt, geom.sig, geom.dsig, geom.ptop, SC, par, real, fault)


def advance(gt, rec, dt, real=np.float64):
    """the three statements of solar_timestep behind the record rec -> theta_n, gt_n"""
    gt_n = np.asarray(gt, dtype=real) + rec.dt_ground * real(dt)
    tt_n = rec.tt + rec.dt_air * real(dt)
    return tt_n * ((real(P0) / rec.tp) ** real(kappa)), gt_n


def closure(rec):
    """the column's energy budget, W / m^2, 0 to rounding: what the air and the ground gain, what the ground reflects
    and what leaves at the top, less what came in"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    a_g_swd0 = f(rec.swd0) - f(rec.sw_sfc)
    ground = f(rec.dt_ground) * Cg * .1
    return np.sum(f(rec.heat) * f(rec.dt_air), axis=0) + ground + a_g_swd0 + f(rec.olr) - f(rec.SC)


# ---------------------------------------------------------------- the tests' own inputs
UTC = 5 * 3600.0 + 1234.5        # the clock of the explicit calls: a day side and a night side, no column on the terminator
# the parameter sets the GPU test takes every shape through: all three insolations, declination 0 and 0.4, equal weight
# pairs (the reference's: one power per level) and unequal ones
CASES = collections.OrderedDict((
    ("defaults", dict()),
    ("uniform_unequal", dict(k_co2_sw=1e-3)),
    ("zenith0", dict(insolation="zenith", k_co2_sw=1e-3, k_h2o_sw=0.05)),
    ("zenith_d", dict(insolation="zenith", declination=0.4, k_co2_sw=1e-3)),
    ("daily0", dict(insolation="daily")),
    ("daily_d", dict(insolation="daily", declination=0.4, k_co2_sw=1e-3, ground_albedo=0.25, solar_constant=1360.0)),
))
# the case on which a planted fault must show: every fault shows on any of them, but for the weights (unequal pairs), the
# declination's sign (a declination) and the latitude's row (an insolation that depends on it, and row0 != 0)
FAULT_CASE = dict(weights_swapped="uniform_unequal", decl_sign="zenith_d", lat_own_row="daily_d")


def state(geom, dtype="f64", seed=15):
    """(p, u, v, theta, q), gt: a resting atmosphere with p = 1e5 + N(0, 500) - ptop, a true temperature in [250, 290],
    q from 1e-6 to 1e-2 with one cell in thirty negative (what the transport can leave) and a ground temperature in
    [280, 300]; f32: rounded to float32, what an fp32 handle holds (the ground temperature is float64 on either)"""
    rng = np.random.default_rng(seed)
    H, W, L = geom.height, geom.width, geom.layers
    p = 1e5 + 500.0 * rng.standard_normal((H, W)) - geom.ptop
    tt = 250.0 + 40.0 * rng.random((L, H, W))
    q = 10.0 ** rng.uniform(-6.0, -2.0, (L, H, W))
    q[rng.random((L, H, W)) < 1 / 30] *= -1
    gt = 280.0 + 20.0 * rng.random((H, W))
    if dtype == "f32":
        p = p.astype(np.float32).astype(np.float64)
    theta = tt * ((P0 / (p * np.asarray(geom.sig, dtype=np.float64).reshape(-1, 1, 1) + geom.ptop)) ** kappa)
    z = np.zeros((L, H, W))
    st = [p, z, z.copy(), theta, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st, gt


# ---------------------------------------------------------------- the comparison rule
def level_scale(want):
    """the maximum of |want| over (j, i), per level for a 3-D field"""
    want = np.abs(np.asarray(want, dtype=np.float64))
    return np.max(want, axis=(-2, -1), keepdims=True)


def bound(want, f32=False):
    """the allowed |got - want| per element: 1e-10 of the scale -- the level's maximum for a 3-D field, the field's for a
    2-D one -- and, f32: what the handle stores in float32, 2^-23 |want| more"""
    want = np.asarray(want, dtype=np.float64)
    b = TOL64 * level_scale(want) + 0 * want
    return b + U32 * np.abs(want) if f32 else b


def shares(got, want, bnds):
    out = []
    for x, y, b in zip(got, want, bnds):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert x.shape == y.shape == np.shape(b), (x.shape, y.shape, np.shape(b))
        err = np.abs(x - y)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0, 0.0, err / b)
        out.append(float(np.max(np.where(np.isfinite(x), share, np.inf))))
    return out


def judge(got, want, names, what, f32=()):
    """every figure printed, then asserted: the worst |got - want| over its bound, per field; f32: the names of the
    fields the handle stores in float32.  -> the shares"""
    bnds = [bound(y, n in f32) for n, y in zip(names, want)]
    s = shares(got, want, bnds)
    print("gas radiation", what, " ".join("%s %.3g" % kv for kv in zip(names, s)))
    for name, x in zip(names, s):
        assert x <= 1.0, (what, name, "error / bound = %.3g" % x)
    return s


def accepts(got, want, f32=()):
    """the rule as a predicate (what judge asserts), for the planted faults; f32: per field, stored in float32"""
    f32 = tuple(f32) + (False,) * (len(want) - len(f32))
    return all(x <= 1.0 for x in shares(got, want, [bound(y, f) for y, f in zip(want, f32)]))
