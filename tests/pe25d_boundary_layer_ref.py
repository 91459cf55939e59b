"""NumPy restatement of the surface fluxes and the boundary-layer mixing of GCM_PE25D (include/gcmcore.h,
gcm_set_boundary_layer): exactly the arithmetic the header states, float64, every operation rounded on its own, in the
header's order -- and the inputs the tests of the phase share.  NumPy only: no torch, no library.  TEST INFRASTRUCTURE,
no test in here; shared by tests/test_pe25d_boundary_layer_cpu.py, tests/test_pe25d_boundary_layer_gpu.py and
tests/column_phase_cases.py.

    (A)  uc = 0.5 (u[0][j][i] + u[0][j][i-1]);  vc = 0.5 (v[0][j][i] + v[0][j-1][i]);  S = sqrt(uc uc + vc vc)
         p_s = p + ptop;  p_a = sig[0] p + ptop;  Pi_a = (p_a / P0)^kappa;  T_a = theta[0] Pi_a
         z_a = ((Rd / G) (T_a (1 + (Rv / Rd - 1) q[0]))) log(p_s / p_a);  cd = cd0 + cd1 min(S, v_cap);  r = S / z_a
         (q_ss, can_s) = saturation(T_s, p_s)
         m = 0 .. L-2:  sig_e = sig[m] - 0.5 dsig[m];  p_e = sig_e p + ptop
            T_e = 0.5 (theta[m] Pi_m + theta[m+1] Pi_{m+1});  rho_e = p_e / (Rd T_e);  gr = (G rho_e) / p
            f = 1 where p_e >= p_pbl, else exp(-(((p_pbl - p_e) / p_strat)^2))
            e[m] = (((S z_a) f) (gr gr)) / (0.5 (dsig[m] + dsig[m+1]))
    (B)  theta: x = (dt ch) r, target T_s / Pi_a, a = (dt ce) e        q: x = (dt ce) r (0 where not can_s), target q_ss, a = (dt ce) e
         u: x = dt (0.5 (cd_i r_i + cd_{i+1} r_{i+1})), target 0, a = dt (0.5 (cd_i e_i + cd_{i+1} e_{i+1}))      v: likewise in j
         X0' = (X[0] + x target) / (1 + x)
         lo[k] = a[k-1] / dsig[k];  up[k] = a[k] / dsig[k];  d = (1 + lo[k]) + up[k]
         w[0] = 1 / d;  w[k] = 1 / (d - lo[k] g[k-1]);  g[k] = up[k] w[k]
         y[0] = X0' w[0];  y[k] = (X[k] + lo[k] y[k-1]) w[k];  X[L-1] = y[L-1];  X[k] = y[k] + g[k] X[k+1]
    sums, m = (dsig[0] p) / G:  shf = ((Cp Pi_a) (theta0' - theta0)) m;  evap = (q0' - q0) m
"""
import numpy as np

import pe25d_inputs as inp
import pe25d_moist_ref as moist

RD, RV, CP, G, P0, KAPPA = moist.RD, moist.RV, moist.CP, moist.G, moist.P0, moist.KAPPA
DEFAULTS = dict(cd0=7.0e-4, cd1=6.5e-5, v_cap=20.0, ch=0.0044, ce=0.0044, p_pbl=85000.0, p_strat=10000.0)
# (H, W, L) as for the moist phase: a partial wave; a row of two tiles of 64; 300 columns, five tiles with the wrap of
# i + 1 inside the last, and L = 42 above what is parked in LDS; L = 3, where the first and the last interface are neighbours
SHAPES = moist.SHAPES
PTOPS = moist.PTOPS


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update({k: float(v) for k, v in over.items()})
    return out


def surface(par, uc, vc, theta0, q0, p, sig0, ptop):
    """the level-0 part of (A) -> dict(S, z_a, cd, r, pi_a)"""
    uc, vc, theta0, q0, p = (np.asarray(a, dtype=np.float64) for a in (uc, vc, theta0, q0, p))
    S = np.sqrt(uc * uc + vc * vc)
    p_s = p + ptop
    p_a = sig0 * p + ptop
    pi_a = (p_a / P0) ** KAPPA
    T_a = theta0 * pi_a
    z_a = ((RD / G) * (T_a * (1.0 + (RV / RD - 1.0) * q0))) * np.log(p_s / p_a)
    cd = par["cd0"] + par["cd1"] * np.minimum(S, par["v_cap"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = S / z_a
    return dict(S=S, z_a=z_a, cd=cd, r=r, pi_a=pi_a)


def interfaces(par, S, z_a, p, t, sig, dsig, ptop):
    """e (L - 1, ...) of (A); t (L, ...) is theta at phase entry"""
    sig, dsig = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (sig, dsig))
    L = sig.size
    e = np.empty((L - 1,) + np.shape(p))
    Sz = S * z_a
    pi = [((sig[k] * p + ptop) / P0) ** KAPPA for k in range(L)]
    for m in range(L - 1):
        sig_e = sig[m] - 0.5 * dsig[m]
        p_e = sig_e * p + ptop
        T_e = 0.5 * (t[m] * pi[m] + t[m + 1] * pi[m + 1])
        rho_e = p_e / (RD * T_e)
        gr = (G * rho_e) / p
        z = (par["p_pbl"] - p_e) / par["p_strat"]
        f = np.where(p_e >= par["p_pbl"], 1.0, np.exp(-(z * z)))
        e[m] = ((Sz * f) * (gr * gr)) / (0.5 * (dsig[m] + dsig[m + 1]))
    return e


def column(dsig, a, x, target, X):
    """(B) for columns X (L, ...) with a (L - 1, ...), x and target (...) -> (X_out (L, ...), X0')"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    X = np.asarray(X, dtype=np.float64)
    L = X.shape[0]
    X0 = (X[0] + x * target) / (1.0 + x)
    y, g = np.empty_like(X), np.empty_like(X)
    zero = np.zeros_like(X[0])
    for k in range(L):
        lo = (a[k - 1] if k > 0 else zero) / dsig[k]
        up = (a[k] if k < L - 1 else zero) / dsig[k]
        d = (1.0 + lo) + up
        if k == 0:
            w = 1.0 / d
            y[k] = X0 * w
        else:
            w = 1.0 / (d - lo * g[k - 1])
            y[k] = (X[k] + lo * y[k - 1]) * w
        g[k] = up * w
    out = np.empty_like(X)
    out[L - 1] = y[L - 1]
    for k in range(L - 2, -1, -1):
        out[k] = y[k] + g[k] * out[k + 1]
    return out, X0


def centre_winds(u0, v0):
    """uc, vc (H, W) of the lowest level's winds, periodic in i and j"""
    return 0.5 * (u0 + np.roll(u0, 1, axis=1)), 0.5 * (v0 + np.roll(v0, 1, axis=0))


def boundary_layer_step(p, u, v, t, q, gt, sig, dsig, ptop, dt, params, dtype="f64"):
    """one application -> (u, v, t, q, shf, evap); p and gt (H, W), the fields (L, H, W); shf and evap (H, W).  dtype
    "f32": the inputs are rounded to float32, the arithmetic is float64 and the fields are rounded to float32 once
    (returned as float64, as the host API hands them out); the sums stay float64"""
    if dtype == "f32":
        p, u, v, t, q = (np.asarray(x).astype(np.float32) for x in (p, u, v, t, q))
    p, u, v, t, q, gt = (np.asarray(x, dtype=np.float64) for x in (p, u, v, t, q, gt))
    sig, dsig = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (sig, dsig))
    par = params
    uc, vc = centre_winds(u[0], v[0])
    sf = surface(par, uc, vc, t[0], q[0], p, sig[0], ptop)
    cd, r, pi_a = sf["cd"], sf["r"], sf["pi_a"]
    _, q_ss, _, can = moist.saturation(gt, p + ptop)
    e = interfaces(par, sf["S"], sf["z_a"], p, t, sig, dsig, ptop)
    a_tq = (dt * par["ce"]) * e
    tn, t0n = column(dsig, a_tq, (dt * par["ch"]) * r, gt / pi_a, t)
    qn, q0n = column(dsig, a_tq, np.where(can, (dt * par["ce"]) * r, 0.0), q_ss, q)
    zero = np.zeros_like(p)
    cr, ce = cd * r, cd[None] * e
    un, _ = column(dsig, dt * (0.5 * (ce + np.roll(ce, -1, axis=2))), dt * (0.5 * (cr + np.roll(cr, -1, axis=1))), zero, u)
    vn, _ = column(dsig, dt * (0.5 * (ce + np.roll(ce, -1, axis=1))), dt * (0.5 * (cr + np.roll(cr, -1, axis=0))), zero, v)
    mass = (dsig[0] * p) / G
    shf = ((CP * pi_a) * (t0n - t[0])) * mass
    evap = (q0n - q[0]) * mass
    if dtype == "f32":
        un, vn, tn, qn = (a.astype(np.float32).astype(np.float64) for a in (un, vn, tn, qn))
    return un, vn, tn, qn, shf, evap


# ---------------------------------------------------------------- inputs
def windy_state(geom, dtype="f64"):
    """moist.humid_state with the winds scaled row by row from calm to a gale, so that S lies on both
    sides of v_cap = 20 m / s (the state's noise is about 8 m / s); f32: rounded to float32 at the end"""
    p, u, v, t, q = moist.humid_state(geom)
    scale = np.linspace(0.2, 5.0, geom.height)[None, :, None]
    st = [p, u * scale, v * scale, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


def ground(geom, st):
    """a ground temperature with cells warmer and cells colder than the air above them: the lowest level's own
    temperature plus the seeded ground field's noise (inp.ground - 288, about +-1 K) times 4"""
    p, t = st[0], st[3]
    sig0 = float(np.asarray(geom.sig, dtype=np.float64).reshape(-1)[0])
    T_a = t[0] * ((sig0 * p + geom.ptop) / P0) ** KAPPA
    return T_a + 4.0 * (inp.ground(geom.height, geom.width) - 288.0)


def resting_state(geom, dtype="f64"):
    """no wind, and a ground as warm as the air above it: (state, ground)"""
    st = windy_state(geom, dtype)
    st[1], st[2] = np.zeros_like(st[1]), np.zeros_like(st[2])
    p, t = st[0], st[3]
    sig0 = float(np.asarray(geom.sig, dtype=np.float64).reshape(-1)[0])
    return st, t[0] * ((sig0 * p + geom.ptop) / P0) ** KAPPA


def column_sum(x, dsig):
    """sum_k x dsig, (H, W)"""
    return np.sum(x * np.asarray(dsig, dtype=np.float64).reshape(-1)[:, None, None], axis=0)


def assert_maximum_principle(st, gt, geom, out):
    """max |u| and max |v| of a column do not grow; theta and q stay within the range of the column and the target"""
    p, u, v, t, q = st
    un, vn, tn, qn = out[:4]
    sig0 = float(np.asarray(geom.sig).reshape(-1)[0])
    pi_a = ((sig0 * p + geom.ptop) / P0) ** KAPPA
    q_ss = moist.saturation(gt, p + geom.ptop)[1]
    eps = 4 * np.finfo(np.float64).eps
    for a, b in ((u, un), (v, vn)):
        assert (np.abs(b).max(axis=0) <= np.abs(a).max(axis=0) * (1 + eps)).all()
    for a, b, target in ((t, tn, gt / pi_a), (q, qn, q_ss)):
        lo, hi = np.minimum(a.min(axis=0), target), np.maximum(a.max(axis=0), target)
        assert (b >= lo - eps * np.abs(lo)).all() and (b <= hi + eps * np.abs(hi)).all()
