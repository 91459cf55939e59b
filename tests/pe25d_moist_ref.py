"""NumPy restatement of the moist physics of GCM_PE25D (include/gcmcore.h, gcm_set_moist): exactly the arithmetic the
header states, float64, every operation rounded on its own, in the header's order -- and the humid inputs the tests of
the phase share.  NumPy only: no torch, no library.  TEST INFRASTRUCTURE, no test in here; shared by
tests/test_pe25d_moist_cpu.py, tests/test_pe25d_moist_gpu.py and tests/column_phase_cases.py.

    p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa;  T = theta Pi;  tc = T - 273.15
    a = 18.678 - tc / 234.5;  b = tc / (257.14 + tc);  e_s = (0.61121 * 1000.0) exp(a b)
    can saturate iff e_s < p_lev:  den = p_lev - (1 - eps) e_s;  q_s = (eps e_s) / den
        dlne = (a * 257.14) / (257.14 + tc)^2 - tc / (234.5 (257.14 + tc));  dq_s = (q_s (p_lev / den)) dlne
    can and q > q_s:  C = (q - q_s) / (1 + (Lv / Cp) dq_s);  q <- q - C;  theta <- theta + ((Lv / Cp) C) / Pi
    P = sum_k C_k ((dsig[k] p) / G), k = 0 .. L - 1 in order, from 0.0
    tau_e > 0, level kb = argmax sig, behind its condensation, T = theta_new Pi:  q_eq = rh_s q_s;  x = dt / tau_e
        can and q_eq > q:  q_new = (q + x q_eq) / (1 + x);  E = (q_new - q) ((dsig[kb] p) / G);  q <- q_new
"""
import numpy as np

import pe25d_inputs as inp

RD, RV, CP, G, P0 = 287.0, 461.0, 1004.0, 9.8, 100000.0       # constants.py (the model's own)
KAPPA = RD / CP
EPS = RD / RV
DEFAULTS = dict(Lv=2.5e6, tau_e=0.0, rh_s=0.8)
# (H, W, L) of the GPU tests: the suite's own two, and one whose row crosses a 256-lane workgroup with a partial tail,
# with L > 40 and L no multiple of the kernel's level batch
SHAPES = ((24, 36, 9), (6, 10, 3), (5, 300, 42))
PTOPS = (0.0, 1000.0)


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update(over)
    return out


def saturation(T, p_lev):
    """-> (e_s, q_s, dq_s, can), float64 arrays of the broadcast shape; q_s and dq_s are 0 where the cell cannot saturate"""
    T, p_lev = np.broadcast_arrays(np.asarray(T, dtype=np.float64), np.asarray(p_lev, dtype=np.float64))
    tc = T - 273.15
    a = 18.678 - tc / 234.5
    d = 257.14 + tc
    b = tc / d
    es = (0.61121 * 1000.0) * np.exp(a * b)
    can = es < p_lev
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = p_lev - (1.0 - EPS) * es
        qs = (EPS * es) / den
        dlne = (a * 257.14) / (d * d) - tc / (234.5 * d)
        dqs = (qs * (p_lev / den)) * dlne
    return es, np.where(can, qs, 0.0), np.where(can, dqs, 0.0), can


def levels(p, sig, ptop):
    """-> (p_lev, Pi), (L, H, W)"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    p_lev = sig[:, None, None] * np.asarray(p, dtype=np.float64)[None] + ptop
    return p_lev, (p_lev / P0) ** KAPPA


def moist_step(p, t, q, sig, dsig, ptop, dt, params, dtype="f64"):
    """one application -> (t, q, precip, evap); p (H, W), t and q (L, H, W); precip and evap (H, W), kg / m^2.  dtype
    "f32": the inputs are rounded to float32, the arithmetic is float64 and the fields are rounded to float32 once
    (returned as float64, as the host API hands them out); precip and evap stay float64"""
    if dtype == "f32":
        p, t, q = (np.asarray(x).astype(np.float32) for x in (p, t, q))
    p, t, q = (np.asarray(x, dtype=np.float64) for x in (p, t, q))
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    L = sig.size
    lc = params["Lv"] / CP
    p_lev, pi = levels(p, sig, ptop)
    _, qs, dqs, can = saturation(t * pi, p_lev)
    w = (dsig[:, None, None] * p[None]) / G
    cond = can & (q > qs)
    with np.errstate(invalid="ignore"):
        C = np.where(cond, (q - qs) / (1.0 + lc * dqs), 0.0)
    qn = np.where(cond, q - C, q)
    tn = np.where(cond, t + (lc * C) / pi, t)
    precip = np.zeros_like(p)
    for k in range(L):
        precip = precip + C[k] * w[k]
    evap = np.zeros_like(p)
    if params["tau_e"] > 0.0:
        kb = int(np.argmax(sig))
        x = dt / params["tau_e"]
        _, qs2, _, can2 = saturation(tn[kb] * pi[kb], p_lev[kb])
        q_eq = params["rh_s"] * qs2
        ev = can2 & (q_eq > qn[kb])
        q2 = (qn[kb] + x * q_eq) / (1.0 + x)
        evap = np.where(ev, (q2 - qn[kb]) * w[kb], 0.0)
        qn[kb] = np.where(ev, q2, qn[kb])
    if dtype == "f32":
        tn, qn = (a.astype(np.float32).astype(np.float64) for a in (tn, qn))
    return tn, qn, precip, evap


def humid_state(geom, dtype="f64", isothermal=False):
    """the seeded state (pe25d_inputs.state_of) made humid: [p, u, v, t, q].  Unless isothermal, theta of level k is
    multiplied by max(2/3, sig[k]^0.19): a 300 K surface and about 200 K aloft.  The relative humidity is
    0.3 + 1.1 random (seed 21), kept 1e-3 clear of saturation (such draws become 1.05), q = min(rh q_s, 0.5) where the
    cell can saturate and 0.02 elsewhere; a capped cell that lands within 1e-3 of saturation becomes 1.05 q_s too.  f32: rounded to float32 at the end (what the handle holds)"""
    p, u, v, t, q = inp.state_of(geom)
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1)
    if not isothermal:
        t = t * np.maximum(2.0 / 3.0, sig ** 0.19)[:, None, None]
    rh = 0.3 + 1.1 * np.random.default_rng(21).random(q.shape)
    rh = np.where(np.abs(rh - 1.0) < 1e-3, 1.05, rh)
    p_lev, pi = levels(p, sig, geom.ptop)
    _, qs, _, can = saturation(t * pi, p_lev)
    q = np.where(can, np.minimum(rh * qs, 0.5), 0.02)
    # (the cap moves a few cells of the isothermal columns' top levels, where q_s passes 0.5, to within 1e-3 of
    # saturation again: they are kept clear by the same rule)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = can & (np.abs(q / qs - 1.0) < 1e-3)
    q = np.where(near, 1.05 * qs, q)
    st = [p, u, v, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


def conditions(p, t, q, sig, ptop):
    """-> (margin, share, guard): min |q / q_s - 1| over the cells that can saturate, the share of all cells that
    condense, the share that cannot saturate"""
    p_lev, pi = levels(p, sig, ptop)
    _, qs, _, can = saturation(np.asarray(t, dtype=np.float64) * pi, p_lev)
    q = np.asarray(q, dtype=np.float64)
    margin = float(np.min(np.abs(q[can] / qs[can] - 1.0)))
    share = float(np.mean(can & (q > qs)))
    return margin, share, float(np.mean(~can))


def column_water(p, q, dsig):
    """sum_k q dsig p / G, (H, W)"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    return np.sum(q * (dsig[:, None, None] * p[None]) / G, axis=0)


def column_enthalpy(p, t, q, sig, dsig, ptop, Lv):
    """sum_k (Cp T + Lv q) dsig p, (H, W)"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    _, pi = levels(p, sig, ptop)
    return np.sum((CP * (t * pi) + Lv * q) * (dsig[:, None, None] * p[None]), axis=0)
