"""NumPy restatement of the Betts-Miller convection of GCM_PE25D (include/gcmcore.h, gcm_set_betts_miller): exactly the
arithmetic the header states, float64, every operation rounded on its own, in the header's order, vectorised over the
columns and marched level by level -- and the convective inputs the tests of the phase share.  NumPy only: no torch, no
library.  TEST INFRASTRUCTURE, no test in here; shared by tests/test_pe25d_betts_miller_cpu.py and
tests/test_pe25d_betts_miller_gpu.py.  The saturation routine is the moist physics' restatement's
(tests/pe25d_moist_ref.py), with pd = p_lev / den formed from its e_s as the header forms it.

    per level:  p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa;  T = theta Pi;  w = (dsig[k] p) / G;  lc = Lv / Cp
    k = 0:  T_p = T;  s = sat(T_p, p_lev)
    no LCL yet:  T_d = theta_0 Pi;  s = sat(T_d, p_lev);  T_p = T_d;  s.q_s <= q_0:  k_lcl = k;
                 C = (q_0 - s.q_s) / (1 + lc s.dq_s);  T_p = T_d + lc C;  s = sat(T_p, p_lev)
    above k_lcl: nsub midpoint steps of h = (p_lev - p_lev[k-1]) / nsub along
                 slope(T, p) = (kappa T + (lc q_s) pd) / ((1 + lc dq_s) p);  T_p = the end;  s = sat(T_p, p_lev)
    an evaluation that cannot saturate ends the ascent below k
    k >= k_lcl:  buoyant = T_p > T;  buoyant: kt = k;  not buoyant with a kt: the ascent ends below k
    taken:       dq = -r (q - rh_bm s.q_s);  dT = -r (T - T_p);  P = P - dq w;  S = S + dT w;  M = M + w
    deep iff kt and P_q > 0 and S_T > 0:  D = (lc P_q - S_T) / (r M_t);  k <= kt:  theta += (dT + r D) / Pi;  q += dq
"""
import numpy as np

import pe25d_inputs as inp
import pe25d_moist_ref as mref

RD, RV, CP, G, P0 = mref.RD, mref.RV, mref.CP, mref.G, mref.P0
KAPPA, EPS = mref.KAPPA, mref.EPS
DEFAULTS = dict(Lv=2.5e6, tau=7200.0, rh_bm=0.7, nsub=2)
# (H, W, L) of the tests: a partial wave; a 3-level column whose top can only be 1 or 2; a row that crosses workgroups
# with a partial tail, L > 40 and L no multiple of any level batch
SHAPES = ((24, 36, 9), (6, 10, 3), (5, 300, 42))
PTOPS = (0.0, 1000.0)
MARGIN = 1e-8                    # columns whose decision margin is below this are kept out of the "same cells" comparisons
OUTCOMES = ("never saturates", "saturates, never buoyant", "S_T <= 0", "P_q <= 0 < S_T", "deep")
STATE_SEED = 47


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update(over)
    return out


def _sat(T, p_lev):
    """-> (q_s, dq_s, pd, can) of the moist physics' routine; pd = p_lev / den"""
    es, qs, dqs, can = mref.saturation(T, p_lev)
    with np.errstate(all="ignore"):
        den = p_lev - (1.0 - EPS) * es
        pd = np.where(can, p_lev / den, 0.0)
    return qs, dqs, pd, can


def _slope(lc, T, p, s):
    qs, dqs, pd, _ = s
    return (KAPPA * T + (lc * qs) * pd) / ((1.0 + lc * dqs) * p)


def _rel(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(all="ignore"):
        return np.where(m > 0.0, np.abs(a - b) / m, 0.0)


def _pick(mask, a, b):
    return tuple(np.where(mask, x, y) for x, y in zip(a, b))


def ascent(p, t, q, sig, dsig, ptop, dt, par, to_the_top=False):
    """the march of every column -> dict(pi, T, Tp (L, H, W): Pi, T and the parcel's temperature at the levels taken (NaN
    elsewhere); dT, dq (L, H, W); k_lcl, kt (H, W) ints, -1: none; P_q, S_T, M_t (H, W) behind level kt; margin (H, W)).
    to_the_top: buoyancy ends no ascent (the parcel's profile through the whole column, for building inputs)"""
    p, t, q = (np.asarray(x, dtype=np.float64) for x in (p, t, q))
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    L, shape = sig.size, p.shape
    lc = par["Lv"] / CP
    x = dt / par["tau"]
    r = x / (1.0 + x)
    nsub = int(par["nsub"])
    zero = np.zeros(shape)
    alive = np.ones(shape, dtype=bool)
    k_lcl, kt = np.full(shape, -1), np.full(shape, -1)
    th0 = q0 = Tp_prev = pl_prev = zero
    s_prev = (zero, zero, zero, np.zeros(shape, dtype=bool))
    P, S, M, Pq, ST, Mt = (zero,) * 6
    aP, aS, aPq, aST = (zero,) * 4
    margin = np.full(shape, np.inf)
    out = dict(pi=np.empty((L,) + shape), T=np.empty((L,) + shape), Tp=np.full((L,) + shape, np.nan),
               dT=np.zeros((L,) + shape), dq=np.zeros((L,) + shape))
    with np.errstate(all="ignore"):
        for k in range(L):
            pl = sig[k] * p + ptop
            pi = (pl / P0) ** KAPPA
            T = t[k] * pi
            out["pi"][k], out["T"][k] = pi, T
            if k == 0:
                th0, q0 = t[0], q[0]
                Tp = T
                s = _sat(Tp, pl)
                alive = alive & s[3]
            else:
                below, above = alive & (k_lcl < 0), alive & (k_lcl >= 0)
                # no LCL yet
                Td = th0 * pi
                sb = _sat(Td, pl)
                below = below & sb[3]
                margin = np.where(below, np.minimum(margin, _rel(sb[0], q0)), margin)
                here = below & (sb[0] <= q0)
                C = (q0 - sb[0]) / (1.0 + lc * sb[1])
                Tl = Td + lc * C
                sl = _sat(Tl, pl)
                k_lcl = np.where(here, k, k_lcl)
                # above k_lcl: the pseudoadiabat
                h = (pl - pl_prev) / float(nsub)
                hh = 0.5 * h
                Tc, sc = Tp_prev, s_prev
                for n in range(nsub):
                    pa = pl_prev + float(n) * h
                    if n > 0:
                        sc = _sat(Tc, pa)
                        above = above & sc[3]
                    f1 = _slope(lc, Tc, pa, sc)
                    Tm, pm = Tc + hh * f1, pa + hh
                    sm = _sat(Tm, pm)
                    above = above & sm[3]
                    f2 = _slope(lc, Tm, pm, sm)
                    Tc = Tc + h * f2
                sa = _sat(Tc, pl)
                above = above & sa[3]
                Tp = np.where(above, Tc, np.where(here, Tl, Td))
                s = _pick(above, sa, _pick(here, sl, sb))
                alive = above | (below & ~here) | (here & sl[3])
            has = alive & (k_lcl >= 0)
            buoyant = has & (Tp > T)
            margin = np.where(has, np.minimum(margin, _rel(Tp, T)), margin)
            if not to_the_top:
                alive = alive & ~(has & ~buoyant & (kt >= 0))
            w = (dsig[k] * p) / G
            dq = -r * (q[k] - par["rh_bm"] * s[0])
            dT = -r * (T - Tp)
            out["dT"][k], out["dq"][k] = np.where(alive, dT, 0.0), np.where(alive, dq, 0.0)
            out["Tp"][k] = np.where(alive, Tp, np.nan)
            P, S, M = np.where(alive, P - dq * w, P), np.where(alive, S + dT * w, S), np.where(alive, M + w, M)
            aP, aS = np.where(alive, aP + np.abs(dq * w), aP), np.where(alive, aS + np.abs(dT * w), aS)
            top = alive & buoyant
            kt = np.where(top, k, kt)
            Pq, ST, Mt = np.where(top, P, Pq), np.where(top, S, ST), np.where(top, M, Mt)
            aPq, aST = np.where(top, aP, aPq), np.where(top, aS, aST)
            Tp_prev, pl_prev = np.where(alive, Tp, Tp_prev), np.where(alive, pl, pl_prev)
            s_prev = _pick(alive, s, s_prev)
        have = kt >= 0
        margin = np.where(have, np.minimum(margin, np.where(aPq > 0.0, np.abs(Pq) / aPq, 0.0)), margin)
        margin = np.where(have, np.minimum(margin, np.where(aST > 0.0, np.abs(ST) / aST, 0.0)), margin)
    out.update(k_lcl=k_lcl, kt=kt, P_q=Pq, S_T=ST, M_t=Mt, margin=margin, lc=lc, r=r)
    return out


def betts_miller_step(p, t, q, sig, dsig, ptop, dt, par, dtype="f64"):
    """one application -> dict(t, q (L, H, W); precip (H, W), kg / m^2, 0 where the column did not convect; deep (H, W)
    bool; kt (H, W), -1 where the column did not convect; k_lcl, margin, P_q, S_T (H, W) as ascent() leaves them).
    dtype "f32": the inputs are rounded to float32, the arithmetic is float64 and the fields are rounded to float32 once
    (returned as float64, as the host API hands them out); the sums stay float64"""
    if dtype == "f32":
        p, t, q = (np.asarray(x).astype(np.float32) for x in (p, t, q))
    p, t, q = (np.asarray(x, dtype=np.float64) for x in (p, t, q))
    a = ascent(p, t, q, sig, dsig, ptop, dt, par)
    kt, lc, r = a["kt"], a["lc"], a["r"]
    with np.errstate(all="ignore"):
        deep = (kt >= 0) & (a["P_q"] > 0.0) & (a["S_T"] > 0.0)
        D = (lc * a["P_q"] - a["S_T"]) / (r * a["M_t"])
        rD = r * D
        tn, qn = t.copy(), q.copy()
        for k in range(t.shape[0]):
            upd = deep & (k <= kt)
            tn[k] = np.where(upd, t[k] + (a["dT"][k] + rD) / a["pi"][k], t[k])
            qn[k] = np.where(upd, q[k] + a["dq"][k], q[k])
    if dtype == "f32":
        tn, qn = (x.astype(np.float32).astype(np.float64) for x in (tn, qn))
    return dict(t=tn, q=qn, precip=np.where(deep, a["P_q"], 0.0), deep=deep, kt=np.where(deep, kt, -1), k_lcl=a["k_lcl"],
                margin=a["margin"], P_q=a["P_q"], S_T=a["S_T"], top=kt)


def outcome(res):
    """-> (H, W) ints 0 .. 4, the index into OUTCOMES of every column of a betts_miller_step result"""
    out = np.full(res["k_lcl"].shape, 4)
    out[res["P_q"] <= 0.0] = 3
    out[res["S_T"] <= 0.0] = 2
    out[res["top"] < 0] = 1
    out[res["k_lcl"] < 0] = 0
    return out


def conditions(geom, dtype="f64", dt=600.0, par=None):
    """-> (share, margin, res): the share of the columns of convective_state(geom, dtype) in each of OUTCOMES, every
    column's decision margin, and the restatement's result they were read from"""
    st = convective_state(geom, dtype)
    res = betts_miller_step(st[0], st[3], st[4], geom.sig, geom.dsig, geom.ptop, dt, par or params(), dtype)
    oc = outcome(res)
    return [float(np.mean(oc == n)) for n in range(len(OUTCOMES))], res["margin"], res


def convective_state(geom, dtype="f64"):
    """the seeded state (pe25d_inputs.state_of: its p and winds) with theta and q built around every column's own parcel
    so that the columns fall into all five OUTCOMES, a fifth each at random (seed 47):
      the parcel: T_0 = 296 + 8 random, q_0 = rh_0 q_s(T_0), lifted through the whole column (ascent, to_the_top);
      T[k] = T_p[k] - b[k], q[k] = rh[k] q_s(T[k]), level 0 as the parcel's:
        0  q_0 = 0: no level saturates the parcel
        1  b < 0 everywhere: the environment is warmer than the parcel
        2  b < 0 but for the two levels above the LCL, which are buoyant by a tenth of it: S_T <= 0
        3  b > 0 up to a random level above the LCL, a dry environment (rh 0.2 against rh_0 = 0.72): P_q <= 0 < S_T
        4  b > 0 up to a random level above the LCL, rh 0.95: deep
      |b| = 0.5 .. 2.5 K, random per cell.  f32: rounded to float32 at the end (what the handle holds)"""
    p, u, v, _, _ = inp.state_of(geom)
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1)
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(-1)
    L, (H, W) = sig.size, p.shape
    rng = np.random.default_rng(STATE_SEED)
    kind = rng.integers(0, 5, (H, W))
    T0 = 296.0 + 8.0 * rng.random((H, W))
    amp = 0.5 + 2.0 * rng.random((L, H, W))
    p_lev, pi = mref.levels(p, sig, geom.ptop)
    rh0 = np.where(kind == 3, 0.72, 0.8)
    q0 = rh0 * mref.saturation(T0, p_lev[0])[1]
    t = np.repeat((T0 / pi[0])[None], L, axis=0)
    q = np.repeat(q0[None], L, axis=0)
    par = params()
    a = ascent(p, t, q, sig, dsig, geom.ptop, 600.0, par, to_the_top=True)
    assert np.isfinite(a["Tp"]).all() and (a["k_lcl"] >= 1).all()
    k = np.arange(L)[:, None, None]
    lcl = a["k_lcl"][None]
    top = np.minimum(lcl + 1 + rng.integers(0, L, (H, W))[None], L - 1)
    b = np.where((kind[None] >= 3) & (k <= top), amp, -amp)
    b = np.where((kind[None] == 2) & (k > lcl) & (k <= lcl + 2), 0.1 * amp, b)
    T = a["Tp"] - b
    T[0] = T0
    rh = np.where(kind == 3, 0.2, np.where(kind == 4, 0.95, 0.5))[None]
    q = rh * mref.saturation(T, p_lev)[1]
    q[0] = np.where(kind == 0, 0.0, q0)
    st = [p, u, v, T / pi, q]
    if dtype == "f32":
        st = [x.astype(np.float32).astype(np.float64) for x in st]
    return st


def quiet_state(geom, dtype="f64"):
    """convective_state with every column's lowest level dry (q[0] = 0): no parcel saturates, no column convects"""
    st = convective_state(geom, dtype)
    st[4][0] = 0.0
    return st


def column_water(p, q, dsig):
    """sum_k q dsig p / G, (H, W)"""
    return mref.column_water(p, q, dsig)


def column_enthalpy(p, t, q, sig, dsig, ptop, Lv):
    """sum_k (Cp T + Lv q) dsig p, (H, W)"""
    return mref.column_enthalpy(p, t, q, sig, dsig, ptop, Lv)
