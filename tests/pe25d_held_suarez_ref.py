"""NumPy restatement of the Held-Suarez forcing of GCM_PE25D (include/gcmcore.h, gcm_set_held_suarez): exactly the
arithmetic the header states, float64, every operation rounded on its own, in the header's order.  TEST INFRASTRUCTURE, no
test in here; shared by tests/test_pe25d_held_suarez_cpu.py and tests/test_pe25d_held_suarez_gpu.py.

    r[k]     = max(0, (sig[k] - sigma_b) / (1 - sigma_b))
    fu[k]    = 1 / (1 + (dt k_f) r[k])
    c2[j]    = cos(lat[j])^2;   s2[j] = sin(lat[j])^2
    kt[k][j] = k_a + (((k_s - k_a) r[k]) c2[j]) c2[j]
    r[k] > 0:  u <- u fu[k],  v <- v fu[k]
    p_lev    = sig[k] p + ptop
    theta_eq = max(T_min (P0 / p_lev)^kappa, T_0 - dT_y s2[j] - (dtheta_z ln(p_lev / P0)) c2[j])
    theta   <- (theta + (dt kt) theta_eq) / (1 + dt kt)
"""
import numpy as np

P0, KAPPA = 100000.0, 287.0 / 1004.0                     # constants.py:31,28 (the model's own)
DEFAULTS = dict(k_f=1.0 / 86400.0, k_a=1.0 / (40.0 * 86400.0), k_s=1.0 / (4.0 * 86400.0), sigma_b=0.7, dT_y=60.0,
                dtheta_z=10.0, T_0=315.0, T_min=200.0)


def params(**over):
    out = dict(DEFAULTS)
    out.update(over)
    return out


def r_of(sig, sigma_b):
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    return np.maximum(0.0, (sig - sigma_b) / (1.0 - sigma_b))


def tables(sig, lat, dt, **over):
    """-> dict(r (L,), fu (L,), kt (L, n), s2 (n,), c2 (n,))"""
    p = params(**over)
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    r = r_of(sig, p["sigma_b"])
    fu = 1.0 / (1.0 + (dt * p["k_f"]) * r)
    c, s = np.cos(lat), np.sin(lat)
    c2, s2 = c * c, s * s
    kt = p["k_a"] + (((p["k_s"] - p["k_a"]) * r)[:, None] * c2[None, :]) * c2[None, :]
    return dict(r=r, fu=fu, kt=kt, s2=s2, c2=c2)


def theta_eq(p, sig, ptop, lat, **over):
    """-> (L, H, W): the equilibrium potential temperature of the state's pressure field; lat: the H rows' latitudes"""
    q = params(**over)
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    s = np.sin(lat)
    c = np.cos(lat)
    s2, c2 = (s * s)[None, :, None], (c * c)[None, :, None]
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    p_lev = sig[:, None, None] * np.asarray(p, dtype=np.float64)[None] + ptop
    cold = q["T_min"] * (P0 / p_lev) ** KAPPA
    warm = (q["T_0"] - q["dT_y"] * s2) - (q["dtheta_z"] * np.log(p_lev / P0)) * c2
    return np.maximum(cold, warm)


def step(p, u, v, t, sig, ptop, lat, dt, dtype="f64", **over):
    """one application -> (u, v, t); p (H, W), the rest (L, H, W); lat: the H rows' latitudes.  dtype "f32": the inputs
    are values of the storage type, the arithmetic is float64 and the result is rounded to float32 once (returned as
    float64, as the host API hands it out)"""
    T = tables(sig, lat, dt, **over)
    fr = T["r"] > 0.0
    fu = T["fu"][:, None, None]
    u, v, t = (np.asarray(x, dtype=np.float64) for x in (u, v, t))
    un, vn = u.copy(), v.copy()
    un[fr] = (u * fu)[fr]
    vn[fr] = (v * fu)[fr]
    a = dt * T["kt"][:, :, None]
    te = theta_eq(p, sig, ptop, lat, **over)
    tn = (t + a * te) / (1.0 + a)
    if dtype == "f32":
        un, vn, tn = (x.astype(np.float32).astype(np.float64) for x in (un, vn, tn))
    return un, vn, tn
