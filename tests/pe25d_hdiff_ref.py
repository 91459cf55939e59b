"""NumPy restatement of the horizontal diffusion of GCM_PE25D (include/gcmcore.h, gcm_set_hdiff): the host tables and one
application, float64, np.roll for the periodic neighbours, every operation in the contract's order and rounded on its
own.  fp32 storage: the values widened, the arithmetic float64, the result rounded once.  The CPU tests hold
gcm_hdiff_tables and gcm_hdiff_apply to it bit for bit, the GPU tests the kernel.  TEST INFRASTRUCTURE, no test in here."""
import collections

import numpy as np

DEFAULTS = collections.OrderedDict(order=2, fields=7, nu=1.0e15, cmax=0.125)
BITS = collections.OrderedDict(u=1, v=2, t=4, q=8)
NAMES = ("ax", "bn", "bs", "area", "axv", "bnv", "bsv", "areav")
DT = 120.0
# (order, nu) of the cases, and per case the centre rows of gen_geometry(24, 36, 9) that run at the cap
CASES = ((1, 1.0e5), (1, 1.0e9), (2, 1.0e15), (2, 1.0e22))
CAPPED_24 = {(1, 1.0e5): 0, (1, 1.0e9): 16, (2, 1.0e15): 0, (2, 1.0e22): 24}


def mask_of(fields):
    if isinstance(fields, str):
        m = 0
        for c in fields:
            m |= BITS[c]
        return m
    return int(fields)


def params(**over):
    out = collections.OrderedDict(DEFAULTS)
    out.update(over)
    out["fields"] = mask_of(out["fields"])
    return out


def tables(dx_j, dx_h, dy, dt, order=2, nu=1.0e15, cmax=0.125, **_):
    """dict of the eight (H,) tables of gcm_hdiff_tables"""
    dx_j = np.asarray(dx_j, dtype=np.float64).reshape(-1)
    dx_h = np.asarray(dx_h, dtype=np.float64).reshape(-1)
    dy, nu, dt, cmax = np.float64(dy), np.float64(nu), np.float64(dt), np.float64(cmax)
    with np.errstate(divide="ignore"):
        s = nu * dt if order == 1 else np.sqrt(nu * dt)
        ay = np.minimum(s / (dy * dy), cmax)
        dx_hn, dx_js = np.roll(dx_h, 1), np.roll(dx_j, -1)     # dx_h[j - 1], dx_j[j + 1]
        ax = np.minimum(s / (dx_j * dx_j), cmax)
        area = ((dx_hn + dx_h) * dy) * 0.5
        bs = (ay * (dx_h * dy)) / area
        bn = (ay * (dx_hn * dy)) / area
        axv = np.minimum(s / (dx_h * dx_h), cmax)
        areav = ((dx_j + dx_js) * dy) * 0.5
        bsv = (ay * (dx_js * dy)) / areav
        bnv = (ay * (dx_j * dy)) / areav
    return dict(zip(NAMES, (ax, bn, bs, area, axv, bnv, bsv, areav)))


def tables_of(geom, dt, **par):
    return tables(geom.dx_j, geom.dx_h, geom.dy, dt, **par)


def centre(tab):
    return tab["ax"], tab["bn"], tab["bs"]


def vrows(tab):
    return tab["axv"], tab["bnv"], tab["bsv"]


def D(X, ax, bn, bs):
    """D(X) of X (..., H, W) with the rows' coefficients (H,)"""
    ax, bn, bs = (np.asarray(a, dtype=np.float64)[:, None] for a in (ax, bn, bs))
    e, w = np.roll(X, -1, axis=-1), np.roll(X, 1, axis=-1)
    s, n = np.roll(X, -1, axis=-2), np.roll(X, 1, axis=-2)
    zx = (e - X) - (X - w)
    gs = s - X
    gn = X - n
    return ax * zx + (bs * gs - bn * gn)


def step(X, coef, order, dtype="f64"):
    """one application to X (..., H, W), float64 holding the storage type's values; coef = (ax, bn, bs)"""
    X = np.asarray(X, dtype=np.float64)
    d = D(X, *coef)
    out = X + d if order == 1 else X - D(d, *coef)
    return out.astype(np.float32).astype(np.float64) if dtype == "f32" else out


def apply(state, tab, order=2, fields=7, dtype="f64", **_):
    """[p, u, v, t, q] behind one application: the selected fields stepped, the others as they are"""
    fields = mask_of(fields)
    out = list(state)
    for n, (f, bit) in enumerate(zip("uvtq", (1, 2, 4, 8)), start=1):
        if fields & bit:
            out[n] = step(state[n], vrows(tab) if f == "v" else centre(tab), order, dtype)
    return out


def square_geometry(H=12, W=16, d=2.0e5):
    """a uniform square geometry: every dx_j, dx_h and dy the same"""
    Sq = collections.namedtuple("Sq", "height width dx_j dx_h dy")
    return Sq(H, W, np.full(H, d), np.full(H, d), d)


def checkerboard(H, W, nlev=1):
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.broadcast_to((-1.0) ** (i + j), (nlev, H, W)).copy()
