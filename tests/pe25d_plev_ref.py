"""NumPy restatement of GCM_PE25D on pressure levels (gcm_plev_columns, gcm_plev_fields, gcm_set_plev_climate,
include/gcmcore.h): the column rule in float64, the five level quantities formed as tests/pe25d_climate_ref.py forms
them (T from np.power, where the device takes its own Exner routine), the thirteen terms with an invalid column as 0.0,
and the climatology's own reduction order, pe25d_climate_ref.row_sum.  Also the inputs the masking tests share: the
seeded state with p scaled per column to stand in for topography, and targets taken from the restatement itself.
TEST INFRASTRUCTURE, no test in here."""
import numpy as np

import pe25d_climate_ref as cref

P0, KAPPA = cref.P0, cref.KAPPA
WORDS = ("count", "uc", "vc", "theta", "T", "q", "ucuc", "vcvc", "TT", "ucvc", "vcT", "vctheta", "vcq")
EXNER_WORDS = (4, 8, 10)         # the words that carry the device's Exner routine
EXACT_WORDS = tuple(w for w in range(len(WORDS)) if w not in EXNER_WORDS)
QUANTITIES = ("uc", "vc", "theta", "T", "q")


def column_rule(pl, x, P):
    """pl, x: (L, ...) with level 0 the bottom; P (N,) -> (out (N, ...), valid (N, ...) bool).  Target n is valid iff
    pl[L - 1] <= P[n] <= pl[0] and pl[L - 1] < pl[0]; k is the largest index in 0 .. L - 2 with pl[k] >= P[n];
    w = (pl[k] - P[n]) / (pl[k] - pl[k + 1]); out = (1 - w) x[k] + w x[k + 1], every operation rounded on its own.  out is
    NaN where the target is invalid"""
    pl, x = np.asarray(pl, dtype=np.float64), np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64).reshape(-1)
    L = pl.shape[0]
    out = np.full((P.size,) + pl.shape[1:], np.nan)
    valid = np.zeros((P.size,) + pl.shape[1:], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, Pn in enumerate(P):
            valid[n] = (pl[L - 1] < pl[0]) & (pl[L - 1] <= Pn) & (Pn <= pl[0])
            ge = pl[:L - 1] >= Pn
            k = np.where(ge.any(axis=0), L - 2 - np.argmax(ge[::-1], axis=0), 0)[None]
            plk, plk1 = np.take_along_axis(pl, k, 0)[0], np.take_along_axis(pl, k + 1, 0)[0]
            xk, xk1 = np.take_along_axis(x, k, 0)[0], np.take_along_axis(x, k + 1, 0)[0]
            w = (plk - Pn) / (plk - plk1)
            out[n] = np.where(valid[n], (1.0 - w) * xk + w * xk1, np.nan)
    return out, valid


def levels(p, u, v, t, q, sig, ptop, v_north=None):
    """-> (pl (L, H, W), [uc, vc, theta, T, q] each (L, H, W)) of one state, formed as pe25d_climate_ref.terms forms
    them; v_north (L, W): row -1 of v where it is not row H - 1 (a band's north ghost row)"""
    p, u, v, t, q = (np.asarray(a, dtype=np.float64) for a in (p, u, v, t, q))
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    vm = np.roll(v, 1, axis=1)
    if v_north is not None:
        vm[:, 0, :] = v_north
    uc = 0.5 * (u + np.roll(u, 1, axis=2))
    vc = 0.5 * (v + vm)
    pl = sig[:, None, None] * p[None] + ptop
    with np.errstate(invalid="ignore"):
        T = t * np.power(pl / P0, KAPPA)
    return pl, [uc, vc, t, T, q]


def fields(p, u, v, t, q, sig, ptop, P, v_north=None):
    """-> (out (5, N, H, W), valid (N, H, W)): gcm_plev_fields, NaN where a target is invalid"""
    pl, xs = levels(p, u, v, t, q, sig, ptop, v_north)
    got = [column_rule(pl, x, P) for x in xs]
    return np.stack([o for o, _ in got]), got[0][1]


def terms(p, u, v, t, q, sig, ptop, P, v_north=None):
    """-> the thirteen (N, H, W) terms of one state, 0.0 where the target is invalid in the column"""
    out, valid = fields(p, u, v, t, q, sig, ptop, P, v_north)
    uc, vc, th, T, qq = out
    raw = [np.ones(valid.shape), uc, vc, th, T, qq, uc * uc, vc * vc, T * T, uc * vc, vc * T, vc * th, vc * qq]
    return [np.where(valid, x, 0.0) for x in raw]


def sample(p, u, v, t, q, sig, ptop, P, v_north=None):
    """-> s (13, N, H): one sample's zonal sums in the device's order"""
    return np.stack([cref.row_sum(x) for x in terms(p, u, v, t, q, sig, ptop, P, v_north)])


def bound(p, u, v, t, q, sig, ptop, P, v_north=None):
    """-> (13, N, H): sum_i |term|, what the parity bound of a word's sum is relative to"""
    return np.stack([np.sum(np.abs(x), axis=-1) for x in terms(p, u, v, t, q, sig, ptop, P, v_north)])


def accumulate(states, sig, ptop, P):
    """-> (n, s): the sums over the samples `states` (each (p, u, v, t, q)) in sample order"""
    s = None
    for st in states:
        a = sample(st[0], st[1], st[2], st[3], st[4], sig, ptop, P)
        s = a if s is None else s + a
    return len(states), s


# ---------------------------------------------------------------- the inputs of the masking tests
def with_topography(st, dtype="f64", seed=21, smooth=False):
    """the state with p scaled per column to span roughly 600 - 1030 hPa (the seeded p is about 1e5 everywhere and masks
    nothing by itself); smooth: two zonal waves whose phase moves with the row instead of noise, for the tests that take
    steps from this state; f32: p rounded to float32 again, what the handle holds"""
    rng = np.random.default_rng(seed)
    H, W = st[0].shape
    if smooth:
        wave = np.sin(4 * np.pi * np.arange(W)[None, :] / W + 0.9 * np.arange(H)[:, None])
        p = st[0] * (0.815 + 0.215 * wave)
    else:
        p = st[0] * (0.6 + 0.43 * rng.random((H, W)))
    if dtype == "f32":
        p = p.astype(np.float32).astype(np.float64)
    return [p] + list(st[1:])


def targets_for(p, sig, ptop, N):
    """N >= 6 strictly decreasing targets taken from the restatement's own level pressures: one under every column's
    ground, the median bottom level (valid in some columns), one column's pl[0] and another's pl[L - 1] exactly, one
    between every column's bottom and top (valid everywhere), one above every top mid-level, and evenly spaced ones
    between the extremes up to N"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    pl = sig[:, None, None] * np.asarray(p, dtype=np.float64)[None] + ptop
    H, W = p.shape
    bottom, top = pl[0], pl[-1]
    assert top.max() < bottom.min(), "no target is valid in every column"
    special = [1.2 * bottom.max(), float(np.median(bottom)), float(bottom[H // 2, W // 3]), float(top[H // 3, W // 2]),
               0.5 * (top.max() + bottom.min()), 0.5 * top.min()]
    assert N >= len(special)
    extra = list(np.linspace(top.min(), bottom.max(), N - len(special) + 2)[1:-1])
    P = np.array(sorted(set(special + extra), reverse=True))
    assert P.size == N and np.all(np.diff(P) < 0)
    return P


def assert_masking_is_exercised(p, sig, ptop, P):
    """the conditions every masking test checks on the restatement before it touches the device"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    pl = sig[:, None, None] * np.asarray(p, dtype=np.float64)[None] + ptop
    _, valid = column_rule(pl, pl, P)
    W = p.shape[1]
    count = valid.sum(axis=-1)
    assert ((count > 0) & (count < W)).any(), "no (target, row) is partly masked"
    assert valid.all(axis=(1, 2)).any(), "no target is valid in every column"
    assert (~valid.any(axis=(1, 2)) & (P < pl[-1].min())).any(), "no target lies above every top mid-level"
    assert np.isin(P, pl).any(), "no target equals a level pressure exactly"
    return valid
