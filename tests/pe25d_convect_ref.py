"""NumPy restatement of the convective adjustment of GCM_PE25D (include/gcmcore.h, gcm_set_convect): exactly the
arithmetic the header states, float64, every operation rounded on its own, in the header's order -- and the unstable
inputs the tests of the phase share.  NumPy only: no torch, no library.  TEST INFRASTRUCTURE, no test in here; shared by
tests/test_pe25d_convect_cpu.py, tests/test_pe25d_convect_gpu.py and tests/column_phase_cases.py.

    p_lev = sig[k] p + ptop;  Pi = (p_lev / P0)^kappa;  r = 1 (kappa_c = 0), else exp((kappa_c - kappa) log(p_lev / P0))
    y = theta / r (kappa_c = 0: theta);  w = (Pi r) dsig[k]
    per column, k = 0 (the bottom) .. L - 1: push (S = w y, Wt = w, Qs = q dsig[k], D = dsig[k], n = 1, value = y);
        while two blocks and top.value < below.value: S = below.S + top.S, likewise Wt, Qs, D, n; value = S / Wt
    blocks with n > 1: theta <- value r (kappa_c = 0: value); mix_q: q <- Qs / D.  n = 1: not written
"""
import numpy as np

import pe25d_inputs as inp

RD, CP, G, P0 = 287.0, 1004.0, 9.8, 100000.0                  # constants.py (the model's own)
KAPPA = RD / CP
DEFAULTS = dict(kappa_c=0.0, mix_q=1)
GAMMA = 6.5e-3                                                # K / m: Manabe-Strickler
SEED = 31
# (L, H, W) and ptop of the kernel tests: widths 70 and 130 leave a ragged last wave and span more than one wave a row,
# L = 5 and 8 are odd and even, L = 24 a deep stack with the LDS sized from L, L = 40 the largest L that must fit
CASES = (((8, 6, 70), 0.0), ((5, 4, 130), 1000.0), ((24, 3, 64), 0.0), ((40, 2, 64), 0.0))
SHAPES = tuple(s for s, _ in CASES)
PTOPS = (0.0, 1000.0)


def kappa_of(gamma):
    return RD * gamma / G


def params(**over):
    unknown = set(over) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update(over)
    return out


def levels(p, sig, ptop):
    """-> (p_lev, Pi), (L, H, W)"""
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    p_lev = sig[:, None, None] * np.asarray(p, dtype=np.float64)[None] + ptop
    return p_lev, (p_lev / P0) ** KAPPA


def neutral(p_lev, kappa_c):
    """r of the neutral profile, or None for the dry adjustment (r = 1, no operation)"""
    return None if kappa_c == 0.0 else np.exp((kappa_c - KAPPA) * np.log(p_lev / P0))


def compared(p, t, sig, dsig, ptop, kappa_c):
    """-> (y, w, r), (L, H, W); r None where dry"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    p_lev, pi = levels(p, sig, ptop)
    r = neutral(p_lev, kappa_c)
    t = np.asarray(t, dtype=np.float64)
    if r is None:
        return t, pi * dsig[:, None, None], None
    return t / r, (pi * r) * dsig[:, None, None], r


class PoolStats:
    """what the pooling of a set of columns went through: the smallest relative gap |a - b| / max(|a|, |b|) at any
    comparison made, the largest block, the pushes that were followed by more than one merge"""

    def __init__(self):
        self.min_gap, self.largest, self.deep_pushes = np.inf, 1, 0


def pool(y, w, q, dsig, mix_q=1, stats=None):
    """pool adjacent violators over columns y, w, q (ncol, L), level 0 the bottom, dsig (L,)
    -> (y_out, q_out, nblock (int32)); levels of unmerged blocks are copied.  Python floats are IEEE doubles: every
    operation below is one rounded float64 operation, in the header's operand order"""
    y, w, q = (np.asarray(a, dtype=np.float64) for a in (y, w, q))
    ncol, L = y.shape
    ds = [float(x) for x in np.asarray(dsig, dtype=np.float64).reshape(-1)]
    y_out, q_out, nblock = y.copy(), q.copy(), np.ones((ncol, L), dtype=np.int32)
    for c in range(ncol):
        yc, wc, qc = y[c].tolist(), w[c].tolist(), q[c].tolist()
        st = []                                               # blocks [S, Wt, Qs, D, n, value]
        for k in range(L):
            st.append([wc[k] * yc[k], wc[k], qc[k] * ds[k], ds[k], 1, yc[k]])
            merges = 0
            while len(st) >= 2:
                a, b = st[-1][5], st[-2][5]
                if stats is not None and a == a and b == b:
                    stats.min_gap = min(stats.min_gap, abs(a - b) / max(abs(a), abs(b)))
                if not a < b:
                    break
                top = st.pop()
                bel = st[-1]
                bel[0] = bel[0] + top[0]
                bel[1] = bel[1] + top[1]
                bel[2] = bel[2] + top[2]
                bel[3] = bel[3] + top[3]
                bel[4] = bel[4] + top[4]
                bel[5] = bel[0] / bel[1]
                merges += 1
            if stats is not None and merges > 1:
                stats.deep_pushes += 1
        k = 0
        for S, Wt, Qs, D, n, val in st:
            if n > 1:
                y_out[c, k:k + n] = val
                if mix_q:
                    q_out[c, k:k + n] = Qs / D
                nblock[c, k:k + n] = n
                if stats is not None:
                    stats.largest = max(stats.largest, n)
            k += n
    return y_out, q_out, nblock


def _cols(a):
    """(L, H, W) -> (H W, L)"""
    L = a.shape[0]
    return np.ascontiguousarray(a.reshape(L, -1).T)


def convect_step(p, t, q, sig, dsig, ptop, params, dtype="f64", stats=None):
    """one application -> (t, q, count, levels); p (H, W), t and q (L, H, W); count and levels (H, W): 1 where the
    column had a merged block, and the levels its merged blocks hold.  dtype "f32": the inputs are rounded to float32,
    the arithmetic is float64 and the written cells are rounded to float32 once (returned as float64, as the host API
    hands them out)"""
    if dtype == "f32":
        p, t, q = (np.asarray(x).astype(np.float32) for x in (p, t, q))
    p, t, q = (np.asarray(x, dtype=np.float64) for x in (p, t, q))
    L, H, W = t.shape
    kappa_c, mix_q = float(params["kappa_c"]), int(params["mix_q"])
    y, w, r = compared(p, t, sig, dsig, ptop, kappa_c)
    yo, qo, nb = pool(_cols(y), _cols(w), _cols(q), dsig, mix_q, stats)
    yo, qo, nb = (a.T.reshape(L, H, W) for a in (yo, qo, nb))
    merged = nb > 1
    tn = np.where(merged, yo if r is None else yo * r, t)
    qn = np.where(merged, qo, q) if mix_q else q.copy()
    if dtype == "f32":
        tn, qn = (a.astype(np.float32).astype(np.float64) for a in (tn, qn))
    count = merged.any(axis=0).astype(np.float64)
    lev = np.where(merged, 1.0, 0.0).sum(axis=0)
    return tn, qn, count, lev


def pairwise(y, w, sweeps):
    """the classic adjustment: `sweeps` sweeps from the bottom up, every unstable pair of neighbours set to its weighted
    mean; columns (ncol, L).  Its limit is what pool() computes at once; a yardstick at L <= 8 only (deep blocks take
    tens of thousands of sweeps)"""
    y = np.array(y, dtype=np.float64)
    for _ in range(sweeps):
        for k in range(y.shape[1] - 1):
            bad = y[:, k + 1] < y[:, k]
            m = (w[:, k] * y[:, k] + w[:, k + 1] * y[:, k + 1]) / (w[:, k] + w[:, k + 1])
            y[:, k] = np.where(bad, m, y[:, k])
            y[:, k + 1] = np.where(bad, m, y[:, k + 1])
    return y


def unstable_state(geom, kappa_c=0.0, dtype="f64", stable=False):
    """the seeded state (pe25d_inputs.state_of: its winds) with an unstable profile, built in the compared value:
    [p, u, v, t, q].  y = 300 + 40 k / L + 3 N(0, 1) (seed 31), theta = y r; every 7th column (row-major over (H, W)) is
    noise-free and therefore stable -- with `stable` all of them; p = 1e5 - ptop + 500 N(0, 1); q = 0.015
    exp(-4 k / L) (1 + 0.3 U(0, 1)), positive and decaying with height.  f32: rounded to float32 at the end (what the handle
    holds)"""
    _, u, v, _, _ = inp.state_of(geom)
    L, H, W = geom.layers, geom.height, geom.width
    rng = np.random.default_rng(SEED)
    noise = 3.0 * rng.standard_normal((L, H, W))
    p = 1e5 - geom.ptop + 500.0 * rng.standard_normal((H, W))
    wet = rng.random((L, H, W))
    quiet = (np.arange(H * W).reshape(H, W) % 7) == 0
    noise = np.where(quiet[None] | stable, 0.0, noise)
    k = np.arange(L, dtype=np.float64)[:, None, None]
    y = 300.0 + 40.0 * k / L + noise
    p_lev, _ = levels(p, geom.sig, geom.ptop)
    r = neutral(p_lev, kappa_c)
    t = y if r is None else y * r
    q = 0.015 * np.exp(-4.0 * k / L) * (1.0 + 0.3 * wet)
    st = [p, u, v, t, q]
    if dtype == "f32":
        st = [a.astype(np.float32).astype(np.float64) for a in st]
    return st


def column_enthalpy(p, t, sig, dsig, ptop):
    """sum_k theta Pi dsig, (H, W): the column's enthalpy up to Cp p / G"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    _, pi = levels(p, sig, ptop)
    return np.sum((t * pi) * dsig[:, None, None], axis=0)


def column_water(q, dsig):
    """sum_k q dsig, (H, W): the column's water up to p / G"""
    dsig = np.asarray(dsig, dtype=np.float64).reshape(-1)
    return np.sum(q * dsig[:, None, None], axis=0)
