"""NumPy restatement of the convective mixing of the passive tracers of GCM_PE25D (include/gcmcore.h,
gcm_set_tracer_convect): the blocks are those of the convective adjustment's restatement (tests/pe25d_convect_ref.pool),
then exactly the two sums the header states, float64, every operation rounded on its own, sequential and ascending from
the block's lowest level.  NumPy only: no torch, no library.  TEST INFRASTRUCTURE, no test in here; shared by
tests/test_pe25d_convect_tracers_cpu.py and tests/test_pe25d_convect_tracers_gpu.py.

    per merged block (n > 1) over levels [k0, k0 + n):
        D  = dsig[k0];          D  = D  + dsig[k]          k = k0 + 1 .. k0 + n - 1
        Cs = c[k0] dsig[k0];    Cs = Cs + c[k] dsig[k]     likewise
        c[k] <- Cs / D;  levels of unmerged blocks are not written
"""
import numpy as np

import pe25d_convect_ref as cref

# (L, H, W) of the kernel tests: (9, 24, 36) takes dynamics steps; (9, 6, 100) is two waves a row, the second partial;
# (24, 4, 130) three waves with a tail of 2 columns at the product's level count; (40, 2, 64) the 112 KB stack
SHAPES = ((9, 24, 36), (9, 6, 100), (24, 4, 130), (40, 2, 64))
NTR = 3


def inputs(geom, kappa_c=0.0, dtype="f64", stable=False):
    """-> (state, tracers (NTR, L, H, W)) of the tests: the adjustment's own unstable state (3 K of noise on 6 of 7
    columns; `stable`: on none) and three tracers -- a profile that decays with height, an increasing one, and one that
    is negative somewhere.  f32: rounded to float32 (what the handle holds)"""
    L, H, W = geom.layers, geom.height, geom.width
    st = cref.unstable_state(geom, kappa_c, dtype, stable)
    rng = np.random.default_rng(77)
    k = np.arange(L, dtype=np.float64)[:, None, None]
    trs = np.stack([np.exp(-3.0 * k / L) * (1.0 + 0.5 * rng.random((L, H, W))),
                    1.0 + k / L + 0.1 * rng.random((L, H, W)),
                    rng.standard_normal((L, H, W))])
    if dtype == "f32":
        trs = trs.astype(np.float32).astype(np.float64)
    return st, trs


def mix_columns(nblock, dsig, c):
    """c (ncol, L) mixed in the blocks nblock (ncol, L: the size of each level's block, as pool() returns it) -> c_out.
    Python floats are IEEE doubles: every operation below is one rounded float64 operation"""
    c = np.asarray(c, dtype=np.float64)
    ncol, L = c.shape
    ds = [float(x) for x in np.asarray(dsig, dtype=np.float64).reshape(-1)]
    out = c.copy()
    for col in range(ncol):
        cc, nb = c[col].tolist(), nblock[col].tolist()
        k = 0
        while k < L:
            n = nb[k]
            if n > 1:
                D, Cs = ds[k], cc[k] * ds[k]
                for kk in range(k + 1, k + n):
                    D = D + ds[kk]
                    Cs = Cs + cc[kk] * ds[kk]
                out[col, k:k + n] = Cs / D
            k += n
    return out


def tracer_columns(y, w, dsig, c, stats=None):
    """the probe's restatement: columns y, w, c (ncol, L) -> (c_out, nblock); the blocks from pool() with zeros for q"""
    y = np.asarray(y, dtype=np.float64)
    _, _, nb = cref.pool(y, w, np.zeros_like(y), dsig, 0, stats)
    return mix_columns(nb, dsig, c), nb


def mix_step(p, t, tracers, on, sig, dsig, ptop, kappa_c, dtype="f64", stats=None):
    """one application on the device's inputs: p (H, W) and t (L, H, W) as they stand ahead of the adjustment, tracers
    (n, L, H, W), `on` the indices that have opted in -> (tracers, merged (L, H, W) bool).  dtype "f32": the inputs
    are rounded to float32, the arithmetic is float64 and the written cells are rounded to float32 once (returned as
    float64, as the host API hands them out)"""
    if dtype == "f32":
        p, t, tracers = (np.asarray(x).astype(np.float32) for x in (p, t, tracers))
    p, t, tracers = (np.asarray(x, dtype=np.float64) for x in (p, t, tracers))
    L, H, W = t.shape
    y, w, _ = cref.compared(p, t, sig, dsig, ptop, float(kappa_c))
    yc = cref._cols(y)
    _, _, nb = cref.pool(yc, cref._cols(w), np.zeros_like(yc), dsig, 0, stats)
    merged = (nb > 1).T.reshape(L, H, W)
    out = tracers.copy()
    for f in on:
        mixed = mix_columns(nb, dsig, cref._cols(tracers[f])).T.reshape(L, H, W)
        if dtype == "f32":
            mixed = mixed.astype(np.float32).astype(np.float64)
        out[f] = np.where(merged, mixed, tracers[f])
    return out, merged
