"""NumPy restatement of the passive tracers' transport schemes of GCM_PE25D (gcm_set_tracer_scheme).

TEST INFRASTRUCTURE.  The mass fluxes spu, spv, sd and the new surface pressure p_n of a stage come from the oracle's
half_timestep (its `_tap`); this module only applies the tracer update on them,

    c_n = (c p - (adq + dqs) dt) / p_n,

with the value of the stage tracer sc that each face carries chosen by the scheme: the mean of the two adjacent cells
(NONE: term for term the oracle's advec_t / advec_sig, so the result equals the oracle's q update bit for bit), the
upwind cell (UPWIND), or the upwind cell plus the van Leer limited correction (VANLEER).  Arrays are [k, j, i]."""
import numpy as np

from oracle import dynamics as od

NONE, UPWIND, VANLEER = 0, 1, 2


def face_value(F, aa, a, b, bb, scheme, ok_aa=True, ok_bb=True):
    """the tracer value a mass flux F carries through the face between cells a and b (F > 0: from a to b); aa / bb:
    the cells behind a / beyond b, ok_aa / ok_bb: where they exist"""
    if scheme == NONE:
        return (a + b) / 2
    pos = F > 0                                        # strict, as donor_cell_flux
    up = np.where(pos, a, b)
    if scheme == UPWIND:
        return up
    down, far = np.where(pos, b, a), np.where(pos, aa, bb)
    ok = np.broadcast_to(np.where(pos, ok_aa, ok_bb), up.shape)
    num, den = up - far, down - up
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.divide(num, den, out=np.zeros_like(num), where=(den != 0))     # calc_r's rule
        phi = (r + np.abs(r)) / (1 + np.abs(r))                                # van_leer
    phi = np.where(ok, phi, 0.0)
    return up + 0.5 * phi * den


def tracer_stage(c, sc, p, p_n, spu, spv, sd, dt, geom, scheme):
    """one stage: base tracer c, stage tracer sc -> c_n"""
    roll = np.roll
    L = sc.shape[0]
    # east face of cell i: between i (A) and i + 1 (B), mass flux spu[i]; south face of row j: j (A), j + 1 (B), spv[j]
    f_i = face_value(spu, roll(sc, 1, 2), sc, roll(sc, -1, 2), roll(sc, -2, 2), scheme)
    f_j = face_value(spv, roll(sc, 1, 1), sc, roll(sc, -1, 1), roll(sc, -2, 1), scheme)
    tpu, tpv = spu * f_i, spv * f_j
    adq = (tpu - roll(tpu, 1, 2)) / geom.dx_j + (tpv - roll(tpv, 1, 1)) / geom.dy
    # level face k: between levels k - 1 (A) and k (B), mass flux sd[k] (sd[0] = 0); the column does not wrap
    k = np.arange(L).reshape(L, 1, 1)
    f_k = face_value(sd, roll(sc, 2, 0), roll(sc, 1, 0), sc, roll(sc, -1, 0), scheme, k >= 2, k + 1 < L)
    flux = f_k * sd
    dqs = -((flux - roll(flux, -1, 0)) / geom.dsig)
    return (c * p - (adq + dqs) * dt) / p_n


def stage_fluxes(base, stage, dt, geom, coriolis=False):
    """the oracle's half_timestep of `base` on `stage` -> (the new state, spu, spv, sd)"""
    tap = {}
    new = od.half_timestep(*base, *stage, dt, geom, _tap=tap, coriolis=coriolis)
    return new, tap["spu"], tap["spv"], tap["sd"]


def flux_history(state, dt, geom, steps, coriolis=False):
    """`steps` Matsuno steps of (p, u, v, t, q) by the oracle -> (the final state, per step the two stages'
    (p, p_n, spu, spv, sd)): everything the tracers of any scheme need"""
    hist = []
    for _ in range(steps):
        star, spu, spv, sd = stage_fluxes(state, state, dt, geom, coriolis)
        pred = (state[0], star[0], spu, spv, sd)
        new, spu, spv, sd = stage_fluxes(state, star, dt, geom, coriolis)
        hist.append((pred, (state[0], new[0], spu, spv, sd)))
        state = new
    return state, hist


def advance(tracers, hist, dt, geom, scheme):
    """the tracers (n, L, H, W) through the steps of a flux_history under `scheme` -> (new tracers, the star tracers of
    the last step)"""
    star = tracers
    for pred, corr in hist:
        p, p_n, spu, spv, sd = pred
        star = np.stack([tracer_stage(c, c, p, p_n, spu, spv, sd, dt, geom, scheme) for c in tracers])
        p, p_n, spu, spv, sd = corr
        tracers = np.stack([tracer_stage(c, sc, p, p_n, spu, spv, sd, dt, geom, scheme)
                            for c, sc in zip(tracers, star)]).reshape(star.shape)
    return tracers, star


def matsuno_step(state, tracers, dt, geom, scheme, coriolis=False, taps=None):
    """one Matsuno step of (p, u, v, t, q) by the oracle, the tracers (n, L, H, W) beside it under `scheme`
    -> (new state, new tracers, star tracers).  `taps`, if a list, receives per stage (p, p_n, spu, spv, sd)."""
    new, hist = flux_history(state, dt, geom, 1, coriolis)
    if taps is not None:
        taps.extend(hist[0])
    if len(tracers) == 0:
        return new, tracers, tracers
    return (new, *advance(tracers, hist, dt, geom, scheme))


def run(state, tracers, dt, geom, steps, scheme, coriolis=False):
    for _ in range(steps):
        state, tracers, _ = matsuno_step(state, tracers, dt, geom, scheme, coriolis)
    return state, tracers


def outflow_bound(p, spu, spv, sd, dt, geom):
    """p - dt * (the mass fluxes that leave a cell, with their 1/dx, 1/dy, 1/dsig factors): where this is >= 0 in every
    cell, one UPWIND stage with stage = base is a convex combination of a cell and its inflow neighbours"""
    roll = np.roll
    pos, neg = lambda x: np.maximum(x, 0.0), lambda x: np.maximum(-x, 0.0)
    sd_up = roll(sd, -1, 0)                            # face k + 1 (the top level's: sd[0] = 0)
    out = ((pos(spu) + neg(roll(spu, 1, 2))) / geom.dx_j + (pos(spv) + neg(roll(spv, 1, 1))) / geom.dy
           + (neg(sd) + pos(sd_up)) / geom.dsig)
    return p - dt * out
