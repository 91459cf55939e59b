"""Limited tracer transport across the float range -- TEST INFRASTRUCTURE, a plain helper module (NumPy only).

The older parity tests feed the van Leer limited tracer paths `rng.random` fields and compare with rel_err, the largest
error over the largest reference value.  Such a field never gives the limiter a denominator outside about 1e-3 .. 1,
and rel_err cannot see a cell whose value is small next to the field's maximum.  A compact tracer blob has exactly such
cells: its flanks pass through the denormals before they reach zero.  This module holds the inputs, the references and
the error rule that tests/test_tracer_range_gpu.py applies to the device and tests/test_tracer_range_cpu.py shows to
bite.

Inputs.  The real type T is the handle's ("f64" / "f32") and every input is rounded to T first.  Winds, p, t and the
PE25D state are the ordinary seeded inputs (test_sw2d_f32_gpu._states, pe25d_inputs.state); only the tracer changes:

  ordinary   rng.random with a plateau of equal cells along every axis (the limiter's b == 0): the control
  plume      A exp(-r^2 / 2), sigma = 1 cell, centred in the grid, r not periodic
  down       ordinary x 2^-900 (f64) / 2^-100 (f32)
  denormal   ordinary x 2^-1040 (f64) / 2^-135 (f32): every cell is a denormal
  up         ordinary x 2^900 (f64) / 2^100 (f32)

References.  Never the code under test.  ordinary and plume: the float64 oracle on the T-rounded input
(oracle.tracer.limited_advection on the time-n winds for the 2-D models, pe25d_tracer_schemes_ref on the oracle's mass
fluxes for PE25D).  The three scaled inputs: np.ldexp(reference(ordinary), e) -- both schemes are homogeneous of degree
one in the tracer and a power of two scales exactly.

The error rule is per cell and local.  With S the largest |q_in| over the cells that can reach a cell in the steps
taken (per step the periodic 5 x 5 box; for PE25D that box over the levels k - 2 .. k + 2), `tiny` T's smallest normal
number and B the bound the project already holds the path to (f64: 1e-10; 2-D f32: F32_STEP[2]["q"] per step; PE25D
f32: F32_LIM_TOL), a cell passes when

    |got - want| <= B S + tiny,

where S is 0 the result must be exactly 0 (of either sign), and every cell must be finite.  The floor `tiny` is
deliberate: below the smallest normal number a difference of neighbouring cells keeps only a few bits, and the
limiter's weight formed from such differences may be anything in its range [0, 2] (PE25D's half weight: [0, 1]) --
which is what the clamp of tracer_face (pe25d_tracer_lim.h) gives where the reciprocal of a sum of denormals overflows,
and what face_flux (gcm_math.h) gives, which takes a face with a denormal difference as donor-cell (weight 0).  A weight
anywhere in that range moves a cell by less than the differences it multiplies, i.e. by less than `tiny`.

The module also holds NumPy models of the device arithmetic in type T (face_flux of gcm_math.h, tracer_face of
pe25d_tracer_lim.h) with the limiter's weight passed in, so that the CPU test can show a true division and the two guarded
reciprocals passing, a reciprocal formed first failing by a non-finite value, and a small planted mistake failing."""
import functools
from collections import namedtuple

import numpy as np

import pe25d_inputs as inp
import pe25d_tracer_schemes_ref as ref
from term_cases import TOL
from test_pe25d_tracer_schemes_gpu import F32_LIM_TOL
from test_sw2d_f32_gpu import DT, DX, F32_STEP

REAL = {"f64": np.float64, "f32": np.float32}
INPUTS = ("ordinary", "plume", "down", "denormal", "up")
SCALED = {"f64": {"down": -900, "denormal": -1040, "up": 900}, "f32": {"down": -100, "denormal": -135, "up": 100}}
SHAPE_2D = (33, 97)                 # the term_cases shape: one strip seam
SHAPE_2D_COLS2 = (8, 122)           # fp32 with two columns per lane: an even width beyond one 120-column strip
SHAPE_PE = (24, 36, 9)              # H, W, L: the first case of test_pe25d_tracer_schemes_gpu.py
SEED_2D, SEED_PE, SEED_PE_TRACER = 61, 3, 62
PE_DT = 60.0
PLUME_A_2D = {"f64": 1.0, "f32": 1.0}
PLUME_A_PE = {"f64": 2.0 ** -900, "f32": 1.0}
UPWIND, VANLEER = 1, 2              # gcm_tracer / gcm_tracer_scheme, and pe25d_tracer_schemes_ref's


def tiny(dtype):
    return float(np.finfo(REAL[dtype]).tiny)


def rounded(a, dtype):
    """a rounded to the real type, held as float64"""
    return np.asarray(a, dtype=np.float64).astype(REAL[dtype]).astype(np.float64)


def bound(model, dtype, steps=1):
    """B of the rule: what the project already holds the path to over `steps` steps"""
    if dtype == "f64":
        return TOL
    return steps * F32_STEP[2]["q"] if model == "sw2d_temp" else F32_LIM_TOL


def _frozen(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def _blob(H, W):
    j = (np.arange(H) - H // 2).reshape(H, 1).astype(np.float64)
    i = (np.arange(W) - W // 2).reshape(1, W).astype(np.float64)
    return np.exp(-(j * j + i * i) / 2.0)


def _all_inputs(ordinary, plume, dtype):
    out = {"ordinary": rounded(ordinary, dtype), "plume": rounded(plume, dtype)}
    for name, e in SCALED[dtype].items():
        out[name] = rounded(np.ldexp(out["ordinary"], e), dtype)
    return _frozen({k: out[k] for k in INPUTS})


# ---- the inputs ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_2d(shape, dtype):
    """u, v, p, t of a GCM_SW2D_TEMP handle: the seeded recipe of test_sw2d_f32_gpu._states, rounded to the real type"""
    from test_sw2d_f32_gpu import _states
    H, W = shape
    s = _states(2, 0, H, W, SEED_2D + H + W)
    return _frozen({k: rounded(a, dtype) for k, a in s.items()})


@functools.lru_cache(maxsize=None)
def tracers_2d(shape, dtype):
    """name -> q, (H, W)"""
    H, W = shape
    q = np.random.default_rng(SEED_2D + 1000 + H + W).random(shape)
    q[:, W - 3:] = q[:, W - 3:W - 2]             # three equal cells along i in every row,
    q[H - 3:, 5] = q[H - 3, 5]                   # and along j in one column
    return _all_inputs(q, PLUME_A_2D[dtype] * _blob(H, W), dtype)


def pe_geometry():
    from oracle import geometry as ogeo
    H, W, L = SHAPE_PE
    return ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)


@functools.lru_cache(maxsize=None)
def state_pe(dtype):
    """(p, u, v, t, q) of the GCM_PE25D handle: pe25d_inputs.state, rounded to the real type"""
    return tuple(_frozen([rounded(a, dtype) for a in inp.state(pe_geometry(), SEED_PE)]))


@functools.lru_cache(maxsize=None)
def tracers_pe(dtype):
    """name -> c, (L, H, W)"""
    H, W, L = SHAPE_PE
    c = np.random.default_rng(SEED_PE_TRACER).random((L, H, W))
    c[:, :, W - 3:] = c[:, :, W - 3:W - 2]
    c[:, H - 3:, 5] = c[:, H - 3:H - 2, 5]
    c[L - 3:, 7, 7] = c[L - 3, 7, 7]
    lev = (1.0 + np.arange(L) / L).reshape(L, 1, 1)
    return _all_inputs(c, PLUME_A_PE[dtype] * _blob(H, W)[None] * lev, dtype)


def stack_pe(dtype):
    """the five PE25D tracers in the order of INPUTS, (5, L, H, W): one handle carries them all"""
    t = tracers_pe(dtype)
    return np.ascontiguousarray(np.stack([t[k] for k in INPUTS]))


def count_denormals(a, dtype):
    a = np.abs(a)
    return int(np.count_nonzero((a > 0) & (a < tiny(dtype))))


# ---- the references -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def winds_2d(shape, dtype, steps):
    """the oracle's (u, v) at the start of each of `steps` steps: the tracer rides on the time-n winds"""
    from oracle import sw2d_temp
    s = state_2d(shape, dtype)
    st, out = (s["u"], s["v"], s["p"], s["t"]), []
    for _ in range(steps):
        out.append((st[0], st[1]))
        st = sw2d_temp.matsumo_scheme(*st, DX, DT)
    return out


def oracle_2d(shape, dtype, tracer, q, steps):
    """`steps` steps of oracle.tracer.limited_advection from q, as test_sw2d_f32_gpu._oracle steps it"""
    from oracle import tracer as otr
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for u, v in winds_2d(shape, dtype, steps):
            q = otr.limited_advection(DT, (DX, DX), np.stack([v, u]), q, limiter=tracer == VANLEER)
    return q


@functools.lru_cache(maxsize=None)
def reference_2d(shape, dtype, tracer, steps):
    """name -> the reference q after `steps` steps"""
    qs = tracers_2d(shape, dtype)
    out = {k: oracle_2d(shape, dtype, tracer, qs[k], steps) for k in ("ordinary", "plume")}
    for name, e in SCALED[dtype].items():
        out[name] = np.ldexp(out["ordinary"], e)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def fluxes_pe(dtype):
    """(the oracle's state after one Matsuno step, its two stages' (p, p_n, spu, spv, sd))"""
    return ref.flux_history(state_pe(dtype), PE_DT, pe_geometry(), 1)


def restatement_pe(dtype, scheme, c):
    """one Matsuno step of the tracers c (n, L, H, W) by the restatement on the oracle's fluxes"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return ref.advance(c, fluxes_pe(dtype)[1], PE_DT, pe_geometry(), scheme)[0]


@functools.lru_cache(maxsize=None)
def reference_pe(dtype, scheme):
    """name -> the reference tracer after one Matsuno step"""
    cs = tracers_pe(dtype)
    got = restatement_pe(dtype, scheme, np.stack([cs["ordinary"], cs["plume"]]))
    out = {"ordinary": got[0], "plume": got[1]}
    for name, e in SCALED[dtype].items():
        out[name] = np.ldexp(out["ordinary"], e)
    return _frozen(out)


# ---- the error rule -----------------------------------------------------------------------------------------------
def reach_max(q_in, radius, level_radius=0):
    """S: per cell the largest |q_in| over the periodic box of `radius` cells along the last two axes and, for a
    3-D field, over `level_radius` levels either way along the first (the column does not wrap)"""
    a = np.abs(np.asarray(q_in, dtype=np.float64))
    for axis in (-2, -1):
        a = np.maximum.reduce([np.roll(a, s, axis) for s in range(-radius, radius + 1)])
    if level_radius:
        L = a.shape[0]
        pad = np.concatenate([np.zeros((level_radius,) + a.shape[1:]), a, np.zeros((level_radius,) + a.shape[1:])])
        a = np.maximum.reduce([pad[s:s + L] for s in range(2 * level_radius + 1)])
    return a


Verdict = namedtuple("Verdict", "ok nonfinite nonzero over use")


def judge(got, want, q_in, B, dtype, steps=1, levels=False):
    """the rule on every cell -> Verdict: ok, the count of non-finite cells, of cells that must be exactly zero and
    are not, of cells over the allowed error, and the worst use of the allowed error (|got - want| / (B S + tiny))"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == np.shape(q_in), (got.shape, want.shape, np.shape(q_in))
    S = reach_max(q_in, 2 * steps, 2 * steps if levels else 0)
    finite = np.isfinite(got)
    with np.errstate(over="ignore", invalid="ignore"):
        use = np.where(finite, np.abs(got - want) / (B * S + tiny(dtype)), np.inf)
    nonfinite = int(np.count_nonzero(~finite))
    nonzero = int(np.count_nonzero((S == 0) & finite & (got != 0)))
    over = int(np.count_nonzero(finite & (use > 1.0)))
    worst = float(np.max(np.where(finite, use, 0.0)))
    return Verdict(nonfinite == 0 and nonzero == 0 and over == 0, nonfinite, nonzero, over, worst)


# ---- NumPy models of the device arithmetic in type T ----------------------------------------------------------------
# the limiter's weight from |num| and |b|: face_flux's is 2 |num| / (|b| + |num|), tracer_face's half of it
def true_division(an, ab, two):
    return (an + an) / (ab + an) if two else an / (ab + an)


def reciprocal_first(an, ab, two):
    r = an.dtype.type(1.0) / (ab + an)
    return (an + an) * r if two else an * r


def reciprocal_clamped(an, ab, two):
    return np.fmin(reciprocal_first(an, ab, two), an.dtype.type(2.0 if two else 1.0))


def reciprocal_of_normals(an, ab, two):
    """face_flux's guard: the limiter only where both differences are normal numbers, donor-cell elsewhere"""
    t = np.finfo(an.dtype).tiny
    return np.where((an >= t) & (ab >= t), reciprocal_first(an, ab, two), an.dtype.type(0.0))


def _weight(num, b, ok, weight, two):
    an, ab = np.abs(num), np.abs(b)
    rpos = ok & (np.signbit(num) == np.signbit(b)) & (an > 0) & (ab > 0)
    return np.where(rpos, weight(an, ab, two), an.dtype.type(0.0))


def model_axis_2d(q, vel, dtdx, axis, limit, weight, half=0.5):
    """face_flux (gcm_math.h) along one axis and the flux-form update, every operation in q's type"""
    T = q.dtype.type
    q1, qm1, q2 = np.roll(q, -1, axis), np.roll(q, 1, axis), np.roll(q, -2, axis)
    pos = vel > 0
    vd = vel * dtdx
    flux = np.where(pos, q, q1) * vd
    if limit:
        f_high = vd * ((q + q1) * T(half))
        phi = _weight(np.where(pos, q - qm1, q2 - q1), q1 - q, True, weight, True)
        flux = flux + phi * (f_high - flux)
    return q - flux + np.roll(flux, 1, axis)


def model_2d(shape, dtype, tracer, q, steps, weight, half=0.5):
    """`steps` steps of the 2-D tracer in type T on the oracle's winds rounded to T"""
    T = REAL[dtype]
    q = np.asarray(q, dtype=T)
    with np.errstate(all="ignore"):
        for u, v in winds_2d(shape, dtype, steps):
            q = model_axis_2d(q, v.astype(T), T(DT / DX), 0, tracer == VANLEER, weight, half)
            q = model_axis_2d(q, u.astype(T), T(DT / DX), 1, tracer == VANLEER, weight, half)
    return q.astype(np.float64)


def _model_face_pe(F, aa, a, b, bb, scheme, weight, ok_aa=True, ok_bb=True, trim=1.0):
    """tracer_face (pe25d_tracer_lim.h) in the arrays' type"""
    pos = F > 0
    up = np.where(pos, a, b)
    if scheme != VANLEER:
        return up
    down, far = np.where(pos, b, a), np.where(pos, aa, bb)
    ok = np.broadcast_to(np.where(pos, ok_aa, ok_bb), up.shape)
    d = down - up
    return up + (_weight(up - far, d, ok, weight, False) * up.dtype.type(trim)) * d


def model_stage_pe(c, sc, p, p_n, spu, spv, sd, dt, geom, scheme, T, weight, trim=1.0):
    """pe_tracer_lim_kernel's update of one stage, every operation in type T (pe25d_tracer_schemes_ref.tracer_stage
    with the face value of tracer_face)"""
    roll = np.roll
    c, sc, p, p_n, spu, spv, sd = (np.asarray(x, dtype=T) for x in (c, sc, p, p_n, spu, spv, sd))
    inv_dx, inv_dy = (1.0 / np.asarray(geom.dx_j)).astype(T), T(1.0 / geom.dy)
    inv_ds = (1.0 / np.asarray(geom.dsig)).astype(T)
    L = sc.shape[0]
    f_i = _model_face_pe(spu, roll(sc, 1, 2), sc, roll(sc, -1, 2), roll(sc, -2, 2), scheme, weight, trim=trim)
    f_j = _model_face_pe(spv, roll(sc, 1, 1), sc, roll(sc, -1, 1), roll(sc, -2, 1), scheme, weight, trim=trim)
    tpu, tpv = spu * f_i, spv * f_j
    adq = (tpu - roll(tpu, 1, 2)) * inv_dx + (tpv - roll(tpv, 1, 1)) * inv_dy
    k = np.arange(L).reshape(L, 1, 1)
    f_k = _model_face_pe(sd, roll(sc, 2, 0), roll(sc, 1, 0), sc, roll(sc, -1, 0), scheme, weight, k >= 2, k + 1 < L, trim)
    flux = f_k * sd
    dqs = -((flux - roll(flux, -1, 0)) * inv_ds)
    return (c * p - (adq + dqs) * T(dt)) * (T(1.0) / p_n)


def model_pe(dtype, scheme, c, weight, trim=1.0):
    """one Matsuno step of the tracers c (n, L, H, W) in type T on the oracle's fluxes rounded to T"""
    T, geom = REAL[dtype], pe_geometry()
    pred, corr = fluxes_pe(dtype)[1][0]
    with np.errstate(all="ignore"):
        star = [model_stage_pe(x, x, *pred, PE_DT, geom, scheme, T, weight, trim) for x in c]
        new = [model_stage_pe(x, s, *corr, PE_DT, geom, scheme, T, weight, trim) for x, s in zip(c, star)]
    return np.stack(new).astype(np.float64)


# ---- the 1-D line of flux_limiter -------------------------------------------------------------------------------------
def line(name):
    """(q, u): row 16 of the float64 2-D input `name` and of the wind along it, 97 cells"""
    return (np.ascontiguousarray(tracers_2d(SHAPE_2D, "f64")[name][16]),
            np.ascontiguousarray(state_2d(SHAPE_2D, "f64")["u"][16]))
