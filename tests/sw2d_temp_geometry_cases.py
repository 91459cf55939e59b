"""The shapes, launch geometries, inputs, float64 references and bounds of tests/test_sw2d_temp_geometry_gpu.py -- TEST
INFRASTRUCTURE, a plain helper module (NumPy only).  GCM_SW2D_TEMP (theta, viscosity and the optional upwind or van
Leer tracer) runs sw2d_fused_kernel<T, true, TRACER, WRAPJ, 0, STREAM, CPL>: the rolling row march alone, never the
preloading and never the two-step kernel.  tests/test_sw2d_temp_geometry_cpu.py shows on the CPU that every reference
here moves by more than 5x its bound from one compared step count to the next, and that the oracle evaluated in
float32 NumPy arithmetic stays inside 0.8 of the fp32 bound on every shape."""
from collections import namedtuple

import numpy as np

from term_cases import TOL
from test_sw2d_f32_gpu import F32_STEP

DX, DT = 300e3, 300.0
STRIP, STRIP2 = 60, 56      # output columns per wave and per column of a lane; the two-step kernel's (never run here)

# (H, W): the smallest shapes that still reach each edge of the row march with theta and a tracer
SHAPES = [
    (1, 2),      # H and W below the tracer's stencil (two cells each way) and below the 2-row / 2-column halo: the rows
                 # ja-2 .. jb+1 and the window qmm / qm / q0 / qp are one row, east and west neighbour are one cell
    (2, 3),      # H < the 2-row halo each way, W < 5: from_east(from_east(qs)) wraps past the own column
    (3, 5),      # H below the five rows of the tracer's j stencil; W its five columns exactly
    (4, 60),     # an exact strip
    (5, 61),     # one column past the strip seam; H is prime: the last band is short for every rows-per-band > 1
    (7, 120),    # the fp32 two-column strip exactly (even width: two columns per lane are allowed)
    (8, 122),    # one pair of columns past the fp32 two-column strip seam
    (13, 113),   # two strips less seven columns; H is prime again, and longer than every rows-per-band but 64
    (33, 97),    # the shape of the term_cases
]

# GCM_FUSED_ROWS, read when the handle is created.  1: the shortest band, three iter calls, leaving after the third
# call site; 2, 3, 4: the three classes of (rows + 2) % 3, i.e. which call site the loop leaves from; 5, 7: long
# loops with short last bands on most shapes; 64 > H: one wave takes all rows.
ROWS = (1, 2, 3, 4, 5, 7, 64)
TRACERS = (0, 1, 2)                                  # none, upwind, van Leer (GCM_TRACER_*)
TRACER_NAMES = ("none", "upwind", "vanleer")
DTYPES = (("f64", 1), ("f32", 1), ("f32", 2))        # (dtype, columns per lane); two columns: even widths only

# One handle is stepped by CALLS in turn and compared after each call, at TOTALS steps; AGAIN: the handle is given
# the initial state again and takes 5 steps in ONE call (five launches with a pointer swap between them).
CALLS, TOTALS, AGAIN = (1, 1, 2, 1), (1, 2, 4, 5), (5,)

# rows: GCM_FUSED_ROWS, None for the staged variant (which has no bands)
Case = namedtuple("Case", "dtype cols tracer rows shape")


def fields(tracer):
    return "uvptq" if tracer else "uvpt"


def width_allows(cols, shape):
    """two columns per lane run on even widths only (an odd width takes one whatever GCM_SW2D_F32_COLS says)"""
    return cols == 1 or shape[1] % 2 == 0


def _cases():
    fused = [Case(dtype, cols, tracer, rows, shape) for dtype, cols in DTYPES for tracer in TRACERS for rows in ROWS
             for shape in SHAPES if width_allows(cols, shape)]
    # staged: once per shape x tracer x dtype, no rows setting.  It is the code test_fused_equals_staged_full_size
    # trusts as its reference, and it has not run below 8x12 either.
    staged = [Case(dtype, 0, tracer, None, shape) for dtype in ("f64", "f32") for tracer in TRACERS for shape in SHAPES]
    return fused + staged


CASES = _cases()


def case_id(c):
    return "%s%s-%s-%s-%dx%d" % (c.dtype, "-cols%d" % c.cols if c.dtype == "f32" and c.rows is not None else "",
                                 TRACER_NAMES[c.tracer], "staged" if c.rows is None else "rows%d" % c.rows, *c.shape)


# Latitude bands (non-periodic handles, WRAPJ = false) of one grid in one process: nb bands of split_rows, the ghost
# rows exchanged every `halo` steps.  halo = 1: step_interior + step_boundary, a band of up to 4 rows takes the
# boundary-only branch of gcm_step_boundary; halo = 2: step(2), whose first launch produces rows [-2, H + 2), so that
# the bands of GCM_FUSED_ROWS start at a negative row.  fp64 on (9, 61): bands of 5 and 4 rows.  fp32 bands need an even
# width: (9, 62) and (12, 122) by 2 and by 3.  A band needs 2 * halo rows: 9 rows by 3 are three 3-row bands, which
# gcm_create refuses at halo = 2 ("a latitude band needs >= 2 * halo_steps rows"), so that combination runs on
# (12, 62), the smallest height by 3 it accepts (three 4-row bands).
Band = namedtuple("Band", "dtype cols tracer rows shape nb halo")
BAND_ROWS = (1, 3, 5, 64)
BAND_TRACERS = (0, 2)
BAND_STEPS = 4


def _band_cases():
    grids = [("f64", 1, (9, 61), 2, 1), ("f64", 1, (9, 61), 2, 2)]
    for cols in (1, 2):
        for shape, nb in (((9, 62), 2), ((9, 62), 3), ((12, 122), 2), ((12, 122), 3)):
            for halo in (1, 2):
                refused = shape[0] // nb < 2 * halo
                grids.append(("f32", cols, (12, 62) if refused else shape, nb, halo))
    return [Band(dtype, cols, tracer, rows, shape, nb, halo) for dtype, cols, shape, nb, halo in grids
            for tracer in BAND_TRACERS for rows in BAND_ROWS]


BAND_CASES = _band_cases()


def band_id(b):
    return "%s%s-%s-rows%d-%dx%d-nb%d-halo%d" % (b.dtype, "-cols%d" % b.cols if b.dtype == "f32" else "",
                                                  TRACER_NAMES[b.tracer], b.rows, *b.shape, b.nb, b.halo)


STAGED_PLAN = dict(variant="staged", rows_per_band=0, cols=0, strip=0, strip2=0, two_step_launches=0, preload=False,
                   stream=False)


def expected_plan(case, nsteps):
    """what Core.sw2d_plan(nsteps) must report, from the case's own parameters: GCM_SW2D_TEMP never pairs and never
    preloads; staged: the dict test_sw2d_geometry_gpu.test_plan_of_other_handles states"""
    if case.rows is None:
        return dict(STAGED_PLAN, single_step_launches=nsteps)
    return dict(variant="fused", rows_per_band=case.rows, cols=case.cols, strip=STRIP * case.cols, strip2=STRIP2,
                two_step_launches=0, single_step_launches=nsteps, preload=False, stream=False)


def inputs(shape, dtype):
    """the project's recipe, seeded per shape: {u, v, p, t, q} (q is drawn whether a tracer runs or not, so that a
    shape has one state); where the shape has the room, the exact-zero limiter denominators and the strict `> 0`
    branch of test_sw2d_temp_tracer_vs_oracle; float32-rounded for fp32"""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    s = {"u": rng.standard_normal(shape), "v": rng.standard_normal(shape), "p": 101325 + rng.standard_normal(shape),
         "t": 273.16 + rng.standard_normal(shape), "q": rng.random(shape)}
    if H >= 4 and W >= 5:
        s["q"][2, 3] = s["q"][2, 4] = s["q"][3, 3]
        s["u"][1, 1] = 0.0
    if dtype == "f32":
        s = {k: a.astype(np.float32).astype(np.float64) for k, a in s.items()}
    return s


def limited_axis_f32(dt, spatial_change, V, q, axis, limiter):
    """oracle.tracer.limited_axis transcribed so that float32 stays float32: the original's np.zeros(q.shape) is
    float64 and widens everything behind it.  Same expressions in the same order."""
    from oracle.tracer import van_leer
    dx = spatial_change[axis]
    q_p_1 = np.roll(q, -1, axis)
    zeroes = np.zeros(q.shape, dtype=q.dtype)
    a_plus = np.maximum(V[axis], zeroes)
    a_minus = np.minimum(V[axis], zeroes)
    f_low = (q * a_plus + q_p_1 * a_minus) * dt / dx
    if limiter:
        f_high = V[axis] * ((q + q_p_1) / 2) * dt / dx
        a = q - np.roll(q, 1, axis)
        b = q_p_1 - q
        c = np.roll(b, -1, axis)
        r_pos = np.divide(a, b, out=np.zeros_like(a), where=(b != 0))
        r_neg = np.divide(c, b, out=np.zeros_like(a), where=(b != 0))
        r = np.where(V[axis] > 0, r_pos, r_neg)
        flux = f_low + van_leer(r) * (f_high - f_low)
    else:
        flux = f_low
    return q - flux + np.roll(flux, 1, axis)


def _march(s, tracer, f32):
    """[state after n steps for n = 0 .. max(TOTALS)], each a dict of float64 arrays; the tracer on the time-n winds
    (test_sw2d_f32_gpu._oracle).  f32: every array float32 throughout, asserted after every step"""
    from oracle import sw2d_temp, tracer as otr
    kind = np.float32 if f32 else np.float64
    st, q = tuple(s[k].astype(kind) for k in "uvpt"), s["q"].astype(kind)
    out = [{k: s[k] for k in fields(tracer)}]
    for _ in range(max(TOTALS)):
        if tracer:
            V = np.stack([st[1], st[0]])
            if f32:
                for axis in range(2):
                    q = limited_axis_f32(DT, (DX, DX), V, q, axis, tracer == 2)
            else:
                q = otr.limited_advection(DT, (DX, DX), V, q, limiter=tracer == 2)
        st = sw2d_temp.matsumo_scheme(*st, DX, DT)
        assert all(a.dtype == kind for a in st) and q.dtype == kind
        out.append({k: a.astype(np.float64) for k, a in zip("uvptq", (*st, q)) if k in fields(tracer)})
    return out


_ORACLE = {}


def oracle(shape, tracer, dtype):
    """the float64 oracle (oracle.sw2d_temp.matsumo_scheme, oracle.tracer.limited_advection), on the float32-rounded
    inputs for fp32; computed once per (shape, tracer, dtype) and shared by every case: do not modify"""
    key = (shape, tracer, dtype)
    if key not in _ORACLE:
        _ORACLE[key] = _march(inputs(shape, dtype), tracer, False)
    return _ORACLE[key]


def oracle_f32(shape, tracer):
    """the oracle's steps evaluated in float32 NumPy arithmetic on the fp32 inputs, as oracle()"""
    return _march(inputs(shape, "f32"), tracer, True)


# fp64: term_cases.TOL (1e-10), the project's figure.  fp32: steps x test_sw2d_f32_gpu.F32_STEP[2] (u, v 2e-5, p 8e-7,
# t, q 6e-7 per step), measured on larger shapes.  It is held against the oracle evaluated in float32 NumPy arithmetic
# (oracle_f32), not against the kernel: that evaluation's distance from the float64 oracle, as a share of the bound,
# worst over the shapes and tracers at 1 / 2 / 4 / 5 steps --
#   u 0.56 / 0.45 / 0.38 / 0.38,  v 0.69 / 0.49 / 0.37 / 0.40,  p 0.14 / 0.14 / 0.28 / 0.29,
#   t 0.47 / 0.32 / 0.24 / 0.21,  q 0.18 / 0.17 / 0.19 / 0.24
# (the worst, v after one step, is on 5x61).  tests/test_sw2d_temp_geometry_cpu.py asserts that it stays below 0.8,
# which leaves float32 arithmetic in another order (the kernel's rcp, its float64 Exner table, the DPP order) a margin
# of 1.25x at the least.  No shape needed a bound of its own.
# Measured on an MI355X, worst over the cases of test_sw2d_temp_geometry_gpu.py (fused at every rows-per-band, staged,
# seams, bands), as a share of the bound at 1 / 2 / 4 / 5 steps:
#   u 0.46 / 0.41 / 0.29 / 0.25,  v 0.61 / 0.34 / 0.32 / 0.35,  p 0.10 / 0.12 / 0.19 / 0.21,
#   t 0.30 / 0.24 / 0.19 / 0.21,  q 0.18 / 0.16 / 0.17 / 0.20
# (absolute, the worst at any step count: u 2.5e-5, v 3.5e-5, p 8.6e-7, t 6.2e-7, q 6.1e-7): the kernel is nearer the
# float64 oracle than the float32 NumPy evaluation is.  fp64, worst over all cases and step counts:
# u 9.0e-14, v 1.1e-13, p 2.7e-15, t 1.4e-15, q 1.8e-15 against 1e-10.
def bound(dtype, field, nsteps):
    """the tolerance of one field after nsteps steps (rel_err: L-inf over max|reference|)"""
    return TOL if dtype == "f64" else nsteps * F32_STEP[2][field]
