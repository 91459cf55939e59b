"""The shapes, launch geometries, inputs, float64 references and bounds of tests/test_sw2d_geometry_gpu.py -- TEST
INFRASTRUCTURE, a plain helper module.  tests/test_sw2d_geometry_cpu.py shows on the CPU that every reference here
moves by more than its bound from one compared step count to the next (the bounds are not vacuous), and that the
oracle evaluated in float32 NumPy arithmetic stays inside the fp32 bound on every shape."""
from collections import namedtuple

import numpy as np

from term_cases import TOL
from test_sw2d_f32_gpu import F32_STEP

DX, DT = 300e3, 300.0
FIELDS = "uvp"
STRIP, STRIP2 = 60, 56      # output columns per wave: the single-step kernel (per column of a lane), the two-step kernel

# (H, W): the smallest shapes that still reach each edge of the fused kernels' launch geometry.
SHAPES = [
    (1, 2),      # H = 1: every row neighbour is the row itself, the periodic preload reads one row RPB + 8 times; W = 2:
                 # the east and the west neighbour are the same cell.  (Stands in for (1, 1), where every neighbour is
                 # the cell itself: all differences vanish there, the state never moves and no bound can be non-vacuous.)
    (2, 3),      # H < the 4-row halo
    (3, 5),      # H < halo, and H equals RPB for 3
    (5, 56),     # one exact two-step strip, and H % RPB != 0 for 2, 3 and 4
    (7, 57),     # one column into the second two-step strip
    (9, 60),     # exact single-step strip seam
    (10, 61),    # one column past the single-step strip seam
    (13, 113),   # two strips plus one column of the two-step kernel; H is prime: the last band is short for every RPB
    (17, 120),   # the fp32 two-column strip seam (even width: two columns per lane are allowed)
    (17, 122),   # one pair of columns past the fp32 two-column strip seam
    (33, 97),    # the shape of the term_cases
]

# One handle is stepped by CALLS in turn and compared after each call, at TOTALS steps: a lone single step, then
# single steps and a lone pair on the swapped state.  AGAIN: the handle is given the initial state again and takes that
# many steps in ONE call -- 4: two pairs with a pointer swap between the launches, 5: two pairs and a leftover step.
CALLS, TOTALS, AGAIN = (1, 1, 2, 1), (1, 2, 4, 5), (4, 5)

# rows: GCM_FUSED_ROWS; two_step: GCM_SW2D_TWO_STEP ("1", "0", None = unset: bands of 5 rows and more never pair)
Geometry = namedtuple("Geometry", "family rows two_step")
GEOMETRIES = ([Geometry("fused2", r, "1") for r in (2, 3, 4)] + [Geometry("preload", r, "0") for r in (2, 3, 4)] +
              [Geometry("rolling", r, None) for r in (5, 8, 16, 64)])       # 64: longer than H, one wave takes all rows


def expected_plan(geom, cols, nsteps):
    """what Core.sw2d_plan(nsteps) must report for a geometry, from the case's own parameters"""
    pairs = nsteps // 2 if geom.family == "fused2" else 0
    return dict(variant="fused", rows_per_band=geom.rows, cols=cols, strip=STRIP * cols, strip2=STRIP2,
                two_step_launches=pairs, single_step_launches=nsteps - 2 * pairs, preload=geom.rows <= 4,
                stream=False)


def inputs(shape, dtype):
    """the project's recipe, seeded per shape; float32-rounded for fp32"""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    s = {"u": rng.standard_normal(shape), "v": rng.standard_normal(shape), "p": 8000 + rng.standard_normal(shape)}
    if dtype == "f32":
        s = {k: a.astype(np.float32).astype(np.float64) for k, a in s.items()}
    return s


_ORACLE = {}


def oracle(shape, dtype):
    """[state after n steps for n = 0 .. max(TOTALS)] of the float64 oracle, each a dict u, v, p; computed once per
    (shape, dtype) and shared by every geometry: do not modify"""
    key = (shape, dtype)
    if key not in _ORACLE:
        from oracle import sw2d
        s = inputs(shape, dtype)
        st, out = (s["u"], s["v"], s["p"]), [s]
        for _ in range(max(TOTALS)):
            st = sw2d.matsumo_scheme(*st, DX, DT)
            out.append(dict(zip(FIELDS, st)))
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_f32(shape):
    """the oracle's steps evaluated in float32 NumPy arithmetic on the fp32 inputs (oracle.sw2d carries the dtype
    through: every intermediate is rounded to float32), as oracle()"""
    from oracle import sw2d
    s = inputs(shape, "f32")
    st, out = tuple(s[k].astype(np.float32) for k in FIELDS), [s]
    for _ in range(max(TOTALS)):
        st = sw2d.matsumo_scheme(*st, DX, DT)
        assert all(a.dtype == np.float32 for a in st)
        out.append({k: a.astype(np.float64) for k, a in zip(FIELDS, st)})
    return out


# fp32: steps x test_sw2d_f32_gpu.F32_STEP[1] (u, v 4e-6, p 1e-7 per step), a bound measured on larger shapes.  On the
# shapes above the oracle evaluated in float32 NumPy arithmetic (oracle_f32) lies within 0.53 of it: its distance
# from the float64 oracle, as a share of the bound, worst over the shapes at 1 / 2 / 4 / 5 steps --
#   u 0.52 / 0.53 / 0.43 / 0.38,  v 0.42 / 0.50 / 0.41 / 0.38,  p 0.31 / 0.31 / 0.23 / 0.21
# (absolute, at 5 steps: u 7.6e-6, v 7.7e-6, p 1.0e-7 against 2e-5, 2e-5, 5e-7), so float32 rounding alone stays inside
# it on the tiny grids too (tests/test_sw2d_geometry_cpu.py asserts that), and no shape needed a bound of its own.
# Measured on an MI355X over every case of test_sw2d_geometry_gpu.py, as a share of the bound at 1 / 2 / 4 / 5 steps:
#   u 0.52 / 0.53 / 0.44 / 0.38,  v 0.42 / 0.50 / 0.41 / 0.38,  p 0.31 / 0.31 / 0.23 / 0.21
# (fp64: u 1.1e-14, v 1.2e-14, p 1.1e-16 against 1e-10).
def bound(dtype, field, nsteps):
    """the tolerance of one field after nsteps steps (rel_err: L-inf over max|reference|)"""
    return TOL if dtype == "f64" else nsteps * F32_STEP[1][field]
