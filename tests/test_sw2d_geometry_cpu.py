"""What tests/test_sw2d_geometry_gpu.py can see, stated on the CPU (tests/sw2d_geometry_cases.py): on every shape and
at both dtypes the float64 oracle moves every field by more than the bound from one compared step count to the
next, so that a kernel that takes a step too few or too many fails; and the fp32 bound, measured on larger shapes,
holds what float32 rounding alone costs on these tiny grids."""
import numpy as np
import pytest

from conftest import rel_err
import sw2d_geometry_cases as gc


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", gc.SHAPES, ids=["%dx%d" % s for s in gc.SHAPES])
def test_bound_is_not_vacuous(shape, dtype):
    """the oracle after n - 1 steps misses the oracle after n steps by more than 10x the bound at n, in every field"""
    want = gc.oracle(shape, dtype)
    assert len(want) == max(gc.TOTALS) + 1
    for n in sorted(set(gc.TOTALS) | set(gc.AGAIN)):
        for k in gc.FIELDS:
            moved = rel_err(want[n - 1][k], want[n][k])
            assert moved > 10 * gc.bound(dtype, k, n), (shape, dtype, n, k, moved)


def test_float32_rounding_alone_stays_inside_the_fp32_bound():
    """the oracle evaluated in float32 NumPy arithmetic against the float64 oracle, on every shape: the share of the
    bound it takes is printed (worst over the shapes) and stays below 0.6, the figures in the comment above
    sw2d_geometry_cases.bound"""
    worst = {}
    for shape in gc.SHAPES:
        want, got = gc.oracle(shape, "f32"), gc.oracle_f32(shape)
        for n in gc.TOTALS:
            for k in gc.FIELDS:
                share = rel_err(got[n][k], want[n][k]) / gc.bound("f32", k, n)
                worst[(k, n)] = max(worst.get((k, n), 0.0), share)
    print({"%s@%d" % kn: "%.2f" % x for kn, x in sorted(worst.items())})
    assert max(worst.values()) < 0.6, worst


def test_case_list_covers_every_geometry_on_every_shape():
    import test_sw2d_geometry_gpu as t
    ids = [t._id(c) for c in t.CASES]
    assert len(set(ids)) == len(ids)
    assert len(set(gc.SHAPES)) == len(gc.SHAPES) == 11
    assert sum(1 for s in gc.SHAPES if s[1] % 2 == 0) >= 4
    assert {(geo.family, geo.rows) for geo in gc.GEOMETRIES} == (
        {("fused2", r) for r in (2, 3, 4)} | {("preload", r) for r in (2, 3, 4)} |
        {("rolling", r) for r in (5, 8, 16, 64)})
    for dtype, cols in (("f64", 1), ("f32", 1), ("f32", 2)):
        for geo in gc.GEOMETRIES:
            shapes = {c[3] for c in t.CASES if c[:3] == (dtype, cols, geo)}
            assert shapes == {s for s in gc.SHAPES if cols == 1 or s[1] % 2 == 0}, (dtype, cols, geo)
    # the plan a case asserts follows from its id alone
    assert gc.expected_plan(gc.Geometry("fused2", 3, "1"), 1, 5)["two_step_launches"] == 2
    assert gc.expected_plan(gc.Geometry("preload", 3, "0"), 1, 5)["two_step_launches"] == 0
    assert gc.expected_plan(gc.Geometry("rolling", 8, None), 2, 4) == dict(
        variant="fused", rows_per_band=8, cols=2, strip=120, strip2=56, two_step_launches=0, single_step_launches=4,
        preload=False, stream=False)
