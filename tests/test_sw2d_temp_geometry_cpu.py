"""What tests/test_sw2d_temp_geometry_gpu.py can see, stated on the CPU (tests/sw2d_temp_geometry_cases.py): on every
shape, with every tracer and at both dtypes the float64 oracle moves every field by more than 5x the bound from one
compared step count to the next, so that a kernel that takes a step too few, or leaves a cell unwritten, fails; the
fp32 bound, measured on larger shapes, holds what float32 rounding alone costs on these tiny grids; and the case
lists reach every rows-per-band class, short last bands and the band heights the issue names."""
import numpy as np
import pytest

from conftest import rel_err
import sw2d_temp_geometry_cases as gc

IDS = ["%dx%d" % s for s in gc.SHAPES]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tracer", gc.TRACERS, ids=gc.TRACER_NAMES)
@pytest.mark.parametrize("shape", gc.SHAPES, ids=IDS)
def test_bound_is_not_vacuous(shape, tracer, dtype):
    """the oracle after n - 1 steps misses the oracle after n steps by more than 5x the bound at n, in every field.
    (The plain suite's 10x does not hold for t: the fp32 bound grows with n, what a step moves does not.)"""
    want = gc.oracle(shape, tracer, dtype)
    assert len(want) == max(gc.TOTALS) + 1
    for n in sorted(set(gc.TOTALS) | set(gc.AGAIN)):
        assert set(want[n]) == set(gc.fields(tracer))
        for k in gc.fields(tracer):
            moved = rel_err(want[n - 1][k], want[n][k])
            assert moved > 5 * gc.bound(dtype, k, n), (shape, tracer, dtype, n, k, moved / gc.bound(dtype, k, n))


def test_the_planted_values_are_there():
    """exact-zero limiter denominators along both axes and a wind of exactly 0, on every shape with the room"""
    planted = [s for s in gc.SHAPES if s[0] >= 4 and s[1] >= 5]
    assert len(planted) == 6
    for shape in planted:
        for dtype in ("f64", "f32"):
            s = gc.inputs(shape, dtype)
            assert s["q"][2, 3] == s["q"][2, 4] == s["q"][3, 3] and s["u"][1, 1] == 0.0


def test_float32_rounding_alone_stays_inside_the_fp32_bound():
    """the oracle evaluated in float32 NumPy arithmetic (every array float32 after every step: asserted in
    sw2d_temp_geometry_cases._march) against the float64 oracle, on every shape and tracer: the share of the bound it
    takes is printed per field and step count (worst over the shapes) and stays below 0.8 -- the figures in the
    comment above sw2d_temp_geometry_cases.bound"""
    worst, at = {}, {}
    for shape in gc.SHAPES:
        for tracer in gc.TRACERS:
            want, got = gc.oracle(shape, tracer, "f32"), gc.oracle_f32(shape, tracer)
            for n in gc.TOTALS:
                for k in gc.fields(tracer):
                    share = rel_err(got[n][k], want[n][k]) / gc.bound("f32", k, n)
                    if share > worst.get((k, n), 0.0):
                        worst[(k, n)], at[(k, n)] = share, (shape, gc.TRACER_NAMES[tracer])
    for k in "uvptq":
        print(k, " / ".join("%.2f" % worst[(k, n)] for n in gc.TOTALS), "at", [at[(k, n)] for n in gc.TOTALS])
    assert max(worst.values()) < 0.8, worst


def test_limited_axis_f32_is_the_oracles_function():
    """the float32 transcription of oracle.tracer.limited_axis gives the oracle's own numbers on float64 input, bit for
    bit, and keeps float32 where the original widens"""
    from oracle import tracer as otr
    rng = np.random.default_rng(5)
    V, q = rng.standard_normal((2, 6, 7)), rng.random((6, 7))
    q[2, 3] = q[2, 4] = q[3, 3]
    V[1, 1, 1] = 0.0
    for axis in (0, 1):
        for limiter in (False, True):
            assert np.array_equal(gc.limited_axis_f32(gc.DT, (gc.DX, gc.DX), V, q, axis, limiter),
                                  otr.limited_axis(gc.DT, (gc.DX, gc.DX), V, q, axis, limiter))
            got = gc.limited_axis_f32(gc.DT, (gc.DX, gc.DX), V.astype(np.float32), q.astype(np.float32), axis, limiter)
            assert got.dtype == np.float32
            assert otr.limited_axis(gc.DT, (gc.DX, gc.DX), V.astype(np.float32), q.astype(np.float32), axis,
                                    limiter).dtype == np.float64


def test_case_list_covers_every_geometry_on_every_shape():
    ids = [gc.case_id(c) for c in gc.CASES]
    assert len(set(ids)) == len(ids)
    assert len(set(gc.SHAPES)) == len(gc.SHAPES) == 9
    assert sum(1 for s in gc.SHAPES if s[1] % 2 == 0) >= 3
    fused = [c for c in gc.CASES if c.rows is not None]
    assert {c.rows for c in fused} == set(gc.ROWS) == {1, 2, 3, 4, 5, 7, 64}
    assert {(r + 2) % 3 for r in gc.ROWS} == {0, 1, 2}
    for rows in (3, 4, 5, 7):                                # a short last band
        assert any(s[0] % rows for s in gc.SHAPES if s[0] > rows), rows
    assert all(s[0] < 64 for s in gc.SHAPES)                 # 64: one wave takes all rows
    for dtype, cols in gc.DTYPES:
        for tracer in gc.TRACERS:
            for rows in gc.ROWS:
                shapes = {c.shape for c in fused if c[:4] == (dtype, cols, tracer, rows)}
                assert shapes == {s for s in gc.SHAPES if gc.width_allows(cols, s)}, (dtype, cols, tracer, rows)
    staged = [c for c in gc.CASES if c.rows is None]
    assert sorted((c.dtype, c.tracer, c.shape) for c in staged) == sorted(
        (d, t, s) for d in ("f64", "f32") for t in gc.TRACERS for s in gc.SHAPES)
    # the plan a case asserts follows from its parameters alone
    assert gc.expected_plan(gc.Case("f32", 2, 2, 7, (8, 122)), 5) == dict(
        variant="fused", rows_per_band=7, cols=2, strip=120, strip2=56, two_step_launches=0, single_step_launches=5,
        preload=False, stream=False)
    assert gc.expected_plan(gc.Case("f64", 0, 1, None, (8, 122)), 2) == dict(
        variant="staged", rows_per_band=0, cols=0, strip=0, strip2=0, two_step_launches=0, single_step_launches=2,
        preload=False, stream=False)


def test_band_cases_reach_the_heights_and_seams_they_name():
    from gcmiipy_amd.bands import split_rows
    ids = [gc.band_id(b) for b in gc.BAND_CASES]
    assert len(set(ids)) == len(ids)
    heights = {n for b in gc.BAND_CASES for _, n in split_rows(b.shape[0], b.nb)}
    assert {4, 5} <= heights, heights
    for b in gc.BAND_CASES:
        parts = split_rows(b.shape[0], b.nb)
        assert sum(n for _, n in parts) == b.shape[0]
        assert all(n >= 2 * b.halo for _, n in parts), b     # what gcm_create accepts
        assert b.dtype == "f64" or b.shape[1] % 2 == 0, b    # fp32 bands need an even width
        assert gc.BAND_STEPS % b.halo == 0
    f64 = {(b.shape, b.nb, b.halo) for b in gc.BAND_CASES if b.dtype == "f64"}
    assert f64 == {((9, 61), 2, 1), ((9, 61), 2, 2)} and [n for _, n in split_rows(9, 2)] == [5, 4]
    for cols in (1, 2):
        got = {(b.shape, b.nb, b.halo) for b in gc.BAND_CASES if (b.dtype, b.cols) == ("f32", cols)}
        # (9, 62) by 3 is three 3-row bands, refused at halo = 2: (12, 62) stands in
        assert got == {((9, 62), 2, 1), ((9, 62), 2, 2), ((9, 62), 3, 1), ((12, 62), 3, 2),
                       ((12, 122), 2, 1), ((12, 122), 2, 2), ((12, 122), 3, 1), ((12, 122), 3, 2)}
    for key in {(b.dtype, b.cols, b.shape, b.nb, b.halo) for b in gc.BAND_CASES}:
        combos = {(b.tracer, b.rows) for b in gc.BAND_CASES if (b.dtype, b.cols, b.shape, b.nb, b.halo) == key}
        assert combos == {(t, r) for t in (0, 2) for r in (1, 3, 5, 64)}, key
