"""GCM_SW2D_TEMP (theta, viscosity, optional upwind or van Leer tracer) on every launch geometry of its fused row march
against the float64 oracle: sw2d_fused_kernel<T, true, TRACER, WRAPJ, 0, false, CPL> at 1, 2, 3, 4, 5, 7 and 64 rows per
band (the three classes of (rows + 2) % 3, i.e. each call site its three-way rotated loop can leave from, short last
bands, one wave for all rows), at fp64 and at fp32 with one and two columns per lane, with each tracer scheme, on the
smallest shapes that reach each strip seam and on grids shorter and narrower than the tracer's stencil
(tests/sw2d_temp_geometry_cases.py lists them with the reason for each); the staged variant once per shape, tracer
and dtype; and latitude bands (WRAPJ = false) against the oracle of the whole grid.

Every case first asserts through Core.sw2d_plan that the handle launches the variant, rows per band and strip width
its id names, then steps and compares with oracle.sw2d_temp.matsumo_scheme and oracle.tracer.limited_advection (fp32:
on the float32-rounded inputs).  GCM_FUSED_ROWS and GCM_SW2D_F32_COLS are read per handle and set before it is
created.  A failure names the worst cell's (j, i) and its place in the band and in the strip.  Out of scope: the
STREAM instantiation, ensembles, GCM_ALLOC_SKEW."""
import numpy as np
import pytest

import gpu_setups as su
import sw2d_temp_geometry_cases as gc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_sw2d_geometry_gpu import SWITCHES, _seam_mask, _where

pytestmark = pytest.mark.gpu
STAGED_BLOCK = dict(rows_per_band=4, strip=64, strip2=gc.STRIP2)    # the staged kernels' 64 x 4 thread blocks, for _where


def _switches(monkeypatch, dtype, cols, rows):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if rows is not None:
        monkeypatch.setenv("GCM_FUSED_ROWS", str(rows))
    if dtype == "f32" and cols:
        monkeypatch.setenv("GCM_SW2D_F32_COLS", str(cols))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _state(got, tracer):
    """Core.get_state() -> {u, v, p, t[, q]}"""
    return {k: a for k, a in zip("puvtq", got) if k in gc.fields(tracer)}


def _compare(label, nsteps, got, want, dtype, tracer, plan, seams=False):
    """every field of `got` within the bound of the oracle's `want`, no NaN; with `seams`, the seam cells on their
    own too.  -> the error of each field"""
    cells, errs = {}, {}
    for k in gc.fields(tracer):
        a, b = got[k], want[k]
        assert a.shape == b.shape, (label, k, a.shape)
        err = cells[k] = np.abs(a - b) / np.max(np.abs(b))
        assert not np.isnan(err).any(), "%s: %s after %d steps holds a NaN; %s" % (
            label, k, nsteps, _where(np.isnan(err), plan))
        errs[k] = float(err.max())
    lims = {k: gc.bound(dtype, k, nsteps) for k in errs}
    # every figure ahead of the assertions: the error and its share of the bound
    print("ERR %s n=%d %s" % (label, nsteps, " ".join("%s=%.3e/%.2f" % (k, e, e / lims[k]) for k, e in errs.items())))
    for k, err in cells.items():
        assert errs[k] < lims[k], "%s: %s after %d steps misses the oracle by %.3e (bound %.1e); %s" % (
            label, k, nsteps, errs[k], lims[k], _where(err, plan))
        if seams:
            on_seam = np.where(_seam_mask(err.shape, plan), err, 0.0)
            assert on_seam.max() < lims[k], "%s: %s after %d steps misses the oracle by %.3e on a seam (bound %.1e); " \
                "%s" % (label, k, nsteps, on_seam.max(), lims[k], _where(on_seam, plan))
    return errs


def _drive(g, monkeypatch, case, seams=False):
    H, W = case.shape
    label = gc.case_id(case)
    _switches(monkeypatch, case.dtype, case.cols, case.rows)
    s = {k: a for k, a in gc.inputs(case.shape, case.dtype).items() if k in gc.fields(case.tracer)}
    want = gc.oracle(case.shape, case.tracer, case.dtype)
    variant = g._lib.VARIANT_STAGED if case.rows is None else g._lib.VARIANT_FUSED
    c = g.Core(g._lib.SW2D_TEMP, W, H, dx=gc.DX, tracer=case.tracer, variant=variant, dtype=case.dtype)
    try:
        c.set_state(**s)
        done = 0

        def step(n, total):
            plan = c.sw2d_plan(n)
            assert plan == gc.expected_plan(case, n), (label, n, plan)
            c.step(n, gc.DT)
            _compare(label, total, _state(c.get_state(), case.tracer), want[total], case.dtype, case.tracer,
                     STAGED_BLOCK if case.rows is None else plan, seams)

        for n in gc.CALLS:
            done += n
            step(n, done)
        assert done == gc.TOTALS[-1]
        for n in gc.AGAIN:                              # n steps in one call, from the initial state
            c.set_state(**s)
            step(n, n)
    finally:
        c.close()


def test_the_tracer_constants_are_the_case_lists(g):
    assert (g._lib.TRACER_NONE, g._lib.TRACER_UPWIND, g._lib.TRACER_VANLEER) == gc.TRACERS


@pytest.mark.parametrize("case", gc.CASES, ids=[gc.case_id(c) for c in gc.CASES])
def test_geometry_vs_oracle(g, monkeypatch, case):
    """the plan the id names, then 1, 2, 4 and 5 steps against the oracle: by calls of 1, 1, 2 and 1 steps on one
    handle, and 5 steps in one call from the initial state"""
    _drive(g, monkeypatch, case)


SEAM_CASES = [gc.Case(dtype, 1, 2, rows, shape) for dtype in ("f64", "f32") for rows, shape in ((4, (13, 113)), (7, (5, 61)))]


@pytest.mark.parametrize("case", SEAM_CASES, ids=[gc.case_id(c) for c in SEAM_CASES])
def test_seams_within_the_interior_bound(g, monkeypatch, case):
    """van Leer: the cells on a strip seam (columns 59 | 60, W-1 | 0) and on a band seam (the multiples of
    rows_per_band, H-1 | 0) are within the bound that holds for the interior: implied by the L-inf comparison, stated
    apart so that a failure names the seam"""
    mask = _seam_mask(case.shape, gc.expected_plan(case, 1))
    for i in (59, 60, case.shape[1] - 1, 0):
        assert mask[:, i].all(), i
    for j in list(range(0, case.shape[0], case.rows)) + [case.shape[0] - 1]:
        assert mask[j].all(), j
    assert not mask.all()
    _drive(g, monkeypatch, case, seams=True)


@pytest.mark.parametrize("band", gc.BAND_CASES, ids=[gc.band_id(b) for b in gc.BAND_CASES])
def test_bands_vs_oracle(g, monkeypatch, band):
    """nb non-periodic handles (WRAPJ = false) of one grid, the ghost rows moved by device copies every `halo` steps,
    four steps: the gathered state is within the bounds of the ORACLE of the whole grid, which a fault shared with the
    periodic handle cannot pass, and equals a periodic handle of the same dtype and columns per lane bit for bit: a
    cell's arithmetic does not depend on where the bands of a launch start.

    That last part found a fault.  With the fp32 2-D kernels built under -ffp-contract=fast, 66 of the 128 fp32
    cases here (38 with one column per lane, 28 with two; rows 3, 5 and 64, never rows 1; all 16 fp64 cases passed)
    were inside the oracle's bound but differed from the periodic handle in 1 to 11 cells of a field, by one rounding
    (up to 8.3e-6 of max|u|).  The cases that passed were those in which every row falls, in the band handle as in the
    periodic one, into the same of the three inlined copies of FusedCtx::iter that the rotated loop holds, which
    (row - first row of its band + 1) % 3 names; two periodic fp32 handles that differed in GCM_FUSED_ROWS alone
    differed in the same way.  Under "fast" the compiler fuses multiplies and adds across statements in each inlined
    copy on its own, and the copies came out with different fused sets.  The fp32 unit is now built with
    -ffp-contract=on (csrc/Makefile): contraction within an expression only, the same in every copy.
    test_bands_host_loop_equal_single_domain and test_bands_in_process_2d could not see it: their bands start at even
    rows under 2-row bands in both handles."""
    import torch
    from gcmiipy_amd.bands import split_rows
    H, W = band.shape
    label = gc.band_id(band)
    _switches(monkeypatch, band.dtype, band.cols, band.rows)
    s = {k: a for k, a in gc.inputs(band.shape, band.dtype).items() if k in gc.fields(band.tracer)}
    want = gc.oracle(band.shape, band.tracer, band.dtype)[gc.BAND_STEPS]
    kw = dict(dx=gc.DX, tracer=band.tracer, variant=g._lib.VARIANT_FUSED, dtype=band.dtype)
    cores = []
    try:
        one = g.Core(g._lib.SW2D_TEMP, W, H, **kw)
        cores.append(one)
        plan = one.sw2d_plan(gc.BAND_STEPS)
        assert plan == gc.expected_plan(gc.Case(band.dtype, band.cols, band.tracer, band.rows, band.shape), gc.BAND_STEPS)
        one.set_state(**s)
        one.step(gc.BAND_STEPS, gc.DT)
        single = _state(one.get_state(), band.tracer)
        parts = split_rows(H, band.nb)
        for r, (row0, n) in enumerate(parts):
            c = g.Core(g._lib.SW2D_TEMP, W, n, nranks=band.nb, rank=r, global_height=H, row0=row0,
                       halo_steps=band.halo, **kw)
            cores.append(c)
            assert c.sw2d_plan(band.halo) == gc.expected_plan(
                gc.Case(band.dtype, band.cols, band.tracer, band.rows, (n, W)), band.halo), (label, r)
            c.set_state(**{k: a[row0:row0 + n] for k, a in s.items()})
        for _ in range(gc.BAND_STEPS // band.halo):
            su.exchange(cores[1:], torch)
            for c in cores[1:]:
                if band.halo == 1:
                    c.step_interior(gc.DT)
                    c.step_boundary(gc.DT)
                else:
                    c.step(band.halo, gc.DT)
        got = _state([np.concatenate(x, axis=0) if x[0] is not None else None
                      for x in zip(*[c.get_state() for c in cores[1:]])], band.tracer)
    finally:
        for c in cores:
            c.close()
    _compare(label, gc.BAND_STEPS, got, want, band.dtype, band.tracer, plan)
    starts = [row0 for row0, _ in parts]
    diffs = {k: got[k] != single[k] for k in gc.fields(band.tracer)}
    print("BITS %s %s" % (label, " ".join("%s=%d/%.1e" % (
        k, d.sum(), _rel(got[k], single[k])) for k, d in diffs.items())))
    for k, d in diffs.items():
        assert not d.any(), "%s: %s differs from the periodic handle in %d of %d cells, by up to %.1e of max|value|; " \
            "rows %s; bands start at rows %s" % (label, k, d.sum(), d.size, _rel(got[k], single[k]), sorted(set(np.argwhere(d)[:, 0].tolist())), starts)
