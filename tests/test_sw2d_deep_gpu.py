"""The deep form of GCM_SW2D_TEMP's fused row march, sw2d_fused_kernel<double, true, TRACER, WRAPJ, 0, STREAM, 1, 3>:
three rows of requests in flight, two waves per SIMD.  The library picks it for float64 GCM_SW2D_TEMP handles whose
launch streams (more than 256 MB read); GCM_SW2D_DEPTH=3, read when the handle is created, pins it at any size, which
is how the shapes here reach it.

Periodic handles: every shape x rows per band x tracer of tests/sw2d_temp_geometry_cases.py -- the smallest at which
the march's two peeled rows, its clamped refill (rows 1 .. 4 of a band ask for rows beyond jb + 1), the whole trips and
the one or two rows behind them can go wrong -- against the float64 oracle at the project's 1e-10, after first
asserting that the handle reports depth 3 and the launch plan of the case.  Latitude bands (WRAPJ = false): the fp64
BAND_CASES against the oracle of the whole grid; a read past row jb + 1 would show as a NaN beside a ghost row or as a
fault.  Selection: which handles take the deep form by default.  Depth 1 and depth 3 are not compared bit for bit: the
fp64 unit is built with -ffp-contract=fast and the inlined copies of the row step may fuse differently."""
import numpy as np
import pytest

import gpu_setups as su
import sw2d_temp_geometry_cases as gc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_sw2d_geometry_gpu import SWITCHES
from test_sw2d_temp_geometry_gpu import _compare, _state

pytestmark = pytest.mark.gpu
DEPTH_SWITCH = "GCM_SW2D_DEPTH"
DEEP_WAVES_PER_CU = 2 * 4       # the deep kernel's launch bounds: two waves on each of a compute unit's four SIMDs

PERIODIC = [gc.Case("f64", 1, tracer, rows, shape) for tracer in gc.TRACERS for rows in gc.ROWS for shape in gc.SHAPES]
BANDS = [b for b in gc.BAND_CASES if b.dtype == "f64"]


def _switches(monkeypatch, rows=None, depth=None):
    for k in SWITCHES + (DEPTH_SWITCH,):
        monkeypatch.delenv(k, raising=False)
    if rows is not None:
        monkeypatch.setenv("GCM_FUSED_ROWS", str(rows))
    if depth is not None:
        monkeypatch.setenv(DEPTH_SWITCH, str(depth))


@pytest.mark.parametrize("case", PERIODIC, ids=[gc.case_id(c) for c in PERIODIC])
def test_deep_geometry_vs_oracle(g, monkeypatch, case):
    """depth 3 and the plan the id names, then 1, 2, 4 and 5 steps against the oracle: by calls of 1, 1, 2 and 1 steps
    on one handle, and 5 steps in one call from the initial state"""
    H, W = case.shape
    label = "deep-" + gc.case_id(case)
    _switches(monkeypatch, case.rows, 3)
    s = {k: a for k, a in gc.inputs(case.shape, case.dtype).items() if k in gc.fields(case.tracer)}
    want = gc.oracle(case.shape, case.tracer, case.dtype)
    c = g.Core(g._lib.SW2D_TEMP, W, H, dx=gc.DX, tracer=case.tracer, variant=g._lib.VARIANT_FUSED, dtype=case.dtype)
    try:
        assert c.sw2d_fused_depth() == 3, label
        c.set_state(**s)

        def step(n, total):
            plan = c.sw2d_plan(n)
            assert plan == gc.expected_plan(case, n), (label, n, plan)
            c.step(n, gc.DT)
            _compare(label, total, _state(c.get_state(), case.tracer), want[total], case.dtype, case.tracer, plan)

        done = 0
        for n in gc.CALLS:
            done += n
            step(n, done)
        assert done == gc.TOTALS[-1]
        for n in gc.AGAIN:
            c.set_state(**s)
            step(n, n)
    finally:
        c.close()


@pytest.mark.parametrize("band", BANDS, ids=[gc.band_id(b) for b in BANDS])
def test_deep_bands_vs_oracle(g, monkeypatch, band):
    """nb non-periodic handles of one grid at depth 3, the ghost rows moved by device copies every `halo` steps, four
    steps: the gathered state is within the bound of the oracle of the whole grid, and the rows beside the ghost rows
    of every band hold no NaN"""
    import torch
    from gcmiipy_amd.bands import split_rows
    H, W = band.shape
    label = "deep-" + gc.band_id(band)
    _switches(monkeypatch, band.rows, 3)
    s = {k: a for k, a in gc.inputs(band.shape, band.dtype).items() if k in gc.fields(band.tracer)}
    want = gc.oracle(band.shape, band.tracer, band.dtype)[gc.BAND_STEPS]
    kw = dict(dx=gc.DX, tracer=band.tracer, variant=g._lib.VARIANT_FUSED, dtype=band.dtype)
    parts = split_rows(H, band.nb)
    cores = []
    try:
        for r, (row0, n) in enumerate(parts):
            c = g.Core(g._lib.SW2D_TEMP, W, n, nranks=band.nb, rank=r, global_height=H, row0=row0,
                       halo_steps=band.halo, **kw)
            cores.append(c)
            assert c.sw2d_fused_depth() == 3, (label, r)
            assert c.sw2d_plan(band.halo) == gc.expected_plan(
                gc.Case(band.dtype, band.cols, band.tracer, band.rows, (n, W)), band.halo), (label, r)
            c.set_state(**{k: a[row0:row0 + n] for k, a in s.items()})
        for _ in range(gc.BAND_STEPS // band.halo):
            su.exchange(cores, torch)
            for c in cores:
                if band.halo == 1:
                    c.step_interior(gc.DT)
                    c.step_boundary(gc.DT)
                else:
                    c.step(band.halo, gc.DT)
        per_band = [_state(c.get_state(), band.tracer) for c in cores]
    finally:
        for c in cores:
            c.close()
    for r, st in enumerate(per_band):
        for k, a in st.items():
            edge = np.concatenate([a[:2], a[-2:]])
            assert not np.isnan(edge).any(), "%s: band %d, %s holds a NaN beside its ghost rows" % (label, r, k)
    got = {k: np.concatenate([st[k] for st in per_band], axis=0) for k in gc.fields(band.tracer)}
    plan = gc.expected_plan(gc.Case(band.dtype, band.cols, band.tracer, band.rows, band.shape), gc.BAND_STEPS)
    _compare(label, gc.BAND_STEPS, got, want, band.dtype, band.tracer, plan)


def _core(g, W, H, dtype="f64", tracer=2, model=None):
    return g.Core(g._lib.SW2D_TEMP if model is None else model, W, H, dx=gc.DX, tracer=tracer,
                  variant=g._lib.VARIANT_FUSED, dtype=dtype)


def test_the_streaming_grid_goes_deep_in_one_resident_round(g, monkeypatch):
    """4096x2048 GCM_SW2D_TEMP + van Leer at float64, created and not stepped: depth 3, the STREAM form, and bands
    long enough that all waves of the launch are resident at once at the deep kernel's two waves per SIMD"""
    import torch
    _switches(monkeypatch)
    W, H = 4096, 2048
    c = _core(g, W, H)
    try:
        assert c.sw2d_fused_depth() == 3
        plan = c.sw2d_plan(1)
    finally:
        c.close()
    assert plan["stream"] and not plan["preload"] and plan["cols"] == 1, plan
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    strips = -(-W // plan["strip"])
    bands = -(-H // plan["rows_per_band"])
    print("SELECT 4096x2048: rows_per_band %d, %d strips x %d bands = %d waves, %d slots" % (
        plan["rows_per_band"], strips, bands, strips * bands, DEEP_WAVES_PER_CU * cus))
    assert strips * bands <= DEEP_WAVES_PER_CU * cus, (plan, cus)
    # ... and the round is filled: one band fewer per strip would have fitted as well
    assert strips * (bands + 1) > DEEP_WAVES_PER_CU * cus or plan["rows_per_band"] == 8, (plan, cus)


def test_small_grids_and_fp32_stay_at_depth_1(g, monkeypatch):
    """720x360 reads far less than the Infinity Cache holds: depth 1; the switch pins float64 GCM_SW2D_TEMP handles only:
    fp32 handles and plain GCM_SW2D report depth 1 with GCM_SW2D_DEPTH=3 set, and GCM_SW2D_DEPTH=1 keeps the streaming
    grid at depth 1"""
    _switches(monkeypatch)
    c = _core(g, 720, 360)
    try:
        assert c.sw2d_fused_depth() == 1
    finally:
        c.close()
    _switches(monkeypatch, depth=3)
    for kw in (dict(dtype="f32"), dict(dtype="f32", tracer=0), dict(model=g._lib.SW2D, tracer=0)):
        c = _core(g, 720, 360, **kw)
        try:
            assert c.sw2d_fused_depth() == 1, kw
        finally:
            c.close()
    c = _core(g, 720, 360)
    try:
        assert c.sw2d_fused_depth() == 3
    finally:
        c.close()
    _switches(monkeypatch, depth=1)
    c = _core(g, 4096, 2048)
    try:
        assert c.sw2d_fused_depth() == 1
        assert c.sw2d_plan(1)["stream"]
    finally:
        c.close()
