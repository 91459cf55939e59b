"""The wave pair of float64 GCM_SW2D_TEMP (sw2d_pair_kernel<TRACER, STREAM>): two Matsuno steps per launch, the first
step's rows handed from one wave of a workgroup to the other through a ring of row slots in LDS.

Against the float64 oracle at the project's 1e-10, with GCM_SW2D_PAIR=1 (read when the handle is created), on every
shape of sw2d_temp_geometry_cases.SHAPES x the three tracer settings x the pair's band lengths 1, 2, 3, 4, 5, 7 and 64
(GCM_SW2D_PAIR_ROWS).  The shapes reach a band shorter than the halo, rows that wrap more than once (H = 1, 2, 3 with
four halo rows each way) and widths below the stencil; the band lengths reach the two peeled rows, the clamped refill,
whole three-row trips and one or two rows behind them -- i.e. every count of barriers modulo the trip.  The calls are
gc.CALLS (1, 1, 2, 1 steps: single launches and a pair launch alternate on one handle) and 5 steps in one call (two
pairs and a single).  Every case first asserts the plan (n // 2 two-step launches, n % 2 single steps) and the band
length Core.sw2d_pair() reports.  Then the seams of the 56-column strips (widths 55, 56, 57 and 113 at H = 7), the
4096x2048 grid against the same handle with the pair off, and which handles pair at all."""
import numpy as np
import pytest

import sw2d_temp_geometry_cases as gc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_sw2d_geometry_gpu import SWITCHES
from test_sw2d_temp_geometry_gpu import _compare, _state

pytestmark = pytest.mark.gpu
PAIR_SWITCHES = ("GCM_SW2D_PAIR", "GCM_SW2D_PAIR_ROWS", "GCM_SW2D_DEPTH")
PAIR_ROWS = (1, 2, 3, 4, 5, 7, 64)
SEAM_SHAPES = ((7, 55), (7, 56), (7, 57), (7, 113))   # a strip less one column, a strip, a strip and one, two and one
SEAM_ROWS = (3, 64)
# 4096x2048, two steps, pair against single steps: the two runs share every expression and differ in which inlined
# copy of FusedCtx::iter computes a row, i.e. in what -ffp-contract=fast fuses.  One such rounding of the geopotential
# (8e3 m, ulp 9e-13) enters u and v through dt g / dx = 9.8e-3: 9e-15 of max|u| ~ 5; two steps of two stages each with
# a few such terms stay below 1e-13, as fused and staged do (test_fused_equals_staged_full_size asserts 1e-13 over
# three steps).  The bound is ten times that.
FULL_SIZE_BOUND = 1e-12


def _switches(monkeypatch, pair=None, rows=None):
    for k in SWITCHES + PAIR_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if pair is not None:
        monkeypatch.setenv("GCM_SW2D_PAIR", str(pair))
    if rows is not None:
        monkeypatch.setenv("GCM_SW2D_PAIR_ROWS", str(rows))


def _core(g, W, H, tracer=2, **kw):
    kw.setdefault("model", g._lib.SW2D_TEMP)
    model = kw.pop("model")
    return g.Core(model, W, H, dx=gc.DX, tracer=tracer, variant=g._lib.VARIANT_FUSED, **kw)


def _drive(g, monkeypatch, shape, tracer, rows, seams=False):
    H, W = shape
    label = "pair-%s-rows%d-%dx%d" % (gc.TRACER_NAMES[tracer], rows, H, W)
    _switches(monkeypatch, pair=1, rows=rows)
    s = {k: a for k, a in gc.inputs(shape, "f64").items() if k in gc.fields(tracer)}
    want = gc.oracle(shape, tracer, "f64")
    c = _core(g, W, H, tracer)
    try:
        assert c.sw2d_pair() == dict(active=True, rows_per_band=rows), (label, c.sw2d_pair())
        c.set_state(**s)
        done = 0

        def step(n, total):
            plan = c.sw2d_plan(n)
            assert (plan["two_step_launches"], plan["single_step_launches"]) == (n // 2, n % 2), (label, n, plan)
            assert plan["variant"] == "fused" and plan["strip2"] == gc.STRIP2, (label, plan)
            c.step(n, gc.DT)
            # where a failure is named: the pair's bands and its 56-column strips
            _compare(label, total, _state(c.get_state(), tracer), want[total], "f64", tracer,
                     dict(plan, rows_per_band=rows), seams)

        for n in gc.CALLS:
            done += n
            step(n, done)
        assert done == gc.TOTALS[-1]
        for n in gc.AGAIN:                              # two pairs and a single step in one call
            c.set_state(**s)
            step(n, n)
    finally:
        c.close()


@pytest.mark.parametrize("shape", gc.SHAPES, ids=["%dx%d" % s for s in gc.SHAPES])
@pytest.mark.parametrize("rows", PAIR_ROWS)
@pytest.mark.parametrize("tracer", gc.TRACERS, ids=gc.TRACER_NAMES)
def test_pair_vs_oracle(g, monkeypatch, tracer, rows, shape):
    """the plan and the pinned band length, then 1, 2, 4 and 5 steps against the oracle"""
    _drive(g, monkeypatch, shape, tracer, rows)


@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=["%dx%d" % s for s in SEAM_SHAPES])
@pytest.mark.parametrize("rows", SEAM_ROWS)
@pytest.mark.parametrize("tracer", gc.TRACERS, ids=gc.TRACER_NAMES)
def test_pair_strip_seams(g, monkeypatch, tracer, rows, shape):
    """the seams of the 56-column strips, where a wrong lane mask of either step shows: the cells on a seam are held
    to the bound on their own as well"""
    _drive(g, monkeypatch, shape, tracer, rows, seams=True)


def test_pair_full_size_against_single_steps(g, monkeypatch):
    """4096x2048 + van Leer, two steps: the pair (one launch, the STREAM form, its own one-round band length) against
    the same state stepped with GCM_SW2D_PAIR=0 (two deep single-step launches)"""
    H, W = 2048, 4096
    rng = np.random.default_rng(0)
    s = dict(u=rng.standard_normal((H, W)), v=rng.standard_normal((H, W)), p=101325 + rng.standard_normal((H, W)),
             t=273.16 + rng.standard_normal((H, W)), q=rng.random((H, W)))
    res = {}
    for pair in (1, 0):
        _switches(monkeypatch, pair=pair)
        c = _core(g, W, H)
        try:
            plan, info = c.sw2d_plan(2), c.sw2d_pair()
            assert info["active"] == bool(pair) and info["rows_per_band"] >= 8, info
            assert (plan["two_step_launches"], plan["single_step_launches"]) == ((1, 0) if pair else (0, 2)), plan
            assert plan["stream"], plan
            if pair:
                print("PAIR 4096x2048: rows_per_band %d, %d strips x %d bands" % (
                    info["rows_per_band"], -(-W // plan["strip2"]), -(-H // info["rows_per_band"])))
            c.set_state(**s)
            c.step(2, gc.DT)
            res[pair] = _state(c.get_state(), 2)
            assert c.diag(g._lib.DIAG_ANY_NAN) == 0.0
        finally:
            c.close()
    diffs = {k: float(np.max(np.abs(res[1][k] - res[0][k])) / np.max(np.abs(res[0][k]))) for k in "uvptq"}
    print("PAIR 4096x2048 vs single steps, two steps: " + " ".join("%s=%.3e" % kv for kv in diffs.items()))
    for k, d in diffs.items():
        assert d < FULL_SIZE_BOUND, (k, d)


def test_which_handles_pair(g, monkeypatch):
    """switches unset: the streaming grid pairs at n = 2 and not at n = 1, 720x360 does not; GCM_SW2D_PAIR=1 pins a
    float64 GCM_SW2D_TEMP handle of any size and nothing the rule excludes: fp32, plain GCM_SW2D (which keeps its own
    two-step kernel), an ensemble of two members, a latitude band"""
    _switches(monkeypatch)
    c = _core(g, 4096, 2048)
    try:
        assert c.sw2d_pair()["active"], c.sw2d_pair()
        p1, p2, p5 = c.sw2d_plan(1), c.sw2d_plan(2), c.sw2d_plan(5)
    finally:
        c.close()
    assert (p1["two_step_launches"], p1["single_step_launches"]) == (0, 1), p1
    assert (p2["two_step_launches"], p2["single_step_launches"]) == (1, 0), p2
    assert (p5["two_step_launches"], p5["single_step_launches"]) == (2, 1), p5
    assert {k: v for k, v in p1.items() if "launches" not in k} == {k: v for k, v in p2.items() if "launches" not in k}
    c = _core(g, 720, 360)
    try:
        assert not c.sw2d_pair()["active"] and c.sw2d_plan(2)["two_step_launches"] == 0
    finally:
        c.close()
    _switches(monkeypatch, pair=1)
    c = _core(g, 720, 360)
    try:
        assert c.sw2d_pair()["active"] and c.sw2d_plan(2)["two_step_launches"] == 1
    finally:
        c.close()
    excluded = (("fp32", dict(dtype="f32")), ("ensemble", dict(members=2)),
                ("band", dict(nranks=2, rank=0, global_height=720, row0=0)))
    for name, kw in excluded:
        c = _core(g, 720, 360, **kw)
        try:
            assert c.sw2d_pair() == dict(active=False, rows_per_band=0), (name, c.sw2d_pair())
            plan = c.sw2d_plan(2)
            assert (plan["two_step_launches"], plan["single_step_launches"]) == (0, 2), (name, plan)
        finally:
            c.close()
    c = _core(g, 720, 360, tracer=0, model=g._lib.SW2D)
    try:
        assert c.sw2d_pair() == dict(active=False, rows_per_band=0), c.sw2d_pair()
        plan = c.sw2d_plan(2)      # (plain shallow water on a small grid: its own two-step kernel, as before)
    finally:
        c.close()
    _switches(monkeypatch)
    c = _core(g, 720, 360, tracer=0, model=g._lib.SW2D)
    try:
        assert c.sw2d_plan(2) == plan
    finally:
        c.close()
