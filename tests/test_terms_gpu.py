"""GPU parity on the cases of tests/term_cases.py: every kernel path against the float64 oracle on inputs where
every term of the step shows (tests/test_term_visibility_cpu.py) -- SW2D_TEMP at a small dx, where the viscosity
is ~6e-3 of u per step instead of ~1e-13 at the 300 km of the older tests."""
import numpy as np
import pytest

from conftest import rel_err
import gpu_setups as su
import term_cases as tc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _by_field(got, names):
    """get_state's [p, u, v, t, q] as a tuple in the order `names`"""
    return tuple(got["puvtq".index(k)] for k in names)


def _run_2d(g, case, monkeypatch):
    model = g._lib.SW2D if case.model == "sw2d" else g._lib.SW2D_TEMP
    H, W = case.shape
    s = tc.state(case)
    names = tc.fields(case)
    kw = dict(dx=case.dx, tracer=case.tracer, dtype=case.dtype)
    planned = "plan" in case.extra           # the plain-SW2D geometry cases: the launch plan is asserted before the step
    if planned:
        for k in ("GCM_FUSED_ROWS", "GCM_SW2D_TWO_STEP", "GCM_SW2D_F32_COLS"):
            monkeypatch.delenv(k, raising=False)
    if "rows" in case.extra:
        monkeypatch.setenv("GCM_FUSED_ROWS", str(case.extra["rows"]))
    if "cols" in case.extra:
        monkeypatch.setenv("GCM_SW2D_F32_COLS", str(case.extra["cols"]))
    staged = case.path.startswith("staged") or case.extra.get("staged")
    kw["variant"] = g._lib.VARIANT_STAGED if staged else g._lib.VARIANT_FUSED
    if case.path == "dropin":
        from gcmiipy_amd.matsumo_temp import matsumo_scheme
        st = (s["u"], s["v"], s["p"], s["t"])
        for _ in range(case.steps):
            st = matsumo_scheme(*st, case.dx, case.dt)
        return st
    if case.path == "band":
        import torch
        from gcmiipy_amd.bands import split_rows
        nb = case.extra["bands"]
        cores = []
        for r, (row0, n) in enumerate(split_rows(H, nb)):
            c = g.Core(model, W, n, nranks=nb, rank=r, global_height=H, row0=row0, **kw)
            c.set_state(**{k: a[row0:row0 + n] for k, a in s.items()})
            if planned:
                tc.check_plan(case, c.sw2d_plan(1))
            cores.append(c)
        for _ in range(case.steps):
            su.exchange(cores, torch)
            for c in cores:
                c.step_interior(case.dt)
            for c in cores:
                c.step_boundary(case.dt)
        got = [None if x[0] is None else np.concatenate(x, axis=0) for x in zip(*[c.get_state() for c in cores])]
        for c in cores:
            c.close()
        return _by_field(got, names)
    if case.path == "stream":
        M = case.extra["members"]
        assert H * W * 8 * len(names) * M > 256 << 20        # the launch streams
        c = g.Core(model, W, H, members=M, **kw)
        c.set_state(**s)
        if planned:
            tc.check_plan(case, c.sw2d_plan(case.steps))
        c.step(case.steps, case.dt)
        got = [_by_field(c.get_member(m), names) for m in case.extra["picks"]]
        assert c.diag(g._lib.DIAG_ANY_NAN) == 0.0
        c.close()
        return got
    c = g.Core(model, W, H, **kw)
    c.set_state(**s)
    if case.path == "staged_half":
        c.half_step(0, case.dt)
        got = _by_field(c.get_star(), names)
    else:
        if planned:
            tc.check_plan(case, c.sw2d_plan(case.steps))
        c.step(case.steps, case.dt)
        got = _by_field(c.get_state(), names)
    c.close()
    return got


def _run(g, case, monkeypatch):
    if case.model in ("sw2d", "sw2d_temp"):
        return _run_2d(g, case, monkeypatch)
    s = tc.state(case)
    if case.model == "oned":
        from gcmiipy_amd import no_limits
        return no_limits.run(*(s[k] for k in "putq"), case.dt, case.dx, case.steps)
    if case.model == "pe2d":
        H, W = case.shape
        c = g.Core(g._lib.PE2D, W, H, dx=case.dx)
    else:
        L, H, W = case.shape
        c = g.Core(g._lib.PE25D, W, H, L, geom=tc.pe25d_geometry(case, product=True), dtype=case.dtype,
                   coriolis=case.extra.get("coriolis", False))
    c.set_state(*(s[k] for k in "puvtq"))
    c.step(case.steps, case.dt)
    got = tuple(c.get_state())
    c.close()
    return got


@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_case_vs_oracle(g, monkeypatch, case):
    """the case's kernel path against the oracle, every field within the case's tolerance; the tolerance is not
    vacuous: the step moves every compared field by more than it"""
    got = _run(g, case, monkeypatch)
    want = tc.oracle_run(case)
    s = tc.state(case)
    if case.extra.get("members"):
        runs = list(zip(got, want, ({k: a[m] for k, a in s.items()} for m in case.extra["picks"])))
    else:
        runs = [(got, want, s)]
    for gm, wm, sm in runs:
        errs = {k: rel_err(x, y) for k, x, y in zip(tc.fields(case), gm, wm)}
        print(case.name, " ".join("%s %.2e" % kv for kv in errs.items()))
        for k, e in errs.items():
            assert e < tc.bound(case, k), (case.name, k, e)
            if case.model != "pe2d" or k != "q":                 # PE2D carries q through unchanged
                assert rel_err(sm[k], wm[tc.fields(case).index(k)]) > tc.bound(case, k), (case.name, k)


def test_sw2d_temp_viscosity_regression(g):
    """the viscosity itself at the smallest dx: the GPU step minus the oracle's step without viscosity is the
    oracle's viscous increment, in u and in v (the v equation takes u's Laplacian, matsumo_temp.py:75,91)"""
    case = next(c for c in tc.CASES if c.name == "temp_fused_none")
    case = case._replace(dx=tc.DX_TINY, dt=1e-3 * tc.DX_TINY, steps=1)
    s = tc.state(case)
    c = g.Core(g._lib.SW2D_TEMP, case.shape[1], case.shape[0], dx=case.dx, variant=g._lib.VARIANT_FUSED)
    c.set_state(**s)
    c.step(1, case.dt)
    got = _by_field(c.get_state(), "uvpt")
    c.close()
    want = tc.oracle_run(case)
    dry = tc.oracle_run(case, {"visc_u": 0.0, "visc_v": 0.0})
    for k in (0, 1):
        inc, ginc = want[k] - dry[k], got[k] - dry[k]
        assert rel_err(inc, want[k]) > 1e-2                        # the viscosity is a large part of the step
        assert rel_err(ginc, inc) < 1e-8, ("uv"[k], rel_err(ginc, inc))
