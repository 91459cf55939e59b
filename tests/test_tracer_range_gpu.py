"""GPU: limited tracer transport held to the oracle across the float range, cell by cell (tests/tracer_range_cases.py:
the inputs, the references and the error rule; tests/test_tracer_range_cpu.py shows that they bite).  GCM_SW2D_TEMP
staged and fused at both real types and every fused form, the drop-in two_d.limited_advection, flux_limiter's promise
of NumPy's bits, and the GCM_PE25D passive tracers -- on an ordinary random tracer, a plume whose flanks run through the
denormals into exact zeros, and the random tracer scaled down, into the denormals and up.  UPWIND has no reciprocal: it
is the control that the rule and the references are right."""
import numpy as np
import pytest

import gpu_setups as su
import operator_dropin_cases as oc
import tracer_range_cases as rc
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_sw2d_deep_gpu import DEPTH_SWITCH
from test_sw2d_geometry_gpu import SWITCHES

pytestmark = pytest.mark.gpu
TRACERS = {"upwind": rc.UPWIND, "van_leer": rc.VANLEER}

# (name, real type, shape, variant, switches, what the handle must report)
PATHS_2D = [("f64_staged", "f64", rc.SHAPE_2D, "staged", {}, {"depth": 0}),
            ("f64_fused_depth1", "f64", rc.SHAPE_2D, "fused", {DEPTH_SWITCH: "1"}, {"depth": 1}),
            ("f64_fused_depth3", "f64", rc.SHAPE_2D, "fused", {DEPTH_SWITCH: "3"}, {"depth": 3}),
            ("f32_staged", "f32", rc.SHAPE_2D, "staged", {}, {}),
            ("f32_fused_cols1", "f32", rc.SHAPE_2D, "fused", {"GCM_SW2D_F32_COLS": "1"}, {"cols": 1}),
            ("f32_fused_cols2", "f32", rc.SHAPE_2D_COLS2, "fused", {"GCM_SW2D_F32_COLS": "2"}, {"cols": 2})]


def _report(label, name, v):
    print("%-44s %-9s use %.3g of the allowed error; non-finite %d, nonzero where zero is due %d, over %d"
          % (label, name, v.use, v.nonfinite, v.nonzero, v.over))


@pytest.mark.parametrize("tracer", list(TRACERS))
@pytest.mark.parametrize("path", PATHS_2D, ids=[p[0] for p in PATHS_2D])
def test_sw2d_temp_tracer_vs_oracle(g, monkeypatch, path, tracer):
    """one step and three steps of every input: q under the rule, and u, v, p, t bit for bit those of the handle that
    was given the ordinary tracer (a passive tracer does not reach the dynamics)"""
    label, dtype, shape, variant, switches, reports = path
    for k in SWITCHES + (DEPTH_SWITCH,):
        monkeypatch.delenv(k, raising=False)
    for k, x in switches.items():
        monkeypatch.setenv(k, x)
    H, W = shape
    scheme = TRACERS[tracer]
    var = {"fused": g._lib.VARIANT_FUSED, "staged": g._lib.VARIANT_STAGED}[variant]
    s, qs = rc.state_2d(shape, dtype), rc.tracers_2d(shape, dtype)
    missed, dynamics = [], {}
    for name in rc.INPUTS:
        c = g.Core(g._lib.SW2D_TEMP, W, H, dx=rc.DX, tracer=scheme, variant=var, dtype=dtype)
        try:
            if "depth" in reports:
                assert c.sw2d_fused_depth() == reports["depth"], label
            if "cols" in reports:
                plan = c.sw2d_plan(1)
                assert (plan["variant"], plan["cols"], plan["strip"]) == ("fused", reports["cols"], 60 * reports["cols"]), plan
            c.set_state(q=qs[name], **s)
            done = 0
            for steps in (1, 3):
                c.step(steps - done, rc.DT)
                done = steps
                p, u, v, t, q = c.get_state()
                verdict = rc.judge(q, rc.reference_2d(shape, dtype, scheme, steps)[name], qs[name],
                                   rc.bound("sw2d_temp", dtype, steps), dtype, steps)
                _report("%s %s %d step(s)" % (label, tracer, steps), name, verdict)
                if not verdict.ok:
                    missed.append((name, steps, verdict))
                if name == "ordinary":
                    dynamics[steps] = (p, u, v, t)
                else:
                    for k, a, b in zip("puvt", (p, u, v, t), dynamics[steps]):
                        assert np.array_equal(a, b), (label, name, steps, k)
        finally:
            c.close()
    assert not missed, (label, tracer, missed)


def test_two_d_limited_advection_vs_oracle():
    """the drop-in (advect_axis_kernel of ops2d_kernels.hip), float64, one step on the handle's winds"""
    from gcmiipy_amd import two_d
    shape = rc.SHAPE_2D
    s, qs = rc.state_2d(shape, "f64"), rc.tracers_2d(shape, "f64")
    V = np.stack([s["v"], s["u"]])
    missed = []
    for name in rc.INPUTS:
        got = two_d.limited_advection(rc.DT, (rc.DX, rc.DX), V, qs[name])
        verdict = rc.judge(got, rc.reference_2d(shape, "f64", rc.VANLEER, 1)[name], qs[name],
                           rc.bound("sw2d_temp", "f64"), "f64")
        _report("two_d.limited_advection", name, verdict)
        if not verdict.ok:
            missed.append((name, verdict))
    assert not missed, missed


@pytest.mark.parametrize("name", ["down", "denormal", "up"])
def test_flux_limiter_bit_for_bit_across_the_range(name):
    """calc_r, van_leer and donor_cell_advection on a 97-cell line of the scaled inputs: the bits of oracle.tracer,
    the signs of the zeros included"""
    from gcmiipy_amd import flux_limiter as fl
    from oracle import tracer as otr
    q, u = rc.line(name)
    assert q.shape == (97,)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r = otr.calc_r(q)
        pairs = [("calc_r", fl.calc_r(q), r),
                 ("van_leer(calc_r)", fl.van_leer(r), otr.van_leer(r)),
                 ("van_leer(q)", fl.van_leer(q), otr.van_leer(q)),
                 ("donor_cell_advection", fl.donor_cell_advection(q, u, 10.0, 1.0), otr.donor_cell_advection(q, u, 10.0, 1.0))]
    differ = []
    for what, got, want in pairs:
        same = oc.same_bits(got, want)
        print("flux_limiter %-9s %-22s %s" % (name, what, "bit-identical" if same else "DIFFERS in %d cells"
                                              % np.count_nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))))
        if not same:
            differ.append(what)
    assert not differ, (name, differ)


@pytest.mark.parametrize("scheme", list(TRACERS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pe25d_tracers_vs_restatement(g, dtype, scheme):
    """one Matsuno step with the five inputs as five tracers of one handle, against the restatement on the oracle's
    fluxes under the rule; p, u, v, t and q are bit for bit those of a handle without tracers"""
    H, W, L = rc.SHAPE_PE
    geom = su.geom_of(H, W, L)
    st, trs = rc.state_pe(dtype), rc.stack_pe(dtype)
    res = {}
    for with_tracers in (True, False):
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype, filter=True, coriolis=False,
                   tracer_scheme=scheme if with_tracers else None)
        try:
            c.set_state(*st)
            if with_tracers:
                c.set_tracers(trs)
            c.step(1, rc.PE_DT)
            res[with_tracers] = c.get_state()
            if with_tracers:
                got = c.get_tracers()
        finally:
            c.close()
    missed = []
    for n, name in enumerate(rc.INPUTS):
        verdict = rc.judge(got[n], rc.reference_pe(dtype, TRACERS[scheme])[name], trs[n], rc.bound("pe25d", dtype), dtype,
                           1, levels=True)
        _report("pe25d %s %s" % (dtype, scheme), name, verdict)
        if not verdict.ok:
            missed.append((name, verdict))
    for k, a, b in zip("puvtq", res[True], res[False]):
        assert np.array_equal(a, b), k
    assert not missed, (dtype, scheme, missed)
