"""The cases of tests/tracer_range_cases.py bite, and their references are sound (no GPU): the plumes carry denormal
cells and boxes of exact zeros, the oracle and the PE25D restatement stay finite on every input, the oracle run directly
on a scaled input agrees with the np.ldexp reference under the rule, a NumPy model of the device arithmetic in the
handle's type passes with a true division (and with the guarded reciprocals of the kernels), the same model with the
reciprocal of the limiter's denominator formed first fails `plume` and `denormal` by a non-finite value and nothing
else, and a small planted mistake fails `down` and `up`, where the floor of the rule does not dominate."""
import numpy as np
import pytest

import tracer_range_cases as rc

DTYPES = ("f64", "f32")
# (shape, real type) of the 2-D handles of tests/test_tracer_range_gpu.py
CASES_2D = [(rc.SHAPE_2D, "f64"), (rc.SHAPE_2D, "f32"), (rc.SHAPE_2D_COLS2, "f32")]
STEPS = (1, 3)
SCHEMES = (rc.UPWIND, rc.VANLEER)


def _judge_2d(got, shape, dtype, tracer, steps, name):
    return rc.judge(got, rc.reference_2d(shape, dtype, tracer, steps)[name], rc.tracers_2d(shape, dtype)[name],
                    rc.bound("sw2d_temp", dtype, steps), dtype, steps)


def _judge_pe(got, dtype, scheme, name):
    return rc.judge(got, rc.reference_pe(dtype, scheme)[name], rc.tracers_pe(dtype)[name], rc.bound("pe25d", dtype),
                    dtype, 1, levels=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_plumes_carry_denormals_and_zero_boxes(dtype):
    """at least 20 denormal cells and one box of exact zeros per level (2-D on 33 x 97: 70 / 104 denormal cells and
    732 / 2544 zeros at f64 / f32; PE25D per level: 148 / 70 and 200 / 262), and `denormal` is nothing but denormals"""
    q = rc.tracers_2d(rc.SHAPE_2D, dtype)
    c = rc.tracers_pe(dtype)
    levels = [q["plume"]] + list(c["plume"])
    for a in levels:
        n, zeros = rc.count_denormals(a, dtype), int(np.count_nonzero(rc.reach_max(a, 2) == 0))
        print(dtype, a.shape, "denormal cells", n, "exact zeros", int(np.count_nonzero(a == 0)), "zero boxes", zeros)
        assert n >= 20 and zeros >= 1
    assert np.count_nonzero(rc.reach_max(c["plume"], 2, 2) == 0) >= 1
    for a in (q["denormal"], c["denormal"], rc.tracers_2d(rc.SHAPE_2D_COLS2, dtype)["denormal"]):
        assert rc.count_denormals(a, dtype) == a.size
    for name in ("down", "up"):                              # and the other two scaled inputs are exact and normal
        e = rc.SCALED[dtype][name]
        for t in (q, c):
            assert np.array_equal(t[name], np.ldexp(t["ordinary"], e)) and rc.count_denormals(t[name], dtype) == 0
            assert np.all(np.isfinite(t[name]))


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("tracer", SCHEMES)
@pytest.mark.parametrize("shape,dtype", CASES_2D)
def test_oracle_2d_is_finite_and_scales(shape, dtype, tracer, steps):
    """the oracle on every input: finite, and run directly on a scaled input it agrees with the scaled reference"""
    qs = rc.tracers_2d(shape, dtype)
    for name in rc.INPUTS:
        direct = rc.oracle_2d(shape, dtype, tracer, qs[name], steps)
        assert np.all(np.isfinite(direct)), name
        v = _judge_2d(direct, shape, dtype, tracer, steps, name)
        print("oracle 2-D", shape, dtype, tracer, steps, name, v)
        assert v.ok, (name, v)
        if name in ("down", "up"):
            assert np.array_equal(direct, rc.reference_2d(shape, dtype, tracer, steps)[name]), name


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_restatement_pe_is_finite_and_scales(dtype, scheme):
    direct = rc.restatement_pe(dtype, scheme, rc.stack_pe(dtype))
    assert np.all(np.isfinite(direct))
    for n, name in enumerate(rc.INPUTS):
        v = _judge_pe(direct[n], dtype, scheme, name)
        print("restatement PE25D", dtype, scheme, name, v)
        assert v.ok, (name, v)
        if name in ("down", "up"):
            assert np.array_equal(direct[n], rc.reference_pe(dtype, scheme)[name]), name


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("tracer", SCHEMES)
@pytest.mark.parametrize("shape,dtype", CASES_2D)
def test_models_of_face_flux(shape, dtype, tracer, steps):
    """face_flux in the handle's type.  A true division, a reciprocal whose product is clamped to the weight's range,
    and a reciprocal taken only where both differences are normal numbers (the kernel's guard) pass every input.  The reciprocal formed first and not clamped fails `plume` and `denormal` under VANLEER by
    non-finite cells and passes the rest (UPWIND has no reciprocal: it passes everything).  The correction taken with
    0.4 for 0.5 fails `ordinary`, `down` and `up` under VANLEER."""
    qs = rc.tracers_2d(shape, dtype)
    for name in rc.INPUTS:
        run = lambda weight, half=0.5: _judge_2d(rc.model_2d(shape, dtype, tracer, qs[name], steps, weight, half),
                                                 shape, dtype, tracer, steps, name)
        good, clamped, bad, planted = (run(rc.true_division), run(rc.reciprocal_clamped), run(rc.reciprocal_first),
                                       run(rc.true_division, 0.4))
        guarded = run(rc.reciprocal_of_normals)              # what face_flux does
        print("face_flux model", shape, dtype, tracer, steps, name, "division %.2g, clamped %.2g, normals only %.2g; "
              "reciprocal first: %d non-finite; planted %.2g" % (good.use, clamped.use, guarded.use, bad.nonfinite,
                                                                 planted.use))
        assert good.ok and clamped.ok and guarded.ok, (name, good, clamped, guarded)
        breaks = tracer == rc.VANLEER and name in ("plume", "denormal")
        assert bad.ok == (not breaks) and (bad.nonfinite > 0) == breaks, (name, bad)
        if tracer == rc.VANLEER and name in ("ordinary", "down", "up"):
            assert not planted.ok and planted.nonfinite == 0 and planted.over > 0, (name, planted)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_models_of_tracer_face(dtype, scheme):
    """tracer_face in the handle's type: the true division and the clamped reciprocal (what the kernel does) pass every
    input, the reciprocal without its clamp fails `plume` and `denormal` by non-finite cells, and a half weight taken
    at 0.8 of its value fails `ordinary`, `down` and `up`"""
    c = rc.stack_pe(dtype)
    runs = {k: rc.model_pe(dtype, scheme, c, w) for k, w in (("division", rc.true_division),
                                                            ("clamped", rc.reciprocal_clamped),
                                                            ("first", rc.reciprocal_first))}
    runs["planted"] = rc.model_pe(dtype, scheme, c, rc.true_division, trim=0.8)
    for n, name in enumerate(rc.INPUTS):
        v = {k: _judge_pe(a[n], dtype, scheme, name) for k, a in runs.items()}
        print("tracer_face model", dtype, scheme, name, "division %.2g, clamped %.2g; reciprocal first: %d non-finite; "
              "planted %.2g" % (v["division"].use, v["clamped"].use, v["first"].nonfinite, v["planted"].use))
        assert v["division"].ok and v["clamped"].ok, (name, v)
        breaks = scheme == rc.VANLEER and name in ("plume", "denormal")
        assert v["first"].ok == (not breaks) and (v["first"].nonfinite > 0) == breaks, (name, v["first"])
        if scheme == rc.VANLEER and name in ("ordinary", "down", "up"):
            assert not v["planted"].ok and v["planted"].over > 0, (name, v["planted"])


def test_the_rule_itself():
    """a cell that must be zero and is not, a NaN, and an error just over and just under the allowance"""
    q = np.zeros((9, 11))
    q[4, 5] = 1.0
    want = q.copy()
    B, t = 1e-10, rc.tiny("f64")
    assert rc.judge(want, want, q, B, "f64").ok
    got = want.copy()
    got[0, 0] = 5e-324                                       # outside the 5 x 5 box of the one cell
    assert rc.judge(got, want, q, B, "f64")[:4] == (False, 0, 1, 0)
    got = want.copy()
    got[4, 7] = -0.0                                         # the sign of a zero is ignored
    got[6, 3] = 0.5 * t                                      # the floor, inside the box
    assert rc.judge(got, want, q, B, "f64").ok
    got[4, 8] = 0.5 * t                                      # one column outside it (radius 2), inside that of 2 steps
    assert rc.judge(got, want, q, B, "f64").nonzero == 1 and rc.judge(got, want, q, B, "f64", steps=2).ok
    got = want.copy()
    got[2, 3] = 1.01e-10
    assert rc.judge(got, want, q, B, "f64").over == 1
    got[2, 3] = 0.99e-10
    assert rc.judge(got, want, q, B, "f64").ok
    got[4, 5] = np.nan
    assert rc.judge(got, want, q, B, "f64").nonfinite == 1
    col = np.zeros((7, 9, 11))                               # the column does not wrap
    col[0, 4, 5] = 1.0
    S = rc.reach_max(col, 2, 2)
    assert S[2, 4, 5] == 1.0 and S[3, 4, 5] == 0.0 and S[6, 4, 5] == 0.0 and S[1, 2, 3] == 1.0 and S[1, 1, 3] == 0.0
