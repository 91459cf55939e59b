"""What the GPU parity cases can see (tests/term_cases.py), stated on the CPU through the oracle's named term hooks
(oracle/terms.py): for every kernel path of term_cases.PATHS and every term of its model, some case of that path
moves some field by far more than the case's tolerance when the term is dropped or scaled.  A kernel that drops,
scales or misplaces a term then fails the GPU test of that path (tests/test_terms_gpu.py)."""
import numpy as np
import pytest

from conftest import rel_err
import term_cases as tc

# fp64: dropping a term moves some field by >= DROP x 1e-10 and scaling it by 1.01 by >= SCALE x 1e-10
DROP, SCALE, FP64_SCALE = 1e3, 10.0, 1.01
# fp32: scaling a term by 1.1 moves some field by >= 3x that field's bound
FP32_SCALE, FP32_MARGIN = 1.1, 3.0

_REF = {}


def _ref(case):
    if case.name not in _REF:
        _REF[case.name] = tc.oracle_run(case)
    return _REF[case.name]


def _moves(case, terms):
    """per field, the largest rel_err of the mutated run against the default one, over the tolerance"""
    ref, got = _ref(case), tc.oracle_run(case, terms)
    if case.extra.get("members"):
        pairs = [(a, b) for r, g in zip(ref, got) for a, b in zip(g, r)]
        names = tc.fields(case) * len(ref)
    else:
        pairs, names = list(zip(got, ref)), tc.fields(case)
    out = {}
    for k, (a, b) in zip(names, pairs):
        out[k] = max(out.get(k, 0.0), rel_err(a, b) / tc.bound(case, k))
    return out


def _applies(case, name):
    if name.startswith(("flux_", "vanleer_")):
        return case.tracer == 2 or (case.tracer == 1 and name.startswith("flux_"))
    return True


def _visible(case, name):
    if not _applies(case, name):
        return False
    if case.dtype == "f64":
        return (max(_moves(case, {name: 0.0}).values()) >= DROP
                and max(_moves(case, {name: FP64_SCALE}).values()) >= SCALE)
    return max(_moves(case, {name: FP32_SCALE}).values()) >= FP32_MARGIN


@pytest.mark.parametrize("model,path", sorted(tc.PATHS))
def test_every_term_is_visible(model, path):
    dtype, names = tc.PATHS[(model, path)]
    cases = [c for c in tc.CASES if (c.model, c.path) == (model, path)]
    assert cases, "no GPU case runs path %s of %s" % (path, model)
    assert all(c.dtype == dtype for c in cases), path
    blind = [n for n in names if not any(_visible(c, n) for c in cases)]
    assert not blind, "%s %s: no case sees %s" % (model, path, blind)


def test_every_case_belongs_to_a_path():
    names = [c.name for c in tc.CASES]
    assert len(set(names)) == len(names)
    for c in tc.CASES:
        assert (c.model, c.path) in tc.PATHS, c.name


def test_viscosity_is_invisible_at_300_km():
    """why the small-dx cases exist: on the inputs of test_sw2d_gpu.test_sw2d_temp_tracer_vs_oracle (dx = 300 km,
    3 steps) dropping the viscosity, or taking the v equation's from v, moves no field by 1e-11 -- far below the
    1e-10 that test holds the GPU to"""
    from oracle import sw2d_temp
    for shape in ((16, 61), (40, 200)):
        rng = np.random.default_rng(7)
        u, v = rng.standard_normal(shape), rng.standard_normal(shape)
        p = 101325 + rng.standard_normal(shape)
        t = 273.16 + rng.standard_normal(shape)

        def run(terms):
            st = (u, v, p, t)
            for _ in range(3):
                st = sw2d_temp.matsumo_scheme(*st, 300e3, 300.0, _terms=terms)
            return st

        ref = run(None)
        for terms in ({"visc_u": 0.0, "visc_v": 0.0}, {"visc_v": "visc_v_of_v"}, {"visc_u": 2.0}):
            moved = max(rel_err(a, b) for a, b in zip(run(terms), ref))
            assert 0 < moved < 1e-11, (shape, terms, moved)


def test_hooks_default_and_identity():
    """_terms=None and multipliers of 1 leave the oracle's step bit for bit as it was; an unknown name is refused"""
    from oracle import sw2d_temp
    c = next(c for c in tc.CASES if c.name == "temp_fused_van_leer")
    ref = tc.oracle_run(c)
    for a, b in zip(tc.oracle_run(c, {n: 1.0 for n in tc.PATHS[("sw2d_temp", "fused")][1]}), ref):
        assert np.array_equal(a, b)
    s = tc.state(c)
    with pytest.raises(KeyError):
        sw2d_temp.matsumo_scheme(s["u"], s["v"], s["p"], s["t"], c.dx, c.dt, _terms={"visc": 0.0})
