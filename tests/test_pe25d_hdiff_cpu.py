"""The horizontal diffusion of GCM_PE25D without a device: the host tables (gcm_hdiff_tables) and the host build of the
kernel's cell routine (gcm_hdiff_apply) against the NumPy restatement tests/pe25d_hdiff_ref.py, bit for bit; the
operator's properties on the restatement, which then hold on the device by bit equality; every refused call of the two
probes."""
import ctypes
import math

import numpy as np
import pytest

import gpu_setups as su
import pe25d_hdiff_ref as ref

DT = ref.DT
SHAPES = ((24, 36, 9), (6, 10, 3))


def geometries():
    return [su.geom_of(*s) for s in SHAPES] + [ref.square_geometry()]


def fields_of(geom, nlev=3, seed=31):
    rng = np.random.default_rng(seed)
    return 280.0 + 20.0 * rng.standard_normal((nlev, geom.height, geom.width))


def test_cases_cover_capped_and_uncapped_rows():
    """the four (order, nu) at dt = 120 on gen_geometry(24, 36, 9): no centre row capped, 16 of 24, none, all of them;
    every geometry sees both regimes over the cases; the tables are finite on every row, the pole v row included"""
    geom = su.geom_of(*SHAPES[0])
    for order, nu in ref.CASES:
        t = ref.tables_of(geom, DT, order=order, nu=nu)
        assert int((t["ax"] == 0.125).sum()) == ref.CAPPED_24[(order, nu)], (order, nu)
        assert t["axv"][-1] == 0.125                          # (the pole row of v: dx_h ~ 1e-10)
    for geom in geometries()[:2]:
        capped = [ref.tables_of(geom, DT, order=o, nu=nu)["ax"] == 0.125 for o, nu in ref.CASES]
        assert any(c.any() for c in capped) and any(not c.all() for c in capped)
    for geom in geometries():
        for order, nu in ref.CASES:
            t = ref.tables_of(geom, DT, order=order, nu=nu)
            assert all(np.isfinite(a).all() for a in t.values())
            assert (4 * t["ax"] + 2 * (t["bn"] + t["bs"]) <= 1.0 + 4e-16).all()
            assert (4 * t["axv"] + 2 * (t["bnv"] + t["bsv"]) <= 1.0 + 4e-16).all()


@pytest.mark.parametrize("order,nu", ref.CASES)
def test_tables_equal_the_restatement(order, nu):
    import gcmiipy_amd as g
    for geom in geometries():
        want = ref.tables_of(geom, DT, order=order, nu=nu)
        got = g.hdiff_tables(geom, DT, order=order, nu=nu)
        assert sorted(got) == sorted(ref.NAMES)
        for k in ref.NAMES:
            assert np.array_equal(got[k], want[k]), (k, geom.height)
    # another cap, another dt
    geom = geometries()[0]
    want = ref.tables_of(geom, 45.0, order=order, nu=nu, cmax=0.1)
    got = g.hdiff_tables(geom, 45.0, order=order, nu=nu, cmax=0.1)
    for k in ref.NAMES:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("order,nu", ref.CASES)
def test_apply_equals_the_restatement(order, nu):
    import gcmiipy_amd as g
    for geom in geometries():
        tab = ref.tables_of(geom, DT, order=order, nu=nu)
        X = fields_of(geom)
        for coef in (ref.centre(tab), ref.vrows(tab)):
            got = g.hdiff_apply(X, *coef, order)
            assert np.array_equal(got, ref.step(X, coef, order))
            assert not np.array_equal(got, X)
        assert np.array_equal(g.hdiff_apply(X[0], *ref.centre(tab), order), ref.step(X[0], ref.centre(tab), order))


def test_properties_of_the_restatement():
    # a constant field keeps every bit
    for geom in geometries():
        for order, nu in ref.CASES:
            tab = ref.tables_of(geom, DT, order=order, nu=nu)
            X = np.full((2, geom.height, geom.width), 287.31)
            for coef in (ref.centre(tab), ref.vrows(tab)):
                assert np.array_equal(ref.step(X, coef, order), X)
    # the capped checkerboard on the square geometry is exactly 0 at both orders
    sq = ref.square_geometry()
    for order, nu in ((1, 1.0e9), (2, 1.0e22)):
        tab = ref.tables_of(sq, DT, order=order, nu=nu)
        assert (tab["ax"] == 0.125).all() and (tab["bn"] == 0.125).all() and (tab["bs"] == 0.125).all()
        out = ref.step(ref.checkerboard(sq.height, sq.width, 2), ref.centre(tab), order)
        assert np.array_equal(out, np.zeros_like(out))
    for geom in geometries():
        X = fields_of(geom)
        for order, nu in ref.CASES:
            tab = ref.tables_of(geom, DT, order=order, nu=nu)
            for coef, area in ((ref.centre(tab), tab["area"]), (ref.vrows(tab), tab["areav"])):
                out = ref.step(X, coef, order)
                for k in range(X.shape[0]):
                    # sum area X per level is conserved: |delta| <= 1e-12 sum area |X| (the project's closure figure)
                    w = area[:, None] * np.ones(geom.width)
                    before = math.fsum((w * X[k]).ravel())
                    after = math.fsum((w * out[k]).ravel())
                    assert abs(after - before) <= 1e-12 * math.fsum((w * np.abs(X[k])).ravel()), (order, nu, k)
                    if order == 1:                            # the maximum principle per level
                        assert out[k].max() <= X[k].max() and out[k].min() >= X[k].min()
        # order 2 at the capped coefficient reduces the variance
        tab = ref.tables_of(geom, DT, order=2, nu=1.0e22)
        out = ref.step(X, ref.centre(tab), 2)
        assert out.var() < X.var()


def test_refused_probe_calls():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    geom = geometries()[1]
    H, W = geom.height, geom.width
    nan, inf = float("nan"), float("inf")
    for over in (dict(order=0), dict(order=3), dict(fields=0), dict(fields=16), dict(fields=-1), dict(nu=0.0), dict(nu=-1.0),
                 dict(nu=nan), dict(nu=inf), dict(cmax=0.0), dict(cmax=0.126), dict(cmax=-0.1), dict(cmax=nan)):
        with pytest.raises(ValueError):
            g.hdiff_tables(geom, DT, **over)
    for dt in (nan, inf):
        with pytest.raises(ValueError):
            g.hdiff_tables(geom, dt)
    for over in (dict(nux=1.0), dict(fields="uvx"), dict(fields=""), dict(fields=1.5), dict(order=1.5)):
        with pytest.raises(ValueError):
            g.hdiff_tables(geom, DT, **over)
    dx_j = np.ascontiguousarray(np.asarray(geom.dx_j, dtype=np.float64).reshape(-1))
    dx_h = np.ascontiguousarray(np.asarray(geom.dx_h, dtype=np.float64).reshape(-1))
    out = np.full((8, H), -7.0)
    dp = lambda a: a.ctypes.data_as(L_._dp)
    rec = L_.Hdiff(*ref.DEFAULTS.values())
    tables = lib.gcm_hdiff_tables
    assert tables(H, dp(dx_j), dp(dx_h), geom.dy, rec, DT, dp(out)) == L_.OK
    good = out.copy()
    out[:] = -7.0
    assert tables(0, dp(dx_j), dp(dx_h), geom.dy, rec, DT, dp(out)) == L_.ERR_ARG
    assert tables(H, None, dp(dx_h), geom.dy, rec, DT, dp(out)) == L_.ERR_ARG
    assert tables(H, dp(dx_j), None, geom.dy, rec, DT, dp(out)) == L_.ERR_ARG
    assert tables(H, dp(dx_j), dp(dx_h), geom.dy, None, DT, dp(out)) == L_.ERR_ARG
    assert tables(H, dp(dx_j), dp(dx_h), geom.dy, rec, DT, None) == L_.ERR_ARG
    assert b"gcm_hdiff_tables" in lib.gcm_last_error(None)
    assert (out == -7.0).all()                               # (a refused call writes nothing)
    # the apply probe
    X = fields_of(geom)
    res = np.full_like(X, -7.0)
    tab4 = np.ascontiguousarray(good[:4])
    apply = lib.gcm_hdiff_apply
    assert apply(H, W, 3, dp(tab4), 2, dp(X), dp(res)) == L_.OK
    res[:] = -7.0
    for args in ((0, W, 3, dp(tab4), 2, dp(X), dp(res)), (H, 0, 3, dp(tab4), 2, dp(X), dp(res)),
                 (H, W, 0, dp(tab4), 2, dp(X), dp(res)), (H, W, 3, None, 2, dp(X), dp(res)),
                 (H, W, 3, dp(tab4), 0, dp(X), dp(res)), (H, W, 3, dp(tab4), 3, dp(X), dp(res)),
                 (H, W, 3, dp(tab4), 2, None, dp(res)), (H, W, 3, dp(tab4), 2, dp(X), None)):
        assert apply(*args) == L_.ERR_ARG
    assert b"gcm_hdiff_apply" in lib.gcm_last_error(None)
    assert (res == -7.0).all()
    with pytest.raises(ValueError):
        g.hdiff_apply(X, good[0][:-1], good[1], good[2], 2)
    with pytest.raises(ValueError):
        g.hdiff_apply(X[0, 0], good[0], good[1], good[2], 2)
    # the handle's entry points without a handle
    assert lib.gcm_set_hdiff(None, rec) == L_.ERR_ARG and lib.gcm_hdiff_on(None) == L_.ERR_ARG
    assert lib.gcm_hdiff_step(None, DT, rec) == L_.ERR_ARG
    assert lib.gcm_hdiff_plan(None, (ctypes.c_int * L_.HDIFF_PLAN_WORDS)(), L_.HDIFF_PLAN_WORDS) == L_.ERR_ARG


def test_struct_and_constants_match_header():
    import os
    import re
    import gcmiipy_amd as g
    L_ = g._lib
    src = open(os.path.join(su.ROOT, "include", "gcmcore.h")).read()
    for name in ("U", "V", "T", "Q", "PLAN_WORDS"):
        assert int(re.search(r"#define GCM_HDIFF_%s (\d+)" % name, src).group(1)) == getattr(L_, "HDIFF_" + name)
    end = src.index("} gcm_hdiff;")
    body = re.sub(r"/\*.*?\*/", "", src[src.rindex("typedef struct {", 0, end):end], flags=re.S)
    assert re.findall(r"(?:int32_t|double)\s+(\w+);", body) == [f[0] for f in L_.Hdiff._fields_]
    assert ctypes.sizeof(L_.Hdiff) == 2 * 4 + 2 * 8
    assert g.core.hdiff_params({}) == ref.DEFAULTS and list(g.core.HDIFF_DEFAULTS) == list(ref.DEFAULTS)
    assert g.core.hdiff_params(dict(fields="tq"))["fields"] == 12
