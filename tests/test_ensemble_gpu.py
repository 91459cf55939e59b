"""GPU checks of the ensemble handles (gcm_config.members): every member of an M-member handle advances
exactly as a one-member handle on the same state does, members never see one another, the per-member
diagnostics match NumPy, and the state entry points, snapshots and checkpoints cover all members."""
import numpy as np
import pytest

from conftest import rel_err
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10
DX, DT = 300e3, 300.0


# (name, model, tracer): SW2D and SW2D_TEMP with every tracer scheme
MODELS = [("sw2d", 1, 0), ("temp", 2, 0), ("temp_upwind", 2, 1), ("temp_vanleer", 2, 2)]


def _states(model, tracer, M, H, W, seed):
    """M distinct random states {p, u, v[, t[, q]]} as (M, H, W) arrays"""
    rng = np.random.default_rng(seed)
    s = {"u": rng.standard_normal((M, H, W)), "v": rng.standard_normal((M, H, W))}
    if model == 1:
        s["p"] = 8000 + 10 * rng.standard_normal((M, H, W))
    else:
        s["p"] = 101325 + 10 * rng.standard_normal((M, H, W))
        s["t"] = 273.16 + rng.standard_normal((M, H, W))
        if tracer:
            s["q"] = rng.random((M, H, W))
    return s


def _member(s, m):
    return {k: a[m] for k, a in s.items()}


def _single(g, model, tracer, variant, W, H, state, steps):
    c = g.Core(model, W, H, dx=DX, variant=variant, tracer=tracer)
    c.set_state(**state)
    c.step(steps, DT)
    out = c.get_state()
    c.close()
    return out


_ORACLE = {}


def _sw2d_oracle(state, steps, key):
    """{u, v, p} of the float64 oracle after `steps` steps of plain shallow water, computed once per key"""
    if key not in _ORACLE:
        from oracle import sw2d
        st = (state["u"], state["v"], state["p"])
        for _ in range(steps):
            st = sw2d.matsumo_scheme(*st, DX, DT)
        _ORACLE[key] = dict(zip("uvp", st))
    return _ORACLE[key]


# the band height matters to the fused variant only: short bands (GCM_SW2D: the preloading kernel and fused2
# pairs) and long ones
@pytest.mark.parametrize("variant,rows", [("fused", 3), ("fused", 16), ("staged", None)])
@pytest.mark.parametrize("name,model,tracer", MODELS)
@pytest.mark.parametrize("W,H", [(720, 360), (97, 61)])
def test_every_member_equals_a_single_handle(g, monkeypatch, W, H, name, model, tracer, variant, rows):
    """5 members, 7 steps (GCM_SW2D: three fused2 pairs and a single step when the bands are short):
    bit for bit what a one-member handle computes on each member's state, with the band height pinned.  Plain
    shallow water at (97, 61): the handle launches what the pinned rows mean (Core.sw2d_plan) and member 0 agrees
    with the float64 oracle, so that a fault the ensemble and the single handle share shows too"""
    if rows is not None:
        monkeypatch.setenv("GCM_FUSED_ROWS", str(rows))
    monkeypatch.setenv("GCM_SW2D_TWO_STEP", "1")
    var = {"fused": g._lib.VARIANT_FUSED, "staged": g._lib.VARIANT_STAGED}[variant]
    M = 5
    s = _states(model, tracer, M, H, W, seed=W + H + model + tracer)
    c = g.Core(model, W, H, dx=DX, variant=var, tracer=tracer, members=M)
    assert c.members == M and c.options["members"] == M
    c.set_state(**s)
    plan = c.sw2d_plan(7)
    c.step(7, DT)
    ens = c.get_state()
    c.close()
    for m in range(M):
        one = _single(g, model, tracer, var, W, H, _member(s, m), 7)
        for f, (a, b) in enumerate(zip(ens, one)):
            if b is not None:
                assert np.array_equal(a[m], b), (m, "puvtq"[f])
    if name == "sw2d" and (W, H) == (97, 61):
        pairs = 3 if rows == 3 else 0
        assert (plan["variant"], plan["two_step_launches"], plan["single_step_launches"]) == (variant, pairs, 7 - 2 * pairs)
        if rows is not None:
            assert (plan["rows_per_band"], plan["preload"], plan["stream"]) == (rows, rows <= 4, False), plan
        want = _sw2d_oracle(_member(s, 0), 7, (W, H))
        for k, b in want.items():
            e = rel_err(ens["puvtq".index(k)][0], b)
            assert e < TOL, (k, e, plan)


@pytest.mark.parametrize("name,model,tracer", [MODELS[0], MODELS[3]])
def test_members_match_oracle_unpinned(g, name, model, tracer):
    from oracle import sw2d, sw2d_temp, tracer as otr
    W, H, M, steps = 97, 61, 2, 4
    s = _states(model, tracer, M, H, W, seed=11)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M)
    c.set_state(**s)
    c.step(steps, DT)
    got = c.get_state()
    c.close()
    for m in range(M):
        x = _member(s, m)
        if model == 1:
            st = (x["u"], x["v"], x["p"])
            for _ in range(steps):
                st = sw2d.matsumo_scheme(*st, DX, DT)
            want = {"u": st[0], "v": st[1], "p": st[2]}
        else:
            st, q = (x["u"], x["v"], x["p"], x["t"]), x["q"]
            for _ in range(steps):
                q = otr.limited_advection(DT, (DX, DX), np.stack([st[1], st[0]]), q, limiter=True)
                st = sw2d_temp.matsumo_scheme(*st, DX, DT)
            want = {"u": st[0], "v": st[1], "p": st[2], "t": st[3], "q": q}
        for k, b in want.items():
            e = rel_err(got["puvtq".index(k)][m], b)
            assert e < TOL, (m, k, e)


def test_isolation(g):
    """one member carrying NaNs and wild values leaves every other member bit-identical"""
    W, H, M, bad = 97, 61, 4, 2
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    s = _states(model, tracer, M, H, W, seed=3)
    runs = []
    for poison in (False, True):
        x = {k: a.copy() for k, a in s.items()}
        if poison:
            x["p"][bad, :3, :] = np.nan                        # first rows: their neighbours wrap to the last rows
            x["p"][bad, -2:, 5:9] = np.nan
            x["u"][bad] *= 1e30
            x["t"][bad, :, 0] = -1e300
        c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M)
        c.set_state(**x)
        c.step(5, DT)
        runs.append((c.get_state(), c.diag_members(g._lib.DIAG_ANY_NAN), c.diag(g._lib.DIAG_ANY_NAN)))
        c.close()
    (clean, nan0, any0), (dirty, nan1, any1) = runs
    for m in range(M):
        if m != bad:
            for a, b in zip(clean, dirty):
                if a is not None:
                    assert np.array_equal(a[m], b[m]), m
    assert list(nan0) == [0.0] * M and any0 == 0.0
    assert list(nan1) == [1.0 if m == bad else 0.0 for m in range(M)] and any1 == 1.0


def test_diag_members_match_numpy(g):
    W, H, M = 97, 61, 6
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_UPWIND
    s = _states(model, tracer, M, H, W, seed=9)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M)
    c.set_state(**s)
    c.step(3, DT)
    p, u, v, t, q = c.get_state()
    L = g._lib

    def tv(x):
        return np.abs(x - np.roll(x, -1, axis=1)).sum(axis=(1, 2))     # rows wrap inside each member

    exact = {L.DIAG_MAX_U: u.max(axis=(1, 2)), L.DIAG_MIN_U: u.min(axis=(1, 2)),
             L.DIAG_MAX_V: v.max(axis=(1, 2)), L.DIAG_MIN_V: v.min(axis=(1, 2)), L.DIAG_ANY_NAN: np.zeros(M)}
    close = {L.DIAG_MEAN_P: p.mean(axis=(1, 2)), L.DIAG_SUM_P: p.sum(axis=(1, 2)), L.DIAG_TV_P: tv(p),
             L.DIAG_TV_U: tv(u), L.DIAG_TV_V: tv(v), L.DIAG_TV_T: tv(t), L.DIAG_TV_Q: tv(q)}
    for k, want in exact.items():
        got = c.diag_members(k)
        assert got.shape == (M,) and np.array_equal(got, want), k
    for k, want in close.items():
        got = c.diag_members(k)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (k, got, want)
    # gcm_diag reduces over all members
    assert c.diag(L.DIAG_MAX_U) == u.max() and c.diag(L.DIAG_MIN_V) == v.min()
    assert abs(c.diag(L.DIAG_MEAN_P) - p.mean()) <= 1e-12 * abs(p.mean())
    assert abs(c.diag(L.DIAG_TV_T) - tv(t).sum()) <= 1e-12 * tv(t).sum()
    c.close()


def test_diag_members_match_single_handles(g):
    """every DIAG_* kind of every member of an fp32 ensemble against gcm_diag of a one-member handle holding that
    member's state: max, min and any-NaN are the same values (==); sums and total variations are added up by a
    different number of workgroups per member on the two paths, so both are held to the float64 NumPy figure of the
    fp32-rounded state within 1e-12 (the bound of test_diag_members_match_numpy)"""
    W, H, M = 34, 16, 3
    model, tracer, L = g._lib.SW2D_TEMP, g._lib.TRACER_UPWIND, g._lib
    s = _states(model, tracer, M, H, W, seed=17)
    s["u"][1, 5, 7] = np.nan                                   # one member with a NaN: any-NaN, max and min follow it
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M, dtype="f32")
    c.set_state(**s)
    r = dict(zip("puvtq", c.get_state()))                      # the fp32-rounded state, widened

    def tv(x):
        return np.abs(x - np.roll(x, -1, axis=0)).sum()

    exact = (L.DIAG_ANY_NAN, L.DIAG_MAX_U, L.DIAG_MIN_U, L.DIAG_MAX_V, L.DIAG_MIN_V)
    close = {L.DIAG_MEAN_P: lambda m: r["p"][m].mean(), L.DIAG_SUM_P: lambda m: r["p"][m].sum(),
             L.DIAG_TV_P: lambda m: tv(r["p"][m]), L.DIAG_TV_U: lambda m: tv(r["u"][m]), L.DIAG_TV_V: lambda m: tv(r["v"][m]),
             L.DIAG_TV_T: lambda m: tv(r["t"][m]), L.DIAG_TV_Q: lambda m: tv(r["q"][m])}
    ens = {k: c.diag_members(k) for k in exact + tuple(close)}
    c.close()
    for m in range(M):
        one = g.Core(model, W, H, dx=DX, tracer=tracer, dtype="f32")
        one.set_state(**_member(s, m))
        for k in exact:
            a, b = ens[k][m], one.diag(k)
            assert a == b or (np.isnan(a) and np.isnan(b)), (m, k, a, b)
        for k, f in close.items():
            want = f(m)
            for got in (ens[k][m], one.diag(k)):
                assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-12 * abs(want), (m, k, got, want)
        one.close()
    assert ens[L.DIAG_ANY_NAN].tolist() == [0.0, 1.0, 0.0]


def test_state_entry_points(g):
    W, H, M = 97, 61, 3
    model, L = g._lib.SW2D_TEMP, g._lib
    s = _states(model, 0, M, H, W, seed=21)
    c = g.Core(model, W, H, dx=DX, members=M)
    c.set_state(**s)
    # set_member / get_member round-trip
    got = c.get_member(1)
    for k in "puvt":
        assert np.array_equal(got["puvtq".index(k)], s[k][1])
    other = _states(model, 0, 1, H, W, seed=22)
    c.set_member(1, **_member(other, 0))
    full = c.get_state()
    for k in "puvt":
        assert np.array_equal(full["puvtq".index(k)][1], other[k][0])
        assert np.array_equal(full["puvtq".index(k)][0], s[k][0])
    with pytest.raises(ValueError):
        c.set_member(M, p=s["p"][0])
    with pytest.raises(ValueError):
        c.get_member(-1)
    # perturbing one member changes only that member after a step
    c.set_state(**s)
    c.step(1, DT)
    base = c.get_state()
    c.set_state(**s)
    pert = s["u"][2].copy()
    pert[30, 40] += 1e-3
    c.set_member(2, u=pert)
    c.step(1, DT)
    after = c.get_state()
    for f in range(4):
        for m in range(M):
            same = np.array_equal(base[f][m], after[f][m])
            assert same == (m != 2), (f, m)
    # half steps with M-fold star arrays
    c.set_state(**s)
    c.half_step(0, DT)
    star = c.get_star()
    assert star[0].shape == (M, H, W)
    c.set_star(p=star[0], u=star[1], v=star[2], t=star[3])
    c.half_step(1, DT)
    hs = c.get_state()
    c.set_state(**s)
    c.step(1, DT)
    full_step = c.get_state()
    for a, b in zip(hs, full_step):
        if a is not None:
            assert rel_err(a, b) < 1e-13
    # snapshot / restore reproduce a run bit for bit
    c.set_state(**s)
    c.step(2, DT)
    c.snapshot()
    c.step(5, DT)
    first = c.get_state()
    c.restore()
    c.step(5, DT)
    again = c.get_state()
    for a, b in zip(first, again):
        if a is not None:
            assert np.array_equal(a, b)
    c.close()


def test_checkpoint_resumes_bit_exactly(g, tmp_path):
    from gcmiipy_amd import checkpoint
    W, H, M = 97, 61, 4
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    s = _states(model, tracer, M, H, W, seed=31)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M)
    c.set_state(**s)
    c.step(3, DT)
    path = str(tmp_path / "ens.npz")
    checkpoint.save(path, c, step=3)
    c.step(4, DT)
    want = c.get_state()
    c.close()
    r, ck = checkpoint.restore(path)
    assert r.members == M and ck["options"]["members"] == M
    r.step(4, DT)
    got = r.get_state()
    r.close()
    for a, b in zip(got, want):
        if a is not None:
            assert np.array_equal(a, b)


def test_large_ensemble_streams(g, monkeypatch):
    """32 x 720x360 SW2D_TEMP + van Leer reads over 256 MB per launch (the STREAM instantiation): picked members
    equal single handles, which read the state with ordinary loads, bit for bit.  The band height is pinned for
    both (as the fp32 twin in test_sw2d_f32_gpu.py does): the streaming hint changes how the base state is
    loaded, not what is computed."""
    monkeypatch.setenv("GCM_FUSED_ROWS", "24")
    W, H, M, steps = 720, 360, 32, 10
    model, tracer = g._lib.SW2D_TEMP, g._lib.TRACER_VANLEER
    assert W * H * 8 * 5 * M > 256 << 20
    s = _states(model, tracer, M, H, W, seed=41)
    c = g.Core(model, W, H, dx=DX, tracer=tracer, members=M, variant=g._lib.VARIANT_FUSED)
    c.set_state(**s)
    c.step(steps, DT)
    picks = {m: c.get_member(m) for m in (0, 17, 31)}
    assert c.diag(g._lib.DIAG_ANY_NAN) == 0.0
    c.close()
    for m, got in picks.items():
        one = _single(g, model, tracer, g._lib.VARIANT_FUSED, W, H, _member(s, m), steps)
        for f, (a, b) in enumerate(zip(got, one)):
            if b is not None:
                assert np.array_equal(a, b), (m, "puvtq"[f], rel_err(a, b))


def test_batched_drop_ins(g):
    from gcmiipy_amd import ensemble
    from gcmiipy_amd.matsuno_c_grid import matsumo_scheme, courant_number
    from gcmiipy_amd.matsumo_temp import matsumo_scheme_with_tracer
    W, H, M = 97, 61, 3
    s = _states(1, 0, M, H, W, seed=51)
    un, vn, pn = ensemble.matsumo_scheme(s["u"], s["v"], s["p"], DX, DT)
    for m in range(M):
        for a, b in zip((un, vn, pn), matsumo_scheme(s["u"][m], s["v"][m], s["p"][m], DX, DT)):
            assert rel_err(a[m], b) < TOL
    cn = ensemble.courant_numbers(s["p"], s["u"], DX, DT)
    for m in range(M):
        assert abs(cn[m] - courant_number(s["p"][m], s["u"][m], DX, DT)) <= 1e-12 * cn[m]
    t = _states(2, 2, M, H, W, seed=52)
    out = ensemble.matsumo_temp_scheme(t["u"], t["v"], t["p"], t["t"], DX, DT, q=t["q"], tracer="van_leer")
    for m in range(M):
        ref = matsumo_scheme_with_tracer(t["u"][m], t["v"][m], t["p"][m], t["t"][m], t["q"][m], DX, DT)
        for a, b in zip(out, ref):
            assert rel_err(a[m], b) < TOL
    seen = []
    res = ensemble.run(s["u"], s["v"], s["p"], DX, DT, 6, callback=lambda i, u, v, p: seen.append((i, u.shape)),
                       every=2)
    assert seen == [(2, (M, H, W)), (4, (M, H, W)), (6, (M, H, W))]
    for m in range(M):
        st = (s["u"][m], s["v"][m], s["p"][m])
        for _ in range(6):
            st = matsumo_scheme(*st, DX, DT)
        for a, b in zip(res, st):
            assert rel_err(a[m], b) < TOL
    g.clear_cache()


def test_batched_drop_ins_one_member(g):
    """(1, H, W) input is a one-member ensemble: the results keep the member axis and equal the 2-D drop-ins'"""
    from gcmiipy_amd import ensemble
    from gcmiipy_amd.matsuno_c_grid import matsumo_scheme, courant_number
    from gcmiipy_amd.matsumo_temp import matsumo_scheme_with_tracer
    W, H = 97, 61
    s = _states(1, 0, 1, H, W, seed=61)
    out = ensemble.matsumo_scheme(s["u"], s["v"], s["p"], DX, DT)
    for a, b in zip(out, matsumo_scheme(s["u"][0], s["v"][0], s["p"][0], DX, DT)):
        assert a.shape == (1, H, W) and np.array_equal(a[0], b)
    cn = ensemble.courant_numbers(s["p"], s["u"], DX, DT)
    assert cn.shape == (1,) and cn[0] == courant_number(s["p"][0], s["u"][0], DX, DT)
    t = _states(2, 2, 1, H, W, seed=62)
    out = ensemble.matsumo_temp_scheme(t["u"], t["v"], t["p"], t["t"], DX, DT, q=t["q"])
    ref = matsumo_scheme_with_tracer(t["u"][0], t["v"][0], t["p"][0], t["t"][0], t["q"][0], DX, DT)
    for a, b in zip(out, ref):
        assert a.shape == (1, H, W) and np.array_equal(a[0], b)
    seen = []
    res = ensemble.run(t["u"], t["v"], t["p"], DX, DT, 4, t=t["t"], q=t["q"],
                       callback=lambda i, *st: seen.append([x.shape for x in st]), every=2)
    assert seen == [[(1, H, W)] * 5] * 2 and all(x.shape == (1, H, W) for x in res)
    g.clear_cache()


def test_refusals_on_device(g):
    from gcmiipy_amd import geometry
    geom = geometry.gen_geometry(12, 20, 5, sig_func=geometry.manabe_sig)
    with pytest.raises(g.GcmError, match="members"):
        g.Core(g._lib.PE25D, 20, 12, 5, geom=geom, members=2)
    with pytest.raises(g.GcmError, match="members"):
        g.Core(g._lib.PE2D, 20, 12, dx=DX, members=2)
    c = g.Core(g._lib.SW2D, 20, 12, dx=DX, members=3)
    z = np.zeros((12, 20))
    rc = g._lib.lib.gcm_set_member(c._h, 3, z.ctypes.data, None, None, None, None)
    assert rc == g._lib.ERR_ARG
    assert g._lib.lib.gcm_members(c._h) == 3
    c.close()
