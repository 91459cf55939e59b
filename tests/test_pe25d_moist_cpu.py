"""The moist physics of GCM_PE25D without a GPU: the symbols and the struct of include/gcmcore.h, the handle-free
saturation probe gcm_moist_saturation against the NumPy restatement (tests/pe25d_moist_ref.py) and against humidity.py,
every validation error a call can report without a device, the restatement's own properties, the conditions the humid
inputs of the GPU tests must meet, merge_moist and the checkpoint keys.  What needs a handle:
tests/test_pe25d_moist_gpu.py and tests/test_pe25d_column_phases_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pe25d_moist_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gcm_set_moist", "gcm_moist_on", "gcm_moist_step", "gcm_get_moist", "gcm_put_moist", "gcm_moist_reset",
       "gcm_moist_saturation")
CASES = [(s, ptop) for s in ref.SHAPES for ptop in ref.PTOPS]


def _geom(H, W, L, ptop=0.0):
    from gcmiipy_amd import geometry
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.ptop = ptop
    return geom


def _applied(shape, ptop, dtype="f64", isothermal=False, **over):
    geom = _geom(*shape, ptop)
    st = ref.humid_state(geom, dtype, isothermal)
    par = ref.params(**over)
    out = ref.moist_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, 600.0, par, dtype)
    return geom, st, par, out


def test_symbols_are_exported_and_bound():
    from gcmiipy_amd import _lib
    import gcmiipy_amd
    raw = ctypes.CDLL(_lib.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert callable(gcmiipy_amd.moist_saturation)
    for name in ("set_moist", "moist", "moist_step", "moist_sums", "put_moist", "moist_reset"):
        assert hasattr(gcmiipy_amd.Core, name), name
    assert gcmiipy_amd.Moist._fields == ("nsteps", "seconds", "precip", "evap")
    from gcmiipy_amd.bands import HipBandEngine, merge_moist
    assert callable(merge_moist) and hasattr(HipBandEngine, "set_moist")


def test_struct_layout_matches_header():
    """the ctypes mirror of gcm_moist follows the header field for field (the pattern of test_abi_cpu.py)"""
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import MOIST_DEFAULTS
    src = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    end = src.index("} gcm_moist;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if decl:
            fields += [n.split()[-1].strip() for n in decl.split(",")]
    assert fields == [f[0] for f in _lib.Moist._fields_] == list(MOIST_DEFAULTS)
    assert ctypes.sizeof(_lib.Moist) == 3 * 8
    assert dict(MOIST_DEFAULTS) == ref.DEFAULTS


def _grid():
    """T in [180, 320] K x p_lev in [50, 1.05e5] Pa; no point within 1e-6 of e_s = p_lev"""
    T = np.linspace(180.0, 320.0, 57)[:, None]
    pl = np.geomspace(50.0, 1.05e5, 41)[None, :]
    T, pl = (np.ascontiguousarray(a) for a in np.broadcast_arrays(T, pl))
    es = ref.saturation(T, pl)[0]
    assert np.min(np.abs(es / pl - 1.0)) >= 1e-6
    return T, pl


def test_saturation_probe_equals_the_restatement():
    """can identical; q_s and dq_s within 1e-13 relative: |a b| < 25, so an ulp between two exp routines is a few 1e-15"""
    import gcmiipy_amd as g
    T, pl = _grid()
    qs, dqs, can = g.moist_saturation(T, pl)
    _, rqs, rdqs, rcan = ref.saturation(T, pl)
    assert np.array_equal(can, rcan) and can.any() and not can.all()
    assert np.max(np.abs(qs - rqs)[can] / rqs[can]) <= 1e-13
    assert np.max(np.abs(dqs - rdqs)[can] / np.abs(rdqs[can])) <= 1e-13
    assert not qs[~can].any() and not dqs[~can].any()
    assert (qs[can] > 0).all() and (dqs[can] > 0).all()


def test_saturation_equals_humidity_py():
    import gcmiipy_amd as g
    from gcmiipy_amd import humidity
    T, pl = _grid()
    qs, _, can = g.moist_saturation(T, pl)
    want = humidity.rh_to_mmr(1.0, pl, T)
    assert np.max(np.abs(qs - want)[can] / want[can]) <= 1e-13
    assert np.array_equal(ref.saturation(T, pl)[0], humidity.saturation_vapor_pressure(T))


def test_dq_s_is_the_derivative():
    T = np.linspace(200.0, 310.0, 23)
    h = 1e-3
    for pl in (2e4, 1e5):
        _, lo, _, _ = ref.saturation(T - h, pl)
        _, hi, _, _ = ref.saturation(T + h, pl)
        _, _, dqs, can = ref.saturation(T, pl)
        assert can.all()
        assert np.max(np.abs((hi - lo) / (2 * h) - dqs) / dqs) < 1e-6


def test_validation_without_a_handle():
    import gcmiipy_amd as g
    lib, L = g._lib.lib, g._lib
    dp = L._dp
    good = L.Moist(2.5e6, 0.0, 0.8)
    a, n = np.zeros(4), ctypes.c_int64(7)
    sec = ctypes.c_double(3.0)
    assert lib.gcm_set_moist(None, ctypes.byref(good)) == L.ERR_ARG
    assert lib.gcm_set_moist(None, None) == L.ERR_ARG
    assert lib.gcm_moist_on(None) == L.ERR_ARG
    assert lib.gcm_moist_step(None, 60.0, ctypes.byref(good)) == L.ERR_ARG
    assert lib.gcm_get_moist(None, a.ctypes.data_as(dp), a.ctypes.data_as(dp), ctypes.byref(sec), ctypes.byref(n)) == L.ERR_ARG
    assert lib.gcm_put_moist(None, a.ctypes.data_as(dp), a.ctypes.data_as(dp), 1.0, 1) == L.ERR_ARG
    assert lib.gcm_moist_reset(None) == L.ERR_ARG
    assert n.value == 7 and sec.value == 3.0 and not a.any()
    # the probe: a missing input is refused, missing outputs are not asked for
    assert lib.gcm_moist_saturation(2, None, a.ctypes.data_as(dp), None, None, None) == L.ERR_ARG
    assert lib.gcm_moist_saturation(-1, a.ctypes.data_as(dp), a.ctypes.data_as(dp), None, None, None) == L.ERR_ARG
    assert lib.gcm_moist_saturation(0, None, None, None, None, None) == L.OK
    T, pl, qs = np.full(2, 280.0), np.full(2, 9e4), np.zeros(2)
    assert lib.gcm_moist_saturation(2, T.ctypes.data_as(dp), pl.ctypes.data_as(dp), qs.ctypes.data_as(dp), None, None) == L.OK
    assert (qs > 0).all()


def test_python_layer_refuses_unknown_names():
    from gcmiipy_amd.core import MOIST_DEFAULTS, moist_params
    with pytest.raises(ValueError, match="tau"):
        moist_params(dict(tau=3.0))
    assert moist_params({}) == MOIST_DEFAULTS
    assert moist_params(dict(tau_e=86400))["tau_e"] == 86400.0
    import gcmiipy_amd as g
    with pytest.raises(ValueError):
        g.moist_saturation(np.zeros(3), np.zeros(4))


def test_moist_record_rates():
    import gcmiipy_amd as g
    m = g.Moist(3, 1800.0, np.full((2, 2), 9.0), np.full((2, 2), 0.9))
    assert np.array_equal(m.precip_rate(), np.full((2, 2), 9.0 / 1800.0))
    assert np.array_equal(m.evap_rate(), np.full((2, 2), 0.9 / 1800.0))
    with pytest.raises(ValueError):
        g.Moist(0, 0.0, np.zeros((2, 2)), np.zeros((2, 2))).precip_rate()


# ---------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("shape,ptop", CASES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_humid_inputs_keep_clear_of_saturation(shape, ptop, dtype):
    """the mask "condenses / does not" must not hang on the last bits of exp: a margin of 1e-3 on every state the GPU
    tests use, a third of the cells condensing, and guard cells on the top levels of the isothermal columns"""
    for iso in (False, True):
        geom = _geom(*shape, ptop)
        p, _, _, t, q = ref.humid_state(geom, dtype, iso)
        margin, share, guard = ref.conditions(p, t, q, geom.sig, ptop)
        assert margin >= 1e-3, (iso, margin)
        assert 0.25 <= share <= 0.45, (iso, share)
        if iso and shape in ((24, 36, 9), (5, 300, 42)):
            assert guard >= 0.05, guard
        assert (q > 0).all() and np.isfinite(t).all()


def test_level_next_to_the_surface_is_level_0():
    for shape in ref.SHAPES:
        assert int(np.argmax(np.asarray(_geom(*shape).sig).reshape(-1))) == 0


# ---------------------------------------------------------------- properties of the restatement
@pytest.mark.parametrize("shape,ptop", CASES)
@pytest.mark.parametrize("tau_e", [0.0, 86400.0])
def test_column_water_budget_closes(shape, ptop, tau_e):
    for iso in (False, True):
        geom, st, par, (tn, qn, P, E) = _applied(shape, ptop, isothermal=iso, tau_e=tau_e)
        before = ref.column_water(st[0], st[4], geom.dsig)
        after = ref.column_water(st[0], qn, geom.dsig)
        assert np.max(np.abs((before - after) - (P - E)) / before) <= 1e-14
        assert (P >= 0).all() and (E >= 0).all() and P.max() > 0
        assert (E.max() > 0) == (tau_e > 0)


@pytest.mark.parametrize("shape,ptop", CASES)
def test_column_moist_enthalpy_is_conserved(shape, ptop):
    for iso in (False, True):
        geom, st, par, (tn, qn, P, E) = _applied(shape, ptop, isothermal=iso)
        before = ref.column_enthalpy(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, par["Lv"])
        after = ref.column_enthalpy(st[0], tn, qn, geom.sig, geom.dsig, ptop, par["Lv"])
        assert np.max(np.abs(after - before) / before) <= 1e-14


@pytest.mark.parametrize("shape,ptop", CASES)
def test_never_above_saturation_and_the_undershoot(shape, ptop):
    geom, st, par, (tn, qn, P, E) = _applied(shape, ptop)
    p_lev, pi = ref.levels(st[0], geom.sig, ptop)
    _, qs0, _, can = ref.saturation(st[3] * pi, p_lev)
    _, qs1, _, _ = ref.saturation(tn * pi, p_lev)
    cond = can & (st[4] > qs0)
    assert (qn[cond] <= qs1[cond] * (1 + 1e-15)).all()
    assert (tn[cond] > st[3][cond]).all() and np.array_equal(tn[~cond], st[3][~cond]) and np.array_equal(qn[~cond], st[4][~cond])


def test_the_documented_undershoot():
    """the linearised step ends at or below saturation, by a second-order term: 1/2 (d2 ln q_s / dT2 + (d ln q_s / dT)^2)
    dT^2 with d ln q_s / dT <= 0.1 / K and a warming dT = (Lv / Cp) C <= 6.5 K for 40 % over at 250 .. 310 K: a few per
    cent of q_s at most (the header says up to 5 %), and 1.6e5 times less for an excess 400 times smaller"""
    for T0 in (250.0, 285.0, 300.0, 310.0):
        for plv in (9.5e4, 5e4):
            under = {}
            for over in (1.4, 1.001):
                pl = np.array([[plv]])
                pi = (plv / ref.P0) ** ref.KAPPA
                q0 = over * ref.saturation(T0, plv)[1]
                t1, q1, _, _ = ref.moist_step(pl, np.array([[[T0 / pi]]]), np.array([[[q0]]]), [1.0], [1.0], 0.0, 600.0, ref.params())
                under[over] = (1.0 - q1 / ref.saturation(t1 * pi, pl)[1]).item()
            assert 0.0 <= under[1.4] <= 0.05, (T0, plv, under)
            assert 0.0 <= under[1.001] <= 4e-7, (T0, plv, under)


@pytest.mark.parametrize("shape,ptop", CASES)
def test_unsaturated_state_is_untouched(shape, ptop):
    geom = _geom(*shape, ptop)
    st = ref.humid_state(geom)
    q = np.full_like(st[4], 3e-6)
    tn, qn, P, E = ref.moist_step(st[0], st[3], q, geom.sig, geom.dsig, ptop, 600.0, ref.params())
    assert np.array_equal(tn, st[3]) and np.array_equal(qn, q) and not P.any() and not E.any()


@pytest.mark.parametrize("shape,ptop", CASES)
def test_second_application_condenses_nothing_at_fp64(shape, ptop):
    for iso in (False, True):
        geom, st, par, (tn, qn, P, E) = _applied(shape, ptop, isothermal=iso)
        t2, q2, P2, E2 = ref.moist_step(st[0], tn, qn, geom.sig, geom.dsig, ptop, 600.0, par)
        assert np.array_equal(t2, tn) and np.array_equal(q2, qn) and not P2.any()


def test_evaporation_is_one_sided_and_leaves_theta():
    geom, st, par, (tn, qn, P, E) = _applied((24, 36, 9), 0.0, tau_e=86400.0)
    _, _, par0, (t0, q0, P0_, _) = _applied((24, 36, 9), 0.0)
    assert np.array_equal(tn, t0) and np.array_equal(P, P0_)
    assert np.array_equal(qn[1:], q0[1:]) and (qn[0] >= q0[0]).all() and (qn[0] > q0[0]).any()
    p_lev, pi = ref.levels(st[0], geom.sig, 0.0)
    q_eq = par["rh_s"] * ref.saturation(tn[0] * pi[0], p_lev[0])[1]
    moved = qn[0] > q0[0]
    assert (qn[0][moved] <= q_eq[moved]).all()


@pytest.mark.parametrize("shape,ptop", CASES[:2])
def test_f32_rounds_once(shape, ptop):
    geom = _geom(*shape, ptop)
    st = ref.humid_state(geom, "f32")
    par = ref.params(tau_e=86400.0)
    t32, q32, P32, E32 = ref.moist_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, 600.0, par, "f32")
    t64, q64, P64, E64 = ref.moist_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, 600.0, par, "f64")
    assert np.array_equal(t32, t64.astype(np.float32).astype(np.float64))
    assert np.array_equal(q32, q64.astype(np.float32).astype(np.float64))
    assert np.array_equal(P32, P64) and np.array_equal(E32, E64)


# ---------------------------------------------------------------- merge_moist and the checkpoint
def test_merge_moist_of_a_row_split_equals_the_whole():
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_moist, split_rows
    rng = np.random.default_rng(4)
    whole = g.Moist(5, 3000.0, rng.random((24, 6)), rng.random((24, 6)))
    parts = [g.Moist(5, 3000.0, whole.precip[r0:r0 + n], whole.evap[r0:r0 + n]) for r0, n in split_rows(24, 3)]
    got = merge_moist(parts)
    assert (got.nsteps, got.seconds) == (5, 3000.0)
    assert np.array_equal(got.precip, whole.precip) and np.array_equal(got.evap, whole.evap)
    with pytest.raises(ValueError):
        merge_moist([parts[0], parts[1]._replace(nsteps=4)])
    with pytest.raises(ValueError):
        merge_moist([parts[0], parts[1]._replace(seconds=2400.0)])
    with pytest.raises(ValueError):
        merge_moist([])


class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    tracer_count = 0
    held_suarez = None
    climate_every = 0

    def __init__(self, model, L, H, W, moist=None, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.moist, self.sums = moist, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def moist_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_moist(self, **params):
        self.moist, self.sums = params, None

    def put_moist(self, nsteps, seconds, precip, evap):
        import gcmiipy_amd as g
        self.sums = g.Moist(nsteps, seconds, precip, evap)


def test_checkpoint_round_trip_of_the_five_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.core import MOIST_DEFAULTS
    L, H, W = 3, 4, 6
    rng = np.random.default_rng(9)
    sums = g.Moist(7, 4200.0, rng.random((H, W)), rng.random((H, W)))
    par = dict(MOIST_DEFAULTS, tau_e=43200.0, rh_s=0.7)
    path = str(tmp_path / "moist.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, moist=par, sums=sums), step=40)
    d = np.load(path)
    assert {"moist", "moist_n", "moist_seconds", "moist_precip", "moist_evap"} <= set(d.files)
    assert list(d["moist"]) == [par[k] for k in MOIST_DEFAULTS]
    ck = checkpoint.load(path)
    assert ck["moist"]["params"] == par and ck["moist"]["n"] == 7 and ck["moist"]["seconds"] == 4200.0
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.moist == par and (core.sums.nsteps, core.sums.seconds) == (7, 4200.0)
    assert np.array_equal(core.sums.precip, sums.precip) and np.array_equal(core.sums.evap, sums.evap)
    # a file without the keys restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("moist") for k in np.load(path).files)
    assert checkpoint.load(path)["moist"] is None
    core, _ = checkpoint.restore(path)
    assert core.moist is None and core.sums is None


def test_checkpoint_refuses_a_phase_it_cannot_describe(tmp_path):
    """a phase registered through the C call directly has no parameters on the Python side: save raises instead of
    dropping the phase and its sums"""
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    core = _Recorded(g._lib.PE25D, 3, 4, 6)
    core.moist_registered = True
    with pytest.raises(g.GcmError, match="gcm_set_moist"):
        checkpoint.save(str(tmp_path / "x.npz"), core)
