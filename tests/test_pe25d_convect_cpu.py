"""The convective adjustment of GCM_PE25D without a GPU: the symbols and the struct of include/gcmcore.h, the handle-free
pooling probe gcm_convect_columns against the NumPy restatement (tests/pe25d_convect_ref.py) bit for bit, every
validation error a call can report without a device, the restatement's own properties, the conditions the unstable
inputs of the GPU tests must meet, merge_convect and the checkpoint keys.  What needs a handle:
tests/test_pe25d_convect_gpu.py and tests/test_pe25d_column_phases_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pe25d_convect_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gcm_set_convect", "gcm_convect_on", "gcm_convect_step", "gcm_get_convect", "gcm_put_convect", "gcm_convect_reset",
       "gcm_convect_columns")
KAPPAS = (0.0, ref.kappa_of(ref.GAMMA))                   # dry, and gamma = 6.5e-3
ALL = [(s, ptop, kc) for s in ref.SHAPES for ptop in ref.PTOPS for kc in KAPPAS]


def _geom(L, H, W, ptop=0.0):
    from gcmiipy_amd import geometry
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    geom.ptop = ptop
    return geom


_applied_cache = {}


def _applied(shape, ptop, kappa_c, dtype="f64", mix_q=1):
    """the restatement on the inputs of the GPU tests, computed once per case and left unchanged"""
    key = (shape, ptop, kappa_c, dtype, mix_q)
    if key not in _applied_cache:
        geom = _geom(*shape, ptop)
        st = ref.unstable_state(geom, kappa_c, dtype)
        stats = ref.PoolStats()
        out = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, ref.params(kappa_c=kappa_c, mix_q=mix_q), dtype,
                               stats)
        for a in list(st) + list(out):
            a.setflags(write=False)
        _applied_cache[key] = (geom, st, out, stats)
    return _applied_cache[key]


def test_symbols_are_exported_and_bound():
    from gcmiipy_amd import _lib
    import gcmiipy_amd
    raw = ctypes.CDLL(_lib.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert callable(gcmiipy_amd.convect_columns)
    for name in ("set_convect", "convect", "convect_step", "convect_sums", "put_convect", "convect_reset"):
        assert hasattr(gcmiipy_amd.Core, name), name
    assert gcmiipy_amd.Convect._fields == ("nsteps", "seconds", "count", "levels")
    from gcmiipy_amd.bands import HipBandEngine, merge_convect
    assert callable(merge_convect) and hasattr(HipBandEngine, "set_convect")


def test_struct_layout_matches_header():
    """the ctypes mirror of gcm_convect follows the header field for field (the pattern of test_abi_cpu.py)"""
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import CONVECT_DEFAULTS
    src = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    end = src.index("} gcm_convect;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if decl:
            fields += [(decl.split()[0], n.split()[-1].strip()) for n in decl.split(",")]
    assert [f[1] for f in fields] == [f[0] for f in _lib.Convect._fields_] == list(CONVECT_DEFAULTS)
    assert [f[0] for f in fields] == ["double", "int32_t"]
    assert [f[1] for f in _lib.Convect._fields_] == [ctypes.c_double, ctypes.c_int32]
    assert ctypes.sizeof(_lib.Convect) == 16 and _lib.Convect.mix_q.offset == 8
    assert dict(CONVECT_DEFAULTS) == ref.DEFAULTS


def test_validation_without_a_handle():
    import gcmiipy_amd as g
    lib, L = g._lib.lib, g._lib
    dp = L._dp
    good = L.Convect(0.0, 1)
    a, n = np.zeros(4), ctypes.c_int64(7)
    sec = ctypes.c_double(3.0)
    assert lib.gcm_set_convect(None, ctypes.byref(good)) == L.ERR_ARG
    assert lib.gcm_set_convect(None, None) == L.ERR_ARG
    assert lib.gcm_convect_on(None) == L.ERR_ARG
    assert lib.gcm_convect_step(None, ctypes.byref(good)) == L.ERR_ARG
    assert lib.gcm_get_convect(None, a.ctypes.data_as(dp), a.ctypes.data_as(dp), ctypes.byref(sec), ctypes.byref(n)) == L.ERR_ARG
    assert lib.gcm_put_convect(None, a.ctypes.data_as(dp), a.ctypes.data_as(dp), 1.0, 1) == L.ERR_ARG
    assert lib.gcm_convect_reset(None) == L.ERR_ARG
    assert n.value == 7 and sec.value == 3.0 and not a.any()
    # the probe: a missing input, a bad size or a bad switch is refused, missing outputs are not asked for
    y = np.array([3.0, 2.0, 1.0, 4.0])
    one = np.ones(4)
    out = np.zeros(4)
    args = [p.ctypes.data_as(dp) for p in (y, one, one, one)]
    assert lib.gcm_convect_columns(1, 4, None, *args[1:], 1, None, None, None) == L.ERR_ARG
    assert lib.gcm_convect_columns(1, 4, *args[:3], None, 1, None, None, None) == L.ERR_ARG
    assert lib.gcm_convect_columns(-1, 4, *args, 1, None, None, None) == L.ERR_ARG
    assert lib.gcm_convect_columns(1, 0, *args, 1, None, None, None) == L.ERR_ARG
    assert lib.gcm_convect_columns(1, 4, *args, 2, None, None, None) == L.ERR_ARG
    assert lib.gcm_convect_columns(0, 4, None, None, None, None, 1, None, None, None) == L.OK
    assert lib.gcm_convect_columns(1, 4, *args, 1, out.ctypes.data_as(dp), None, None) == L.OK
    assert np.array_equal(out, [2.0, 2.0, 2.0, 4.0])


def test_python_layer_refuses_unknown_names_and_two_profiles():
    from gcmiipy_amd.core import CONVECT_DEFAULTS, convect_params
    with pytest.raises(ValueError, match="kappa"):
        convect_params(dict(kappa=0.1))
    with pytest.raises(ValueError, match="not both"):
        convect_params(dict(gamma=6.5e-3, kappa_c=0.19))
    with pytest.raises(ValueError):
        convect_params(dict(mix_q=2))
    assert convect_params({}) == CONVECT_DEFAULTS
    assert convect_params(dict(gamma=None, kappa_c=None)) == CONVECT_DEFAULTS
    assert convect_params(dict(gamma=ref.GAMMA)) == dict(kappa_c=287.0 * 6.5e-3 / 9.8, mix_q=1)
    assert convect_params(dict(kappa_c=0.25, mix_q=False)) == dict(kappa_c=0.25, mix_q=0)
    assert list(convect_params(dict(mix_q=0, gamma=1e-3))) == list(CONVECT_DEFAULTS)
    import gcmiipy_amd as g
    with pytest.raises(ValueError):
        g.convect_columns(np.zeros((2, 3)), np.zeros((2, 4)), np.zeros((2, 3)), np.ones(3))
    with pytest.raises(ValueError):
        g.convect_columns(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.ones(4))


def test_convect_record_frequency_and_mean_depth():
    import gcmiipy_amd as g
    count = np.array([[0.0, 2.0], [4.0, 1.0]])
    levels = np.array([[0.0, 6.0], [10.0, 2.0]])
    c = g.Convect(4, 480.0, count, levels)
    assert np.array_equal(c.frequency, count / 4)
    assert np.array_equal(c.mean_depth, [[0.0, 3.0], [2.5, 2.0]])
    with pytest.raises(ValueError):
        g.Convect(0, 0.0, count, levels).frequency
    assert np.array_equal(g.Convect(0, 0.0, 0 * count, 0 * levels).mean_depth, np.zeros((2, 2)))


# ---------------------------------------------------------------- the probe against the restatement's pooling
def _probe_equals_ref(y, w, q, dsig, mix_q=1):
    import gcmiipy_amd as g
    got = g.convect_columns(y, w, q, dsig, mix_q)
    want = ref.pool(y, w, q, dsig, mix_q)
    for a, b, what in zip(got, want, ("y", "q", "nblock")):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), what
    return got


@pytest.mark.parametrize("L", [2, 5, 8, 24, 40])
@pytest.mark.parametrize("mix_q", [0, 1])
def test_probe_equals_the_restatement_on_random_columns(L, mix_q):
    rng = np.random.default_rng(100 + L)
    y = 300.0 + 2.0 * np.arange(L) + 3.0 * rng.standard_normal((200, L))
    w, q, dsig = 0.5 + rng.random((200, L)), rng.random((200, L)), 0.1 + rng.random(L)
    yo, qo, nb = _probe_equals_ref(y, w, q, dsig, mix_q)
    assert (nb > 1).any() and (np.diff(yo, axis=1) >= 0).all()
    assert np.array_equal(yo[nb == 1], y[nb == 1]) and np.array_equal(qo[nb == 1], q[nb == 1])
    if not mix_q:
        assert np.array_equal(qo, q)


def test_probe_edge_columns():
    one = np.ones((1, 4))
    ds = np.array([0.4, 0.3, 0.2, 0.1])
    # L = 1
    yo, qo, nb = _probe_equals_ref(np.array([[5.0]]), np.array([[2.0]]), np.array([[0.3]]), np.array([1.0]))
    assert yo.item() == 5.0 and qo.item() == 0.3 and nb.item() == 1
    # an already monotone column: output identical, nblock all 1
    y = np.array([[1.0, 2.0, 3.5, 7.0]])
    q = np.array([[0.4, 0.3, 0.2, 0.1]])
    yo, qo, nb = _probe_equals_ref(y, one, q, ds)
    assert np.array_equal(yo, y) and np.array_equal(qo, q) and (nb == 1).all()
    # a strictly decreasing column: one block
    y = np.array([[4.0, 3.0, 2.0, 1.0]])
    w = np.array([[1.0, 2.0, 3.0, 4.0]])
    yo, qo, nb = _probe_equals_ref(y, w, q, ds)
    assert (nb == 4).all() and len(set(yo[0])) == 1 and len(set(qo[0])) == 1
    assert yo[0, 0] == (((1.0 * 4.0 + 2.0 * 3.0) + 3.0 * 2.0) + 4.0 * 1.0) / (((1.0 + 2.0) + 3.0) + 4.0)
    assert qo[0, 0] == (((0.4 * 0.4 + 0.3 * 0.3) + 0.2 * 0.2) + 0.1 * 0.1) / (((0.4 + 0.3) + 0.2) + 0.1)
    # equal neighbours: not merged (the comparison is strict)
    y = np.array([[2.0, 2.0, 2.0, 3.0]])
    yo, qo, nb = _probe_equals_ref(y, w, q, ds)
    assert np.array_equal(yo, y) and np.array_equal(qo, q) and (nb == 1).all()
    # a push followed by two merges: 2 | 3 2.5 -> 2 | 2.75 2.75, then 0 pulls both blocks below it in
    y = np.array([[2.0, 3.0, 2.5, 0.0]])
    stats = ref.PoolStats()
    ref.pool(y, one, q, ds, 1, stats)
    assert stats.deep_pushes == 1 and stats.largest == 4
    yo, qo, nb = _probe_equals_ref(y, one, q, ds)
    assert (nb == 4).all() and (yo == 1.875).all()


def test_probe_with_a_nan_level_returns_and_handles_the_other_blocks():
    """a NaN compares false either way: it stays a block of its own, nothing merges across it, and the violations below
    and above it are pooled as usual"""
    nan = float("nan")
    y = np.array([[3.0, 1.0, nan, 5.0, 4.0, 9.0], [2.0, 1.0, 0.5, 7.0, 6.0, nan]])
    w = np.ones((2, 6))
    q = np.tile(np.array([0.6, 0.5, 0.4, 0.3, 0.2, 0.1]), (2, 1))
    yo, qo, nb = _probe_equals_ref(y, w, q, np.ones(6))
    assert np.array_equal(nb, [[2, 2, 1, 2, 2, 1], [3, 3, 3, 2, 2, 1]])
    assert np.array_equal(yo[0], [2.0, 2.0, nan, 4.5, 4.5, 9.0], equal_nan=True)
    assert np.isnan(yo[1, 5]) and np.isfinite(yo[1, :5]).all()


# ---------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_unstable_inputs_meet_their_conditions(dtype):
    """no parity test can pass by adjusting nothing or by sitting on a tie: every case adjusts a column and leaves one
    alone, 10 % .. 90 % of all columns are adjusted, the L = 24 shape has a block of 4 levels or more, some push is
    followed by more than one merge, and no comparison is closer than 1e-9 relative (a device Exner or exp an ulp off
    cannot flip a decision)"""
    adjusted = total = 0
    deep = 0
    for shape, ptop, kc in ALL:
        geom, st, (tn, qn, count, levels), stats = _applied(shape, ptop, kc, dtype)
        print(shape, ptop, kc, dtype, "adjusted", count.mean(), "largest", stats.largest, "deep pushes", stats.deep_pushes,
              "gap", stats.min_gap)
        assert count.max() == 1.0 and count.min() == 0.0, (shape, ptop, kc)
        assert (levels[count == 1.0] >= 2).all() and not levels[count == 0.0].any()
        assert stats.min_gap >= 1e-9, (shape, ptop, kc, stats.min_gap)
        if shape[0] == 24:
            assert stats.largest >= 4
        if shape == (8, 6, 70):
            assert stats.deep_pushes >= 1
        adjusted += count.sum()
        total += count.size
        deep += stats.deep_pushes
        assert (st[4] > 0).all() and (np.diff(st[4].mean(axis=(1, 2))) < 0).all()      # q: positive, decaying with height
    assert 0.10 <= adjusted / total <= 0.90, adjusted / total
    assert deep >= 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_quiet_inputs_are_stable(dtype):
    for shape, ptop, kc in ALL:
        geom = _geom(*shape, ptop)
        st = ref.unstable_state(geom, kc, dtype, stable=True)
        tn, qn, count, levels = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, ref.params(kappa_c=kc), dtype)
        assert np.array_equal(tn, st[3]) and np.array_equal(qn, st[4]) and not count.any() and not levels.any()


# ---------------------------------------------------------------- properties of the restatement
@pytest.mark.parametrize("shape,ptop,kc", ALL)
def test_output_is_monotone_and_conserves(shape, ptop, kc):
    geom, st, (tn, qn, count, levels), _ = _applied(shape, ptop, kc)
    y0, w, r = ref.compared(st[0], st[3], geom.sig, geom.dsig, ptop, kc)
    y1 = ref.compared(st[0], tn, geom.sig, geom.dsig, ptop, kc)[0]
    # non-decreasing in k: exactly where dry (the block's value is stored as it is), to the rounding of (value r) / r else
    slack = 0.0 if kc == 0.0 else 4 * np.finfo(np.float64).eps * np.max(np.abs(y1))
    assert (np.diff(y1, axis=0) >= -slack).all()
    assert (np.diff(y0, axis=0) < 0).any()
    h0 = ref.column_enthalpy(st[0], st[3], geom.sig, geom.dsig, ptop)
    h1 = ref.column_enthalpy(st[0], tn, geom.sig, geom.dsig, ptop)
    assert np.max(np.abs(h1 - h0) / h0) <= 1e-13
    w0, w1 = ref.column_water(st[4], geom.dsig), ref.column_water(qn, geom.dsig)
    assert np.max(np.abs(w1 - w0) / w0) <= 1e-13
    # stable columns come back bit for bit, and so does the stable part of any column
    quiet = count == 0.0
    assert quiet.any() and np.array_equal(tn[:, quiet], st[3][:, quiet]) and np.array_equal(qn[:, quiet], st[4][:, quiet])
    assert (tn != st[3]).any() and (qn != st[4]).any()
    assert np.array_equal((tn != st[3]).any(axis=0), count == 1.0)


@pytest.mark.parametrize("shape,ptop,kc", ALL)
def test_second_application(shape, ptop, kc):
    """bit-identical when dry (a block's levels are equal, and equal neighbours are not merged); otherwise (value r) / r
    is the value to an ulp, and what a second pooling does to such ties stays within 1e-13"""
    geom, st, (tn, qn, count, levels), _ = _applied(shape, ptop, kc)
    t2, q2, c2, l2 = ref.convect_step(st[0], tn, qn, geom.sig, geom.dsig, ptop, ref.params(kappa_c=kc))
    if kc == 0.0:
        assert np.array_equal(t2, tn) and np.array_equal(q2, qn) and not c2.any() and not l2.any()
    else:
        assert np.max(np.abs(t2 - tn)) / np.max(np.abs(tn)) <= 1e-13
        assert np.max(np.abs(q2 - qn)) / np.max(np.abs(qn)) <= 1e-13


@pytest.mark.parametrize("shape,ptop,kc", [c for c in ALL if c[0][0] <= 8])
def test_restatement_equals_the_pairwise_sweep(shape, ptop, kc):
    """the classic pairwise adjustment converges to the pooled profile: 200 sweeps agree to 1e-9 K at L <= 8 (blocks of
    at most 3 levels: the error shrinks by a constant factor a sweep)"""
    geom, st, (tn, qn, count, levels), _ = _applied(shape, ptop, kc)
    y0, w, r = ref.compared(st[0], st[3], geom.sig, geom.dsig, ptop, kc)
    yo = ref.pool(ref._cols(y0), ref._cols(w), ref._cols(st[4]), geom.dsig)[0]
    sweep = ref.pairwise(ref._cols(y0), ref._cols(w), 200)
    err = float(np.max(np.abs(sweep - yo)))
    print("pairwise", shape, ptop, kc, err)
    assert err <= 1e-9, err


@pytest.mark.parametrize("shape,ptop,kc", ALL[:4])
def test_mix_q_off_leaves_q(shape, ptop, kc):
    geom, st, (tn, qn, count, levels), _ = _applied(shape, ptop, kc)
    _, _, (t0, q0, c0, l0), _ = _applied(shape, ptop, kc, mix_q=0)
    assert np.array_equal(q0, st[4]) and np.array_equal(t0, tn) and np.array_equal(c0, count) and np.array_equal(l0, levels)


@pytest.mark.parametrize("shape,ptop,kc", ALL[:4])
def test_f32_rounds_once(shape, ptop, kc):
    geom = _geom(*shape, ptop)
    st = ref.unstable_state(geom, kc, "f32")
    par = ref.params(kappa_c=kc)
    t32, q32, c32, l32 = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, par, "f32")
    t64, q64, c64, l64 = ref.convect_step(st[0], st[3], st[4], geom.sig, geom.dsig, ptop, par, "f64")
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    assert np.array_equal(t32, f32(t64)) and np.array_equal(q32, f32(q64))
    assert np.array_equal(c32, c64) and np.array_equal(l32, l64)
    # stable columns are bit-identical in float32: they are not written
    quiet = c32 == 0.0
    assert quiet.any() and np.array_equal(t32[:, quiet], st[3][:, quiet]) and np.array_equal(q32[:, quiet], st[4][:, quiet])
    assert np.array_equal(t32[:, quiet].astype(np.float32), st[3][:, quiet].astype(np.float32))


# ---------------------------------------------------------------- merge_convect and the checkpoint
def test_merge_convect_of_a_row_split_equals_the_whole():
    import gcmiipy_amd as g
    from gcmiipy_amd.bands import merge_convect, split_rows
    rng = np.random.default_rng(4)
    whole = g.Convect(5, 3000.0, rng.integers(0, 6, (24, 6)).astype(float), rng.integers(0, 40, (24, 6)).astype(float))
    parts = [g.Convect(5, 3000.0, whole.count[r0:r0 + n], whole.levels[r0:r0 + n]) for r0, n in split_rows(24, 3)]
    got = merge_convect(parts)
    assert (got.nsteps, got.seconds) == (5, 3000.0)
    assert np.array_equal(got.count, whole.count) and np.array_equal(got.levels, whole.levels)
    with pytest.raises(ValueError):
        merge_convect([parts[0], parts[1]._replace(nsteps=4)])
    with pytest.raises(ValueError):
        merge_convect([parts[0], parts[1]._replace(seconds=2400.0)])
    with pytest.raises(ValueError):
        merge_convect([])


class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    tracer_count = 0
    held_suarez = None
    climate_every = 0
    moist = None

    def __init__(self, model, L, H, W, convect=None, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.convect, self.sums = convect, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def convect_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_convect(self, **params):
        self.convect, self.sums = params, None

    def put_convect(self, nsteps, seconds, count, levels):
        import gcmiipy_amd as g
        self.sums = g.Convect(nsteps, seconds, count, levels)


def test_checkpoint_round_trip_of_the_five_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.core import CONVECT_DEFAULTS
    L, H, W = 3, 4, 6
    rng = np.random.default_rng(9)
    sums = g.Convect(7, 4200.0, rng.integers(0, 8, (H, W)).astype(float), rng.integers(0, 20, (H, W)).astype(float))
    par = dict(CONVECT_DEFAULTS, kappa_c=ref.kappa_of(ref.GAMMA), mix_q=0)
    path = str(tmp_path / "convect.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, convect=par, sums=sums), step=40)
    d = np.load(path)
    assert {"convect", "convect_n", "convect_seconds", "convect_count", "convect_levels"} <= set(d.files)
    assert list(d["convect"]) == [par[k] for k in CONVECT_DEFAULTS]
    ck = checkpoint.load(path)
    assert ck["convect"]["params"] == par and ck["convect"]["n"] == 7 and ck["convect"]["seconds"] == 4200.0
    assert isinstance(ck["convect"]["params"]["mix_q"], int)
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.convect == par and (core.sums.nsteps, core.sums.seconds) == (7, 4200.0)
    assert np.array_equal(core.sums.count, sums.count) and np.array_equal(core.sums.levels, sums.levels)
    # a file without the keys restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("convect") for k in np.load(path).files)
    assert checkpoint.load(path)["convect"] is None
    core, _ = checkpoint.restore(path)
    assert core.convect is None and core.sums is None


def test_checkpoint_refuses_a_phase_it_cannot_describe(tmp_path):
    """a phase registered through the C call directly has no parameters on the Python side: save raises instead of
    dropping the phase and its sums"""
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    core = _Recorded(g._lib.PE25D, 3, 4, 6)
    core.convect_registered = True
    with pytest.raises(g.GcmError, match="gcm_set_convect"):
        checkpoint.save(str(tmp_path / "x.npz"), core)
