"""The convective mixing of the passive tracers of GCM_PE25D without a GPU: the symbols of include/gcmcore.h and their
bindings, the handle-free probe gcm_convect_tracer_columns against the NumPy restatement
(tests/pe25d_convect_tracers_ref.py) bit for bit, the properties the header states (a stable column's bits, the closed
column sum, a constant tracer, the maximum principle, a NaN level), every refusal a call can report without a device, the
conditions the inputs of the GPU tests must meet, and the checkpoint's key.  What needs a handle:
tests/test_pe25d_convect_tracers_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pe25d_convect_ref as cref
import pe25d_convect_tracers_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gcm_set_tracer_convect", "gcm_tracer_convected", "gcm_convect_tracer_columns")
LEVELS = (1, 2, 9, 24, 40)
NCOL = 120


def columns(L, kind, seed=0):
    """NCOL columns of L levels -> (y, w, dsig, c).  y is built from integers and quarters, so that no comparison of two
    levels is a near tie; a block's value S / Wt is compared too, so the weights are small integers and eighths.
    kind: "stable" (strictly increasing), "partly" (an increasing profile with integer noise: some columns stay stable,
    others pool a few levels), "wholly" (strictly decreasing: one block)"""
    rng = np.random.default_rng(1000 * L + seed)
    k = np.arange(L, dtype=np.float64)
    if kind == "stable":
        y = 300.0 + 2.0 * k + 0.25 * rng.integers(0, 4, (NCOL, L))
    elif kind == "partly":
        # (the 64ths differ between neighbouring levels: two levels are never equal)
        y = 300.0 + 2.0 * k + 0.25 * rng.integers(-24, 25, (NCOL, L)) + (k % 8) / 64.0
        y[::5] = 300.0 + 2.0 * k                                   # (every fifth column is stable)
    else:
        y = 400.0 - 2.0 * k - 0.25 * rng.integers(0, 4, (NCOL, L))
    w = 1.0 + 0.125 * rng.integers(0, 16, (NCOL, L))
    dsig = (1.0 + rng.integers(0, 8, L)) / 64.0
    c = 1.0 + rng.random((NCOL, L))
    return y, w, dsig, c


def probe(y, w, dsig, c):
    import gcmiipy_amd as g
    got, nb = g.convect_tracer_columns(y, w, dsig, c, nblock=True)
    want, want_nb = ref.tracer_columns(y, w, dsig, c)
    assert nb.dtype == np.int32 and np.array_equal(nb, want_nb)
    assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(g.convect_tracer_columns(y, w, dsig, c), got, equal_nan=True)
    return got, nb


# ---------------------------------------------------------------- the ABI
def test_symbols_are_declared_exported_and_bound():
    from gcmiipy_amd import _lib
    import gcmiipy_amd
    raw = ctypes.CDLL(_lib.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
    assert "int gcm_set_tracer_convect(gcm_handle *h, int tracer, int on);" in text
    assert "int gcm_tracer_convected(const gcm_handle *h, int tracer);" in text
    assert ("int gcm_convect_tracer_columns(int ncol, int L, const double *y, const double *w, const double *dsig, "
            "const double *c,") in text
    dp = _lib._dp
    assert _lib.SYMBOLS["gcm_set_tracer_convect"] == (ctypes.c_int, [_lib._H, ctypes.c_int, ctypes.c_int])
    assert _lib.SYMBOLS["gcm_tracer_convected"] == (ctypes.c_int, [_lib._H, ctypes.c_int])
    assert _lib.SYMBOLS["gcm_convect_tracer_columns"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp,
                                                                         ctypes.POINTER(ctypes.c_int)])
    assert callable(gcmiipy_amd.convect_tracer_columns) and "convect_tracer_columns" in gcmiipy_amd.__all__
    for name in ("set_tracer_convection", "tracer_convected", "tracer_convections"):
        assert hasattr(gcmiipy_amd.Core, name), name
    from gcmiipy_amd.bands import HipBandEngine
    assert hasattr(HipBandEngine, "set_tracer_convection")
    # the summation order is part of the contract, and the header says that it is not the adjustment's
    assert "NOT the" in text and "merge-tree order" in text


def test_refusals_without_a_device():
    """a null handle is GCM_ERR_ARG from both handle calls; a box without a GPU cannot make a handle at all, and says so
    (no CPU fallback) instead of crashing; the probe refuses a missing array and a bad size and needs no device"""
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    dp = L_._dp
    assert lib.gcm_set_tracer_convect(None, 0, 1) == L_.ERR_ARG
    assert lib.gcm_set_tracer_convect(None, -1, 0) == L_.ERR_ARG
    assert lib.gcm_tracer_convected(None, 0) == L_.ERR_ARG
    if g.device_count() == 0:
        from gcmiipy_amd import geometry
        geom = geometry.gen_geometry(24, 36, 9, sig_func=geometry.manabe_sig)
        with pytest.raises(g.GcmError, match="no CPU fallback"):
            g.Core(L_.PE25D, 36, 24, 9, geom=geom).set_tracer_convection(0)
    y, one, out = np.array([3.0, 2.0, 1.0, 4.0]), np.ones(4), np.zeros(4)
    a = [x.ctypes.data_as(dp) for x in (y, one, one, y)]
    o = out.ctypes.data_as(dp)
    for n in range(4):
        bad = list(a)
        bad[n] = None
        assert lib.gcm_convect_tracer_columns(1, 4, *bad, o, None) == L_.ERR_ARG
        assert b"gcm_convect_tracer_columns" in lib.gcm_last_error(None)
    assert lib.gcm_convect_tracer_columns(1, 4, *a, None, None) == L_.ERR_ARG
    assert lib.gcm_convect_tracer_columns(-1, 4, *a, o, None) == L_.ERR_ARG
    assert lib.gcm_convect_tracer_columns(1, 0, *a, o, None) == L_.ERR_ARG
    assert not out.any()
    assert lib.gcm_convect_tracer_columns(0, 4, None, None, None, None, None, None) == L_.OK
    assert lib.gcm_convect_tracer_columns(1, 4, *a, o, None) == L_.OK         # nblk may be null
    assert np.array_equal(out, [2.0, 2.0, 2.0, 4.0])
    with pytest.raises(ValueError):
        g.convect_tracer_columns(np.zeros((2, 3)), np.zeros((2, 4)), np.ones(3), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        g.convect_tracer_columns(np.zeros((2, 3)), np.zeros((2, 3)), np.ones(4), np.zeros((2, 3)))


# ---------------------------------------------------------------- the probe against the restatement
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("kind", ["stable", "partly", "wholly"])
def test_probe_equals_the_restatement_bit_for_bit(L, kind):
    y, w, dsig, c = columns(L, kind, seed=2)                  # (a seed whose pooling meets no tie at any L)
    stats = cref.PoolStats()
    _, nb0 = ref.tracer_columns(y, w, dsig, c, stats)
    if L > 1:
        assert stats.min_gap >= 1e-6, stats.min_gap          # (no comparison of the inputs is a near tie)
    got, nb = probe(y, w, dsig, c)
    merged = nb > 1
    if kind == "stable" or L == 1:
        assert not merged.any() and np.array_equal(got, c)
    elif kind == "wholly":
        assert (nb == L).all() and (got != c).any()
    else:
        per_col = merged.any(axis=1)
        assert per_col.any() and not per_col.all()            # some columns pool, every fifth is stable
        assert stats.largest >= min(3, L)
        if L > 2:
            assert not merged[per_col].all()                  # and a column that pools keeps unmerged levels
    # levels of unmerged blocks are copied: their bits are the input's
    assert np.array_equal(got[~merged], c[~merged])
    # the blocks are the adjustment's probe's: one routine
    import gcmiipy_amd as g
    assert np.array_equal(g.convect_columns(y, w, c, dsig)[2], nb)


@pytest.mark.parametrize("L", LEVELS)
def test_a_stable_column_comes_back_bit_identical(L):
    y, w, dsig, c = columns(L, "stable", seed=1)
    c[0, 0] = -0.0
    got, nb = probe(y, w, dsig, c)
    assert (nb == 1).all()
    assert got.tobytes() == c.tobytes()


@pytest.mark.parametrize("L", LEVELS[1:])
@pytest.mark.parametrize("kind", ["partly", "wholly"])
def test_column_sum_is_closed_and_the_range_does_not_widen(L, kind):
    """sum_k c dsig per column to 1e-12 relative; every output lies within its block's input range (the mean of
    non-negative weights, to the rounding of one division: the bound is taken with 4 ulp of the block's largest value)"""
    y, w, dsig, c = columns(L, kind, seed=2)
    got, nb = probe(y, w, dsig, c)
    before, after = (c * dsig).sum(axis=1), (got * dsig).sum(axis=1)
    rel = np.max(np.abs(after - before) / np.abs(before))
    print("column sum", L, kind, rel)
    assert rel <= 1e-12
    eps = np.finfo(np.float64).eps
    for col in range(NCOL):
        k = 0
        while k < L:
            n = int(nb[col, k])
            lo, hi = c[col, k:k + n].min(), c[col, k:k + n].max()
            assert (got[col, k:k + n] >= lo - 4 * eps * abs(hi)).all() and (got[col, k:k + n] <= hi + 4 * eps * abs(hi)).all()
            if n > 1:
                assert len(set(got[col, k:k + n].tolist())) == 1
            k += n


@pytest.mark.parametrize("L", LEVELS[1:])
def test_a_constant_tracer_stays_constant_to_one_ulp(L):
    """one block of L levels.  Where the products and both sums are exact -- the columns' own dsig, multiples of 1 / 64,
    and constants of a few bits -- the quotient is the constant to 1 ulp (it is exact).  With weights and constants
    that do round, n products and n - 1 additions of positive terms in Cs, n - 1 additions in D and one division each
    contribute at most one relative rounding u = 2^-53: |c_out / c - 1| <= (3 n) u to first order, asserted as such"""
    y, w, dsig, c = columns(L, "wholly", seed=3)
    for value in (1.0, 0.375, 7.0, 1024.5, -3.25):
        got, nb = probe(y, w, dsig, np.full_like(c, value))
        assert (nb == L).all()
        assert np.max(np.abs(got - value)) <= np.spacing(abs(value)), (L, value)
    rough = 0.01 + np.random.default_rng(5).random(L)
    u = 2.0 ** -53
    for value in (0.3, 1e-9, 7.77e5):
        got, nb = probe(y, w, rough, np.full_like(c, value))
        rel = np.max(np.abs(got / value - 1.0))
        print("constant", L, value, rel / u, "u")
        assert (nb == L).all() and rel <= 3 * L * u * (1 + 1e-6), (L, value, rel / u)


def test_nan_in_y_compares_false_and_neither_hangs_nor_merges():
    """a NaN level stays a block of its own; the violations below and above it are pooled as usual, and the tracer of the
    NaN level is not written"""
    nan = float("nan")
    y = np.array([[3.0, 1.0, nan, 5.0, 4.0, 9.0], [2.0, 1.0, 0.5, 7.0, 6.0, nan], [nan] * 6])
    w = np.ones((3, 6))
    c = np.tile(np.array([0.6, 0.5, 0.4, 0.3, 0.2, 0.1]), (3, 1))
    got, nb = probe(y, w, np.ones(6), c)
    assert np.array_equal(nb, [[2, 2, 1, 2, 2, 1], [3, 3, 3, 2, 2, 1], [1] * 6])
    assert np.array_equal(got[0], [0.55, 0.55, 0.4, 0.25, 0.25, 0.1])
    assert np.array_equal(got[2], c[2])
    # a NaN in the tracer stays in its block
    c2 = c.copy()
    c2[0, 3] = nan
    got2, _ = probe(y, w, np.ones(6), c2)
    assert np.isnan(got2[0, 3:5]).all() and np.isfinite(got2[0, :3]).all() and got2[0, 5] == 0.1


def test_the_sums_are_sequential_from_the_blocks_lowest_level():
    """the order is the contract: ((c0 d0 + c1 d1) + c2 d2) + c3 d3 over ((d0 + d1) + d2) + d3 -- not the order in which
    the adjustment's merges form Qs and D.  The column 2 | 3 2.5 | 0 merges the upper pair first, then the bottom, then
    the top: the adjustment's D is d0 + ((d1 + d2) + d3)"""
    y = np.array([[2.0, 3.0, 2.5, 0.0]])
    w = np.ones((1, 4))
    ds = np.array([0.1, 0.2, 0.3, 0.7])
    c = np.array([[0.1, 0.7, 0.3, 0.9]])
    got, nb = probe(y, w, ds, c)
    assert (nb == 4).all()
    cs = ((0.1 * 0.1 + 0.7 * 0.2) + 0.3 * 0.3) + 0.9 * 0.7
    d = ((0.1 + 0.2) + 0.3) + 0.7
    assert (got == cs / d).all()
    import gcmiipy_amd as g
    q_tree = g.convect_columns(y, w, c, ds, 1)[1]
    assert np.max(np.abs(q_tree - got)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(got))


# ---------------------------------------------------------------- the inputs of the GPU tests
GPU_SHAPES = ref.SHAPES


def gpu_inputs(shape, kappa_c, dtype="f64"):
    from gcmiipy_amd import geometry
    L, H, W = shape
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    return (geom,) + ref.inputs(geom, kappa_c, dtype)


@pytest.mark.parametrize("shape", GPU_SHAPES)
@pytest.mark.parametrize("kappa_c", [0.0, cref.kappa_of(cref.GAMMA)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_inputs_have_no_near_tie(shape, kappa_c, dtype):
    """the restatement alone has no near-tied comparison on the inputs of the GPU tests (no case there is skipped or
    filtered for one): the perturbations of theta are 3 K, far above 1e-3 K, and the smallest relative gap at any
    comparison made is above 1e-9, which a device Exner or exp an ulp off cannot flip.  Some columns are adjusted, some
    are not, and the mixing moves the tracers"""
    geom, st, trs = gpu_inputs(shape, kappa_c, dtype)
    stats = cref.PoolStats()
    out, merged = ref.mix_step(st[0], st[3], trs, (0, 2), geom.sig, geom.dsig, geom.ptop, kappa_c, dtype, stats)
    print(shape, kappa_c, dtype, "gap", stats.min_gap, "largest", stats.largest, "merged", merged.mean())
    assert stats.min_gap >= 1e-9
    cols = merged.any(axis=0)
    assert cols.any() and not cols.all()
    assert np.array_equal(out[1], trs[1]) and np.array_equal(out[:, ~merged], trs[:, ~merged])
    assert (out[0] != trs[0]).any() and (out[2] != trs[2]).any()


# ---------------------------------------------------------------- the checkpoint's key
class _Recorded:
    """what checkpoint.save asks of a core that carries tracers, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    held_suarez = None
    climate_every = 0

    def __init__(self, model, L, H, W, opted=(), with_method=True):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]
        self.tracers = np.arange(3.0 * L * H * W).reshape(3, L, H, W)
        self.tracer_count = 3
        self.opted = list(opted)
        if with_method:
            self.tracer_convections = lambda: sorted(self.opted)

    def get_state(self):
        return self.state

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def get_tracers(self):
        return self.tracers

    def set_tracers(self, c):
        self.tracers = c

    def tracer_forcings(self):
        return {}

    def tracer_mixings(self):
        return {}

    def set_tracer_convection(self, i, on=True):
        self.opted.append(i)


def test_checkpoint_carries_the_opt_ins_and_loads_a_file_without_them(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    L, H, W = 3, 4, 6
    path = str(tmp_path / "tracers.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, opted=(2, 0)), step=3)
    assert list(np.load(path)["tracer_convect"]) == [0, 2]
    assert checkpoint.load(path)["tracer_convect"] == [0, 2]
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.opted == [0, 2]
    # none opted in: no key; and a file written without the field (a core that knows nothing of it) loads with none
    for old in (_Recorded(g._lib.PE25D, L, H, W), _Recorded(g._lib.PE25D, L, H, W, with_method=False)):
        checkpoint.save(path, old, step=1)
        assert "tracer_convect" not in np.load(path).files
        assert checkpoint.load(path)["tracer_convect"] == []
        core, _ = checkpoint.restore(path)
        assert core.opted == [] and core.tracers.shape == (3, L, H, W)
