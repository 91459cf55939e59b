"""The zonal-mean climatology of GCM_PE25D without a device: the NumPy restatement tests/pe25d_climate_ref.py against
plain means, the derived properties of the Climate record on a planted wave, merge_climate, the C surface and the
checkpoint's four keys."""
import os
import re

import numpy as np
import pytest

import pe25d_climate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gcm_set_climate", "gcm_climate_every", "gcm_climate_sample", "gcm_climate_reset", "gcm_get_climate",
                "gcm_put_climate")


def random_state(H, W, L, seed=3):
    rng = np.random.default_rng(seed)
    p = 1e5 + 100 * rng.standard_normal((H, W))
    u, v = 8 * rng.standard_normal((L, H, W)), 8 * rng.standard_normal((L, H, W))
    t = 300 + 5 * rng.standard_normal((L, H, W))
    sig = (np.arange(L) + 0.5) / L
    return p, u, v, t, sig


@pytest.mark.parametrize("W", [10, 70, 130, 300, 1440])
def test_restatement_means_equal_plain_means(W):
    """a reordered sum of W float64 terms differs from another order by at most (W - 1) 2^-53 sum|term| each: the two
    means agree within W 2^-52 mean|term|, for every moment"""
    H, L = 5, 3
    p, u, v, t, sig = random_state(H, W, L)
    for ptop in (0.0, 1000.0):
        t3, t2 = ref.terms(p, u, v, t, sig, ptop)
        m3, m2 = ref.sample(p, u, v, t, sig, ptop)
        for w, (x, s) in enumerate(zip(t3 + t2, list(m3) + list(m2))):
            tol = W * 2.0 ** -52 * np.mean(np.abs(x), axis=-1)
            assert np.all(np.abs(s / W - np.mean(x, axis=-1)) <= tol), (w, W, ptop)


def test_row_sum_order_is_the_documented_one():
    """one row of 300 terms by hand: lane t holds x[t] + x[t + 256] for t < 44; the butterfly; the four waves in order"""
    x = np.random.default_rng(5).standard_normal(300) * 10.0 ** np.random.default_rng(6).integers(-8, 8, 300)
    lane = np.zeros(256)
    for t in range(256):
        lane[t] = 0.0 + x[t]
        if t + 256 < 300:
            lane[t] = lane[t] + x[t + 256]
    waves = []
    for w in range(4):
        a = lane[64 * w: 64 * w + 64].copy()
        for d in (32, 16, 8, 4, 2, 1):
            a = np.array([a[i] + a[i ^ d] for i in range(64)])
        assert np.all(a == a[0])
        waves.append(a[0])
    want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert ref.row_sum(x) == want
    assert ref.row_sum(x[None, None])[0, 0] == want


def test_accumulate_adds_in_sample_order():
    H, W, L = 4, 20, 2
    sts = [random_state(H, W, L, seed)[:4] for seed in (1, 2, 3)]
    sig = random_state(H, W, L)[4]
    n, m3, m2 = ref.accumulate(sts, sig, 0.0)
    parts = [ref.sample(*st, sig, 0.0) for st in sts]
    assert n == 3
    assert np.array_equal(m3, (parts[0][0] + parts[1][0]) + parts[2][0])
    assert np.array_equal(m2, (parts[0][1] + parts[1][1]) + parts[2][1])


@pytest.mark.parametrize("m,W", [(1, 36), (3, 36), (5, 130)])
def test_planted_wave_gives_the_analytic_eddy_fluxes(m, W):
    """u = U(k, j) + A cos(2 pi m i / W), v = B cos(2 pi m i / W + phi), constant in j.  u sits half a cell east of the
    cell centre: uc = U + A cos(pi m / W) cos(2 pi m i / W - pi m / W), vc = v, so
        [u'v'] = 1/2 A B cos(pi m / W) cos(phi + pi m / W)
    -- 1/2 A B cos(phi') cos(pi m / W) with phi' = phi + pi m / W, the phase between the two waves at the cell centre
    -- and eke = 1/4 (A^2 + B^2), up to rounding"""
    from gcmiipy_amd import Climate
    H, L = 6, 3
    A, B, phi = 7.0, 3.0, 0.4
    th = 2 * np.pi * m * np.arange(W) / W
    U = 10.0 + np.arange(L)[:, None, None] + 0.5 * np.arange(H)[None, :, None]
    u = U + A * np.cos(th)[None, None, :]
    v = np.broadcast_to(B * np.cos(th + phi), (L, H, W)).copy()
    p = np.full((H, W), 1e5)
    t = np.full((L, H, W), 300.0)
    sig = (np.arange(L) + 0.5) / L
    m3, m2 = ref.sample(p, u, v, t, sig, 0.0)
    c = Climate.from_sums(2, m3 + m3, m2 + m2, W)
    assert c.n == 2 and c.u.shape == (L, H) and c.p.shape == (H,)
    want = 0.5 * A * B * np.cos(np.pi * m / W) * np.cos(phi + np.pi * m / W)
    scale = (np.max(np.abs(U)) + A) * B
    assert np.max(np.abs(c.eddy_momentum_flux - want)) <= 64 * 2.0 ** -52 * scale
    assert np.max(np.abs(c.u - U[..., 0])) <= 64 * 2.0 ** -52 * np.max(np.abs(U))
    assert np.max(np.abs(c.v)) <= 64 * 2.0 ** -52 * B
    assert np.max(np.abs(c.eke - 0.25 * (A * A + B * B))) <= 64 * 2.0 ** -52 * (np.max(np.abs(U)) + A) ** 2
    # T is constant along a row: no eddy heat flux, no variance
    T = c.T
    assert np.max(np.abs(c.eddy_heat_flux)) <= 64 * 2.0 ** -52 * B * np.max(T)
    assert np.max(np.abs(c.T_variance)) <= 64 * 2.0 ** -52 * np.max(T) ** 2
    assert np.allclose(c.p, 1e5, rtol=1e-15) and np.allclose(c.pp, 1e10, rtol=1e-15)


def test_no_samples_give_nan_means():
    from gcmiipy_amd import Climate
    c = Climate.from_sums(0, np.zeros((10, 2, 3)), np.zeros((2, 3)), 8)
    assert c.n == 0 and np.isnan(c.u).all() and np.isnan(c.p).all()


def test_merge_climate_of_a_row_split_equals_the_whole():
    from gcmiipy_amd import Climate
    from gcmiipy_amd.bands import merge_climate, split_rows
    H, W, L = 24, 36, 4
    p, u, v, t, sig = random_state(H, W, L)
    m3, m2 = ref.sample(p, u, v, t, sig, 0.0)
    whole = Climate.from_sums(1, m3, m2, W)
    parts = []
    for row0, n in split_rows(H, 3):
        sl = slice(row0, row0 + n)
        north = v[:, row0 - 1, :]                               # (row0 = 0: the last row, the roll of the single domain)
        a, b = ref.sample(p[sl], u[:, sl], v[:, sl], t[:, sl], sig, 0.0, v_north=north)
        parts.append(Climate.from_sums(1, a, b, W))
    merged = merge_climate(parts)
    assert merged.n == 1
    for f, a, b in zip(Climate._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b), f
    with pytest.raises(ValueError):
        merge_climate([parts[0], parts[1]._replace(n=2)])
    with pytest.raises(ValueError):
        merge_climate([])


def test_header_declares_the_contract():
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    assert re.search(r"#define\s+GCM_CLIM_WORDS3\s+10\b", text) and re.search(r"#define\s+GCM_CLIM_WORDS2\s+2\b", text)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_symbols_exist_and_refuse_a_null_handle():
    import ctypes as C
    import gcmiipy_amd as g
    lib = g._lib.lib
    for name in ENTRY_POINTS:
        assert name in g._lib.SYMBOLS and hasattr(lib, name), name
    assert (g._lib.CLIM_WORDS3, g._lib.CLIM_WORDS2) == (len(ref.WORDS3), len(ref.WORDS2)) == (10, 2)
    m3, m2, n = np.zeros(10), np.zeros(2), C.c_int64(7)
    dp = g._lib._dp
    assert lib.gcm_set_climate(None, 1) == g._lib.ERR_ARG
    assert lib.gcm_get_climate(None, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), C.byref(n)) == g._lib.ERR_ARG
    assert lib.gcm_put_climate(None, m3.ctypes.data_as(dp), m2.ctypes.data_as(dp), 1) == g._lib.ERR_ARG
    assert lib.gcm_climate_sample(None) == g._lib.ERR_ARG and lib.gcm_climate_reset(None) == g._lib.ERR_ARG
    assert lib.gcm_climate_every(None) == g._lib.ERR_ARG
    assert n.value == 7 and not m3.any()
    from gcmiipy_amd.core import CLIMATE_WORDS3, CLIMATE_WORDS2
    assert CLIMATE_WORDS3 == ref.WORDS3 and CLIMATE_WORDS2 == ref.WORDS2
    assert g.Climate._fields == ("n",) + ref.WORDS3 + ref.WORDS2


class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    tracer_count = 0
    held_suarez = None

    def __init__(self, model, L, H, W, every=0, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.climate_every, self.sums = every, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def climate_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_climate(self, every):
        self.climate_every, self.sums = every, None

    def put_climate(self, n, m3, m2):
        self.sums = (n, m3, m2)


def test_checkpoint_round_trip_of_the_four_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    L, H, W = 3, 4, 6
    rng = np.random.default_rng(9)
    sums = (5, rng.standard_normal((10, L, H)), rng.standard_normal((2, H)))
    path = str(tmp_path / "clim.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, every=8, sums=sums), step=40)
    d = np.load(path)
    assert {"climate_every", "climate_n", "climate_m3", "climate_m2"} <= set(d.files)
    ck = checkpoint.load(path)
    assert ck["climate"]["every"] == 8 and ck["climate"]["n"] == 5
    assert np.array_equal(ck["climate"]["m3"], sums[1]) and np.array_equal(ck["climate"]["m2"], sums[2])
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.climate_every == 8 and core.sums[0] == 5
    assert np.array_equal(core.sums[1], sums[1]) and np.array_equal(core.sums[2], sums[2])
    # a file without the keys restores without a climatology
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("climate_") for k in np.load(path).files)
    assert checkpoint.load(path)["climate"] is None
    core, _ = checkpoint.restore(path)
    assert core.climate_every == 0 and core.sums is None


def test_run_model_takes_climate():
    import inspect
    from gcmiipy_amd import no_limits_2_5d
    assert inspect.signature(no_limits_2_5d.run_model).parameters["climate"].default == 0
