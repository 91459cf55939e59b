"""The zonal wavenumber spectra of GCM_PE25D without a device: the NumPy restatement tests/pe25d_spectra_ref.py against
the climatology's restatement (Parseval), the weights and the scaling of the Spectra record, merge_spectra, the C
surface and the checkpoint's four keys."""
import os
import re

import numpy as np
import pytest

import pe25d_climate_ref as clim
import pe25d_spectra_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gcm_set_spectra", "gcm_spectra_every", "gcm_spectra_mmax", "gcm_spectra_plan", "gcm_spectra_sample",
                "gcm_spectra_reset", "gcm_get_spectra", "gcm_put_spectra")


def random_state(H, W, L, seed=3):
    rng = np.random.default_rng(seed)
    p = 1e5 + 100 * rng.standard_normal((H, W))
    u, v = 8 * rng.standard_normal((L, H, W)), 8 * rng.standard_normal((L, H, W))
    t = 300 + 5 * rng.standard_normal((L, H, W))
    sig = (np.arange(L) + 0.5) / L
    return p, u, v, t, sig


@pytest.mark.parametrize("W", [10, 36, 70, 130, 300, 1440])
def test_restatement_obeys_parseval_against_the_climatology(W):
    """sum_m w_m Re(X_m conj Y_m) / W = sum_i x_i y_i: the one-sided sums of words 2 - 5 are the climatology's words
    6 - 9.  Both sides are float64 sums of W terms bounded by B_x B_y / W each way: within the parity bound's
    (8 eps log2 W) B_x B_y, without the Exner term (both take T from np.power)"""
    H, L = 5, 3
    p, u, v, t, sig = random_state(H, W, L)
    for ptop in (0.0, 1000.0):
        s, unit = ref.sample(p, u, v, t, sig, ptop, W // 2)
        m3, _ = clim.sample(p, u, v, t, sig, ptop)
        assert s.shape == (6, L, H, W // 2 + 1) and unit.shape == (6, L, H)
        wm, fac = ref.weights(W // 2 + 1, W), ref.bound_factor(W, exner=False)
        for w, cw in ref.CLIMATE_WORD.items():
            total = np.sum(s[w] * wm, axis=-1) / W
            assert np.all(np.abs(total - m3[cw]) <= fac[w] * unit[w]), (ref.WORDS[w], W, ptop)
            assert np.max(np.abs(total - m3[cw]) / np.abs(m3[cw]).max()) < 1e-12
        # the unit bounds every coefficient's product
        assert np.all(np.abs(s) <= unit[..., None] * (1 + 1e-14))


def test_restatement_truncates_and_takes_the_band_ghost_row():
    H, W, L = 6, 20, 2
    p, u, v, t, sig = random_state(H, W, L)
    full, _ = ref.sample(p, u, v, t, sig, 0.0, W // 2)
    low, _ = ref.sample(p, u, v, t, sig, 0.0, 3)
    assert np.array_equal(low, full[..., :4])
    sl = slice(2, 5)
    band, _ = ref.sample(p[sl], u[:, sl], v[:, sl], t[:, sl], sig, 0.0, 3, v_north=v[:, 1, :])
    assert np.array_equal(band, low[:, :, sl])
    n, s, unit = ref.accumulate([(p, u, v, t), (p, 2 * u, v, t)], sig, 0.0, 3)
    assert n == 2 and np.array_equal(s, low + ref.sample(p, 2 * u, v, t, sig, 0.0, 3)[0])
    assert ref.EXNER_FACTORS == (0, 0, 2, 0, 1, 0) and ref.WORDS == ("uu", "vv", "TT", "uv", "vT", "vtheta")
    f = ref.bound_factor(1440)
    assert f[0] == 8 * 2.0 ** -53 * np.log2(1440) and f[2] == f[0] + 2e-10 and f[4] == f[0] + 1e-10


def test_weights_and_the_scaling_of_the_record():
    from gcmiipy_amd import Spectra
    from gcmiipy_amd.core import SPECTRA_WORDS, spectra_weights
    assert SPECTRA_WORDS == ref.WORDS and Spectra._fields == ("n",) + ref.WORDS
    assert spectra_weights(6, 10).tolist() == [1, 2, 2, 2, 2, 1]          # m = 5 is the Nyquist wavenumber of W = 10
    assert spectra_weights(4, 10).tolist() == [1, 2, 2, 2]
    assert spectra_weights(6, 11).tolist() == [1, 2, 2, 2, 2, 2]          # an odd width has none
    assert spectra_weights(1, 10).tolist() == [1]
    for M, W in ((6, 10), (4, 10), (6, 11), (721, 1440)):
        assert np.array_equal(spectra_weights(M, W), ref.weights(M, W))
    H, W, L = 4, 10, 2
    p, u, v, t, sig = random_state(H, W, L)
    s, _ = ref.sample(p, u, v, t, sig, 0.0, W // 2)
    rec = Spectra.from_sums(3, 3 * s, W)
    assert rec.n == 3 and rec.uu.shape == (L, H, W // 2 + 1)
    for w, name in enumerate(ref.WORDS):
        assert np.array_equal(getattr(rec, name), (3 * s[w]) * (ref.weights(W // 2 + 1, W) / (10.0 * 10.0 * 3.0))), name
    # with all wavenumbers a row's entries sum to the zonal mean of the product
    uc, vc, th, T = ref.rows(p, u, v, t, sig, 0.0)
    assert np.allclose(rec.uv.sum(axis=-1), np.mean(uc * vc, axis=-1), rtol=0, atol=1e-12 * np.abs(uc * vc).max())
    assert np.allclose(rec.kinetic_energy.sum(axis=-1), 0.5 * np.mean(uc * uc + vc * vc, axis=-1), rtol=1e-13)
    none = Spectra.from_sums(0, np.zeros((6, 2, 3, 4)), 8)
    assert none.n == 0 and np.isnan(none.uu).all()


def test_merge_spectra_of_a_row_split_equals_the_whole():
    from gcmiipy_amd import Spectra
    from gcmiipy_amd.bands import merge_spectra, split_rows
    H, W, L, mmax = 24, 36, 4, 7
    p, u, v, t, sig = random_state(H, W, L)
    whole = Spectra.from_sums(1, ref.sample(p, u, v, t, sig, 0.0, mmax)[0], W)
    parts = []
    for row0, n in split_rows(H, 3):
        sl = slice(row0, row0 + n)
        north = v[:, row0 - 1, :]                               # (row0 = 0: the last row, the roll of the single domain)
        parts.append(Spectra.from_sums(1, ref.sample(p[sl], u[:, sl], v[:, sl], t[:, sl], sig, 0.0, mmax, v_north=north)[0], W))
    merged = merge_spectra(parts)
    assert merged.n == 1 and merged.uu.shape == (L, H, mmax + 1)
    for f, a, b in zip(Spectra._fields[1:], merged[1:], whole[1:]):
        assert np.array_equal(a, b), f
    with pytest.raises(ValueError):
        merge_spectra([parts[0], parts[1]._replace(n=2)])
    fewer = Spectra(1, *[a[..., :4] for a in parts[1][1:]])
    with pytest.raises(ValueError):
        merge_spectra([parts[0], fewer])
    with pytest.raises(ValueError):
        merge_spectra([])


def test_header_declares_the_contract():
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    assert re.search(r"#define\s+GCM_SPEC_WORDS\s+6\b", text) and re.search(r"#define\s+GCM_SPEC_PLAN_WORDS\s+6\b", text)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+GCM_ABI_VERSION\s+1\b", text)
    enum = re.search(r"typedef enum \{([^}]*)\} gcm_pe25d_phase;", text).group(1)
    assert len(re.findall(r"GCM_PHASE_[A-Z_]+ = \d+", enum)) == 4             # the spectra are no member of the phase enum


def test_symbols_exist_and_refuse_a_null_handle():
    import ctypes as C
    import gcmiipy_amd as g
    lib = g._lib.lib
    for name in ENTRY_POINTS:
        assert name in g._lib.SYMBOLS and hasattr(lib, name), name
    assert g._lib.SPEC_WORDS == len(ref.WORDS) == 6 and g._lib.SPEC_PLAN_WORDS == 6
    assert "Spectra" in g.__all__
    s, n = np.zeros(6), C.c_int64(7)
    out = (C.c_int * 6)()
    dp = g._lib._dp
    assert lib.gcm_set_spectra(None, 1, -1) == g._lib.ERR_ARG
    assert lib.gcm_get_spectra(None, s.ctypes.data_as(dp), C.byref(n)) == g._lib.ERR_ARG
    assert lib.gcm_put_spectra(None, s.ctypes.data_as(dp), 1) == g._lib.ERR_ARG
    assert lib.gcm_spectra_sample(None) == g._lib.ERR_ARG and lib.gcm_spectra_reset(None) == g._lib.ERR_ARG
    assert lib.gcm_spectra_every(None) == g._lib.ERR_ARG and lib.gcm_spectra_mmax(None) == g._lib.ERR_ARG
    assert lib.gcm_spectra_plan(None, out, 6) == g._lib.ERR_ARG
    assert n.value == 7 and not s.any() and not any(out)


class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    has_ground = False
    tracer_count = 0
    held_suarez = None
    climate_every = 0

    def __init__(self, model, L, H, W, every=0, mmax=0, sums=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.spectra_every, self.spectra_mmax, self.sums = every, mmax, sums
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]

    def get_state(self):
        return self.state

    def spectra_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_spectra(self, every, mmax=None):
        self.spectra_every, self.spectra_mmax, self.sums = every, mmax, None

    def put_spectra(self, n, s):
        self.sums = (n, s)


def test_checkpoint_round_trip_of_the_four_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    L, H, W = 3, 4, 6
    sums = (5, np.random.default_rng(9).standard_normal((6, L, H, 3)))
    path = str(tmp_path / "spec.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, every=8, mmax=2, sums=sums), step=40)
    d = np.load(path)
    assert {"spectra_every", "spectra_mmax", "spectra_n", "spectra_s"} <= set(d.files)
    assert not any(k.startswith("climate_") for k in d.files)
    ck = checkpoint.load(path)
    assert ck["spectra"]["every"] == 8 and ck["spectra"]["mmax"] == 2 and ck["spectra"]["n"] == 5
    assert np.array_equal(ck["spectra"]["s"], sums[1]) and ck["climate"] is None
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.spectra_every == 8 and core.spectra_mmax == 2 and core.sums[0] == 5
    assert np.array_equal(core.sums[1], sums[1])
    # a handle without spectra writes none of the keys, and such a file restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("spectra_") for k in np.load(path).files)
    assert checkpoint.load(path)["spectra"] is None
    core, _ = checkpoint.restore(path)
    assert core.spectra_every == 0 and core.sums is None


def test_run_model_and_the_band_engine_take_spectra():
    import inspect
    from gcmiipy_amd import bands, no_limits_2_5d
    assert inspect.signature(no_limits_2_5d.run_model).parameters["spectra"].default == 0
    assert list(inspect.signature(bands.HipBandEngine.set_spectra).parameters) == ["self", "every", "mmax"]
