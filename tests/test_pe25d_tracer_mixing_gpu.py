"""GPU tests of the implicit vertical mixing of the tracers of GCM_PE25D (gcm_set_tracer_mixing / Core.set_tracer_mixing):
the column solve on the device, once per Matsuno step behind the corrector and in front of the forcing.  The kernel
rounds every operation on its own and takes its tables from the routine the CPU tests pin, so the criterion is
np.array_equal throughout: with the NumPy restatement (tests/pe25d_tracer_mixing_ref.py, then the forcing's,
tests/pe25d_tracer_forcing_ref.py) applied on the host to an unmixed, unforced handle's result, with the get / mix /
force / set round trip per step, and -- on latitude bands, under every orchestration -- with the mixed single domain.
The band set-ups are those of tests/gpu_setups.py (in-process bands with device-copied ghost rows and
the loopback band of gcm_band_run): tests/band_engines.py holds NumPy engines of the dynamics without tracers, which
have nothing to drive here."""
import numpy as np
import pytest

import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from pe25d_tracer_forcing_ref import force
from pe25d_tracer_mixing_ref import column_sum_drift, mix, profile

pytestmark = pytest.mark.gpu
SCHEMES = ["centred", "upwind", "van_leer"]
NTR = 3                                                           # 0 mixed, 1 mixed and forced (a pin), 2 neither
DT = 120.0


def _setup(H, W, L):
    """-> geom, state, tracers (each with a gradient in the column), mixing {i: K}, forcing {i: record}"""
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, NTR)
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(1, L, 1, 1)
    trs = np.ascontiguousarray(trs * (0.5 + 2.0 * sig))
    k0 = int(np.argmax(np.asarray(geom.sig)))                     # the lowest level
    mask = np.zeros((L, H, W), dtype=bool)
    mask[k0] = True
    emission = np.zeros((L, H, W))
    emission[k0] = 1e-3 * np.random.default_rng(21).random((H, W))
    mixing = {0: profile(L, seed=1), 1: profile(L, seed=2, zero_at=(L - 1) // 2 if L >= 3 else None)}
    forcing = {1: dict(source=0.25, decay=1.0e-4, emission=emission, pin_mask=mask, pin_value=7.5)}
    return geom, st, trs, mixing, forcing


def _core(g, geom, st, trs, mixing=None, forcing=None, dtype="f64", scheme="van_leer"):
    c = su.single(g, geom, st, trs, recs=forcing, dtype=dtype, scheme=scheme)
    for i, k in (mixing or {}).items():
        c.set_tracer_mixing(i, k)
    return c


def _bands(g, geom, nb, st, trs, mixing, forcing, dtype="f64", scheme="van_leer", rows=2):
    cores = su.bands(g, geom, nb, st, trs, recs=forcing, dtype=dtype, scheme=scheme, rows=rows)
    for c in cores:
        for i, k in mixing.items():
            c.set_tracer_mixing(i, k)
    return cores


def _restate(tr, dt, geom, mixing, forcing, dtype):
    """mix, then force: the restatements on (n, L, H, W) float64 values that the type holds exactly"""
    out = tr.copy()
    for i, k in mixing.items():
        out[i] = mix(out[i], dt, k, geom.dsig, dtype)
    for i, rec in forcing.items():
        out[i] = force(out[i], dt, rec, dtype)
    return out


def _equal_state(a, b, what=""):
    for f in range(5):
        assert np.array_equal(a[f], b[f]), (what, "puvtq"[f])


def _single(g, geom, st, trs, mixing, forcing, steps, dt=DT, dtype="f64", scheme="van_leer", runs=None):
    one = _core(g, geom, st, trs, mixing, forcing, dtype, scheme)
    for n in (runs or [steps]):
        one.step(n, dt)
    out = one.get_state(), one.get_tracers()
    one.close()
    return out


# ---------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(24, 36, 9), (6, 10, 3)])
def test_one_step_bit_for_bit(g, shape, dtype, scheme):
    """handle A steps unmixed and unforced, and mix() then force() are applied to what it returns; handle B steps mixed
    and forced: equal bits.  Tracer 1's pinned level holds the pin's value (the forcing came last), the tracer that
    registered nothing has A's bits, and so have the state and the predictor's tracers"""
    H, W, L = shape
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    a = _core(g, geom, st, trs, None, None, dtype, scheme)
    b = _core(g, geom, st, trs, mixing, forcing, dtype, scheme)
    assert [b.tracer_mixing(i) is not None for i in range(NTR)] == [True, True, False]
    assert np.array_equal(b.get_tracers(), a.get_tracers())       # registering applies nothing
    a.step(1, DT)
    b.step(1, DT)
    ta, tb = a.get_tracers(), b.get_tracers()
    want = _restate(ta, DT, geom, mixing, forcing, dtype)
    for i in range(NTR):
        assert np.array_equal(tb[i], want[i]), (shape, dtype, scheme, "tracer", i)
    assert np.array_equal(tb[2], ta[2])
    assert not np.array_equal(tb[0], ta[0]) and not np.array_equal(tb[1], ta[1])
    assert np.all(tb[1][int(np.argmax(np.asarray(geom.sig)))] == 7.5)
    # (force, then mix would have smeared the pin)
    other = mix(force(ta[1], DT, forcing[1], dtype), DT, mixing[1], geom.dsig, dtype)
    assert not np.array_equal(other, want[1])
    _equal_state(b.get_state(), a.get_state(), (shape, dtype, scheme))
    # the two stages by hand: the predictor mixes nothing
    c = _core(g, geom, st, trs, mixing, forcing, dtype, scheme)
    t0 = c.get_tracers()
    c.half_step(0, DT)
    a.set_state(*st)
    a.set_tracers(trs)
    a.half_step(0, DT)
    assert np.array_equal(c.get_tracers(star=True), a.get_tracers(star=True))
    assert np.array_equal(c.get_tracers(), t0)
    c.half_step(1, DT)
    assert np.array_equal(c.get_tracers(), tb)
    for x in (a, b, c):
        x.close()


# ---------------------------------------------------------------- 2. n steps in one call, 4. another dt
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_five_steps_in_one_call_and_a_change_of_dt(g, dtype):
    """B runs step(5) in one call; A runs five rounds of step(1), get, mix, force, set_tracers.  The predictor that
    follows is the unmixed one.  Then both go on with another dt: the tables were built again"""
    H, W, L = 24, 36, 9
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    a = _core(g, geom, st, trs, None, None, dtype)
    b = _core(g, geom, st, trs, mixing, forcing, dtype)

    def rounds(n, dt):
        for _ in range(n):
            a.step(1, dt)
            a.set_tracers(_restate(a.get_tracers(), dt, geom, mixing, forcing, dtype))

    rounds(5, DT)
    b.step(5, DT)
    assert np.array_equal(b.get_tracers(), a.get_tracers())
    _equal_state(b.get_state(), a.get_state())
    before = b.get_tracers()
    a.half_step(0, DT)
    b.half_step(0, DT)
    assert np.array_equal(b.get_tracers(star=True), a.get_tracers(star=True))
    assert np.array_equal(b.get_tracers(), before)
    a.half_step(1, DT)
    a.set_tracers(_restate(a.get_tracers(), DT, geom, mixing, forcing, dtype))
    b.half_step(1, DT)
    assert np.array_equal(b.get_tracers(), a.get_tracers())
    t6 = b.get_tracers()
    rounds(2, 45.0)
    b.step(2, 45.0)
    tb = b.get_tracers()
    assert np.array_equal(tb, a.get_tracers())
    # (tables left at dt = 120 give other bits)
    assert not np.array_equal(mix(t6[0], DT, mixing[0], geom.dsig, dtype), mix(t6[0], 45.0, mixing[0], geom.dsig, dtype))
    rounds(1, DT)
    b.step(1, DT)
    assert np.array_equal(b.get_tracers(), a.get_tracers())
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. the level counts: the caps and the fallback
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("L", [2, 24, 25, 40, 41])
def test_level_counts_at_and_above_the_caps(g, L, dtype):
    """6 x 10 columns: L = 24 and 40 fill a register instantiation, 25 is the first of the second, 41 the first that
    parks y in c itself, 2 the fewest levels there are: two steps, the restatement's bits"""
    H, W = 6, 10
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    a = _core(g, geom, st, trs, None, None, dtype, "upwind")
    b = _core(g, geom, st, trs, mixing, forcing, dtype, "upwind")
    for _ in range(2):
        a.step(1, DT)
        a.set_tracers(_restate(a.get_tracers(), DT, geom, mixing, forcing, dtype))
    b.step(2, DT)
    ta, tb = a.get_tracers(), b.get_tracers()
    for i in range(NTR):
        assert np.array_equal(tb[i], ta[i]), (L, dtype, "tracer", i)
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. bands
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("mode", ["whole", "phase"])
def test_host_driven_mixed_bands_equal_single_domain(g, mode, nb):
    """host-driven bands with real neighbours, whole stages and edge-first phases.  The neighbour's ghost rows come
    from mixed and forced edge rows: one unmixed message would show after a step"""
    import torch
    H, W, L, steps = 24, 36, 9, 3
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    want = _single(g, geom, st, trs, mixing, forcing, steps)
    cores = _bands(g, geom, nb, st, trs, mixing, forcing)
    if mode == "whole":
        su.whole_steps(cores, torch, steps, DT)
    else:
        su.phase_steps(cores, torch, steps, DT)
    su.assert_equal(su.gather(cores), want, (mode, nb))


def test_unsplittable_short_mixed_bands_equal_single_domain(g):
    """bands of 4 and 3 rows: the one tracer launch of the edge rows, and the mixing behind it"""
    import torch
    H, W, L, steps = 14, 20, 5, 3
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    want = _single(g, geom, st, trs, mixing, forcing, steps)
    cores = _bands(g, geom, 4, st, trs, mixing, forcing)
    assert sorted(c.H for c in cores) == [3, 3, 4, 4]
    su.phase_steps(cores, torch, steps, DT)
    su.assert_equal(su.gather(cores), want)


def test_mixed_bands_with_one_ghost_row_and_upwind(g):
    """band_tracer_rows=1 (the tracers' own row 0 then sits one row into a field) against rows=2 with van Leer above"""
    import torch
    H, W, L, steps = 24, 36, 9, 2
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    want = _single(g, geom, st, trs, mixing, forcing, steps, scheme="upwind")
    cores = _bands(g, geom, 3, st, trs, mixing, forcing, scheme="upwind", rows=1)
    su.phase_steps(cores, torch, steps, DT)
    su.assert_equal(su.gather(cores), want)


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mixed_band_run_loopback_equals_single_domain(g, dtype, overlap):
    """gcm_band_run with the loopback exchange at 24 x 36 x 9 (two tracer ghost rows, van Leer), runs of 3 + 2 steps
    and then one of another dt, with and without gcm_set_band_overlap"""
    import torch
    H, W, L = 24, 36, 9
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    ref = _core(g, geom, st, trs, mixing, forcing, dtype)
    ref.step(3, DT)
    ref.step(2, DT)
    ref.step(1, 45.0)
    want = ref.get_state(), ref.get_tracers()
    ref.close()
    c, eng, runner = su.loopback_band(g, torch, geom, NTR, dtype, scheme="van_leer", rows=2)
    assert runner.native
    if overlap:
        c.set_band_overlap(True)
    c.set_state(*st)
    c.set_tracers(trs)
    for i, rec in forcing.items():
        c.set_tracer_forcing(i, **rec)
    for i, k in mixing.items():
        c.set_tracer_mixing(i, k)
    for n, dt in ((3, DT), (2, DT), (1, 45.0)):
        runner.run(n, dt)
        torch.cuda.synchronize()
    got = c.get_state(), c.get_tracers()
    c.close()
    su.assert_equal(got, want, (dtype, overlap))


# ---------------------------------------------------------------- 6. the mass budget, through the monitor
def test_mass_budget_of_a_surface_heavy_tracer(g):
    """a tracer that decays upwards from the lowest level, K > 0, no forcing, donor-cell transport, ten steps, beside
    the same run without mixing.  The transport conserves the monitor's mass = sum c p dsig under every scheme, and the
    solve conserves each column's sum_k c dsig -- p is one number per column -- up to the drift the restatement shows:
    |mass_mixed - mass_plain| <= 8 x drift x mass, drift = the largest relative change of a column sum over ten
    restated solves of this tracer's own columns (column_sum_drift, computed here, not by the code under test).  The
    margin of 8 covers the order of the monitor's reduction and the rounding of the two transports, whose fields
    differ.  Figures of one run: drift 1.02e-15, so a bound of 8.2e-15 of the mass (1.45e-7 of 1.78e7); the two
    masses differed by 7.5e-9, 4.2e-16 of the mass"""
    H, W, L, steps = 24, 36, 9, 10
    geom, st, trs, _, _ = _setup(H, W, L)
    sig = np.asarray(geom.sig, dtype=np.float64)
    heavy = np.exp(-(sig.max() - sig) / 0.15).reshape(L, 1, 1) * (1.0 + 0.5 * np.random.default_rng(4).random((L, H, W)))
    trs = np.ascontiguousarray(np.stack([heavy, heavy]))
    k = profile(L, seed=7)
    assert np.all(k > 0)
    a = su.single(g, geom, st, trs, scheme="upwind")
    b = su.single(g, geom, st, trs, scheme="upwind")
    b.set_tracer_mixing(0, k)
    a.step(steps, DT)
    b.step(steps, DT)
    sa, sb = a.tracer_stats(), b.tracer_stats()
    drift = column_sum_drift(heavy, DT, k, geom.dsig, "f64", steps)
    bound = 8 * drift * sa.mass[0]
    diff = abs(sb.mass[0] - sa.mass[0])
    print("mass plain %.17e mixed %.17e, |difference| %.3e, drift %.3e, bound %.3e" % (sa.mass[0], sb.mass[0], diff, drift, bound))
    assert drift > 0
    assert diff <= bound
    assert sb.negative[0] == 0 and sa.negative[0] == 0 and sb.nan[0] == 0
    assert sb.mass[1] == sa.mass[1]                               # the unmixed twin
    ca, cb = a.get_tracers(), b.get_tracers()
    assert np.array_equal(cb[1], ca[1]) and not np.array_equal(cb[0], ca[0])
    top, bottom = int(np.argmin(sig)), int(np.argmax(sig))
    assert cb[0][top].mean() > ca[0][top].mean() and cb[0][bottom].mean() < ca[0][bottom].mean()   # mixed upwards
    a.close()
    b.close()


# ---------------------------------------------------------------- 7. life cycle and refusals
def test_life_cycle_and_refusals(g):
    import ctypes as C
    from gcmiipy_amd import _lib
    lib = _lib.lib
    H, W, L = 12, 20, 5
    geom, st, trs, mixing, _ = _setup(H, W, L)
    c = _core(g, geom, st, trs, {1: mixing[1]})
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    good = mixing[0]
    mixed = lambda h, n=NTR: [lib.gcm_tracer_mixed(h._h, i) for i in range(n)]
    assert mixed(c) == [0, 1, 0]
    for i in (-1, NTR, 99):
        assert lib.gcm_tracer_mixed(c._h, i) == _lib.ERR_ARG
    # every refusal, and that it changed nothing
    for i in (-1, NTR, 99):
        assert lib.gcm_set_tracer_mixing(c._h, i, dp(good), L - 1) == _lib.ERR_ARG
    for i in (-2, NTR):
        assert lib.gcm_set_tracer_mixing(c._h, i, None, 0) == _lib.ERR_ARG
    for nk in (L, L - 2, 0):
        assert lib.gcm_set_tracer_mixing(c._h, 1, dp(np.resize(good, max(nk, 1))), nk) == _lib.ERR_ARG
    for bad in (np.nan, np.inf, -1e-12):
        k = good.copy()
        k[2] = bad
        assert lib.gcm_set_tracer_mixing(c._h, 1, dp(k), L - 1) == _lib.ERR_ARG, bad
        assert lib.gcm_set_tracer_mixing(c._h, 2, dp(k), L - 1) == _lib.ERR_ARG, bad
        with pytest.raises(ValueError):
            c.set_tracer_mixing(1, k)
    with pytest.raises(ValueError, match="k has shape"):
        c.set_tracer_mixing(1, np.zeros(L))
    assert mixed(c) == [0, 1, 0]
    assert np.array_equal(c.tracer_mixing(1), mixing[1]) and c.tracer_mixing(2) is None   # the profile in force
    ref = _core(g, geom, st, trs, {1: mixing[1]})
    ref.step(1, DT)
    c.step(1, DT)
    assert np.array_equal(c.get_tracers(), ref.get_tracers())     # tracer 1 is mixed as registered, nothing else is
    # it survives set_tracers with the same count, a change of scheme and set_state
    c.set_tracers(trs)
    c.set_tracer_scheme("upwind")
    c.set_tracer_scheme("van_leer")
    c.set_state(*st)
    assert mixed(c) == [0, 1, 0]
    c.step(1, DT)
    assert np.array_equal(c.get_tracers(), ref.get_tracers())
    # an all-zero K is legal and is the identity; replacing a profile takes effect
    plain = _core(g, geom, st, trs)
    plain.step(1, DT)
    c.set_tracer_mixing(1, np.zeros(L - 1))
    c.set_tracers(trs)
    c.set_state(*st)
    c.step(1, DT)
    assert mixed(c) == [0, 1, 0] and np.array_equal(c.get_tracers(), plain.get_tracers())
    # clearing one, then all
    c.set_tracer_mixing(1, mixing[1])
    c.set_tracer_mixing(2, good)
    c.clear_tracer_mixing(1)
    assert mixed(c) == [0, 0, 1] and c.tracer_mixing(1) is None
    c.set_tracer_mixing(0, good)
    c.clear_tracer_mixing()
    assert mixed(c) == [0, 0, 0] and c.tracer_mixings() == {}
    c.set_tracers(trs)
    c.set_state(*st)
    c.step(1, DT)
    assert np.array_equal(c.get_tracers(), plain.get_tracers())   # cleared: the unmixed step
    # another count drops it
    c.set_tracer_mixing(0, good)
    c.set_tracers(trs[:2])
    assert mixed(c, 2) == [0, 0] and c.tracer_mixing(0) is None
    c.set_tracer_mixing(0, good)
    c.set_tracers(None)
    assert lib.gcm_tracer_mixed(c._h, 0) == _lib.ERR_ARG and c.tracer_count == 0
    assert lib.gcm_set_tracer_mixing(c._h, 0, dp(good), L - 1) == _lib.ERR_ARG       # no tracers: no index is valid
    assert lib.gcm_set_tracer_mixing(c._h, -1, None, 0) == _lib.OK
    for x in (c, ref, plain):
        x.close()
    # a band's reallocation drops it; the same depth again allocates nothing and keeps it
    band = g.Core(_lib.PE25D, W, 6, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, band_tracers=2)
    band.set_tracer_mixing(1, good)
    assert lib.gcm_tracer_mixed(band._h, 1) == 1
    assert lib.gcm_set_band_tracer_rows(band._h, 1) == _lib.OK and lib.gcm_tracer_mixed(band._h, 1) == 1
    assert lib.gcm_set_band_tracer_rows(band._h, 2) == _lib.OK
    assert band.tracer_count == 2 and lib.gcm_tracer_mixed(band._h, 1) == 0 and band.tracer_mixing(1) is None
    band.set_tracer_mixing(1, good)
    assert lib.gcm_set_band_tracers(band._h, 2) == _lib.OK
    assert lib.gcm_tracer_mixed(band._h, 1) == 0
    band.close()
    # one level: nothing to mix across
    geom1 = su.geom_of(6, 10, 1)
    st1, trs1 = su.initial(geom1, 1)
    one = su.single(g, geom1, st1, trs1, scheme="van_leer")
    assert lib.gcm_set_tracer_mixing(one._h, 0, dp(np.zeros(1)), 0) == _lib.ERR_ARG
    assert lib.gcm_tracer_mixed(one._h, 0) == 0
    one.close()
    # other models
    sw = g.Core(_lib.SW2D, 130, 8, dx=300e3)
    assert lib.gcm_set_tracer_mixing(sw._h, 0, dp(good), L - 1) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_set_tracer_mixing(sw._h, -1, None, 0) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_tracer_mixed(sw._h, 0) == _lib.ERR_UNSUPPORTED
    sw.close()


# ---------------------------------------------------------------- 8. checkpoints
def test_checkpoint_single_domain(g, tmp_path):
    """saved after 2 of 4 steps and restored from the file alone: the uninterrupted run bit for bit; a file saved
    without mixing restores with none"""
    from gcmiipy_amd import checkpoint
    H, W, L = 16, 20, 5
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    want = _single(g, geom, st, trs, mixing, forcing, 4, runs=[2, 2])
    c = _core(g, geom, st, trs, mixing, forcing)
    c.step(2, DT)
    path = str(tmp_path / "mixed.npz")
    checkpoint.save(path, c, step=2, geom=geom)
    c.close()
    with np.load(path) as d:
        assert d["mixing_0"].dtype == np.float64 and d["mixing_0"].shape == (L - 1,) and "mixing_2" not in d.files
    c, ck = checkpoint.restore(path)
    assert sorted(ck["tracer_mixing"]) == [0, 1] and sorted(ck["tracer_forcing"]) == [1]
    for i, k in mixing.items():
        assert np.array_equal(c.tracer_mixing(i), k)
    assert c.tracer_mixing(2) is None
    c.step(2, DT)
    su.assert_equal((c.get_state(), c.get_tracers()), want)
    c.close()
    plain = _core(g, geom, st, trs)
    path = str(tmp_path / "plain.npz")
    checkpoint.save(path, plain, geom=geom)
    plain.close()
    assert not [k for k in np.load(path).files if k.startswith("mixing_")]
    c, ck = checkpoint.restore(path)
    assert ck["tracer_mixing"] == {} and c.tracer_count == NTR and c.tracer_mixings() == {}
    c.close()


def test_checkpoint_bands(g, tmp_path):
    """both bands of a mixed 2-band run saved after 2 steps, restored and continued for 2: the single domain"""
    import torch
    from gcmiipy_amd import checkpoint
    H, W, L = 16, 20, 5
    geom, st, trs, mixing, forcing = _setup(H, W, L)
    want = _single(g, geom, st, trs, mixing, forcing, 4)
    cores = _bands(g, geom, 2, st, trs, mixing, forcing)
    su.whole_steps(cores, torch, 2, DT)
    for r, c in enumerate(cores):
        checkpoint.save(str(tmp_path / ("b%d.npz" % r)), c, step=2, geom=geom)
        c.close()
    cores = [checkpoint.restore(str(tmp_path / ("b%d.npz" % r)))[0] for r in range(2)]
    for c in cores:
        assert sorted(c.tracer_mixings()) == [0, 1] and sorted(c.tracer_forcings()) == [1]
    su.whole_steps(cores, torch, 2, DT)
    su.assert_equal(su.gather(cores), want)
