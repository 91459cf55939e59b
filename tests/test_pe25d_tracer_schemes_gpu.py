"""GPU tests of the passive tracers' transport schemes of GCM_PE25D (gcm_set_tracer_scheme): the donor-cell and van
Leer limited kernels against the NumPy restatement of the scheme (tests/pe25d_tracer_schemes_ref.py) on every cell,
scheme NONE untouched by the new setter, a state that does not notice the tracers, one stream against two, UPWIND on
latitude bands, VANLEER refused there, checkpoints, the drop-in functions and the fp32 handles."""
import numpy as np
import pytest

from conftest import rel_err

import gpu_setups as su
import pe25d_inputs as inp
import pe25d_tracer_schemes_ref as ref
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10
# fp32 handle vs fp64 handle after one step, smooth tracers (test_fp32_limited_schemes_vs_fp64).  The centred figure
# is F32_TOL = 2e-6 of tests/test_pe25d_tracers_gpu.py; the constant here is twice the maximum measured over both
# schemes and all tracers on the first GPU run: 1.881e-07 (UPWIND, tracer 2; VANLEER 1.777e-07; the centred scheme on
# the same tracers 1.883e-07), a tenth of the centred figure.
F32_LIM_TOL = 3.8e-7
SCHEMES = {"upwind": ref.UPWIND, "van_leer": ref.VANLEER}


def _tracers(H, W, L, n, seed):
    """inp.tracers; below three, in the order step function, random positive (one tracer: the step function)"""
    return inp.tracers(H, W, L, n, seed) if n >= 3 else inp.tracers(H, W, L, 2, seed)[[1, 0][:n]]


# (H, W, L, filter, coriolis, topography bump, GCM_PE_LEVEL_SEGMENTS, tracer counts): odd and even L, with and without
# the filter, Coriolis, topography and two level segments; 48 x 1440 x 24: several column tiles.  7 tracers: chunks of
# 4, 2 and 1; 3: 2 and 1; 1: 1
CASES = [(24, 36, 9, True, False, False, None, (1, 3, 7)),
         (24, 36, 8, True, True, True, None, (7,)),
         (24, 36, 9, False, True, False, "2", (7,)),
         (24, 36, 8, False, False, True, "2", (3,)),
         (48, 1440, 24, True, True, True, None, (7,))]


def _ids(cases):
    return ["-".join(str(x) for x in c[:7]) for c in cases]


@pytest.mark.parametrize("case", [c for c in CASES if c[3]], ids=_ids([c for c in CASES if c[3]]))
def test_limited_tracers_vs_restatement(g, case):
    """UPWIND and VANLEER, fp64: the star set after the first predictor and the tracers after 5 full steps, every cell
    of every tracer, within the project's 1e-10 of the restatement"""
    H, W, L, filt, cor, bump, seg, counts = case
    geom, og = su.geoms_of(H, W, L, bump=bump)
    st = inp.state(geom, 3)
    dt, steps = 60.0, 5
    _, hist = ref.flux_history(st, dt, og, steps, cor)
    for ntr in counts:
        trs = _tracers(H, W, L, ntr, 4)
        for name, scheme in SCHEMES.items():
            c = g.Core(g._lib.PE25D, W, H, L, geom=geom, filter=filt, coriolis=cor, tracer_scheme=name)
            assert c.tracer_scheme == scheme
            c.set_state(*st)
            c.set_tracers(trs)
            c.half_step(0, dt)
            star = c.get_tracers(star=True)
            c.half_step(1, dt)
            c.step(steps - 1, dt)
            got = c.get_tracers()
            c.close()
            _, want_star = ref.advance(trs, hist[:1], dt, og, scheme)
            want, _ = ref.advance(trs, hist, dt, og, scheme)
            for n in range(ntr):
                e_star, e = rel_err(star[n], want_star[n]), rel_err(got[n], want[n])
                print("%s %s ntr %d tracer %d: star %.2e, 5 steps %.2e" % (case[:7], name, ntr, n, e_star, e))
                assert e_star < TOL, (name, ntr, "star", n)
                assert e < TOL, (name, ntr, n)


@pytest.mark.parametrize("case", [c for c in CASES if not c[3]], ids=_ids([c for c in CASES if not c[3]]))
def test_limited_tracers_without_filter_vs_restatement_on_handle_fluxes(g, case, monkeypatch):
    """the handles without the polar filter (the oracle always filters): one predictor, with the restatement applied
    to the stage's own spu, pit and p_n as the handle exposes them (gcm_get_intermediate) and sigma-dot rebuilt from
    them by the oracle's aflux"""
    from oracle import dynamics as od
    H, W, L, filt, cor, bump, seg, counts = case
    monkeypatch.setenv("GCM_PE_LEVEL_SEGMENTS", seg)
    geom, og = su.geoms_of(H, W, L, bump=bump)
    st = inp.state(geom, 3)
    dt = 60.0
    trs = _tracers(H, W, L, counts[-1], 4)
    for name, scheme in SCHEMES.items():
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, filter=False, coriolis=cor, tracer_scheme=name)
        c.set_state(*st)
        c.set_tracers(trs)
        c.half_step(0, dt)
        star = c.get_tracers(star=True)
        spu, p_n = c.get_intermediate(g._lib.INT_SPU), c.get_intermediate(g._lib.INT_PN)
        c.close()
        spv = od.calc_pv(st[0], st[2])
        _, sd = od.aflux(spu, spv, og)
        for n in range(len(trs)):
            want = ref.tracer_stage(trs[n], trs[n], st[0], p_n, spu, spv, sd, dt, og, scheme)
            assert rel_err(star[n], want) < TOL, (name, n)


def test_scheme_none_is_untouched_and_switching_mid_run(g):
    """a handle that was given scheme NONE through the new setter (also after a detour through VANLEER, before any
    step) is bit-identical to one that never called it; VANLEER for 2 steps, then NONE for 2, is what the restatement
    gives; the setter drops the predicted tracers"""
    from gcmiipy_amd.core import GcmError
    H, W, L, dt = 24, 36, 9, 120.0
    geom, og = su.geoms_of(H, W, L)
    st = inp.state(geom, 5)
    trs = _tracers(H, W, L, 7, 6)
    res = []
    for mode in ("never", "none", "detour"):
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
        c.set_state(*st)
        if mode == "none":
            c.set_tracer_scheme("centred")
        c.set_tracers(trs)
        if mode == "detour":
            c.set_tracer_scheme("van_leer")
            c.set_tracer_scheme(g._lib.TRACER_NONE)
        assert c.tracer_scheme == g._lib.TRACER_NONE
        c.step(4, dt)
        res.append((c.get_tracers(), c.get_state()))
        c.close()
    for tr, state in res[1:]:
        assert np.array_equal(tr, res[0][0])
        for a, b in zip(state, res[0][1]):
            assert np.array_equal(a, b)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, tracer_scheme="van_leer")
    c.set_state(*st)
    c.set_tracers(trs)
    c.step(2, dt)
    c.half_step(0, dt)
    assert c.get_tracers(star=True).shape == trs.shape
    c.set_tracer_scheme("centred")
    with pytest.raises(GcmError, match="no predicted tracers"):
        c.get_tracers(star=True)
    c.half_step(0, dt)                                       # the predictor again, now centred
    c.half_step(1, dt)
    c.step(1, dt)
    got = c.get_tracers()
    c.close()
    _, hist = ref.flux_history(st, dt, og, 4)
    want, _ = ref.advance(trs, hist[:2], dt, og, ref.VANLEER)
    want, _ = ref.advance(want, hist[2:], dt, og, ref.NONE)
    for n in range(len(trs)):
        assert rel_err(got[n], want[n]) < TOL, n


@pytest.mark.parametrize("scheme", ["upwind", "van_leer"])
def test_state_and_q_do_not_notice_the_tracers(g, scheme):
    """p, u, v, t, q after 5 steps with 5 limited tracers are bit-identical to a handle with no tracers"""
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L, bump=True)
    st = inp.state(geom, 9)
    res = []
    for ntr in (5, 0):
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, tracer_scheme=scheme if ntr else None)
        c.set_state(*st)
        if ntr:
            c.set_tracers(np.concatenate([st[4][None], _tracers(H, W, L, 4, 2)]))
        c.step(5, 300.0)
        res.append(c.get_state())
        if ntr:
            assert not np.array_equal(c.get_tracers()[0], res[0][4])     # q := c does not stay q under a limited scheme
        c.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("scheme", ["upwind", "van_leer"])
def test_single_stream_vs_two_streams(g, scheme, monkeypatch):
    """48 x 1440 x 24, 7 tracers, 4 steps: the limited kernels on the second stream beside K3 / K4 give the bits of a
    run with every kernel on one stream (GCM_PE_SINGLE_STREAM=1)"""
    H, W, L = 48, 1440, 24
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 13)
    trs = _tracers(H, W, L, 7, 14)
    res = {}
    for single in ("0", "1"):
        monkeypatch.setenv("GCM_PE_SINGLE_STREAM", single)
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, tracer_scheme=scheme)
        c.set_state(*st)
        c.set_tracers(trs)
        c.step(4, 60.0)
        res[single] = (c.get_tracers(), c.get_state()[4])
        c.close()
    assert np.array_equal(res["0"][0], res["1"][0])
    assert np.array_equal(res["0"][1], res["1"][1])
    assert not np.array_equal(res["0"][0], trs)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_upwind_on_eight_bands_equals_single_domain(g, dtype):
    """UPWIND reads rows j -+ 1 only: 8 in-process latitude bands of a 64 x 1440 x 24 grid with 3 tracers, the ghost
    rows moved by device copies (two exchanges per step), equal the single domain bit for bit after 3 steps -- state
    and tracers"""
    import torch
    H, W, L, steps, nb, dt = 64, 1440, 24, 3, 8, 60.0
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, 3)
    want = su.single_run(g, geom, st, trs, steps, dt, dtype=dtype, scheme="upwind")
    cores = su.bands(g, geom, nb, st, trs, dtype=dtype, scheme="upwind")
    for c in cores:
        assert c.tracer_scheme == g._lib.TRACER_UPWIND
    su.whole_steps(cores, torch, steps, dt)
    got = su.gather(cores)
    su.assert_equal(got, want)
    assert not np.array_equal(got[1], trs)


@pytest.mark.parametrize("overlap", [False, True])
def test_upwind_band_run_loopback_equals_single_domain(g, overlap):
    """gcm_band_run with the loopback exchange (the band is its own neighbour): the split stage launches the tracers'
    edge rows and interior rows apart; UPWIND gives the single domain's bits"""
    import torch
    H, W, L, dt = 23, 36, 9, 120.0
    geom = su.geom_of(H, W, L)
    st, trs = su.initial(geom, 3)
    want = su.single_run(g, geom, st, trs, 5, dt, scheme="upwind")
    c, eng, runner = su.loopback_band(g, torch, geom, 3, scheme="upwind")
    assert runner.native
    if overlap:
        c.set_band_overlap(True)
    c.set_state(*st)
    c.set_tracers(trs)
    runner.run(3, dt)
    runner.run(2, dt)
    torch.cuda.synchronize()
    got = c.get_state(), c.get_tracers()
    c.close()
    su.assert_equal(got, want)


def test_refusals(g):
    """VANLEER on a latitude band: GCM_ERR_UNSUPPORTED, and the message names the reason; an unknown scheme:
    GCM_ERR_ARG; another model: GCM_ERR_UNSUPPORTED; a refused call leaves the scheme as it was"""
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import GcmError
    lib = _lib.lib
    H, W, L = 12, 20, 5
    geom = su.geom_of(H, W, L)
    band = g.Core(_lib.PE25D, W, H // 2, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, band_tracers=1)
    band.set_tracer_scheme("upwind")
    assert lib.gcm_set_tracer_scheme(band._h, _lib.TRACER_VANLEER) == _lib.ERR_UNSUPPORTED
    msg = lib.gcm_last_error(band._h).decode()
    assert "ghost row" in msg and "band" in msg
    assert band.tracer_scheme == _lib.TRACER_UPWIND
    with pytest.raises(GcmError, match="ghost row"):
        band.set_tracer_scheme("van_leer")
    assert band.options["tracer_scheme"] == _lib.TRACER_UPWIND
    band.close()
    with pytest.raises(GcmError, match="ghost row"):
        g.Core(_lib.PE25D, W, H // 2, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0, tracer_scheme="van_leer")
    c = g.Core(_lib.PE25D, W, H, L, geom=geom)
    assert c.tracer_scheme == _lib.TRACER_NONE
    for bad in (-1, 3, 99):
        assert lib.gcm_set_tracer_scheme(c._h, bad) == _lib.ERR_ARG
    assert lib.gcm_set_tracer_scheme(c._h, _lib.TRACER_VANLEER) == _lib.OK      # without tracers set
    assert c.tracer_scheme == _lib.TRACER_VANLEER and c.tracer_count == 0
    c.close()
    sw = g.Core(_lib.SW2D, 32, 16, dx=300e3)
    assert lib.gcm_set_tracer_scheme(sw._h, _lib.TRACER_UPWIND) == _lib.ERR_UNSUPPORTED
    assert lib.gcm_set_tracer_scheme(sw._h, 5) == _lib.ERR_ARG
    assert lib.gcm_tracer_scheme(sw._h) == _lib.TRACER_NONE
    sw.close()


@pytest.mark.parametrize("scheme", ["upwind", "van_leer"])
def test_checkpoint_keeps_the_scheme_and_the_bits(g, scheme, tmp_path):
    """save after step 2, restore, step 4 == the uninterrupted run bit for bit; the file carries the scheme among the
    handle's options, and a file without it restores as centred"""
    from gcmiipy_amd import checkpoint
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 17)
    trs = _tracers(H, W, L, 3, 8)
    a = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    a.set_state(*st)
    a.set_tracers(trs)
    a.set_tracer_scheme(scheme)                              # after construction: the options follow the setter
    a.step(2, 300.0)
    path = str(tmp_path / "ck.npz")
    checkpoint.save(path, a, step=2, time=600.0, geom=geom)
    a.step(2, 300.0)
    want, want_tr = a.get_state(), a.get_tracers()
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["options"]["tracer_scheme"] == SCHEMES[scheme] and b.tracer_scheme == SCHEMES[scheme]
    b.step(2, 300.0)
    for x, y in zip(b.get_state(), want):
        assert np.array_equal(x, y)
    assert np.array_equal(b.get_tracers(), want_tr)
    b.close()
    d = dict(np.load(path))
    del d["opt_tracer_scheme"]                               # a file written before the option existed
    old = str(tmp_path / "old.npz")
    np.savez(old, **d)
    c, ck2 = checkpoint.restore(old)
    assert "tracer_scheme" not in ck2["options"] and c.tracer_scheme == g._lib.TRACER_NONE and c.tracer_count == 3
    c.close()


def test_dropins_take_a_scheme(g):
    """dynamics.matsuno_timestep / half_timestep / run and no_limits_2_5d.run_model with tracer_scheme=: the Core's
    tracers, a state that is what it is without tracers, and a cached handle that is centred again afterwards"""
    from gcmiipy_amd import dynamics, no_limits_2_5d
    H, W, L, dt = 12, 20, 5, 60.0
    geom, og = su.geoms_of(H, W, L)
    st = inp.state(geom, 21)
    trs = np.stack([st[4], _tracers(H, W, L, 1, 3)[0]])
    plain = dynamics.matsuno_timestep(*st, dt, geom)
    _, hist = ref.flux_history(st, dt, og, 3)
    for name, scheme in SCHEMES.items():
        out = dynamics.matsuno_timestep(*st, dt, geom, tracers=trs, tracer_scheme=name)
        for a, b in zip(out[:5], plain):
            assert np.array_equal(a, b)
        want, _ = ref.advance(trs, hist[:1], dt, og, scheme)
        assert rel_err(out[5][1], want[1]) < TOL and rel_err(out[5][0], want[0]) < TOL
        centred = dynamics.matsuno_timestep(*st, dt, geom, tracers=trs)    # the cached handle forgot the scheme
        assert np.array_equal(centred[5][0], centred[4])
        r = dynamics.run(*st, dt, geom, 3, tracers=trs, tracer_scheme=name)
        want3, _ = ref.advance(trs, hist, dt, og, scheme)
        assert rel_err(r[5][1], want3[1]) < TOL
        h = dynamics.half_timestep(*st, *st, dt, geom, tracers=trs, tracer_scheme=name)
        _, want_star = ref.advance(trs, hist[:1], dt, og, scheme)
        assert len(h) == 6 and rel_err(h[5][1], want_star[1]) < TOL
        stats = {k: [] for k in ("u_max", "u_min", "v_max", "v_min", "ke")}
        m = no_limits_2_5d.run_model(8, 8, 3, 1800.0, 3, None, stats=stats, tracers=np.ones((1, 3, 8, 8)), tracer_scheme=name)
        assert len(m) == 8 and np.max(np.abs(m[7] - 1.0)) < 1e-12          # a constant stays constant
    assert np.array_equal(dynamics.matsuno_timestep(*st, dt, geom)[4], plain[4])


def _smooth_tracers(H, W, L, geom):
    lat = np.asarray(geom.lat).reshape(1, H, 1)
    lon = (2 * np.pi * np.arange(W) / W).reshape(1, 1, W)
    lev = np.linspace(0.0, 1.0, L).reshape(L, 1, 1)
    return np.stack([2.0 + np.sin(lon) * np.cos(lat) + 0.0 * lev,
                     1.0 + 0.5 * np.cos(2 * lon) * np.cos(lat) ** 2 + 0.3 * lev,
                     3.0 + np.sin(lat) * (1.0 - lev) + 0.2 * np.sin(3 * lon) * np.cos(lat)])


def test_fp32_limited_schemes_vs_fp64(g):
    """fp32 handles under UPWIND and VANLEER against the fp64 handle after one step on smooth tracers.  The yardstick
    is the centred scheme's figure, F32_TOL = 2e-6; a limiter switch can amplify a rounding difference at isolated
    cells, so the constant is twice the measured maximum.  Measured on an MI355X (rel. L-inf per tracer): centred
    1.883e-07 / 1.601e-07 / 1.586e-07, UPWIND 1.706e-07 / 1.755e-07 / 1.881e-07, VANLEER 1.767e-07 / 1.777e-07 /
    1.392e-07: the limited schemes round like the centred one, no amplification at these cells."""
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 5)
    trs = _smooth_tracers(H, W, L, geom)
    worst = 0.0
    for name in ("centred", "upwind", "van_leer"):
        res = {}
        for dtype in ("f64", "f32"):
            c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype, tracer_scheme=name)
            c.set_state(*st)
            c.set_tracers(trs)
            c.step(1, 60.0)
            res[dtype] = c.get_tracers()
            c.close()
        for n in range(3):
            e = rel_err(res["f32"][n], res["f64"][n])
            print("fp32 vs fp64, %s, tracer %d: %.3e" % (name, n, e))
            if name != "centred":
                worst = max(worst, e)
    print("fp32 vs fp64, limited schemes, maximum: %.3e" % worst)
    assert worst < F32_LIM_TOL
