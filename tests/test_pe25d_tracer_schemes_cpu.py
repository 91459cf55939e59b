"""CPU tests of the passive tracers' transport schemes of GCM_PE25D (gcm_set_tracer_scheme): the C and Python surface
without a device, and the properties of the scheme itself on its NumPy restatement (tests/pe25d_tracer_schemes_ref.py),
which the GPU tests hold the kernels to."""
import os
import re

import numpy as np
import pytest

import pe25d_inputs as inp
import pe25d_tracer_schemes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, L = 24, 36, 9


def _og(h=H, w=W, l=L):
    from oracle import geometry as ogeo
    return ogeo.gen_geometry(h, w, l, sig_func=ogeo.manabe_sig)


def flow_state(og, U=30.0, V=15.0):
    """a zonal jet of U m/s and a meridional wind of V m/s that changes sign with longitude, at rest otherwise"""
    l, h, w = og.layers, og.height, og.width
    lat = np.asarray(og.lat).reshape(h, 1)
    lon = 2 * np.pi * np.arange(w) / w
    p = np.full((h, w), 1e5)
    u = np.broadcast_to(U * np.cos(lat), (l, h, w)).copy()
    v = np.broadcast_to(V * np.cos(lat) * np.sin(lon)[None, :], (l, h, w)).copy()
    v[:, -1, :] = 0
    t = 300.0 * ((1e5 / (p * og.sig + og.ptop)) ** (287.0 / 1004.0)) * np.ones((l, h, w))
    return p, u, v, t, np.full((l, h, w), 3e-6)


def latitude_step(l=L, h=H, w=W):
    c = np.zeros((l, h, w))
    c[:, h // 3: 2 * h // 3, :] = 1.0
    return c


def test_scheme_surface_without_a_device():
    """both entry points are declared, exported and bound; a null handle is refused; a bad scheme never reaches the
    device"""
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, core, dynamics, geometry, no_limits_2_5d
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcmcore.h")).read(), flags=re.S)
    assert re.search(r"int\s+gcm_set_tracer_scheme\s*\(\s*gcm_handle\s*\*\s*h\s*,\s*int\s+scheme\s*\)", src)
    assert re.search(r"int\s+gcm_tracer_scheme\s*\(\s*const\s+gcm_handle\s*\*\s*h\s*\)", src)
    assert "gcm_set_tracer_scheme" in _lib.SYMBOLS and "gcm_tracer_scheme" in _lib.SYMBOLS
    lib = _lib.lib
    for scheme in (_lib.TRACER_NONE, _lib.TRACER_VANLEER, 7, -1):
        assert lib.gcm_set_tracer_scheme(None, scheme) == _lib.ERR_ARG
    assert lib.gcm_tracer_scheme(None) == _lib.ERR_ARG
    assert core.tracer_scheme_id(None) == _lib.TRACER_NONE
    assert [core.tracer_scheme_id(s) for s in ("centred", "upwind", "van_leer")] == [0, 1, 2]
    assert [core.tracer_scheme_id(s) for s in (_lib.TRACER_NONE, _lib.TRACER_UPWIND, np.int64(2))] == [0, 1, 2]
    geom = geometry.gen_geometry(4, 6, 2)
    for bad in ("bogus", "vanleer", 3, -1, 1.5, True, [1]):
        with pytest.raises(ValueError, match="tracer_scheme"):
            core.tracer_scheme_id(bad)
        with pytest.raises(ValueError, match="tracer_scheme"):       # before gcm_create: no device is asked for
            g.Core(_lib.PE25D, 6, 4, 2, geom=geom, tracer_scheme=bad)
    with pytest.raises(ValueError, match="GCM_PE25D"):
        g.Core(_lib.SW2D, 32, 16, dx=300e3, tracer_scheme="upwind")
    a3, a2 = np.ones((2, 4, 6)), np.ones((4, 6))
    st = (a2, a3, a3, a3, a3)
    with pytest.raises(ValueError, match="tracer_scheme"):
        dynamics.matsuno_timestep(*st, 1.0, geom, tracers=a3[None], tracer_scheme="bogus")
    with pytest.raises(ValueError, match="tracer_scheme"):
        dynamics.half_timestep(*st, *st, 1.0, geom, tracers=a3[None], tracer_scheme="bogus")
    with pytest.raises(ValueError, match="tracer_scheme"):
        dynamics.run(*st, 1.0, geom, 1, tracers=a3[None], tracer_scheme="bogus")
    with pytest.raises(ValueError, match="tracer_scheme"):
        no_limits_2_5d.run_model(4, 6, 2, 1.0, 1, None, tracers=a3[None], tracer_scheme="bogus")


def test_tool_takes_a_scheme():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tools_tracer_time", os.path.join(ROOT, "tools", "tools_tracer_time.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a = m.parser().parse_args(["--scheme", "none", "upwind", "van_leer"])
    assert [m.SCHEMES[s] for s in a.scheme] == [0, 1, 2]
    assert m.parser().parse_args([]).scheme == ["none"]
    # VANLEER requests the own column once per level and i -+ 1, 2 / j -+ 1, 2 from cache: the counted bytes are the
    # centred kernel's
    assert m.tracer_bytes_per_step(720, 1440, 24, 4) == 4 * 40 * 720 * 1440 * 24 + 2 * (2 * 720 * 1440 * 24 + 720 * 1440) * 8


@pytest.mark.parametrize("coriolis", [False, True])
def test_centred_restatement_is_the_oracle_bit_for_bit(coriolis):
    """scheme NONE of the restatement == oracle.dynamics.matsuno_timestep run with q := c, bit for bit, 3 steps"""
    from oracle import dynamics as od
    og = _og()
    og.heightmap[H // 2, W // 3] = 1500.0
    st = inp.state(og, 3)
    rng = np.random.default_rng(4)
    trs = np.stack([1.0 + rng.random((L, H, W)), latitude_step(), st[4]])
    state, got = st, trs
    for _ in range(3):
        state, got, _ = ref.matsuno_step(state, got, 120.0, og, ref.NONE, coriolis)
    for n in range(3):
        s = (*st[:4], trs[n])
        for _ in range(3):
            s = od.matsuno_timestep(*s, 120.0, og, coriolis=coriolis)
        assert np.array_equal(got[n], s[4]), n
    assert np.array_equal(got[2], state[4])                  # the tracer that started as q is q


@pytest.mark.parametrize("scheme", [ref.NONE, ref.UPWIND, ref.VANLEER])
def test_constant_tracer_stays_constant(scheme):
    """sd is consistent with pit (the continuity equation in flux form), so a constant tracer stays constant under
    every scheme: a few ulps per stage (the update is ~10 rounded operations on terms no larger than c p), 10 steps of
    the strong flow -- bound: 8 ulps per stage, accumulating linearly"""
    og = _og()
    _, tr = ref.run(flow_state(og), np.full((1, L, H, W), 2.5), 300.0, og, 10, scheme)
    err = np.max(np.abs(tr - 2.5)) / (np.finfo(float).eps * 2.5)
    print("scheme %d: constant tracer off by %.1f ulps after 10 steps" % (scheme, err))
    assert err < 8 * 2 * 10


def test_upwind_predictor_is_a_convex_combination():
    """where no cell loses more mass in a stage than it holds, one UPWIND stage with stage = base gives each cell a
    convex combination of itself and its inflow neighbours: the range of c0 is kept up to rounding"""
    og = _og()
    st = flow_state(og)
    st, _ = ref.run(st, np.zeros((0, L, H, W)), 300.0, og, 5, ref.NONE)   # (a flow that has developed sigma-dot)
    rng = np.random.default_rng(8)
    c0 = np.stack([latitude_step(), rng.random((L, H, W)), -3.0 + 5.0 * rng.random((L, H, W))])
    dt = 300.0
    taps = []
    _, _, star = ref.matsuno_step(st, c0, dt, og, ref.UPWIND, taps=taps)
    p, p_n, spu, spv, sd = taps[0]
    assert np.abs(sd).max() > 0 and np.abs(spv).max() > 0
    assert ref.outflow_bound(p, spu, spv, sd, dt, og).min() >= 0          # the precondition, from the tapped fluxes
    for n in range(3):
        lo, hi = c0[n].min(), c0[n].max()
        slack = 16 * np.finfo(float).eps * max(abs(lo), abs(hi))    # ~10 rounded operations on terms <= |c| p
        assert star[n].min() >= lo - slack and star[n].max() <= hi + slack, n


def test_step_function_undershoot_and_overshoot():
    """the latitude step function in a flow of tens of m/s, 200 full Matsuno steps of 300 s: the centred scheme
    undershoots and overshoots by ~0.3 of the step height; UPWIND and VANLEER do no worse in either direction.  (No
    absolute bound: the corrector applies star-state fluxes to the base state, so the 1-D TVD proof does not carry
    over.  Measured: centred min -3.2006e-01, max 1 + 3.0346e-01; UPWIND min 1.4e-23, max 1 - 8.7e-09; VANLEER min
    -8.3e-51, max 1 + 4.4e-16.)"""
    og = _og()
    res = {}
    for scheme in (ref.NONE, ref.UPWIND, ref.VANLEER):
        _, tr = ref.run(flow_state(og), latitude_step()[None], 300.0, og, 200, scheme)
        res[scheme] = (max(0.0, -tr.min()), max(0.0, tr.max() - 1.0))
        print("scheme %d: undershoot %.4e overshoot %.4e" % (scheme, *res[scheme]))
    assert res[ref.NONE][0] > 1e-3 and res[ref.NONE][1] > 1e-3
    for scheme in (ref.UPWIND, ref.VANLEER):
        assert res[scheme][0] <= res[ref.NONE][0] and res[scheme][1] <= res[ref.NONE][1], scheme


def test_van_leer_face_value_pieces():
    """face_value against the reference's pieces as the oracle restates them (van_leer, calc_r, donor_cell_flux) on a
    periodic 1-D array, and the zero-denominator rule"""
    from oracle import tracer as otr
    rng = np.random.default_rng(2)
    q = rng.random(32)
    q[5:9] = 0.25                                            # flat stretches: zero denominators
    for sign in (1.0, -1.0):
        F = sign * (0.5 + rng.random(32))
        a, b, aa, bb = q, np.roll(q, -1), np.roll(q, 1), np.roll(q, -2)
        assert np.array_equal(ref.face_value(F, aa, a, b, bb, ref.UPWIND) * F, otr.donor_cell_flux(q, F))
        r = otr.calc_r(q)                                    # (q[i] - q[i-1]) / (q[i+1] - q[i])
        if sign > 0:
            want = a + 0.5 * otr.van_leer(r) * (b - a)
        else:                                                # mirrored: the ratio at cell i + 1 seen from the other side
            rm = np.roll(np.divide(np.roll(q, -1) - q, q - np.roll(q, 1), out=np.zeros(32), where=(q - np.roll(q, 1)) != 0), -1)
            want = b + 0.5 * otr.van_leer(rm) * (a - b)
        assert np.array_equal(ref.face_value(F, aa, a, b, bb, ref.VANLEER), want)
    assert np.array_equal(ref.face_value(np.zeros(32), aa, a, b, bb, ref.UPWIND), b)   # F = 0 is not > 0
