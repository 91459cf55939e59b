"""The surface fluxes and the boundary-layer mixing of GCM_PE25D without a device: the two host probes
(gcm_boundary_layer_surface, gcm_boundary_layer_column -- the routines the kernels call, compiled for the host) against
the NumPy restatement tests/pe25d_boundary_layer_ref.py, the properties of the restatement that the GPU test then
checks on the device, the probes' refused calls and the checkpoint keys.  What needs a handle:
tests/test_pe25d_boundary_layer_gpu.py and tests/test_pe25d_column_phases_gpu.py.

Bounds.  The column probe is + - x / with contraction off: bit for bit.  The surface probe goes through sqrt, log and
the Exner routine (5.3e-16 against pow): 1e-12 relative.  The budgets are sums of L <= 42 terms of one sign, each
rounded to 1.1e-16, compared with their total: 1e-12 of the column's content."""
import numpy as np
import pytest

import gpu_setups as su
import pe25d_boundary_layer_ref as ref

DT = 600.0


def _case(shape, ptop, dtype="f64"):
    geom = su.geom_of(*shape, ptop)
    st = ref.windy_state(geom, dtype)
    return geom, st, ref.ground(geom, st)


def _step(geom, st, gt, dt=DT, dtype="f64", **over):
    return ref.boundary_layer_step(st[0], st[1], st[2], st[3], st[4], gt, geom.sig, geom.dsig, geom.ptop, dt,
                                   ref.params(**over), dtype)


# ---------------------------------------------------------------- the inputs are what the tests need them to be
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_inputs_cover_both_sides(shape):
    geom, st, gt = _case(shape, 0.0)
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1)
    assert (np.diff(sig) < 0).all(), "level 0 is the bottom"
    uc, vc = ref.centre_winds(st[1][0], st[2][0])
    sf = ref.surface(ref.params(), uc, vc, st[3][0], st[4][0], st[0], sig[0], 0.0)
    assert sf["S"].min() < ref.DEFAULTS["v_cap"] < sf["S"].max()
    T_a = st[3][0] * sf["pi_a"]
    assert (gt > T_a).any() and (gt < T_a).any()
    assert (sf["z_a"] > 0.0).all() and np.isfinite(sf["z_a"]).all()
    p_e = (sig[:-1] - 0.5 * np.asarray(geom.dsig).reshape(-1)[:-1])[:, None, None] * st[0][None]
    # (the three levels of the smallest shape have no interface below p_pbl: every f is the decaying branch there)
    assert (p_e < ref.DEFAULTS["p_pbl"]).any() and ((p_e >= ref.DEFAULTS["p_pbl"]).any() or shape[2] == 3)


# ---------------------------------------------------------------- the probes against the restatement
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_surface_probe_equals_the_restatement(shape, ptop):
    import gcmiipy_amd as g
    geom, st, gt = _case(shape, ptop)
    sig0 = float(np.asarray(geom.sig).reshape(-1)[0])
    uc, vc = ref.centre_winds(st[1][0], st[2][0])
    for over in ({}, dict(cd0=1e-3, cd1=1e-4, v_cap=7.5)):
        S, z_a, cd = g.boundary_layer_surface(uc, vc, st[3][0], st[4][0], st[0], sig0, ptop, **over)
        want = ref.surface(ref.params(**over), uc, vc, st[3][0], st[4][0], st[0], sig0, ptop)
        errs = {k: float(np.max(np.abs(a - want[k]) / np.abs(want[k]))) for k, a in (("S", S), ("z_a", z_a), ("cd", cd))}
        print("surface probe", shape, ptop, over, errs)
        assert max(errs.values()) <= 1e-12, errs
    # the cap holds cd
    S, _, cd = g.boundary_layer_surface([5.0, 20.0, 30.0, 300.0], 0.0, 300.0, 0.01, 1e5, sig0)
    assert np.array_equal(S, [5.0, 20.0, 30.0, 300.0]) and cd[1] == cd[2] == cd[3] == 7.0e-4 + 6.5e-5 * 20.0 > cd[0]


@pytest.mark.parametrize("L", [2, 3, 9, 42])
def test_column_probe_equals_the_restatement_bit_for_bit(L):
    import gcmiipy_amd as g
    rng = np.random.default_rng(31 + L)
    n = 300
    dsig = 0.2 / L + rng.random(L)
    dsig = dsig / dsig.sum()
    a = rng.random((n, L - 1)) * np.array([0.0, 1e-3, 1.0, 1e3])[rng.integers(0, 4, (n, 1))]
    x = rng.random(n) * np.array([0.0, 1e-2, 10.0])[rng.integers(0, 3, n)]
    target = 280.0 + 20.0 * rng.random(n)
    X = 300.0 + 10.0 * rng.standard_normal((n, L))
    got, got0 = g.boundary_layer_column(dsig, a, x, target, X)
    want, want0 = ref.column(dsig, a.T, x, target, X.T)
    assert np.array_equal(got, want.T), float(np.max(np.abs(got - want.T)))
    assert np.array_equal(got0, want0)
    assert (got != X).any()


def test_probes_refuse_bad_calls():
    import gcmiipy_amd as g
    lib, L_ = g._lib.lib, g._lib
    nan, inf = float("nan"), float("inf")
    one = np.ones(1)
    for over in (dict(cd0=-1e-3), dict(cd1=-1.0), dict(ch=-1.0), dict(ce=-1.0), dict(v_cap=0.0), dict(v_cap=-1.0),
                 dict(p_strat=0.0), dict(p_strat=-5.0), dict(cd0=nan), dict(p_pbl=inf), dict(ce=nan), dict(v_cap=inf)):
        with pytest.raises(ValueError):
            g.boundary_layer_surface(one, one, 300.0 * one, 0.01 * one, 1e5 * one, 0.99, **over)
    with pytest.raises(ValueError):
        g.boundary_layer_surface(one, one, one, one, one, 0.99, drag=1.0)
    dp = lambda a: a.ctypes.data_as(L_._dp)                                        # noqa: E731
    rec = L_.BoundaryLayer(*ref.DEFAULTS.values())
    assert lib.gcm_boundary_layer_surface(1, None, 0.0, 0.99, *[dp(one)] * 8) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_surface(-1, rec, 0.0, 0.99, *[dp(one)] * 8) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_surface(1, rec, 0.0, 0.99, None, *[dp(one)] * 7) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_surface(1, rec, nan, 0.99, *[dp(one)] * 8) == L_.ERR_ARG
    two = np.ones(2)
    assert lib.gcm_boundary_layer_column(1, 1, dp(two), dp(one), dp(one), dp(one), dp(two), dp(two), None) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_column(-1, 2, dp(two), dp(one), dp(one), dp(one), dp(two), dp(two), None) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_column(1, 2, None, dp(one), dp(one), dp(one), dp(two), dp(two), None) == L_.ERR_ARG
    assert lib.gcm_boundary_layer_column(1, 2, dp(two), dp(one), dp(one), dp(one), dp(two), None, None) == L_.ERR_ARG
    out = np.zeros(2)
    assert lib.gcm_boundary_layer_column(1, 2, dp(two), dp(one), dp(one), dp(one), dp(two), dp(out), None) == L_.OK
    assert np.array_equal(out, two)                                                # (X = target: nothing moves)


def test_aquaplanet_sst():
    import gcmiipy_amd as g
    lat = np.deg2rad(np.array([-90.0, -26.0, 0.0, 26.0, 90.0]))
    sst = g.aquaplanet_sst(lat)
    assert sst[2] == 300.0 and np.array_equal(sst, sst[::-1])
    assert abs(sst[1] - (29.0 * np.exp(-0.5) + 271.0)) <= 1e-12 and 271.0 < sst[0] < 271.1
    assert g.aquaplanet_sst(0.0, dT=10.0, T_min=280.0) == 290.0


# ---------------------------------------------------------------- properties of the restatement
@pytest.mark.parametrize("ptop", ref.PTOPS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_budgets_close(shape, ptop):
    geom, st, gt = _case(shape, ptop)
    p, u, v, t, q = st
    un, vn, tn, qn, shf, evap = _step(geom, st, gt)
    assert (evap > 0).any() and (shf > 0).any() and (shf < 0).any()
    water = ref.column_sum(q, geom.dsig) * p / ref.G
    dwater = (ref.column_sum(qn, geom.dsig) - ref.column_sum(q, geom.dsig)) * p / ref.G
    err_w = float(np.max(np.abs(dwater - evap) / water))
    sig0 = float(np.asarray(geom.sig).reshape(-1)[0])
    cpm = ref.CP * ((sig0 * p + ptop) / ref.P0) ** ref.KAPPA * p / ref.G
    heat = cpm * ref.column_sum(t, geom.dsig)
    dheat = cpm * (ref.column_sum(tn, geom.dsig) - ref.column_sum(t, geom.dsig))
    err_h = float(np.max(np.abs(dheat - shf) / heat))
    print("budgets", shape, ptop, err_w, err_h)
    assert err_w <= 1e-12 and err_h <= 1e-12, (err_w, err_h)


@pytest.mark.parametrize("dt", [DT, 86400.0])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_maximum_principle(shape, dt):
    geom, st, gt = _case(shape, 1000.0)
    ref.assert_maximum_principle(st, gt, geom, _step(geom, st, gt, dt))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_rest_and_dt_zero_keep_every_bit(shape, dtype):
    geom = su.geom_of(*shape, 1000.0)
    st, gt = ref.resting_state(geom, dtype)
    out = _step(geom, st, gt, dtype=dtype)
    for k, a, b in zip("uvtq", out[:4], st[1:]):
        assert np.array_equal(a, b), ("rest", k)
    assert not out[4].any() and not out[5].any()
    st = ref.windy_state(geom, dtype)
    out = _step(geom, st, ref.ground(geom, st), dt=0.0, dtype=dtype)
    for k, a, b in zip("uvtq", out[:4], st[1:]):
        assert np.array_equal(a, b), ("dt = 0", k)
    assert not out[4].any() and not out[5].any()


# ---------------------------------------------------------------- the checkpoint keys
class _Recorded:
    """what checkpoint.save asks of a core, and what checkpoint.restore does to one: no library call"""
    options = {}
    tracer_count = 0
    held_suarez = None
    climate_every = 0
    moist = convect = None

    def __init__(self, model, L, H, W, boundary_layer=None, sums=None, ground=None):
        self.model, self.L, self.H, self.W = model, L, H, W
        self.boundary_layer, self.sums, self.ground = boundary_layer, sums, ground
        self.state = [np.zeros((H, W))] + [np.zeros((L, H, W)) for _ in range(4)]
        self.calls = []

    has_ground = property(lambda self: self.ground is not None)

    def get_state(self):
        return self.state

    def get_ground(self):
        return self.ground

    def set_ground(self, gt):
        self.ground = gt
        self.calls.append("ground")

    def boundary_layer_sums(self):
        return self.sums

    def set_state(self, p=None, u=None, v=None, t=None, q=None):
        self.state = [p, u, v, t, q]

    def set_boundary_layer(self, **params):
        self.boundary_layer, self.sums = params, None
        self.calls.append("boundary_layer")

    def put_boundary_layer(self, nsteps, seconds, shf, evap):
        import gcmiipy_amd as g
        self.sums = g.BoundaryLayer(nsteps, seconds, shf, evap)


def test_checkpoint_round_trip_of_the_five_keys(tmp_path, monkeypatch):
    import gcmiipy_amd as g
    from gcmiipy_amd import checkpoint
    from gcmiipy_amd.core import BOUNDARY_LAYER_DEFAULTS, COLUMN_PHASES
    assert [ph.name for ph in COLUMN_PHASES] == ["boundary_layer", "convect", "moist"], "the model's order"
    assert dict(BOUNDARY_LAYER_DEFAULTS) == ref.DEFAULTS and list(BOUNDARY_LAYER_DEFAULTS) == list(ref.DEFAULTS)
    L, H, W = 3, 4, 6
    rng = np.random.default_rng(9)
    sums = g.BoundaryLayer(7, 4200.0, rng.standard_normal((H, W)), rng.standard_normal((H, W)))
    par = ref.params(cd0=1e-3, p_pbl=80000.0)
    gt = 290.0 + rng.random((H, W))
    path = str(tmp_path / "bl.npz")
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W, boundary_layer=par, sums=sums, ground=gt), step=40)
    d = np.load(path)
    keys = {"boundary_layer", "boundary_layer_n", "boundary_layer_seconds", "boundary_layer_shf", "boundary_layer_evap"}
    assert keys <= set(d.files)
    assert list(d["boundary_layer"]) == [par[k] for k in BOUNDARY_LAYER_DEFAULTS]
    ck = checkpoint.load(path)
    assert ck["boundary_layer"]["params"] == par and ck["boundary_layer"]["n"] == 7
    assert ck["boundary_layer"]["seconds"] == 4200.0 and ck["convect"] is None and ck["moist"] is None
    made = []

    def fake_core(model, W_, H_, L_, **kw):
        made.append(_Recorded(model, L_, H_, W_))
        return made[-1]
    monkeypatch.setattr(checkpoint, "Core", fake_core)
    core, _ = checkpoint.restore(path)
    assert core is made[-1] and core.boundary_layer == par and (core.sums.nsteps, core.sums.seconds) == (7, 4200.0)
    assert np.array_equal(core.sums.shf, sums.shf) and np.array_equal(core.sums.evap, sums.evap)
    assert core.calls == ["ground", "boundary_layer"], "the registration needs the ground temperature in place"
    # a file without the keys restores with none
    checkpoint.save(path, _Recorded(g._lib.PE25D, L, H, W), step=1)
    assert not any(k.startswith("boundary_layer") for k in np.load(path).files)
    assert checkpoint.load(path)["boundary_layer"] is None
    core, _ = checkpoint.restore(path)
    assert core.boundary_layer is None and core.sums is None
