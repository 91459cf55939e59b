"""GPU tests of the passive tracers of GCM_PE25D (gcm_set_tracers / gcm_get_tracers): a tracer advances with
exactly the update of q (bit for bit), matches the oracle's matsuno_timestep run with q := c, changes nothing
else, and is the same under one stream or two, across a checkpoint and in every refusal."""
import numpy as np
import pytest

from conftest import golden, rel_err
import gpu_setups as su
import pe25d_inputs as inp
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-10
F32_TOL = 2e-6          # test_fp32_tolerance_sweep: fp32 vs fp64 after one step


def _tracers3(H, W, L, seed):
    """random positive, a latitude step function, a constant"""
    rng = np.random.default_rng(seed)
    step = np.zeros((L, H, W))
    step[:, H // 3: 2 * H // 3, :] = 1.0
    return np.stack([1.0 + rng.random((L, H, W)), step, np.full((L, H, W), 2.5)])


# (H, W, L, dtype, filter, coriolis, topography bump, GCM_PE_LEVEL_SEGMENTS).  fp64 only: in the fp32 update
# kernel the compiler pairs the theta and q chains into packed instructions (v_pk_mul_f32), which fixes for q a
# set of roundings a kernel without the theta chain does not reproduce; fp32 tracers are held to the fp32
# tolerance instead (test_fp32_tracers_vs_oracle)
CASES = [(24, 36, 9, "f64", True, False, False, None),
         (24, 36, 8, "f64", True, True, True, None),        # L even: K4's ODDTOP march
         (24, 36, 9, "f64", False, True, False, "2"),
         (24, 36, 8, "f64", False, False, True, "2"),
         (48, 1440, 24, "f64", True, True, True, None),     # several 62-column tiles of K4, 64-column ones here
         (48, 1440, 24, "f64", True, False, False, None),
         (48, 1440, 9, "f64", True, False, True, "2")]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_tracer_equal_to_q_stays_q_bit_for_bit(g, case, monkeypatch):
    """a tracer set to q stays q bit for bit: 5 full steps, then one predictor (the star set)"""
    H, W, L, dtype, filt, cor, bump, seg = case
    if seg:
        monkeypatch.setenv("GCM_PE_LEVEL_SEGMENTS", seg)
    geom = su.geom_of(H, W, L, bump=bump)
    p, u, v, t, q = inp.state(geom, 7)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, filter=filt, coriolis=cor, dtype=dtype)
    c.set_state(p, u, v, t, q)
    other = 1.0 + np.random.default_rng(1).random((L, H, W))
    c.set_tracers(np.stack([q, other, q]))                   # chunks of 2 and 1: q in both
    assert c.tracer_count == 3
    c.step(5, 120.0)
    qs = c.get_state()[4]
    tr = c.get_tracers()
    assert np.array_equal(tr[0], qs) and np.array_equal(tr[2], qs)
    assert not np.array_equal(tr[1], other)                  # it moved
    c.half_step(0, 120.0)
    qstar = c.get_star((4,))[4]
    trs = c.get_tracers(star=True)
    assert np.array_equal(trs[0], qstar) and np.array_equal(trs[2], qstar)
    c.half_step(1, 120.0)
    assert np.array_equal(c.get_tracers()[0], c.get_state()[4])
    c.close()


@pytest.mark.parametrize("hwl,steps", [((24, 36, 9), 5), ((720, 1440, 24), 3)])
def test_tracers_vs_oracle(g, hwl, steps):
    """three distinct tracers against the oracle's matsuno_timestep run with q := c (no new oracle code), and the
    star set against the oracle's half_timestep (predictor)"""
    from oracle import dynamics as od, geometry as ogeo
    H, W, L = hwl
    geom = su.geom_of(H, W, L)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    st = inp.state(geom, 3)
    trs = _tracers3(H, W, L, 4)
    dt = 60.0
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*st)
    c.set_tracers(trs)
    c.half_step(0, dt)
    star = c.get_tracers(star=True)
    c.half_step(1, dt)
    c.step(steps - 1, dt)
    got = c.get_tracers()
    c.close()
    for n in range(3):
        if W <= 64:                                          # (an oracle stage at C4 takes ~10 s of CPU)
            want_star = od.half_timestep(*st[:4], trs[n], *st[:4], trs[n], dt, og)[4]
            assert rel_err(star[n], want_star) < TOL, ("star", n)
        s = (*st[:4], trs[n])
        for _ in range(steps):
            s = od.matsuno_timestep(*s, dt, og)
        assert rel_err(got[n], s[4]) < TOL, n


def test_fp32_tracers_vs_oracle(g):
    """the fp32 handle's tracers after one step, within the fp32 tolerance of test_fp32_tolerance_sweep"""
    from oracle import dynamics as od, geometry as ogeo
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L)
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    st = inp.state(geom, 5)
    trs = _tracers3(H, W, L, 6)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype="f32")
    c.set_state(*st)
    c.set_tracers(trs)
    c.step(1, 60.0)
    got = c.get_tracers()
    c.close()
    for n in range(3):
        want = od.matsuno_timestep(*st[:4], trs[n], 60.0, og)[4]
        assert rel_err(got[n], want) < F32_TOL, n


@pytest.mark.parametrize("physics", [False, True])
def test_tracers_are_passive_and_zero_costs_nothing(g, physics):
    """p, u, v, t, q after 5 steps are bit-identical between a handle with 4 tracers, one with n = 0 set and one that
    never heard of tracers"""
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L, bump=True)
    st = inp.state(geom, 9)
    gt = 288.0 + np.random.default_rng(3).standard_normal((H, W))
    res = []
    for mode in ("four", "zero", "never"):
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
        c.set_state(*st)
        if physics:
            c.set_ground(gt)
            c.set_physics(geom, 3600.0)
        if mode == "four":
            c.set_tracers(1.0 + np.random.default_rng(2).random((4, L, H, W)))
        elif mode == "zero":
            c.set_tracers(np.empty((0, L, H, W)))
            assert c.tracer_count == 0
        c.step(5, 300.0)
        res.append(c.get_state())
        if mode == "four":
            assert c.get_tracers().shape == (4, L, H, W)
        c.close()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("physics", [False, True])
def test_tracers_single_stream_vs_two_streams(g, physics, monkeypatch):
    """C4 size, 4 steps: the tracers (on the second stream beside K3 / K4 by default) are bit-identical to a run
    with every kernel on one stream (GCM_PE_SINGLE_STREAM=1)"""
    H, W, L = 720, 1440, 24
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 13)
    trs = _tracers3(H, W, L, 14)
    gt = 288.0 + np.random.default_rng(3).standard_normal((H, W))
    res = {}
    for single in ("0", "1"):
        monkeypatch.setenv("GCM_PE_SINGLE_STREAM", single)
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
        c.set_state(*st)
        if physics:
            c.set_ground(gt)
            c.set_physics(geom, 0.0)
        c.set_tracers(trs)
        c.step(4, 60.0)
        res[single] = (c.get_tracers(), c.get_state()[4])
        c.close()
    assert np.array_equal(res["0"][0], res["1"][0])
    assert np.array_equal(res["0"][1], res["1"][1])


def test_checkpoint_resume_with_tracers_bit_exact(g, tmp_path):
    """save after step 2, restore, step 4 == the uninterrupted run bit for bit, tracers included; a file without
    tracers loads as before"""
    from gcmiipy_amd import checkpoint
    d = golden("g8_pe25d")
    H, W, L = 24, 36, 9
    geom = su.geom_of(H, W, L)
    ic = [d["dense_%s0" % k] for k in "puvtq"]
    trs = _tracers3(H, W, L, 8)
    a = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    a.set_state(*ic)
    a.set_tracers(trs)
    a.step(2, 300.0)
    path = str(tmp_path / "ck.npz")
    checkpoint.save(path, a, step=2, time=600.0, geom=geom)
    a.step(2, 300.0)
    want, want_tr = a.get_state(), a.get_tracers()
    a.set_tracers(None)
    plain = str(tmp_path / "plain.npz")
    checkpoint.save(plain, a, step=4, geom=geom)
    a.close()
    b, ck = checkpoint.restore(path)
    assert ck["tracers"].shape == (3, L, H, W) and b.tracer_count == 3
    b.step(2, 300.0)
    for x, y in zip(b.get_state(), want):
        assert np.array_equal(x, y)
    assert np.array_equal(b.get_tracers(), want_tr)
    b.close()
    c, ck2 = checkpoint.restore(plain)
    assert ck2["tracers"] is None and c.tracer_count == 0
    c.close()


def test_dropins_carry_tracers(g):
    """dynamics.matsuno_timestep / run and no_limits_2_5d.run_model with tracers=: the state is what it is without
    them, and a tracer equal to q comes back equal to q"""
    from gcmiipy_amd import dynamics, no_limits_2_5d
    H, W, L = 12, 20, 5
    geom = su.geom_of(H, W, L)
    st = inp.state(geom, 21)
    trs = np.stack([st[4], np.ones((L, H, W))])
    plain = dynamics.matsuno_timestep(*st, 60.0, geom)
    out = dynamics.matsuno_timestep(*st, 60.0, geom, tracers=trs)
    assert len(out) == 6
    for a, b in zip(out[:5], plain):
        assert np.array_equal(a, b)
    assert np.array_equal(out[5][0], out[4])
    assert np.array_equal(dynamics.matsuno_timestep(*st, 60.0, geom)[4], plain[4])   # the cached handle forgot them
    r = dynamics.run(*st, 60.0, geom, 3, tracers=trs)
    r0 = dynamics.run(*st, 60.0, geom, 3)
    for a, b in zip(r[:5], r0):
        assert np.array_equal(a, b)
    assert np.array_equal(r[5][0], r[4])
    m = no_limits_2_5d.run_model(8, 8, 3, 1800.0, 3, None, stats={k: [] for k in ("u_max", "u_min", "v_max", "v_min", "ke")},
                                 tracers=np.ones((1, 3, 8, 8)))
    m0 = no_limits_2_5d.run_model(8, 8, 3, 1800.0, 3, None, stats={k: [] for k in ("u_max", "u_min", "v_max", "v_min", "ke")})
    assert len(m) == 8 and m[7].shape == (1, 3, 8, 8)
    for a, b in zip(m[:5], m0[:5]):
        assert np.array_equal(a, b)


def test_tracer_refusals(g):
    import ctypes as C
    from gcmiipy_amd.core import GcmError
    lib = g._lib.lib
    H, W, L = 12, 20, 5
    geom = su.geom_of(H, W, L)
    band = g.Core(g._lib.PE25D, W, H // 2, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0)
    x = np.ones((1, L, H // 2, W))
    assert lib.gcm_set_tracers(band._h, 1, x.ctypes.data_as(C.c_void_p)) == g._lib.ERR_UNSUPPORTED
    band.close()
    sw = g.Core(g._lib.SW2D, 32, 16, dx=300e3)
    with pytest.raises(GcmError, match="GCM_PE25D only"):
        sw.set_tracers(np.ones((1, 1, 16, 32)))
    assert lib.gcm_get_tracers(sw._h, 0, None) == g._lib.ERR_UNSUPPORTED
    sw.close()
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom)
    c.set_state(*inp.state(geom, 1))
    big = np.ones((17, L, H, W))
    assert lib.gcm_set_tracers(c._h, 17, big.ctypes.data_as(C.c_void_p)) == g._lib.ERR_ARG
    assert lib.gcm_set_tracers(c._h, -1, None) == g._lib.ERR_ARG
    with pytest.raises(ValueError):
        c.set_tracers(big)
    with pytest.raises(ValueError):
        c.set_tracers(np.ones((2, L, H, W + 1)))
    c.set_tracers(np.ones((2, L, H, W)))
    assert lib.gcm_get_tracers(c._h, 1, np.empty((2, L, H, W)).ctypes.data_as(C.c_void_p)) == g._lib.ERR_STATE
    with pytest.raises(GcmError, match="no predicted tracers"):
        c.get_tracers(star=True)
    assert lib.gcm_get_tracers(c._h, 2, np.empty((2, L, H, W)).ctypes.data_as(C.c_void_p)) == g._lib.ERR_ARG
    c.step(1, 60.0)
    with pytest.raises(GcmError, match="no predicted tracers"):
        c.get_tracers(star=True)                          # a full step leaves no predicted state, as gcm_get_star
    c.set_tracers(None)
    assert c.tracer_count == 0 and c.get_tracers().shape == (0, L, H, W)
    c.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_resizing_the_tracer_set_on_one_handle(g, dtype):
    """one single-domain handle through 2 forced tracers -> 3 -> the same 3 again -> none: another count takes new
    storage and drops the forcing, the same count keeps both, and at every point the tracers are bit for bit those of
    a fresh handle given the same inputs; after n = 0 the state steps as on a handle that never had tracers"""
    lib = g._lib.lib
    L, H, W = 3, 8, 16
    geom = su.geom_of(H, W, L)
    rng = np.random.default_rng(31)
    emis = 1e-3 * rng.random((L, H, W))
    pin = np.zeros((L, H, W), dtype=bool)
    pin[0, 2:4, 5:9] = True
    force = dict(source=0.5, decay=1e-4, emission=emis, pin_mask=pin, pin_value=3.0)
    tr2, tr3, tr3b = (1.0 + rng.random((n, L, H, W)) for n in (2, 3, 3))

    def fresh(state, tracers, forced):
        """-> (tracers as set, tracers and state after one step) of a new handle"""
        f = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
        f.set_state(*state)
        if tracers is not None:
            f.set_tracers(tracers)
        if forced is not None:
            f.set_tracer_forcing(forced, **force)
        at_set = f.get_tracers()
        f.step(1, 60.0)
        out = at_set, f.get_tracers(), f.get_state()
        f.close()
        return out

    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
    st = inp.state(geom, 30)
    c.set_state(*st)
    c.set_tracers(tr2)
    c.set_tracer_forcing(1, **force)
    assert [lib.gcm_tracer_forced(c._h, i) for i in range(2)] == [0, 1]
    want = fresh(st, tr2, 1)
    assert np.array_equal(c.get_tracers(), want[0])
    c.step(1, 60.0)
    assert np.array_equal(c.get_tracers(), want[1])
    # another count: new storage, and the forcing went with the old tracers
    st = c.get_state()
    c.set_tracers(tr3)
    assert c.tracer_count == 3 and [lib.gcm_tracer_forced(c._h, i) for i in range(3)] == [0, 0, 0]
    want = fresh(st, tr3, None)
    assert np.array_equal(c.get_tracers(), want[0])
    c.step(1, 60.0)
    assert np.array_equal(c.get_tracers(), want[1])
    # the same count: the storage and a forcing registered in between stay
    st = c.get_state()
    c.set_tracer_forcing(2, **force)
    c.set_tracers(tr3b)
    assert c.tracer_count == 3 and [lib.gcm_tracer_forced(c._h, i) for i in range(3)] == [0, 0, 1]
    want = fresh(st, tr3b, 2)
    assert np.array_equal(c.get_tracers(), want[0])
    c.step(1, 60.0)
    assert np.array_equal(c.get_tracers(), want[1])
    assert not np.array_equal(want[1][2], fresh(st, tr3b, None)[1][2])     # (the forcing does act at this size)
    # none: the state goes on as on a handle that never had tracers
    st = c.get_state()
    c.set_tracers(None)
    assert c.tracer_count == 0 and c.get_tracers().shape == (0, L, H, W)
    assert lib.gcm_tracer_forced(c._h, 0) == g._lib.ERR_ARG
    c.step(1, 60.0)
    for a, b in zip(c.get_state(), fresh(st, None, None)[2]):
        assert np.array_equal(a, b)
    c.close()
