"""The Held-Suarez forcing of GCM_PE25D without a GPU: the symbols and the struct of include/gcmcore.h, the handle-free
table routine gcm_held_suarez_tables against the NumPy restatement (tests/pe25d_held_suarez_ref.py), every validation
error a call can report without a device, and the restatement's own properties.  What needs a handle (the errors of
gcm_set_held_suarez on a live handle, other models): tests/test_pe25d_held_suarez_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pe25d_held_suarez_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24, 36, 9), (6, 10, 3))                       # (H, W, L) of the tracer tests
NEW = ("gcm_set_held_suarez", "gcm_held_suarez_on", "gcm_held_suarez_step", "gcm_held_suarez_tables")


def _geom(H, W, L):
    from gcmiipy_amd import geometry
    return geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)


def _sig_lat(H, W, L):
    g = _geom(H, W, L)
    sig, lat = np.asarray(g.sig, dtype=np.float64).reshape(-1), np.asarray(g.lat, dtype=np.float64).reshape(-1)
    r = ref.r_of(sig, ref.DEFAULTS["sigma_b"])
    assert (r > 0).any() and (r == 0).any(), "the geometry needs a friction level and a free level"
    return sig, lat


def ulp_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def test_symbols_are_exported_and_bound():
    from gcmiipy_amd import _lib
    import gcmiipy_amd
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(gcmiipy_amd.held_suarez_tables)
    for name in ("set_held_suarez", "held_suarez_step", "held_suarez"):
        assert hasattr(gcmiipy_amd.Core, name), name


def test_struct_layout_matches_header():
    """the ctypes mirror of gcm_held_suarez follows the header field for field (the pattern of test_abi_cpu.py)"""
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import HELD_SUAREZ_DEFAULTS
    src = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    end = src.index("} gcm_held_suarez;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        names = decl.split(",")
        fields.append(names[0].split()[-1].lstrip("*"))
        fields += [n.strip().lstrip("*") for n in names[1:]]
    assert fields == [f[0] for f in _lib.HeldSuarez._fields_]
    assert ctypes.sizeof(_lib.HeldSuarez) == 8 * 8 + 8
    assert list(HELD_SUAREZ_DEFAULTS) == fields[:8]
    assert dict(HELD_SUAREZ_DEFAULTS) == ref.DEFAULTS


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("over", [{}, dict(sigma_b=0.45, k_f=3e-5, k_a=2e-7, k_s=5e-6), dict(k_f=0.0, k_a=0.0, k_s=0.0)])
def test_tables_equal_the_restatement(shape, over):
    """fu is pure arithmetic: bit for bit.  s2, c2 and kt within 16 ulp: libm's and NumPy's cos / sin may each differ by
    an ulp, and the fourth power multiplies that"""
    import gcmiipy_amd as g
    sig, lat = _sig_lat(*shape)
    for dt in (60.0, 1800.0, 0.37):
        got = g.held_suarez_tables(sig, lat, dt, **over)
        want = ref.tables(sig, lat, dt, **over)
        assert got["fu"].shape == (shape[2],) and got["kt"].shape == (shape[2], shape[0])
        assert np.array_equal(got["fu"], want["fu"])
        for k in ("s2", "c2", "kt"):
            assert ulp_diff(got[k], want[k]) <= 16, (k, ulp_diff(got[k], want[k]))
        assert (got["fu"] > 0).all() and (got["fu"] <= 1).all() and (got["kt"] >= 0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_r_is_bit_for_bit(shape):
    """the routine hands out no r of its own; with k_a = 0, k_s = 1 at the equator (c2 = 1 exactly) kt IS r, and with
    dt k_f = 1 fu = 1 / (1 + r): both bit for bit the restatement's"""
    import gcmiipy_amd as g
    sig, _ = _sig_lat(*shape)
    for sigma_b in (0.7, 0.45, 0.0):
        got = g.held_suarez_tables(sig, np.zeros(1), 1.0, k_a=0.0, k_s=1.0, k_f=1.0, sigma_b=sigma_b)
        r = ref.r_of(sig, sigma_b)
        assert np.array_equal(got["kt"][:, 0], r)
        assert np.array_equal(got["fu"], 1.0 / (1.0 + r))


def _raw_tables(L=3, nlat=4, sig=True, lat=True, hs=True, dt=60.0, out=True, **over):
    from gcmiipy_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    s = np.linspace(0.9, 0.1, max(L, 1))
    la = np.linspace(-1.2, 1.2, max(nlat, 1))
    rec = _lib.HeldSuarez(*ref.params(**over).values())
    rec.lat = la.ctypes.data_as(dp)
    bufs = [np.full(max(L, 1) * max(nlat, 1), 7.0) for _ in range(4)]
    ptr = lambda a, on=True: a.ctypes.data_as(dp) if on else None
    rc = _lib.lib.gcm_held_suarez_tables(L, ptr(s, sig), nlat, ptr(la, lat), ctypes.byref(rec) if hs else None, dt,
                                         ptr(bufs[0], out), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]))
    return rc, _lib.lib.gcm_last_error(None).decode(), bufs


def test_validation_errors_without_a_handle():
    """every parameter error of the contract, through the handle-free routine (gcm_set_held_suarez and
    gcm_held_suarez_step run the same check); the message comes from gcm_last_error(NULL); nothing is written"""
    from gcmiipy_amd import _lib
    assert _raw_tables()[0] == _lib.OK
    nan, inf = float("nan"), float("inf")
    bad = [dict(k_f=-1e-9), dict(k_a=-1.0), dict(k_s=-1e-300), dict(sigma_b=1.0), dict(sigma_b=-0.01), dict(sigma_b=1.5)]
    bad += [{k: x} for k in ref.DEFAULTS for x in (nan, inf, -inf)]
    for over in bad:
        rc, msg, bufs = _raw_tables(**over)
        assert rc == _lib.ERR_ARG and "gcm_held_suarez_tables" in msg, (over, rc, msg)
        assert all((b == 7.0).all() for b in bufs), over
    for kw in (dict(L=0), dict(nlat=0), dict(sig=False), dict(lat=False), dict(hs=False), dict(out=False), dict(dt=nan),
               dict(dt=inf)):
        rc, msg, bufs = _raw_tables(**kw)
        assert rc == _lib.ERR_ARG and msg, (kw, rc, msg)
        assert all((b == 7.0).all() for b in bufs), kw
    # sigma_b = 0 and the rates' zero are legal
    assert _raw_tables(sigma_b=0.0, k_f=0.0, k_a=0.0, k_s=0.0)[0] == _lib.OK


def test_null_handle_is_an_argument_error():
    from gcmiipy_amd import _lib
    lat = np.zeros(4)
    rec = _lib.HeldSuarez(*ref.DEFAULTS.values())
    rec.lat = lat.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert _lib.lib.gcm_set_held_suarez(None, ctypes.byref(rec)) == _lib.ERR_ARG
    assert _lib.lib.gcm_set_held_suarez(None, None) == _lib.ERR_ARG
    assert _lib.lib.gcm_held_suarez_on(None) == _lib.ERR_ARG
    assert _lib.lib.gcm_held_suarez_step(None, 60.0, ctypes.byref(rec)) == _lib.ERR_ARG


def test_python_layer_refuses_unknown_parameters():
    import gcmiipy_amd as g
    with pytest.raises(ValueError, match="unknown parameter"):
        g.held_suarez_tables(np.array([0.9, 0.5]), np.zeros(2), 60.0, k_x=1.0)
    with pytest.raises(ValueError):
        g.held_suarez_tables(np.array([0.9, 0.5]), np.zeros(2), 60.0, sigma_b=1.0)


def _state(H, W, L, ptop=0.0, seed=3):
    rng = np.random.default_rng(seed)
    sig, lat = _sig_lat(H, W, L)
    p = 1e5 - ptop + 2000 * rng.standard_normal((H, W))
    u, v = 10 * rng.standard_normal((L, H, W)), 10 * rng.standard_normal((L, H, W))
    t = (280 + 30 * rng.standard_normal((L, H, W))) * ((1e5 / (p * sig[:, None, None] + ptop)) ** ref.KAPPA)
    return p, u, v, t, sig, lat


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ptop", [0.0, 1000.0])
def test_restatement_properties(shape, ptop):
    """backward Euler: theta ends between theta and theta_eq, |u| does not grow, levels with r = 0 keep their winds, n
    applications of the friction are fu**n within rounding -- for a small and for a huge dt"""
    H, W, L = shape
    p, u, v, t, sig, lat = _state(H, W, L, ptop)
    te = ref.theta_eq(p, sig, ptop, lat)
    for dt in (60.0, 86400.0 * 1000):
        un, vn, tn = ref.step(p, u, v, t, sig, ptop, lat, dt)
        lo, hi = np.minimum(t, te), np.maximum(t, te)
        eps = 4 * np.spacing(hi)
        assert (tn >= lo - eps).all() and (tn <= hi + eps).all()
        assert (np.abs(tn - te) <= np.abs(t - te) + eps).all()
        assert (np.abs(un) <= np.abs(u)).all() and (np.abs(vn) <= np.abs(v)).all()
        T = ref.tables(sig, lat, dt)
        free = T["r"] == 0
        assert np.array_equal(un[free], u[free]) and np.array_equal(vn[free], v[free])
        assert (np.abs(un[~free]) < np.abs(u[~free])).all()
    n, dt = 7, 600.0
    uk, vk, tk = u, v, t
    for _ in range(n):
        uk, vk, tk = ref.step(p, uk, vk, tk, sig, ptop, lat, dt)
    fu = ref.tables(sig, lat, dt)["fu"][:, None, None]
    assert np.allclose(uk, u * fu ** n, rtol=4 * n * np.finfo(np.float64).eps, atol=0)
    assert np.allclose(vk, v * fu ** n, rtol=4 * n * np.finfo(np.float64).eps, atol=0)


def test_restatement_f32_rounds_once():
    H, W, L = SHAPES[1]
    p, u, v, t, sig, lat = _state(H, W, L)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    p, u, v, t = f32(p), f32(u), f32(v), f32(t)
    un, vn, tn = ref.step(p, u, v, t, sig, 0.0, lat, 600.0, dtype="f32")
    ud, vd, td = ref.step(p, u, v, t, sig, 0.0, lat, 600.0)
    for a, b in ((un, ud), (vn, vd), (tn, td)):
        assert np.array_equal(a, f32(b))
