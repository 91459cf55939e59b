"""CPU tests of the passive tracers' device monitor of GCM_PE25D (gcm_tracer_stats): the C and Python surface without
a device, bands.merge_tracer_stats on hand-made records, and -- on the NumPy restatement of the transport schemes
(tests/pe25d_tracer_schemes_ref.py) -- the claim the monitor's `mass` rests on: the UNWEIGHTED sum of c p dsig_k is
what every scheme conserves."""
import math
import os
import re

import numpy as np
import pytest

import pe25d_inputs as inp
import pe25d_tracer_schemes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def test_surface_without_a_device():
    """declared, exported, bound; a null handle or a null `out` is GCM_ERR_ARG before any device use"""
    import ctypes as C
    from gcmiipy_amd import _lib
    text = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+gcm_tracer_stats\s*\(\s*gcm_handle\s*\*\s*h\s*,\s*int\s+which\s*,\s*int\s+with_q\s*,"
                     r"\s*double\s*\*\s*out\s*,\s*int\s+cap\s*\)", src)
    m = re.search(r"#define\s+GCM_TRACER_STATS_WORDS\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.TRACER_STATS_WORDS == 6
    assert "gcm_tracer_stats" in _lib.SYMBOLS
    lib = _lib.lib
    assert hasattr(lib, "gcm_tracer_stats")
    out = np.full(12, 7.0)
    ptr = out.ctypes.data_as(C.c_void_p)
    for which in (0, 1):
        for with_q in (0, 1):
            assert lib.gcm_tracer_stats(None, which, with_q, ptr, 12) == _lib.ERR_ARG
    assert np.all(out == 7.0)
    # a null `out` is refused ahead of everything that would need the handle: an address that is no handle is never read
    assert lib.gcm_tracer_stats(None, 0, 0, None, 0) == _lib.ERR_ARG


def _rec(mn, mx, mass, air, neg, nan):
    from gcmiipy_amd.core import TracerStats
    f = lambda x: np.asarray(x, dtype=np.float64)
    return TracerStats(f(mn), f(mx), f(mass), f(air), np.asarray(neg, dtype=np.int64), np.asarray(nan, dtype=np.int64))


def test_merge_tracer_stats_on_hand_made_records():
    from gcmiipy_amd.bands import merge_tracer_stats
    from gcmiipy_amd.core import TracerStats
    a = _rec([1.0, -2.0, 0.5], [4.0, 3.0, 0.5], [10.0, 0.1, 1.0], [100.0] * 3, [0, 5, 0], [0, 0, 0])
    b = _rec([0.5, np.nan, 0.5], [3.0, np.nan, 0.75], [20.0, np.nan, 2.0], [50.0] * 3, [1, 2, 0], [0, 3, 0])
    c = _rec([2.0, -7.0, -0.25], [9.0, 1.0, 0.5], [30.0, 0.2, 4.0], [25.0] * 3, [0, 1, 2], [0, 0, 0])
    m = merge_tracer_stats([a, b, c])
    assert isinstance(m, TracerStats)
    assert np.array_equal(m.min, [0.5, np.nan, -0.25], equal_nan=True)          # a NaN band makes the field's min NaN
    assert np.array_equal(m.max, [9.0, np.nan, 0.75], equal_nan=True)
    assert np.array_equal(m.mass[[0, 2]], [(10.0 + 20.0) + 30.0, (1.0 + 2.0) + 4.0]) and np.isnan(m.mass[1])
    assert np.array_equal(m.air, [175.0] * 3)
    assert np.array_equal(m.negative, [1, 8, 2]) and np.array_equal(m.nan, [0, 3, 0])
    assert m.negative.dtype == np.int64 and m.nan.dtype == np.int64
    assert m.min.dtype == m.max.dtype == m.mass.dtype == m.air.dtype == np.float64
    # the NaN band first or last: the same answer
    for order in ([b, a, c], [a, c, b]):
        o = merge_tracer_stats(order)
        assert np.array_equal(o.min, m.min, equal_nan=True) and np.array_equal(o.max, m.max, equal_nan=True)
        assert np.array_equal(o.negative, m.negative) and np.array_equal(o.nan, m.nan)
    # the sums run in list order
    x, y, z = 1.0, 2.0 ** -53, 2.0 ** -53
    recs = [_rec([0.0], [0.0], [v], [v], [0], [0]) for v in (x, y, z)]
    assert merge_tracer_stats(recs).mass[0] == (x + y) + z != x + (y + z)
    assert merge_tracer_stats(recs[::-1]).mass[0] == (z + y) + x
    one = merge_tracer_stats([a])
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(one, a))
    e = merge_tracer_stats([_rec([], [], [], [], [], []), _rec([], [], [], [], [], [])])      # bands without tracers
    assert e.min.shape == (0,) and e.negative.dtype == np.int64
    with pytest.raises(ValueError):
        merge_tracer_stats([])
    with pytest.raises(ValueError):
        merge_tracer_stats([a, _rec([1.0], [1.0], [1.0], [1.0], [0], [0])])


def test_tracer_stats_mean():
    from gcmiipy_amd import TracerStats
    s = _rec([0.0, 1.0], [2.0, 3.0], [6.0, 1.0], [4.0, 4.0], [0, 0], [0, 0])
    assert isinstance(s, TracerStats) and s._fields == ("min", "max", "mass", "air", "negative", "nan")
    assert np.array_equal(s.mean, [1.5, 0.25])
    assert np.array_equal(s.mean, s.mass / s.air)


@pytest.mark.parametrize("scheme", [ref.NONE, ref.UPWIND, ref.VANLEER])
def test_unweighted_mass_is_conserved_by_the_restatement(scheme):
    """12 x 16 x 5, manabe sigma, a random state, 3 tracers, 3 Matsuno steps: sum c p dsig_k after the steps lies
    within (N + 2) 2^-53 sum |c p dsig_k| of the value before (N cells; any order of summation stays inside, and two
    product roundings per term) -- measured change: exactly 0.0 relative under all three schemes.  The update is in
    flux form and the meridional flux divergence carries 1 / dy only, so the sum telescopes WITHOUT a row weight;
    weighted by the row's dx_j it drifts by 1e-8 .. 1e-6, which is why gcm_tracer_stats reports the unweighted sum."""
    from oracle import geometry as ogeo
    H, W, L = 12, 16, 5
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    rng = np.random.default_rng(21)
    p, u, v, t, q = inp.state(og, rng)
    c0 = np.stack([1.0 + rng.random((L, H, W)), rng.standard_normal((L, H, W)), np.full((L, H, W), 2.5)])
    c0[1, :, H // 3: 2 * H // 3] += 1.0
    dsig = np.asarray(og.dsig, dtype=np.float64).reshape(L, 1, 1)
    st1, c1 = ref.run((p, u, v, t, q), c0, 120.0, og, 3, scheme)
    assert not np.array_equal(c1[0], c0[0]) and not np.array_equal(st1[0], p)
    N = L * H * W
    for n in range(3):
        before = (c0[n] * p * dsig).ravel()
        after = (c1[n] * st1[0] * dsig).ravel()
        m0, m1 = math.fsum(before), math.fsum(after)
        bound = (N + 2) * U * math.fsum(np.abs(before))
        print("scheme %d tracer %d: mass %.17g -> %.17g, |change| %.3e, bound %.3e" % (scheme, n, m0, m1, abs(m1 - m0), bound))
        assert abs(m1 - m0) <= bound, (scheme, n)
