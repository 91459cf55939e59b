"""CPU tests of the passive tracers on GCM_PE25D latitude bands: the checks of Core(band_tracers=...) that run before
any device use, the C entry point's refusal of a null handle, and the exchange-byte model of tools/tools_band_time.py
(which must agree with the formula the header documents for gcm_halo_bytes)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tools_band_time", os.path.join(ROOT, "tools", "tools_band_time.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_band_tracers_argument_checks_before_create():
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import Core
    from gcmiipy_amd.geometry import gen_geometry, manabe_sig
    geom = gen_geometry(12, 20, 5, sig_func=manabe_sig)
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.PE25D, 20, 12, 5, geom=geom, band_tracers=1)                       # a single domain
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.SW2D, 130, 8, dx=300e3, nranks=2, rank=0, global_height=16, band_tracers=1)
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.PE2D, 20, 6, 1, nranks=2, rank=0, global_height=12, band_tracers=2)
    for bad in (-1, _lib.MAX_TRACERS + 1):
        with pytest.raises(ValueError, match="band_tracers"):
            Core(_lib.PE25D, 20, 6, 5, geom=geom, nranks=2, rank=0, global_height=12, band_tracers=bad)


def test_band_tracers_entry_point_refuses_a_null_handle():
    from gcmiipy_amd import _lib
    assert _lib.lib.gcm_set_band_tracers(None, 1) == _lib.ERR_ARG


def test_exchange_byte_model():
    m = _tool()
    W, L = 1440, 24
    state = 8 * 2 * W * (1 + 4 * L) + 8 * 2 * W              # p, u, v, t, q (2 rows) + the ground temperature
    assert m.halo_bytes_pe25d(W, L, 8) == state
    assert m.halo_bytes_pe25d(W, L, 8, 4) == state + 4 * 8 * L * W        # one row x L levels per tracer
    assert m.halo_bytes_pe25d(W, L, 4, 1) == 4 * 2 * W * (1 + 4 * L) + 8 * 2 * W + 4 * L * W
    assert m.exchange_bytes_per_step(W, L, 8, 1) == 4 * m.halo_bytes_pe25d(W, L, 8, 1)   # 2 exchanges x 2 sides
