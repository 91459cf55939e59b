"""CPU tests of van Leer transport on GCM_PE25D latitude bands (gcm_set_band_tracer_rows): the checks of
Core(band_tracer_rows=...) that run before any device use, the new entry points' refusal of a null handle, the
exchange-byte model of tools/tools_band_time.py at depth 2 against the header's formula, and the teeth of the GPU parity
inputs: on the seeded state and tracers of tests/test_pe25d_band_van_leer_gpu.py a band fed one ghost row per side
cannot produce the single domain's bits, a band fed two does."""
import importlib.util
import os
import types

import numpy as np
import pytest

import pe25d_inputs as inp
import pe25d_tracer_schemes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tools_band_time", os.path.join(ROOT, "tools", "tools_band_time.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_band_tracer_rows_argument_checks_before_create():
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import Core
    from gcmiipy_amd.geometry import gen_geometry, manabe_sig
    geom = gen_geometry(12, 20, 5, sig_func=manabe_sig)
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.PE25D, 20, 12, 5, geom=geom, band_tracer_rows=2)                   # a single domain
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.SW2D, 130, 8, dx=300e3, nranks=2, rank=0, global_height=16, band_tracer_rows=2)
    with pytest.raises(ValueError, match="latitude band"):
        Core(_lib.PE2D, 20, 6, 1, nranks=2, rank=0, global_height=12, band_tracer_rows=2)
    for bad in (0, 3, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="band_tracer_rows"):
            Core(_lib.PE25D, 20, 6, 5, geom=geom, nranks=2, rank=0, global_height=12, band_tracers=1, band_tracer_rows=bad)


def test_band_tracer_rows_entry_points_refuse_a_null_handle():
    """(on the parent commit the symbols do not exist)"""
    from gcmiipy_amd import _lib
    assert "gcm_set_band_tracer_rows" in _lib.SYMBOLS and "gcm_band_tracer_rows" in _lib.SYMBOLS
    assert _lib.lib.gcm_set_band_tracer_rows(None, 2) == _lib.ERR_ARG
    assert _lib.lib.gcm_band_tracer_rows(None) == _lib.ERR_ARG


def test_exchange_byte_model_at_depth_two():
    m = _tool()
    W, L = 1440, 24
    for esz in (8, 4):
        state = esz * 2 * W * (1 + 4 * L) + 8 * 2 * W
        for ntr in (0, 1, 4):
            for R in (1, 2):
                want = state + ntr * esz * R * L * W              # the header's formula for gcm_halo_bytes
                assert m.halo_bytes_pe25d(W, L, esz, ntr, R) == want == inp.halo_bytes(W, L, esz, ntr, R)
                assert m.halo_bytes_pe25d(W, L, esz, ntr, rows=R) == want
                assert m.exchange_bytes_per_step(W, L, esz, ntr, R) == 4 * want     # 2 exchanges x 2 sides
            assert m.halo_bytes_pe25d(W, L, esz, ntr) == m.halo_bytes_pe25d(W, L, esz, ntr, 1)
            assert m.exchange_bytes_per_step(W, L, esz, ntr) == m.exchange_bytes_per_step(W, L, esz, ntr, 1)


def _strip(a, r0, r1, G):
    """rows [r0 - G, r1 + G) of a (..., H, W) array, periodic in the row index as the single domain's Idx"""
    return np.take(a, np.arange(r0 - G, r1 + G), axis=-2, mode="wrap")


@pytest.mark.parametrize("band", [3, 0])
def test_one_ghost_row_cannot_give_the_single_domains_bits(band):
    """The parity inputs of the GPU tests have teeth.  One VANLEER predictor stage of the restatement on the seeded
    64 x 1440 x 24 state and its 3 tracers, globally and on the strip a band holds (its own rows plus two TRUE ghost rows
    per side, mass fluxes as the band's state kernels form them from two ghost rows of state): the band's own rows are
    the global result bit for bit.  The same strip with the outer ghost row replaced by a copy of the inner one -- the
    most a one-row message could supply -- differs on the band's row 0 or row H - 1.

    band 3 (rows 24 .. 31): interior boundaries on both sides.  band 0: its north side is the pole boundary; v of the
    global last row is zero, so spv through the face between global rows H - 1 and 0 is zero and the depth-2 ghost
    values there carry zero weight (the face value is multiplied by a zero mass flux): there only the south side of
    band 0 can and must show the difference."""
    from oracle import geometry as ogeo
    c = inp.EIGHT
    H, W, L, nb, dt = c["H"], c["W"], c["L"], c["nb"], c["dt"]
    og = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    st = inp.state(og)
    trs = inp.tracers(H, W, L, c["ntr"])
    star, spu, spv, sd = ref.stage_fluxes(st, st, dt, og)
    p, p_n = st[0], star[0]
    glob = np.stack([ref.tracer_stage(x, x, p, p_n, spu, spv, sd, dt, og, ref.VANLEER) for x in trs])
    n = H // nb
    r0, r1 = band * n, (band + 1) * n
    G = 2
    sg = types.SimpleNamespace(dx_j=_strip(og.dx_j, r0, r1, G), dy=og.dy, dsig=og.dsig)
    sub = [_strip(a, r0, r1, G) for a in (p, p_n, spu, spv, sd)]

    def band_rows(strip_tr):
        # (np.roll wraps at the strip's ends: that reaches the ghost rows' results only, which are dropped)
        out = np.stack([ref.tracer_stage(x, x, *sub, dt, sg, ref.VANLEER) for x in strip_tr])
        return out[:, :, G:-G]

    true = _strip(trs, r0, r1, G)
    assert np.array_equal(band_rows(true), glob[:, :, r0:r1])
    one_row = true.copy()
    one_row[:, :, 0] = one_row[:, :, 1]
    one_row[:, :, -1] = one_row[:, :, -2]
    got = band_rows(one_row)
    assert np.array_equal(got[:, :, 2:-2], glob[:, :, r0 + 2:r1 - 2])      # rows that read own rows only
    north = not np.array_equal(got[:, :, 0], glob[:, :, r0])
    south = not np.array_equal(got[:, :, -1], glob[:, :, r1 - 1])
    assert north or south
    if band == 3:
        assert north and south
    else:
        assert south and not north                                          # zero weight across the pole boundary
