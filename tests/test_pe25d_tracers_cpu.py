"""CPU tests of the passive tracers' host side: the shape checks in front of gcm_set_tracers, the C entry points'
argument refusals without a handle, and the byte model of tools/tools_tracer_time.py."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tools_tracer_time", os.path.join(ROOT, "tools", "tools_tracer_time.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_tracer_array_shape_checks():
    from gcmiipy_amd import _lib
    from gcmiipy_amd.core import tracer_array
    L, H, W = 3, 4, 5
    a = tracer_array(np.ones((2, L, H, W), dtype=np.float32), L, H, W)
    assert a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (2, L, H, W)
    assert tracer_array(None, L, H, W).shape == (0, L, H, W)
    assert tracer_array(np.empty((0, L, H, W)), L, H, W).shape == (0, L, H, W)
    assert tracer_array(np.ones((_lib.MAX_TRACERS, L, H, W)), L, H, W).shape[0] == 16
    for bad in (np.ones((L, H, W)), np.ones((1, L, H, W + 1)), np.ones((1, L + 1, H, W)), np.ones((1, 1, L, H, W))):
        with pytest.raises(ValueError, match="tracers have shape"):
            tracer_array(bad, L, H, W)
    with pytest.raises(ValueError, match="at most 16"):
        tracer_array(np.ones((17, L, H, W)), L, H, W)


def test_tracer_entry_points_refuse_a_null_handle():
    from gcmiipy_amd import _lib
    lib = _lib.lib
    assert lib.gcm_set_tracers(None, 0, None) == _lib.ERR_ARG
    assert lib.gcm_get_tracers(None, 0, None) == _lib.ERR_ARG
    assert lib.gcm_tracer_count(None) == _lib.ERR_ARG


def test_tracer_byte_model():
    m = _tool()
    assert [m.chunks(n) for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 16)] == [0, 1, 1, 2, 1, 2, 2, 3, 2, 4]
    H, W, L = 720, 1440, 24
    cells = H * W * L
    assert m.tracer_bytes_per_step(H, W, L, 0) == 0
    # one fp64 tracer: 16 B per cell (predictor) + 24 B (corrector), plus spu, sv (3-D) and pit (2-D) per stage
    one = 40 * cells + 2 * (2 * cells + H * W) * 8
    assert m.tracer_bytes_per_step(H, W, L, 1) == one
    assert m.tracer_bytes_per_step(H, W, L, 4) == 4 * 40 * cells + 2 * (2 * cells + H * W) * 8
    assert m.tracer_bytes_per_step(H, W, L, 3, 4) == 3 * 20 * cells + 2 * 2 * (2 * cells + H * W) * 4
    # the issue's estimate at 4.5 TB/s: ~0.4 ms for one fp64 tracer on C4, ~1.1 ms for four
    assert 0.38 < one / 4.5e12 * 1e3 < 0.42
    assert 1.0 < m.tracer_bytes_per_step(H, W, L, 4) / 4.5e12 * 1e3 < 1.1
