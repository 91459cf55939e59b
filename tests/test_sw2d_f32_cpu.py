"""CPU-side checks of the fp32 2-D handles (gcm_config.dtype = GCM_F32 on GCM_SW2D / GCM_SW2D_TEMP): the
Python surface takes `dtype`, a bad one is refused before any device use, gcm_create refuses a bad dtype and an
odd-width fp32 band ahead of the device check, and the header says which models honour the field."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(model, dtype, width=32, nranks=1):
    from gcmiipy_amd import _lib
    cfg = _lib.Config()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.model = model
    cfg.width, cfg.height, cfg.layers = width, 16, 1
    cfg.dx = 300e3
    cfg.nranks, cfg.rank, cfg.global_height = nranks, 0, 16 * nranks
    cfg.device = -1
    cfg.dtype = dtype
    h = _lib._H()
    rc = _lib.lib.gcm_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == _lib.OK:
        _lib.lib.gcm_destroy(h)
    return rc, _lib.lib.gcm_last_error(None).decode()


def test_config_layout_unchanged():
    from gcmiipy_amd import _lib
    assert ctypes.sizeof(_lib.Config) == 168 and _lib.ABI_VERSION == 1


def test_header_names_the_models_that_honour_dtype():
    src = open(os.path.join(ROOT, "include", "gcmcore.h")).read()
    m = re.search(r"int32_t dtype;\s*/\*(.*?)\*/", src, flags=re.S)
    assert m, "no dtype comment"
    text = " ".join(m.group(1).split())
    for model in ("GCM_PE25D", "GCM_SW2D", "GCM_SW2D_TEMP"):
        assert re.search(r"\b%s\b" % model, text), model
    assert "GCM_PE25D only" not in text
    assert "GCM_PE2D" in text and "fp64" in text         # the model that stays fp64 is named too


def test_create_refuses_bad_dtype_and_odd_fp32_bands_before_device_use():
    from gcmiipy_amd import _lib
    for model in (_lib.SW2D, _lib.SW2D_TEMP):
        rc, msg = _create(model, 7)
        assert rc == _lib.ERR_ARG and "dtype" in msg, (rc, msg)
        rc, msg = _create(model, _lib.F32, width=131, nranks=2)
        assert rc == _lib.ERR_UNSUPPORTED and "even width" in msg, (rc, msg)


def test_create_without_device_still_says_so():
    """fp32 2-D configs that pass the argument checks meet the device check: single domain, even bands"""
    from gcmiipy_amd import _lib
    if _lib.lib.gcm_device_count() != 0:
        pytest.skip("a HIP device is present")
    for model in (_lib.SW2D, _lib.SW2D_TEMP):
        for width, nranks in ((31, 1), (32, 2)):
            rc, msg = _create(model, _lib.F32, width=width, nranks=nranks)
            assert rc == _lib.ERR_NODEVICE, (model, width, nranks, rc, msg)


def test_core_refuses_bad_dtype_before_device_use():
    import gcmiipy_amd as g
    for bad in ("f16", "float32", None, 1):
        with pytest.raises(ValueError, match="dtype"):
            g.Core(g._lib.SW2D, 32, 16, dx=1.0, dtype=bad)
    with pytest.raises(g.GcmError, match="even width"):
        g.Core(g._lib.SW2D_TEMP, 31, 16, dx=1.0, dtype="f32", nranks=2, rank=0, global_height=32)


def test_drop_ins_take_dtype_keyword_only():
    from gcmiipy_amd import ensemble, matsumo_temp, matsuno_c_grid
    fns = (matsuno_c_grid.matsumo_scheme, matsuno_c_grid.run, matsuno_c_grid.courant_number,
           matsumo_temp.matsumo_scheme, matsumo_temp.matsumo_scheme_with_tracer, matsumo_temp.run_with_callbacks,
           ensemble.matsumo_scheme, ensemble.matsumo_temp_scheme, ensemble.run, ensemble.courant_numbers)
    for fn in fns:
        p = inspect.signature(fn).parameters.get("dtype")
        assert p is not None and p.kind == p.KEYWORD_ONLY and p.default == "f64", fn.__qualname__


def test_drop_ins_refuse_bad_dtype_before_device_use():
    from gcmiipy_amd import ensemble, matsumo_temp, matsuno_c_grid
    z2, z3 = np.zeros((4, 5)), np.zeros((2, 4, 5))
    calls = [lambda: matsuno_c_grid.matsumo_scheme(z2, z2, z2, 1.0, 1.0, dtype="f16"),
             lambda: matsuno_c_grid.run(z2, z2, z2, 1.0, 1.0, 1, dtype="f16"),
             lambda: matsuno_c_grid.courant_number(z2, z2, 1.0, 1.0, dtype="f16"),
             lambda: matsumo_temp.matsumo_scheme(z2, z2, z2, z2, 1.0, 1.0, dtype="f16"),
             lambda: matsumo_temp.matsumo_scheme_with_tracer(z2, z2, z2, z2, z2, 1.0, 1.0, dtype="f16"),
             lambda: ensemble.matsumo_scheme(z3, z3, z3, 1.0, 1.0, dtype="f16"),
             lambda: ensemble.matsumo_temp_scheme(z3, z3, z3, z3, 1.0, 1.0, dtype="f16"),
             lambda: ensemble.run(z3, z3, z3, 1.0, 1.0, 1, dtype="f16"),
             lambda: ensemble.courant_numbers(z3, z3, 1.0, 1.0, dtype="f16")]
    for call in calls:
        with pytest.raises(ValueError, match="dtype"):
            call()
