"""CPU-side checks of the ensemble handles (gcm_config.members): the config field sits in the padding in
front of dx, the new entry points are declared and exported, gcm_create refuses bad member counts before
any device use, and the batched drop-ins check their shapes before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gcm_members", "gcm_set_member", "gcm_get_member", "gcm_diag_members")


def _header():
    return open(os.path.join(ROOT, "include", "gcmcore.h")).read()


def test_members_field_follows_halo_steps_in_the_padding():
    from gcmiipy_amd import _lib
    body = _header()
    body = body[body.index("typedef struct {"):body.index("} gcm_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:int32_t|double|const double \*|void \*)\s*\*?(\w+);", body)
    k = fields.index("halo_steps")
    assert fields[k + 1:k + 3] == ["members", "dx"]
    names = [f[0] for f in _lib.Config._fields_]
    assert names[names.index("halo_steps") + 1] == "members"
    assert _lib.Config.members.offset == 60 and _lib.Config.dx.offset == 64
    assert ctypes.sizeof(_lib.Config) == 168                 # unchanged: the field took the padding
    assert _lib.ABI_VERSION == 1


def test_new_entry_points_declared_and_exported():
    from gcmiipy_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n


def _create(members, model=None, nranks=1):
    from gcmiipy_amd import _lib
    cfg = _lib.Config()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.model = _lib.SW2D if model is None else model
    cfg.width, cfg.height, cfg.layers = 32, 16, 1
    cfg.nranks, cfg.rank, cfg.global_height = nranks, 0, 16 * nranks
    cfg.device = -1
    cfg.dx = 1.0
    cfg.members = members
    h = _lib._H()
    rc = _lib.lib.gcm_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == _lib.OK:
        _lib.lib.gcm_destroy(h)
    return rc, _lib.lib.gcm_last_error(None).decode()


def test_create_refuses_bad_member_counts_before_device_use():
    """decided next to the other argument checks, ahead of gcm_device_count(): the same codes on a box
    without a GPU, where every create that passes them fails with GCM_ERR_NODEVICE"""
    from gcmiipy_amd import _lib
    rc, msg = _create(-1)
    assert rc == _lib.ERR_ARG and "members" in msg
    rc, msg = _create(4, nranks=2)
    assert rc == _lib.ERR_UNSUPPORTED and "members" in msg
    rc, msg = _create(4, model=_lib.PE25D)
    assert rc == _lib.ERR_UNSUPPORTED and "members" in msg
    rc, msg = _create(4, model=_lib.PE2D)
    assert rc == _lib.ERR_UNSUPPORTED and "members" in msg


def test_core_maps_member_refusals():
    import gcmiipy_amd as g
    with pytest.raises(ValueError, match="members"):
        g.Core(g._lib.SW2D, 32, 16, dx=1.0, members=-1)
    with pytest.raises(g.GcmError, match="members"):
        g.Core(g._lib.SW2D, 32, 16, dx=1.0, members=4, nranks=2, rank=0, global_height=32)
    with pytest.raises(g.GcmError, match="members"):
        g.Core(g._lib.SW2D_TEMP, 32, 16, dx=1.0, members=4, nranks=2, rank=1, global_height=32)


def test_create_without_device_still_says_so():
    """members = 0 / 1 / 8 on a valid 2-D config pass the argument checks and meet the device check"""
    from gcmiipy_amd import _lib
    if _lib.lib.gcm_device_count() != 0:
        pytest.skip("a HIP device is present")
    for m in (0, 1, 8):
        rc, msg = _create(m)
        assert rc == _lib.ERR_NODEVICE, (m, rc, msg)


def test_batched_drop_ins_check_shapes():
    from gcmiipy_amd import ensemble
    z3, z2 = np.zeros((3, 4, 5)), np.zeros((4, 5))
    with pytest.raises(ValueError, match="3-D"):
        ensemble.matsumo_scheme(z2, z2, z2, 1.0, 1.0)
    with pytest.raises(ValueError, match="v has shape"):
        ensemble.matsumo_scheme(z3, np.zeros((2, 4, 5)), z3, 1.0, 1.0)
    with pytest.raises(ValueError, match="p has shape"):
        ensemble.matsumo_scheme(z3, z3, np.zeros((3, 4, 6)), 1.0, 1.0)
    with pytest.raises(ValueError, match="t has shape"):
        ensemble.matsumo_temp_scheme(z3, z3, z3, z2, 1.0, 1.0)
    with pytest.raises(ValueError, match="q has shape"):
        ensemble.matsumo_temp_scheme(z3, z3, z3, z3, 1.0, 1.0, q=np.zeros((3, 5, 4)))
    with pytest.raises(ValueError, match="tracer"):
        ensemble.matsumo_temp_scheme(z3, z3, z3, z3, 1.0, 1.0, q=z3, tracer="none")
    with pytest.raises(ValueError, match="3-D"):
        ensemble.run(np.zeros(5), np.zeros(5), np.zeros(5), 1.0, 1.0, 3)
    with pytest.raises(ValueError, match="needs the temperature model"):
        ensemble.run(z3, z3, z3, 1.0, 1.0, 3, q=z3)
    with pytest.raises(ValueError, match="u has shape"):
        ensemble.courant_numbers(z3, z2, 1.0, 1.0)


def test_single_member_drop_ins_still_refuse_3d():
    from gcmiipy_amd.matsuno_c_grid import matsumo_scheme
    from gcmiipy_amd.matsumo_temp import matsumo_scheme as ms_t
    z3 = np.zeros((3, 4, 5))
    with pytest.raises(ValueError):
        matsumo_scheme(z3, z3, z3, 1.0, 1.0)
    with pytest.raises(ValueError):
        ms_t(z3, z3, z3, z3, 1.0, 1.0)
