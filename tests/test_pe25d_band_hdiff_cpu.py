"""The horizontal diffusion on latitude bands, what needs no device: the host build of the band walk
(gcm_hdiff_apply_band) against gcm_hdiff_apply over the periodic whole, bit for bit; the new symbols of the C ABI as the
header declares them; Core's argument checks ahead of gcm_create; and the runner's physics_diffuse protocol on stand-in
engines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gcmiipy_amd as g
from gcmiipy_amd import _lib, bands, geometry

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcmcore.h")
L = 3
DT = 600.0
PARAMS = {1: dict(order=1, nu=2.0e5, cmax=0.125), 2: dict(order=2, nu=1.0e15, cmax=0.1)}
# (H, W, [(row0, Hb)]): bands of 2 and 4 rows with rank 0 and the last rank (the pole wrap), and 12 rows in 3 bands
CASES = [(8, 5, [(0, 2), (2, 2), (4, 2), (6, 2)]), (8, 5, [(0, 4), (4, 4)]), (12, 7, [(0, 4), (4, 4), (8, 4)])]

_cache = {}


def whole(H, W, order, rows):
    """(the global tables' three rows, the random field (L, H, W), gcm_hdiff_apply over the periodic whole), once"""
    key = (H, W, order, rows)
    if key not in _cache:
        geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
        tabs = g.hdiff_tables(geom, DT, **PARAMS[order])
        names = ("ax", "bn", "bs") if rows == "centre" else ("axv", "bnv", "bsv")
        co = [tabs[n] for n in names]
        X = np.random.default_rng(17 * H + W).standard_normal((L, H, W)) * 10.0 + 280.0
        want = g.hdiff_apply(X, *co, order)
        assert not np.array_equal(want, X)
        for a in co + [X, want]:
            a.setflags(write=False)
        _cache[key] = (co, X, want)
    return _cache[key]


@pytest.mark.parametrize("rows", ["centre", "v"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("H,W,split", CASES)
def test_apply_band_equals_the_rows_of_apply_over_the_whole(H, W, split, order, rows):
    """rows [row0 - 2, row0 + Hb + 2), wrapped, of the field and of the global tables through gcm_hdiff_apply_band are
    rows [row0, row0 + Hb) of gcm_hdiff_apply: the same cells, the same operations in the same order"""
    co, X, want = whole(H, W, order, rows)
    for row0, Hb in split:
        idx = np.arange(row0 - 2, row0 + Hb + 2) % H
        got = g.hdiff_apply_band(X[:, idx, :], *[c[idx] for c in co], order)
        assert got.shape == (L, Hb, W)
        assert np.array_equal(got, want[:, row0:row0 + Hb, :]), (H, W, row0, Hb, order, rows)
    # one level as a 2-D array
    row0, Hb = split[-1]
    idx = np.arange(row0 - 2, row0 + Hb + 2) % H
    got = g.hdiff_apply_band(X[1][idx], *[c[idx] for c in co], order)
    assert np.array_equal(got, want[1, row0:row0 + Hb])


def test_apply_band_refuses_bad_arguments():
    lib = _lib.lib
    dp = C.POINTER(C.c_double)
    X = np.zeros((1, 6, 5))
    tab = np.zeros((4, 6))
    out = np.zeros((1, 2, 5))
    p = lambda a: a.ctypes.data_as(dp)
    assert lib.gcm_hdiff_apply_band(2, 5, 1, p(tab), 2, p(X), p(out)) == _lib.OK
    for Hb, W, nlev in ((0, 5, 1), (2, 0, 1), (2, 5, 0), (-1, 5, 1)):
        assert lib.gcm_hdiff_apply_band(Hb, W, nlev, p(tab), 2, p(X), p(out)) == _lib.ERR_ARG
        assert b"gcm_hdiff_apply_band: Hb, W and nlev must be 1 or more" in lib.gcm_last_error(None)
    for order in (0, 3, -1):
        assert lib.gcm_hdiff_apply_band(2, 5, 1, p(tab), order, p(X), p(out)) == _lib.ERR_ARG
        assert b"order must be 1 or 2" in lib.gcm_last_error(None)
    for args in ((None, p(X), p(out)), (p(tab), None, p(out)), (p(tab), p(X), None)):
        assert lib.gcm_hdiff_apply_band(2, 5, 1, args[0], 1, args[1], args[2]) == _lib.ERR_ARG
        assert b"a null pointer" in lib.gcm_last_error(None)
    assert not out.any()
    # the Python probe's own checks
    with pytest.raises(ValueError, match="expected \\(nlev, Hb \\+ 4, W\\)"):
        g.hdiff_apply_band(np.zeros(5), tab[0], tab[1], tab[2], 1)
    with pytest.raises(ValueError, match="two ghost rows a side"):
        g.hdiff_apply_band(np.zeros((4, 5)), np.zeros(4), np.zeros(4), np.zeros(4), 1)
    with pytest.raises(ValueError):
        g.hdiff_apply_band(X, np.zeros(5), tab[1], tab[2], 1)       # coefficients of another height
    with pytest.raises(ValueError, match="order must be 1 or 2"):
        g.hdiff_apply_band(X, tab[0], tab[1], tab[2], 3)


def prototype(name):
    """(return type, [parameter types]) of `name` as include/gcmcore.h declares it"""
    text = open(HEADER).read()
    m = re.search(r"^(\w[\w ]*?)\b%s\(([^)]*)\);" % name, text, re.M)
    assert m, name + " is not declared in include/gcmcore.h"
    pars = [re.sub(r"\s*\w+$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    return m.group(1).strip(), pars


_DP = C.POINTER(C.c_double)
CTYPES = {"gcm_handle*": C.c_void_p, "constgcm_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double,
          "constdouble*": _DP, "double*": _DP}


@pytest.mark.parametrize("name,pars", [("gcm_set_band_hdiff", ["gcm_handle*", "int"]),
                                       ("gcm_band_hdiff", ["constgcm_handle*"]),
                                       ("gcm_end_step_diffuse", ["gcm_handle*", "double"]),
                                       ("gcm_hdiff_apply_band", ["int", "int", "int", "constdouble*", "int", "constdouble*",
                                                                 "double*"])])
def test_new_symbols_are_bound_with_the_headers_signatures(name, pars):
    ret, got = prototype(name)
    assert ret == "int" and got == pars
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int and args == [CTYPES[p] for p in pars]
    fn = getattr(_lib.lib, name)                                 # (exported, and bound as declared)
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    if pars[0].endswith("gcm_handle*"):
        # a null handle is an argument error, with no device in sight
        assert fn(None, *([1] if pars[1:] == ["int"] else [60.0] if pars[1:] else [])) == _lib.ERR_ARG


def test_core_checks_the_opt_in_before_it_creates_anything():
    for kw in (dict(model=_lib.PE25D, width=36, height=12, layers=9),                  # a single domain
               dict(model=_lib.SW2D, width=32, height=16, dx=1e5),
               dict(model=_lib.SW2D, width=32, height=16, dx=1e5, nranks=2),           # a band, but of another model
               dict(model=_lib.SW2D_TEMP, width=32, height=16, dx=1e5, nranks=2)):
        with pytest.raises(ValueError, match="band_horizontal_diffusion needs a GCM_PE25D latitude band"):
            g.Core(band_horizontal_diffusion=True, **kw)
    for bad in ("yes", 2, None, 1.5):
        with pytest.raises(ValueError, match="band_horizontal_diffusion must be True or False"):
            g.Core(_lib.PE25D, 36, 6, 9, nranks=2, global_height=12, band_horizontal_diffusion=bad)
    # (a valid opt-in gets as far as the geometry check, which comes next)
    with pytest.raises(ValueError, match="GCM_PE25D needs a geometry"):
        g.Core(_lib.PE25D, 36, 6, 9, nranks=2, global_height=12, band_horizontal_diffusion=True)


class _Ring:
    """torch.distributed's part in BandRunner.exchange_start, moving nothing"""
    isend, irecv = "isend", "irecv"

    class P2POp:
        def __init__(self, op, tensor, peer):
            self.op, self.tensor, self.peer = op, tensor, peer

    def batch_isend_irecv(self, ops):
        assert [o.op for o in ops] == ["isend", "isend", "irecv", "irecv"]
        return []


class _Engine:
    """the least a host-driven edge-first runner touches, recording the order of the calls"""
    edge_first = True
    phases = 2

    def __init__(self):
        self.log = []

    def pack_both(self):
        self.log.append("pack")
        return "n", "s"

    def unpack_both(self):
        self.log.append("unpack")

    def comm_begin(self):
        pass

    def comm_end(self):
        pass

    def recv_buffer(self, side):
        return "r%d" % side

    def compute_edges(self, stage, dt):
        self.log.append("edges%d" % stage)

    def compute_interior(self, stage, dt):
        self.log.append("interior%d" % stage)


class _Pair(_Engine):
    """physics_begin / physics_end, no physics_diffuse: an engine from before the diffusion's part"""
    def __init__(self, exchange):
        super().__init__()
        self.exchange = exchange

    def physics_begin(self, dt):
        self.log.append("begin")
        return self.exchange

    def physics_end(self, dt):
        self.log.append("end")

    def physics_step(self, dt):
        self.log.append("step")


class _Diffusing(_Pair):
    def __init__(self, diffuses, exchange):
        super().__init__(exchange)
        self.diffuses = diffuses

    def physics_diffuse(self, dt):
        self.log.append("diffuse")
        return self.diffuses


class _Whole(_Engine):
    def physics_step(self, dt):
        self.log.append("step")


STAGES = ["edges0", "pack", "interior0", "unpack", "edges1", "pack", "interior1", "unpack"]


def drive(engine):
    runner = bands.BandRunner(engine, 0, 2, _Ring(), north=0, south=0)
    assert not runner.native
    runner.primed = True                                         # (the initial state's exchange is not what is looked at)
    runner.step(60.0)
    return engine.log


@pytest.mark.parametrize("diffuses,exchange,tail", [
    (True, False, ["diffuse", "pack", "unpack", "begin", "end"]),
    (True, True, ["diffuse", "pack", "unpack", "begin", "pack", "unpack", "end"]),      # with the boundary layer: four exchanges
    (False, False, ["diffuse", "begin", "end"]),
    (False, True, ["diffuse", "begin", "pack", "unpack", "end"])])
def test_runner_exchanges_behind_physics_diffuse(diffuses, exchange, tail):
    """physics_diffuse -> True: one more exchange of the current state ahead of physics_begin; False: none"""
    assert drive(_Diffusing(diffuses, exchange)) == STAGES + tail


@pytest.mark.parametrize("engine,tail", [(_Pair(True), ["begin", "pack", "unpack", "end"]), (_Pair(False), ["begin", "end"]),
                                         (_Whole(), ["step"]), (_Engine(), [])])
def test_engines_without_physics_diffuse_are_driven_as_before(engine, tail):
    """(these hold on the parent commit too: they guard behaviour this change must leave alone)"""
    assert drive(engine) == STAGES + tail


def test_hip_band_engine_has_the_new_members():
    assert callable(bands.HipBandEngine.physics_diffuse) and callable(bands.HipBandEngine.set_horizontal_diffusion)
    for name in ("band_horizontal_diffusion", "horizontal_diffusion_registered"):
        assert isinstance(getattr(g.Core, name), property)
    assert callable(g.Core.end_step_diffuse)
