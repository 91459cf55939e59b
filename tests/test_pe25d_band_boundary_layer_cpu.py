"""The boundary layer on latitude bands, what needs no device: bands.merge_boundary_layer, the new symbols of the C ABI
as the header declares them, Core's argument checks ahead of gcm_create, and the runner's physics_begin / physics_end
protocol on stand-in engines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gcmiipy_amd as g
from gcmiipy_amd import _lib, bands

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcmcore.h")


def sums(n, seconds, H, W=5, seed=0):
    rng = np.random.default_rng(seed)
    return g.BoundaryLayer(n, seconds, rng.standard_normal((H, W)), rng.standard_normal((H, W)))


def test_merge_boundary_layer_concatenates_the_rows():
    parts = [sums(3, 360.0, 4, seed=1), sums(3, 360.0, 2, seed=2), sums(3, 360.0, 3, seed=3)]
    m = bands.merge_boundary_layer(parts)
    assert isinstance(m, g.BoundaryLayer) and (m.nsteps, m.seconds) == (3, 360.0)
    assert m.shf.shape == m.evap.shape == (9, 5)
    assert np.array_equal(m.shf, np.concatenate([p.shf for p in parts], axis=0))
    assert np.array_equal(m.evap, np.concatenate([p.evap for p in parts], axis=0))
    one = bands.merge_boundary_layer(iter(parts[:1]))            # (any iterable; one band is itself)
    assert np.array_equal(one.shf, parts[0].shf) and np.array_equal(one.evap, parts[0].evap)


def test_merge_boundary_layer_refuses_bands_that_disagree():
    with pytest.raises(ValueError, match="merge_boundary_layer: the bands hold 3, 4 applications"):
        bands.merge_boundary_layer([sums(3, 360.0, 4), sums(4, 360.0, 4)])
    with pytest.raises(ValueError, match="merge_boundary_layer: the bands hold"):
        bands.merge_boundary_layer([sums(3, 360.0, 4), sums(3, 480.0, 4)])
    with pytest.raises(ValueError, match="merge_boundary_layer: no records"):
        bands.merge_boundary_layer([])


def prototype(name):
    """(return type, [parameter types]) of `name` as include/gcmcore.h declares it"""
    text = open(HEADER).read()
    m = re.search(r"^(\w[\w ]*?)\b%s\(([^)]*)\);" % name, text, re.M)
    assert m, name + " is not declared in include/gcmcore.h"
    pars = [re.sub(r"\s*\w+$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    return m.group(1).strip(), pars


CTYPES = {"gcm_handle*": C.c_void_p, "constgcm_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double}


@pytest.mark.parametrize("name,pars", [("gcm_set_band_boundary_layer", ["gcm_handle*", "int"]),
                                       ("gcm_band_boundary_layer", ["constgcm_handle*"]),
                                       ("gcm_end_step_begin", ["gcm_handle*", "double"]),
                                       ("gcm_end_step_finish", ["gcm_handle*", "double"])])
def test_new_symbols_are_bound_with_the_headers_signatures(name, pars):
    ret, got = prototype(name)
    assert ret == "int" and got == pars
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int and args == [CTYPES[p] for p in pars]
    fn = getattr(_lib.lib, name)                                 # (exported, and bound as declared)
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    # a null handle is an argument error, with no device in sight
    assert fn(None, *([1] if len(pars) > 1 and pars[1] == "int" else [60.0] if len(pars) > 1 else [])) == _lib.ERR_ARG


def test_core_checks_the_opt_in_before_it_creates_anything():
    for kw in (dict(model=_lib.PE25D, width=36, height=12, layers=9),                  # a single domain
               dict(model=_lib.SW2D, width=32, height=16, dx=1e5),
               dict(model=_lib.SW2D, width=32, height=16, dx=1e5, nranks=2),           # a band, but of another model
               dict(model=_lib.SW2D_TEMP, width=32, height=16, dx=1e5, nranks=2)):
        with pytest.raises(ValueError, match="band_boundary_layer needs a GCM_PE25D latitude band"):
            g.Core(band_boundary_layer=True, **kw)
    for bad in ("yes", 2, None, 1.5):
        with pytest.raises(ValueError, match="band_boundary_layer must be True or False"):
            g.Core(_lib.PE25D, 36, 6, 9, nranks=2, global_height=12, band_boundary_layer=bad)
    # (a valid opt-in gets as far as the geometry check, which comes next)
    with pytest.raises(ValueError, match="GCM_PE25D needs a geometry"):
        g.Core(_lib.PE25D, 36, 6, 9, nranks=2, global_height=12, band_boundary_layer=True)


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


class _Split(_Engine):
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


class _Whole(_Engine):
    def physics_step(self, dt):
        self.log.append("step")


STAGES = ["edges0", "pack", "interior0", "unpack", "edges1", "pack", "interior1", "unpack"]


@pytest.mark.parametrize("engine,tail", [(_Split(True), ["begin", "pack", "unpack", "end"]), (_Split(False), ["begin", "end"]),
                                         (_Whole(), ["step"]), (_Engine(), [])])
def test_runner_drives_the_physics_pair_and_keeps_physics_step(engine, tail):
    """physics_begin -> True: one more exchange of the current state, then physics_end; False: none; an engine with
    physics_step only is driven through it as before, one with neither ends its steps itself (the last two hold on the
    parent commit too: they guard behaviour this change must leave alone)"""
    runner = bands.BandRunner(engine, 0, 2, _Ring(), north=0, south=0)
    assert not runner.native
    runner.primed = True                                         # (the initial state's exchange is not what is looked at)
    runner.step(60.0)
    assert engine.log == STAGES + tail
