"""The GCM_PE_* switches of pe25d_create that no other test sets: GCM_PE_UPDATE_ROWS, GCM_PE_K4_ODDTOP,
GCM_PE_FILTER_NO_LOOP on a single domain against the float64 oracle, GCM_PE_EDGE_SEGMENTS on a loopback band against
the single domain's bits.  (GCM_PE_PIT2D and GCM_PE_LEVEL_SEGMENTS: test_pe25d_variants_gpu.test_level_counts_vs_oracle;
GCM_PE_SINGLE_STREAM, GCM_PE_K1_SPLIT and GCM_PE_STOP_EVENTS: test_bands_gpu.test_band_run_chains_at_overlapping_size;
GCM_PE_RAD_GENERIC: test_pe25d_variants_gpu.test_radiation_generic_form_matches_default.)  The switches are read once
per handle, when it is created: every case sets its variable before it builds its Core."""
import numpy as np
import pytest

import gpu_setups as su
from gpu_setups import g  # noqa: F401  (the module-scoped fixture)
from test_pe25d_variants_gpu import TOL, _check, _oracle, _run, _state

pytestmark = pytest.mark.gpu
SWITCHES = ("GCM_PE_UPDATE_ROWS", "GCM_PE_K4_ODDTOP", "GCM_PE_FILTER_NO_LOOP", "GCM_PE_EDGE_SEGMENTS")
NSTEPS, DT = 2, 60.0
# 9 rows: a 7-row workgroup of K4 has a remainder (and three 3-row ones have none); 30 columns: the generic filter
# path; 24 levels: K4 starts its march on an odd level (oddtop), 25: it does not.  120 columns: a plan with its own
# instantiation of the filter kernels (kMask1440), for GCM_PE_FILTER_NO_LOOP only
SHAPES = [(9, 30, 24), (9, 30, 25)]
SETTINGS = {"rows3": {"GCM_PE_UPDATE_ROWS": "3"}, "rows7": {"GCM_PE_UPDATE_ROWS": "7"},
            "oddtop0": {"GCM_PE_K4_ODDTOP": "0"}, "noloop": {"GCM_PE_FILTER_NO_LOOP": "1"}}
CASES = [(hwl, name) for hwl in SHAPES for name in SETTINGS] + [((9, 120, 24), "noloop")]
# The settings whose state must equal the default run's bit for bit.  rows3: at 9 rows the default IS the 3-row K4
# (pe25d_create: H <= 400), the same launch.  rows7 and oddtop0: measured on an MI355X, here and at every case of
# test_pe25d_stage_geometry_gpu.py (where the default is the 7-row K4 and the switch the 3-row one), they give the
# default's bits -- a cell's arithmetic does not depend on the rows of its workgroup or on where the march starts
# (profiles/stage_geometry/README.md).  noloop does not: K1 as one workgroup per pair differs from the looping form in the
# last bits at every shape measured; it is held to the oracle tolerance only, and each case prints which it is
SAME_BITS_AS_DEFAULT = {"rows3", "rows7", "oddtop0"}


_single = {}


def _single_domain(g, hwl):
    """-> (geom, state, oracle after NSTEPS, the default handle's state after NSTEPS), computed once per shape with no
    switch set"""
    if hwl not in _single:
        H, W, L = hwl
        geom, og = su.geoms_of(H, W, L)
        st = _state(H, W, L, og, 7 * W + L)
        want = _oracle(st, NSTEPS, DT, og)
        got = _run(g, geom, st, NSTEPS, DT)
        _check(got, want, (hwl, "default"), TOL)
        _single[hwl] = (geom, st, want, got)
    return _single[hwl]


@pytest.mark.parametrize("hwl,name", CASES, ids=["%dx%dx%d-%s" % (*hwl, name) for hwl, name in CASES])
def test_switch_vs_oracle(g, hwl, name, monkeypatch):
    """two fp64 steps with one switch set, against the oracle at the 1e-10 of test_pe25d_variants_gpu.  rows3, rows7 and
    oddtop0 must also reproduce the default run's bits; noloop is asserted against the oracle only (see
    SAME_BITS_AS_DEFAULT)"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    geom, st, want, default = _single_domain(g, hwl)
    for k, v in SETTINGS[name].items():
        monkeypatch.setenv(k, v)
    got = _run(g, geom, st, NSTEPS, DT)
    for k in SETTINGS[name]:
        monkeypatch.delenv(k)
    same = all(np.array_equal(a, b) for a, b in zip(got, default))
    print(hwl, name, "the default's bits" if same else "differs from the default")
    _check(got, want, (hwl, name), TOL)
    if name in SAME_BITS_AS_DEFAULT:
        for k, a, b in zip("puvtq", got, default):
            assert np.array_equal(a, b), (hwl, name, k)


_band_ref = {}


@pytest.mark.parametrize("edge_segments", [None, "1", "2"])
def test_edge_segments_band_equals_single_domain(g, edge_segments, monkeypatch):
    """a 12 x 30 x 24 loopback band (its own neighbour = the periodic single domain), three fp64 steps inside
    gcm_band_run, with the edge rows' K4 in the default number of level segments, in one and in two: the single
    domain's bits ("a band and the single domain see the same bits", pe25d_dev.h)"""
    import torch
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange
    H, W, L, nsteps = 12, 30, 24, 3
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if not _band_ref:
        geom, og = su.geoms_of(H, W, L)
        st = _state(H, W, L, og, 12)
        _band_ref["x"] = (geom, st, _run(g, geom, st, nsteps, DT))
    geom, st, want = _band_ref["x"]
    if edge_segments is not None:
        monkeypatch.setenv("GCM_PE_EDGE_SEGMENTS", edge_segments)
    c = g.Core(g._lib.PE25D, W, H, L, geom=geom, nranks=2, rank=0, global_height=H, row0=0,
               stream=torch.cuda.current_stream().cuda_stream)
    monkeypatch.delenv("GCM_PE_EDGE_SEGMENTS", raising=False)
    runner = BandRunner(HipBandEngine(c, torch), 0, 2, LoopbackExchange(), north=0, south=0)
    assert runner.native
    c.set_state(*st)
    runner.run(nsteps, DT)
    torch.cuda.synchronize()
    got = c.get_state()
    c.close()
    assert not np.array_equal(got[1], st[1])
    for k, a, b in zip("puvtq", got, want):
        assert np.array_equal(a, b), (edge_segments, k)
