"""The cases that every column phase of GCM_PE25D takes alike -- the moist physics, the convective adjustment and the
boundary layer: one mechanism in the library and the package, one set of cases here.  Latitude bands against the single
domain (in-process bands with device-copied ghost rows, the loopback band of gcm_band_run and its host-driven sequence,
once at a size where the streams really overlap), the explicit step without a registration, the refusals all phases
share, and the checkpoint.  Everything is bit for bit.  The bodies and the phases' descriptors (inputs, parameters,
shapes) are tests/column_phase_cases.py's; what belongs to one phase alone -- its kernel against its restatement, its
budgets, the registered phase against the explicit calls -- is in tests/test_pe25d_<phase>_gpu.py.  The boundary layer
on latitude bands is another protocol (opt-in, a third exchange): tests/test_pe25d_band_boundary_layer_gpu.py."""
import pytest

import column_phase_cases as cc

pytestmark = pytest.mark.gpu

PHASES = [pytest.param(ph, id=ph.name) for ph in cc.PHASES]                   # moist, convect, boundary_layer
ON_BANDS = [pytest.param(ph, id=ph.name) for ph in cc.PHASES if ph.chain]       # moist, convect
# moist: (24, 36, 9) in 2 and 3 bands, (6, 10, 3) in 2 (H, W, L); convect: (9, 12, 36) in 2 and 3 bands (L, H, W)
BAND_CASES = [pytest.param(ph, shape, nb, id="%s-%s-%d" % (ph.name, cc.shape_id(shape), nb))
              for ph in cc.PHASES for shape, nb in ph.band_cases]
# moist: (24, 36, 9) and (6, 10, 3); convect: (9, 12, 36)
LOOPBACK_CASES = [pytest.param(ph, shape, id="%s-%s" % (ph.name, cc.shape_id(shape)))
                  for ph in cc.PHASES for shape in ph.loopback_shapes]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ph,shape,nb", BAND_CASES)
def test_in_process_bands_equal_single_domain(ph, shape, nb, dtype):
    import gcmiipy_amd as g
    cc.in_process_bands_equal_single_domain(ph, g, shape, nb, dtype)


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ph,shape", LOOPBACK_CASES)
def test_loopback_band_run_equals_single_domain(ph, shape, dtype, host_loop, monkeypatch):
    import gcmiipy_amd as g
    cc.loopback_band_run_equals_single_domain(ph, g, shape, dtype, host_loop, monkeypatch)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ph", ON_BANDS)
def test_band_run_chains_with_the_phase(ph, dtype, monkeypatch):
    """moist: 48 x 1440 x 24, tau_e = 600 s; convect: the same grid, gamma = 6.5 K / km; 2 steps of one second"""
    import gcmiipy_amd as g
    cc.band_run_chains_with_the_phase(ph, g, dtype, monkeypatch)


@pytest.mark.parametrize("ph", PHASES)
def test_explicit_step_without_a_registration_keeps_no_sums(ph):
    import gcmiipy_amd as g
    cc.explicit_step_without_a_registration_keeps_no_sums(ph, g)


@pytest.mark.parametrize("ph", PHASES)
def test_refused_calls_change_nothing(ph):
    """the refusals every phase shares; each phase's own file refuses its own calls between the two halves"""
    import gcmiipy_amd as g
    geom, st, gt = cc.refusal_inputs(ph)
    c = cc.handle(ph, g, geom, st, gt=gt)
    was, was_state = cc.refused_without_a_registration(ph, g, c)
    cc.refused_calls_changed_nothing(ph, g, c, was, was_state)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ph", PHASES)
def test_checkpoint_carries_the_phase_and_its_sums(ph, dtype, tmp_path):
    """moist and convect: alone, 2 + 1 steps; the boundary layer: convect and moist registered beside it, 2 + 2 steps"""
    import gcmiipy_amd as g
    cc.checkpoint_carries_the_phase_and_its_sums(ph, g, dtype, tmp_path)
