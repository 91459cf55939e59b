"""The float64 reference of the energy record (tests/pe25d_energy_ref.py) against the oracle's calc_energy and the
golden vector, and the premises of tests/test_pe25d_energy_gpu.py on the reference alone: on the dense state a wrong
west neighbour, a wrong north row or a transposed p moves the figures far beyond the tolerance the kernel is held to.
No GPU."""
import copy

import numpy as np
import pytest

from conftest import golden
from oracle import driver, geometry as ogeo
import pe25d_energy_ref as er

CASES = [((5, 130, 3), 0.0), ((5, 130, 3), 1000.0), ((70, 70, 4), 0.0), ((70, 70, 4), 1000.0)]


def _geom(shape, ptop):
    H, W, L = shape
    geom = ogeo.gen_geometry(H, W, L, sig_func=ogeo.manabe_sig)
    geom.ptop = ptop
    return geom


def _area(shape):
    """what the GPU test hands over: a value per column where the reference's broadcast allows one (H == W), else one"""
    H, W, _ = shape
    return er.column_area(W) if H == W else np.ones(1)


@pytest.mark.parametrize("shape,ptop", CASES)
def test_helper_equals_the_oracle(shape, ptop):
    geom = _geom(shape, ptop)
    st = er.dense_state(geom)
    area = _area(shape)
    og = copy.copy(geom)
    og.area = area                                   # (calc_energy reads geom.area; (5,) would not broadcast against 130)
    want = driver.calc_energy(*st, None, og)
    got, s_abs = er.energy(*st[:4], geom, area)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-13 * abs(b), (a, b)
    # all three sets of terms are positive: sum |terms| is the sum
    assert s_abs == got[:3]
    # np.sum over the helper's terms is the oracle's own figure, bit for bit
    ke, ate, geo = (np.sum(x) for x in er.energy_terms(*st[:4], geom, area))
    assert (ke, ate, geo, ke + ate + geo) == tuple(want)


def test_helper_equals_the_golden_energy():
    """bump3_energy (H = 1, W = 16, L = 17, three steps of the reference's harness state) at the tolerance of
    tests/test_oracle_golden.py, bit for bit: np.sum over the helper's terms, which is what the golden file's figures
    are.  The helper's own sums are math.fsum, another order of the same terms: within sum_bound of them"""
    d = golden("g8_pe25d")
    geom = ogeo.gen_geometry(1, 16, 17, sig_func=ogeo.manabe_sig)
    st = [d["bump3_" + k] for k in "puvt"]
    terms = er.energy_terms(*st, geom, geom.area)
    ke, ate, geo = (np.sum(x) for x in terms)
    assert np.array_equal(np.asarray([ke, ate, geo, ke + ate + geo]), d["bump3_energy"])
    got, s_abs = er.energy(*st, geom, geom.area)
    n = terms[0].size
    for a, b, s in zip(got, d["bump3_energy"], s_abs + (sum(s_abs),)):
        assert abs(a - b) <= er.sum_bound(n, s, 0) and abs(a - b) <= 1e-13 * abs(b)


@pytest.mark.parametrize("shape,ptop", CASES)
def test_dense_state_is_what_the_issue_asks(shape, ptop):
    geom = _geom(shape, ptop)
    p, u, v, t, q = er.dense_state(geom)
    assert np.abs(p / (1e5 - ptop) - 1).max() <= 0.01 and np.abs(p / np.roll(p, 1, 1) - 1).max() > 0.005
    for w in (u, v):
        assert w.min() < -10 and w.max() > 10 and np.abs(w).max() < 40
    tt = t / ((1e5 / (p * geom.sig + ptop)) ** (287.0 / 1004.0))
    assert 1.0 < np.std(tt) < 5.0 and abs(np.mean(tt) - 300) < 1
    for a in (p, u, v, t):
        assert er.neighbours_differ(a)
    area = er.column_area(shape[1])
    assert area.min() > 0 and len(set(area)) == area.size


@pytest.mark.parametrize("shape,ptop", CASES)
def test_premises_wrong_neighbours_move_ke(shape, ptop):
    """u moved one column west is what averaging with the east neighbour gives, v moved one row north what row j + 1
    instead of j - 1 gives: both change ke by more than 1e-3 of it, nine orders above the kernel's tolerance"""
    geom = _geom(shape, ptop)
    p, u, v, t, _ = er.dense_state(geom)
    area = _area(shape)
    ke = er.energy(p, u, v, t, geom, area)[0][0]
    ke_u = er.energy(p, np.roll(u, -1, -1), v, t, geom, area)[0][0]
    ke_v = er.energy(p, u, np.roll(v, -1, -2), t, geom, area)[0][0]
    print("%s ptop %g: u west %.3e, v north %.3e of ke" % (shape, ptop, abs(ke_u / ke - 1), abs(ke_v / ke - 1)))
    assert abs(ke_u / ke - 1) > 1e-3
    assert abs(ke_v / ke - 1) > 1e-3


@pytest.mark.parametrize("ptop", [0.0, 1000.0])
def test_premise_transposed_p_moves_ate(ptop):
    """the square case: p[i][j] for p[j][i] -- an `area` or a p indexed by the wrong axis -- changes ate by more than 1e-6"""
    shape = (70, 70, 4)
    geom = _geom(shape, ptop)
    p, u, v, t, _ = er.dense_state(geom)
    area = _area(shape)
    ate = er.energy(p, u, v, t, geom, area)[0][1]
    ate_t = er.energy(np.ascontiguousarray(p.T), u, v, t, geom, area)[0][1]
    print("ptop %g: transposed p %.3e of ate" % (ptop, abs(ate_t / ate - 1)))
    assert abs(ate_t / ate - 1) > 1e-6


def test_sum_bound():
    assert er.sum_bound(10, 3.0, 2) == 12 * 2.0 ** -53 * 3.0
