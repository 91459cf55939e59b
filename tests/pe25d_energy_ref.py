"""Float64 reference of the GCM_PE25D energy record (gcm_energy / gcm_stats), NumPy only: the per-cell terms of
oracle/driver.py:calc_energy, their math.fsum, the bound a sum of n doubles stays inside, and the dense state the
GPU tests plant in the handle.  tests/test_pe25d_energy_ref_cpu.py holds this file to the oracle and to the golden
vector, and shows on the state below that an energy kernel with a wrong neighbour or a wrong area index would be
seen.  TEST INFRASTRUCTURE, no test in here."""
import math

import numpy as np

from oracle.constants import Cp, G, Rd
from oracle.grid import imh, jmh
from oracle.temperature import to_true_temp

U = 2.0 ** -53


def energy_terms(p, u, v, t, geom, area):
    """(ke, ate, geo) per cell, each (L, H, W) float64: oracle/driver.py:calc_energy line for line, up to its
    np.sum.  area: geom.area as the reference uses it, broadcast along the LAST axis (length 1 or W)"""
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1, 1, 1)
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(-1, 1, 1)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    u_at_center = imh(u)
    v_at_center = jmh(v)
    mag = np.sqrt(u_at_center ** 2 + v_at_center ** 2)
    tp = p * sig + geom.ptop
    tt = to_true_temp(t, tp)
    rho = tp / (Rd * tt)
    dp = p * dsig
    geopotential_depth = dp / (rho * G)
    airmass = rho * geopotential_depth * area
    total_depth = np.cumsum(geopotential_depth, 0)
    geopotential = total_depth * airmass * G
    ke = mag ** 2 * .5 * airmass
    ate = tt * Cp * airmass
    return ke, ate, geopotential


def energy(p, u, v, t, geom, area):
    """((ke, ate, geo, total), (sum |ke terms|, sum |ate terms|, sum |geo terms|)): math.fsum over energy_terms;
    total is the fsum of all three sets of terms"""
    terms = [x.ravel() for x in energy_terms(p, u, v, t, geom, area)]
    sums = [math.fsum(x) for x in terms]
    total = math.fsum(np.concatenate(terms))
    return tuple(sums) + (total,), tuple(math.fsum(np.abs(x)) for x in terms)


def sum_bound(n, s_abs, roundings):
    """|any summation order of n doubles - their exact sum| <= (n - 1) 2^-53 sum |terms|; `roundings` more units
    for the roundings inside one term (the bound tests/test_pe25d_tracer_stats_gpu.py derives)"""
    return (n + roundings) * U * s_abs


# ---------------------------------------------------------------- the dense state
# tests/pe25d_inputs.py:state was not taken as the base: its p varies by 1e-4 from cell to cell and its winds are of
# order 1 m/s, white noise that is uncorrelated with p -- a kernel that took the east neighbour for the west one, or row
# j + 1 for row j - 1, would change ke on it by a few 1e-5 only.  Here the winds carry a pattern of period four whose
# half-point average is large where p is high, so that the sums are sensitive to which neighbour is averaged, and p
# carries a pattern along i that differs from the one along j, so that its transpose is another field.
PERIOD4 = np.asarray([1.0, 1.0, -1.0, -1.0])
SAW4 = np.asarray([-1.0, 1.0, -1.0 / 3, 1.0 / 3])


def dense_state(geom, seed=21):
    """(p, u, v, t, q): p = (1e5 - ptop) (1 + x), |x| <= 1 %, another value in every cell; u and v: +-15 m/s in a
    pattern of period four along i (u) and j (v) plus 3 m/s of noise; theta: 300 K +- a few K of noise, times the
    Exner factor of the level (a true temperature near 300 K, as tests/pe25d_inputs.py has it); q as there"""
    rng = np.random.default_rng(seed)
    H, W, L = geom.height, geom.width, geom.layers
    i, j = np.arange(W), np.arange(H)
    x = 0.005 * SAW4[i % 4][None, :] + 0.004 * SAW4[j % 4][:, None] + 0.001 * rng.uniform(-1, 1, (H, W))
    p = (1e5 - geom.ptop) * (1.0 + x)
    u = 15.0 * PERIOD4[i % 4][None, None, :] + 3.0 * rng.standard_normal((L, H, W))
    v = 15.0 * PERIOD4[j % 4][None, :, None] + 3.0 * rng.standard_normal((L, H, W))
    sig = np.asarray(geom.sig, dtype=np.float64).reshape(-1, 1, 1)
    t = (300.0 + 3.0 * rng.standard_normal((L, H, W))) * ((1e5 / (p * sig + geom.ptop)) ** (287.0 / 1004.0))
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    return p, u, v, t, q


def column_area(W):
    """an `area` of length W: another positive value in every column"""
    i = np.arange(W)
    return 1e9 * (1.0 + 0.5 * SAW4[i % 4] + 0.001 * i)


def neighbours_differ(a):
    """no two cells next to one another along any axis (with the wrap) hold the same value"""
    return all(a.shape[ax] == 1 or not (a == np.roll(a, 1, ax)).any() for ax in range(a.ndim))
