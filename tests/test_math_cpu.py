"""Accuracy of the device algorithm for (p/P0)**kappa, checked on the host: the
table comes from the library (gcm_exner_table), the evaluation (exner_ref.py) mirrors
gcm_math.h's exner() operation for operation in float64, and the yardstick is
x87 extended precision.  The reference uses numpy's pow (temperature.py:10)."""
import numpy as np

from exner_ref import EDGE_ERR_BOUND, ERR_BOUND, KAPPA, exner_emulated, exner_extended, table as _table


def test_table_entries():
    tab = _table()
    assert tab[64] == float(np.exp(-KAPPA * np.log(np.longdouble(1e5))))     # e = 0
    for i in (0, 17, 63):
        rc = tab[128 + 2 * i]
        assert abs(rc * (1 + (i + 0.5) / 64) - 1) < 2e-16
        want = np.power(1 / np.longdouble(rc), np.longdouble(KAPPA))
        assert abs(tab[129 + 2 * i] / float(want) - 1) < 2e-16


def test_exner_accuracy_against_extended_precision():
    tab = _table()
    rng = np.random.default_rng(0)
    for lo, hi in ((9e4, 1.1e5), (1e2, 1.1e5), (1e-3, 1e12)):
        p = np.exp(rng.uniform(np.log(lo), np.log(hi), 200000))
        ref = exner_extended(p)
        mine = exner_emulated(p, tab)
        err = float(np.max(np.abs((mine - ref) / ref)))
        npw = float(np.max(np.abs((np.power(p / 1e5, KAPPA) - ref) / ref)))
        assert err < ERR_BOUND, (lo, hi, err, npw)   # 6e-16; measured 2.9e-16 .. 5.3e-16


def test_exner_interval_edges():
    """mantissa-interval boundaries and powers of two: |t| stays <= 2^-7"""
    tab = _table()
    m = 1 + np.arange(0, 65) / 64.0
    p = np.concatenate([m * 2.0 ** k for k in (-3, 0, 16, 17)])
    p = np.concatenate([p, np.nextafter(p, 0), np.nextafter(p, np.inf)])
    ref = exner_extended(p)
    assert float(np.max(np.abs((exner_emulated(p, tab) - ref) / ref))) < EDGE_ERR_BOUND    # 5e-16
