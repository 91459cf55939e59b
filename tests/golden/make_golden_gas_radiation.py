#!/usr/bin/env python3
"""Generate tests/golden/g15_gas_radiation.npz by RUNNING THE UNMODIFIED REFERENCE SOURCE: grey_solar.grey_radiation
(grey_solar.py:192-320), the grey radiation that absorbs by water vapour and CO2, with clouds off (c = 0.0, as in its
only call, no_limits_2_5d.py:109-115).

Build-container only (needs /root/reference; never runs on the GPU box).  As make_golden.py, whose preamble it runs: the
unit-bookkeeping stand-in ./_pint_standin comes first on sys.path, everything numeric is executed by the reference's own
function, and this script only builds seeded inputs, strips units and saves.  The function prints lw_emissivity[10], so
the state has 12 levels.

Case A: the reference's weights.  Case B: the same state with a drier q and grey_solar.co2_sw_weight patched to 1e-3
(a module global the function reads when it is called), so that short wave reaches the ground and the two powers differ.

Usage:  python tests/golden/make_golden_gas_radiation.py        (rewrites the .npz file)
"""
import make_golden as mg  # noqa: E402  (sys.path, np.float and the reference's modules, as the other vectors use them)

import numpy as np  # noqa: E402

with mg.contextlib.redirect_stdout(mg._sink):
    import grey_solar  # noqa: E402

U = mg.U
L, H, W = 12, 6, 8


def main():
    rng = np.random.default_rng(15)
    geom = mg.quiet(mg.geometry.gen_geometry, H, W, L, sig_func=mg.geometry.manabe_sig)
    ptop = float(mg.m(geom.ptop))
    p = 1e5 + 500.0 * rng.standard_normal((H, W)) - ptop
    tt = 250.0 + 40.0 * rng.random((L, H, W))
    q_a = 10.0 ** rng.uniform(-5.0, -2.0, (L, H, W))
    q_b = 10.0 ** rng.uniform(-6.0, np.log10(2e-4), (L, H, W))
    gt = 280.0 + 20.0 * rng.random((H, W))
    g = mg.no_limits_2_5d.GroundVars(gt * U.K, None, None, None)
    out = dict(p=p, tt=tt, gt=gt, q_a=q_a, q_b=q_b, ptop=ptop, sig=mg.m(geom.sig).reshape(-1), dsig=mg.m(geom.dsig).reshape(-1),
               co2_mmr=float(mg.m(grey_solar.co2_mmr)), h2o_weight=float(mg.m(grey_solar.h2o_weight)),
               co2_weight=float(mg.m(grey_solar.co2_weight)), co2_sw_weight_a=float(mg.m(grey_solar.co2_sw_weight)),
               co2_sw_weight_b=1e-3, solar_constant=float(mg.m(2 * 41840 * U.J * U.m ** -2 * U.minute ** -1)),
               ground_albedo=0.1, co2_vmr=300 / 1e6)
    for tag, q, w in (("a", q_a, None), ("b", q_b, 1e-3)):
        keep = grey_solar.co2_sw_weight
        if w is not None:
            grey_solar.co2_sw_weight = w * U.m ** 2 * U.kg ** -1
        try:
            dtg, dta, up = mg.quiet(grey_solar.grey_radiation, p * U.Pa, q * U.dimensionless, tt * U.K, 0.0, g, 0.0 * U.s,
                                    900.0 * U.s, geom)
        finally:
            grey_solar.co2_sw_weight = keep
        out.update({"dt_ground_" + tag: mg.m(dtg), "dt_air_" + tag: mg.m(dta), "olr_" + tag: mg.m(up)})
        assert all(np.isfinite(out[k + tag]).all() for k in ("dt_ground_", "dt_air_", "olr_"))
    mg.save("g15_gas_radiation", **out)


if __name__ == "__main__":
    main()
