#!/usr/bin/env python3
"""The zonal wavenumber spectra on the C4 grid (1440x720x24): what one sample costs, beside the climatology's sample
from the same process.

Both diagnostics are registered with an interval nothing reaches; after a warm-up, --steps explicit samples of each run
between two synchronisations, --rounds times, alternated (spectra, climatology, spectra, ...).  The bytes a sample must
read are counted from shapes (u, v and theta once per level, p once; the sums it reads and writes: 2 x 6 L H M doubles)
and set against 8 TB/s; the registration's device bytes are counted the same way.  One JSON line per real type and mmax.

  python3 tools/tools_spectra_time.py [--rounds 4] [--steps 50] [--warmup 5] [--mmax -1 720]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12                                            # bytes / s


def state_bytes(H, W, L, itemsize):
    """the least one sample reads of the state: u, v and theta of every level and p, once"""
    return (3 * L + 1) * H * W * itemsize


def timed(core, call, steps):
    core.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    core.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mmax", type=int, nargs="+", default=[-1, 720])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    for dtype in a.dtypes:
        isz = 8 if dtype == "f64" else 4
        core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=dtype)
        core.set_state(**st)
        core.step(2, dt)
        core.set_climate(10 ** 9)
        for mmax in a.mmax:
            core.set_spectra(10 ** 9, None if mmax < 0 else mmax)
            M = core.spectra_mmax + 1
            for _ in range(a.warmup):
                core.spectra_sample()
                core.climate_sample()
            spec, clim = [], []
            for _ in range(a.rounds):
                spec.append(timed(core, core.spectra_sample, a.steps))
                clim.append(timed(core, core.climate_sample, a.steps))
            sums = 8 * _lib.SPEC_WORDS * L * H * M
            nb = state_bytes(H, W, L, isz) + 2 * sums
            ms = statistics.median(spec)
            print(json.dumps({"grid": [W, H, L], "dtype": dtype, "mmax": M - 1, "plan": core.spectra_plan(),
                              "spectra_sample_ms": spec, "spectra_sample_median_ms": ms,
                              "climate_sample_ms": clim, "climate_sample_median_ms": statistics.median(clim),
                              "registration_bytes": 8 * (2 * W + L) + sums, "sample_bytes_budget": nb,
                              "sample_fraction_of_8_TB_per_s": nb / (ms * 1e-3) / HBM_PEAK}), flush=True)
        core.close()


if __name__ == "__main__":
    main()
