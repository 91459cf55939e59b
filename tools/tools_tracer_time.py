#!/usr/bin/env python3
"""Passive tracers on the C4 grid (1440x720x24, fp64 and fp32): ms per step through gcm_time_steps with 0, 1, 2
and 4 tracers, one JSON line per case, with the bytes the tracer kernel moves per step counted from shapes
(tracer_bytes_per_step).  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`
(pe_tracer_kernel; pe_tracer_lim_kernel under --scheme upwind / van_leer); their counted TB/s =
tracer_bytes_per_step / kernel time per step.

  python3 tools/tools_tracer_time.py [--steps 20] [--warmup 3] [--dtype f64 f32] [--tracers 0 1 2 4]
                                     [--scheme none upwind van_leer]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunks(n):
    """launches of the tracer kernel per stage are chunks of 4, then 2, then 1 tracers (pe25d_tracers.hip,
    launch_tracers): the number of chunks"""
    return n // 4 + (n % 4) // 2 + n % 2


def tracer_bytes_per_step(H, W, L, n, itemsize=8):
    """bytes the tracer kernel must move per Matsuno step (predictor + corrector) for n tracers, under any scheme
    (the limited schemes request more neighbours, all of them cells another thread requests as its own):
    per tracer and cell, the predictor reads the stage tracer and writes the star one (2 words: 16 B in fp64) and
    the corrector reads the stage and the base tracer and writes the result (3 words: 24 B); per chunk and stage
    the shared spu and sv (3-D) and pit (2-D) are read once.  Neighbour reads are counted once (cache hits)."""
    cells = H * W * L
    per_tracer = (2 + 3) * cells * itemsize
    shared = 2 * chunks(n) * (2 * cells + H * W) * itemsize
    return n * per_tracer + shared


SCHEMES = {"none": 0, "upwind": 1, "van_leer": 2}      # GCM_TRACER_NONE / _UPWIND / _VANLEER (gcm_set_tracer_scheme)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["f64", "f32"])
    ap.add_argument("--tracers", nargs="+", type=int, default=[0, 1, 2, 4])
    ap.add_argument("--scheme", nargs="+", choices=sorted(SCHEMES), default=["none"],
                    help="the tracers' transport scheme(s); every case is timed under each")
    return ap


def main():
    a = parser().parse_args()
    import numpy as np
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    rng = np.random.default_rng(5)
    base = {}
    for dtype, scheme in ((d, s) for d in a.dtype for s in a.scheme):
        isz = 8 if dtype == "f64" else 4
        for n in a.tracers:
            if n == 0 and dtype in base:
                continue                                # (no tracers: no scheme to tell apart)
            core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=dtype, tracer_scheme=SCHEMES[scheme])
            core.set_state(**st)
            if n:
                core.set_tracers(1.0 + rng.random((n, L, H, W)))
            core.step(a.warmup, dt)
            ms, _ = core.time_steps(a.steps, dt, per_kernel=False)
            core.close()
            per = ms / a.steps
            if n == 0:
                base[dtype] = per
            nb = tracer_bytes_per_step(H, W, L, n, isz)
            print(json.dumps({"grid": [W, H, L], "dtype": dtype, "scheme": scheme if n else None, "tracers": n,
                              "steps": a.steps,
                              "ms_per_step": round(per, 4),
                              "added_ms_per_step": round(per - base[dtype], 4) if dtype in base else None,
                              "tracer_bytes_per_step": nb,
                              "tracer_bytes_per_tracer_step": (nb / n) if n else 0}), flush=True)


if __name__ == "__main__":
    main()
