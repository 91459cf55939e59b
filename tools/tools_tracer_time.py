#!/usr/bin/env python3
"""Passive tracers on the C4 grid (1440x720x24, fp64 and fp32): ms per step through gcm_time_steps with 0, 1, 2
and 4 tracers, one JSON line per case, with the bytes the tracer kernel moves per step counted from shapes
(tracer_bytes_per_step).  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`
(pe_tracer_kernel); their counted TB/s = tracer_bytes_per_step / kernel time per step.

  python3 tools/tools_tracer_time.py [--steps 20] [--warmup 3] [--dtype f64 f32] [--tracers 0 1 2 4]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunks(n):
    """launches of the tracer kernel per stage are chunks of 4, then 2, then 1 tracers (pe25d_kernels.hip,
    launch_tracers): the number of chunks"""
    return n // 4 + (n % 4) // 2 + n % 2


def tracer_bytes_per_step(H, W, L, n, itemsize=8):
    """bytes the tracer kernel must move per Matsuno step (predictor + corrector) for n tracers:
    per tracer and cell, the predictor reads the stage tracer and writes the star one (2 words: 16 B in fp64) and
    the corrector reads the stage and the base tracer and writes the result (3 words: 24 B); per chunk and stage
    the shared spu and sv (3-D) and pit (2-D) are read once.  Neighbour reads are counted once (cache hits)."""
    cells = H * W * L
    per_tracer = (2 + 3) * cells * itemsize
    shared = 2 * chunks(n) * (2 * cells + H * W) * itemsize
    return n * per_tracer + shared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["f64", "f32"])
    ap.add_argument("--tracers", nargs="+", type=int, default=[0, 1, 2, 4])
    a = ap.parse_args()
    import numpy as np
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    rng = np.random.default_rng(5)
    base = {}
    for dtype in a.dtype:
        isz = 8 if dtype == "f64" else 4
        for n in a.tracers:
            core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=dtype)
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
            print(json.dumps({"grid": [W, H, L], "dtype": dtype, "tracers": n, "steps": a.steps,
                              "ms_per_step": round(per, 4),
                              "added_ms_per_step": round(per - base[dtype], 4) if dtype in base else None,
                              "tracer_bytes_per_step": nb,
                              "tracer_bytes_per_tracer_step": (nb / n) if n else 0}), flush=True)


if __name__ == "__main__":
    main()
