#!/usr/bin/env python3
"""The tracers' implicit vertical mixing (gcm_set_tracer_mixing) on the C4 grid (1440x720x24) in fp64 with 4 tracers:
ms per step through gcm_time_steps three ways -- no mixing, all four mixed, all four mixed and forced (source, decay, an
emission field and a mask each) -- the cases alternating over `--rounds` rounds in one process (one handle per case,
kept for all rounds), one JSON line per case and round, with the bytes the mixing kernel should move per step counted
from shapes (mixing_bytes_per_step: every mixed cell read once and written once).  On a tree without the mixing only
the first case runs (the parent's figure, for an alternating comparison); the cost per mixed tracer is
(mixed - none) / 4 of the same process.

  python3 tools/tools_tracer_mixing_time.py [--steps 20] [--warmup 3] [--rounds 3] [--dtype f64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NTR = 4


def mixing_bytes_per_step(H, W, L, mixed, itemsize):
    """per mixed tracer and step: the field read once and written once (the tables are 3 L values)"""
    return mixed * H * W * L * 2 * itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["f64"])
    a = ap.parse_args()
    import numpy as np
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    rng = np.random.default_rng(5)
    has = hasattr(g.Core, "set_tracer_mixing")
    emission = 1e-6 * rng.random((L, H, W))
    mask = np.zeros((L, H, W), dtype=bool)
    mask[int(np.argmax(np.asarray(geom.sig)))] = True
    k = (0.2 + rng.random(L - 1)) * 1.0e-2 / L ** 2               # sigma^2 / s: off-diagonal entries of order one at dt = 120 s
    cases = []
    for dtype in a.dtype:
        trs = 1.0 + rng.random((NTR, L, H, W))
        for case in ("none", "mixed", "mixed+forced"):
            if case != "none" and not has:
                continue
            core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=dtype)
            core.set_state(**st)
            core.set_tracers(trs)
            for i in range(NTR if case != "none" else 0):
                core.set_tracer_mixing(i, k)
                if case == "mixed+forced":
                    core.set_tracer_forcing(i, source=1e-6, decay=2.1e-6, emission=emission, pin_mask=mask)
            core.step(a.warmup, dt)
            cases.append((dtype, case, core))
    for rnd in range(a.rounds):
        for dtype, case, core in cases:
            ms, _ = core.time_steps(a.steps, dt, per_kernel=False)
            isz = 8 if dtype == "f64" else 4
            print(json.dumps({"grid": [W, H, L], "dtype": dtype, "tracers": NTR, "case": case,
                              "mixed": 0 if case == "none" else NTR, "round": rnd, "steps": a.steps,
                              "ms_per_step": round(ms / a.steps, 5),
                              "mixing_bytes_per_step": mixing_bytes_per_step(H, W, L, 0 if case == "none" else NTR, isz),
                              "has_mixing": has}), flush=True)
    for _, _, core in cases:
        core.close()


if __name__ == "__main__":
    main()
