#!/usr/bin/env python3
"""The tracers' forcing (gcm_set_tracer_forcing) on the C4 grid (1440x720x24) with 4 tracers: ms per step through
gcm_time_steps with 0, 1 and 4 forced tracers, fp64 and fp32, the cases alternating over `--rounds` rounds in one
process (one handle per case, kept for all rounds), one JSON line per case and round, with the bytes the forcing kernel
moves per step counted from shapes (forcing_bytes_per_step).  The kernel's own time comes from a run under
`rocprofv3 --kernel-trace --stats` (pe_tracer_force_kernel); its counted TB/s = forcing_bytes_per_step / that time.
On a tree without the forcing only the unforced case runs (the parent's figure, for an alternating comparison).

  python3 tools/tools_tracer_forcing_time.py [--steps 20] [--warmup 3] [--rounds 3] [--dtype f64 f32]
                                             [--forced 0 1 4] [--fields full|none]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NTR = 4


def forcing_bytes_per_step(H, W, L, forced, itemsize, emission, mask):
    """per forced tracer and step: the field read and written once, the emission read once in the handle's real
    type, the mask one byte per cell"""
    cells = H * W * L
    return forced * cells * (2 * itemsize + (itemsize if emission else 0) + (1 if mask else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", nargs="+", default=["f64", "f32"])
    ap.add_argument("--forced", nargs="+", type=int, default=[0, 1, 4])
    ap.add_argument("--fields", choices=["full", "none"], default="full",
                    help="full: source, decay, an emission field and a mask per forced tracer; none: source and decay")
    a = ap.parse_args()
    import numpy as np
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    rng = np.random.default_rng(5)
    has = hasattr(g.Core, "set_tracer_forcing")
    full = a.fields == "full"
    emission = 1e-6 * rng.random((L, H, W)) if full else None
    mask = np.zeros((L, H, W), dtype=bool)
    mask[int(np.argmax(np.asarray(geom.sig)))] = True
    cases = []
    for dtype in a.dtype:
        trs = 1.0 + rng.random((NTR, L, H, W))
        for nf in a.forced:
            if nf and not has:
                continue
            core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=dtype)
            core.set_state(**st)
            core.set_tracers(trs)
            for i in range(nf):
                core.set_tracer_forcing(i, source=1e-6, decay=2.1e-6, emission=emission, pin_mask=mask if full else None)
            core.step(a.warmup, dt)
            cases.append((dtype, nf, core))
    for rnd in range(a.rounds):
        for dtype, nf, core in cases:
            ms, _ = core.time_steps(a.steps, dt, per_kernel=False)
            isz = 8 if dtype == "f64" else 4
            print(json.dumps({"grid": [W, H, L], "dtype": dtype, "tracers": NTR, "forced": nf, "fields": a.fields,
                              "round": rnd, "steps": a.steps, "ms_per_step": round(ms / a.steps, 5),
                              "forcing_bytes_per_step": forcing_bytes_per_step(H, W, L, nf, isz, full, full),
                              "has_forcing": has}), flush=True)
    for _, _, core in cases:
        core.close()


if __name__ == "__main__":
    main()
