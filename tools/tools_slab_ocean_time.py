#!/usr/bin/env python3
"""The slab ocean on the C4 grid (1440x720x24): its launch alone, and what the registered phase adds to a step that
carries the physics and the boundary layer.

One process, one handle, the modes alternated round after round (the state and the ground temperature are set again
before every sample), medians over the rounds:

  base         the step with set_physics() and set_boundary_layer(), no slab
  registered   the same step with set_slab_ocean(): the radiation's BUDGET launch, the boundary layer's two more stores
               per column and the slab launch
  slab_launch  --steps end_step() calls of a handle that has the slab registered and nothing else, between two
               synchronisations: the walk is then the slab launch alone (a host clock: launch overhead included)

The state is the tests' own (tests/pe25d_boundary_layer_ref.py, NumPy only).  One JSON line per sample and one summary.

  python3 tools/tools_slab_ocean_time.py [--rounds 5] [--steps 20] [--warmup 3] [--dtype f64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("base", "registered", "slab_launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--shape", default="720,1440,24", help="H,W,L")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    import pe25d_boundary_layer_ref as bref
    H, W, L = (int(x) for x in a.shape.split(","))
    dt = 60.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bref.windy_state(geom, a.dtype)
    gt = bref.ground(geom, st)
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    core.set_ground(gt)
    samples = {m: [] for m in MODES}
    for rnd in range(a.rounds):
        for mode in MODES:
            core.set_slab_ocean(None)
            core.set_boundary_layer(None)
            core.set_physics(None)
            core.set_state(*st)
            core.set_ground(gt)
            if mode == "slab_launch":
                core.set_slab_ocean()
                for _ in range(a.warmup):
                    core.end_step(dt)
                core.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    core.end_step(dt)
                core.sync()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
            else:
                core.set_physics(geom, 0.0)
                core.set_boundary_layer()
                if mode == "registered":
                    core.set_slab_ocean()
                core.step(a.warmup, dt)
                core.set_state(*st)
                core.set_ground(gt)
                total, _ = core.time_steps(a.steps, dt, per_kernel=False)
                ms = total / a.steps
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, ms=ms)), flush=True)
    core.close()
    med = {m: statistics.median(v) for m, v in samples.items()}
    print(json.dumps(dict(summary=True, shape=[H, W, L], dtype=a.dtype, steps=a.steps, rounds=a.rounds, median_ms=med,
                          spread_ms={m: max(v) - min(v) for m, v in samples.items()},
                          added_ms_per_step=med["registered"] - med["base"])), flush=True)


if __name__ == "__main__":
    main()
