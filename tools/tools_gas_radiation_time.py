#!/usr/bin/env python3
"""The gas radiation on the C4 grid (1440x720x24): its launch alone beside the grey radiation's from the same run, and
what the registered phase changes in a step that carries the physics.

One process, one handle, the modes alternated round after round (the state and the ground temperature are set again
before every sample), medians over the rounds:

  grey_step    the step with set_physics(): the grey radiation in the solar slot
  gas_step     the same step with set_gas_radiation(): the gas radiation in its place
  grey_launch  --steps solar_step() calls between two synchronisations: the grey kernel's launch alone
  gas_launch   --steps gas_radiation_step() calls between two synchronisations: the new kernel's launch alone, with the
               reference's weights (one power per level and scan)
  gas_launch_unequal  the same with unequal weight pairs (two powers per level in the top-down scan)
(the launch modes use a host clock: launch overhead included)

The state is the tests' own (tests/pe25d_gas_radiation_ref.py, NumPy only).  One JSON line per sample and one summary.

  python3 tools/tools_gas_radiation_time.py [--rounds 5] [--steps 20] [--warmup 3] [--dtype f64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("grey_step", "gas_step", "grey_launch", "gas_launch", "gas_launch_unequal")


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
    import pe25d_gas_radiation_ref as ref
    H, W, L = (int(x) for x in a.shape.split(","))
    dt = 60.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st, gt = ref.state(geom, a.dtype)
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    core.set_ground(gt)
    samples = {m: [] for m in MODES}
    for rnd in range(a.rounds):
        for mode in MODES:
            core.set_gas_radiation(None)
            core.set_physics(None)
            core.set_state(*st)
            core.set_ground(gt)
            if mode.endswith("_step"):
                core.set_physics(geom, 0.0)
                if mode == "gas_step":
                    core.set_gas_radiation(insolation="zenith")
                core.step(a.warmup, dt)
                core.set_state(*st)
                core.set_ground(gt)
                total, _ = core.time_steps(a.steps, dt, per_kernel=False)
                ms = total / a.steps
            else:
                over = dict(insolation="zenith", k_co2_sw=1e-3) if mode == "gas_launch_unequal" else dict(insolation="zenith")
                call = (lambda: core.solar_step(geom, dt, 0.0)) if mode == "grey_launch" else \
                    (lambda: core.gas_radiation_step(geom, dt, 0.0, **over))
                for _ in range(a.warmup):
                    call()
                core.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call()
                core.sync()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, ms=ms)), flush=True)
    core.close()
    med = {m: statistics.median(v) for m, v in samples.items()}
    print(json.dumps(dict(summary=True, shape=[H, W, L], dtype=a.dtype, steps=a.steps, rounds=a.rounds, median_ms=med,
                          spread_ms={m: max(v) - min(v) for m, v in samples.items()},
                          step_change_ms=med["gas_step"] - med["grey_step"])), flush=True)


if __name__ == "__main__":
    main()
