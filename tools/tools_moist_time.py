#!/usr/bin/env python3
"""The moist physics on the C4 grid (1440x720x24), humid cold-aloft state: what the phase adds to a step, and the kernel
alone against the bytes it must move.

One process, one handle per real type, the modes alternated A/B/C round after round (the state is set again before every
sample, so every sample starts from the same humid state), medians over the rounds:

  plain      the step without a registration
  moist      the step with set_moist(tau_e=0)
  moist_evap the step with set_moist(tau_e=86400)
  kernel_adjusted    --steps explicit gcm_moist_step calls (tau_e=0) on the ADJUSTED state between two synchronisations:
                     nothing condenses, the launch reads p, theta and q and reads and writes the sums (adjusted_bytes)
  kernel_condensing  four single gcm_moist_step calls, each on the freshly set humid state and between two
                     synchronisations of its own: the launch that condenses a third of the cells, against the upper
                     bound moist_bytes (every theta and q written).  A host clock around one launch: it includes that
                     launch's host overhead; the kernel's own time is the kernel trace's (profiles/moist)
  hs_kernel          --steps explicit gcm_held_suarez_step calls, whose unit has no measured time yet

Bytes, counted from shapes: the moist kernel reads p, theta and q once and writes theta and q where something condensed,
plus two float64 words per column read and written: at most (4 L + 3) H W elements (moist_bytes; the sums are float64
for either type), (2 L + 1) H W elements and the sums where nothing condenses (adjusted_bytes); the Held-Suarez launch:
tools_held_suarez_time.held_suarez_bytes.  The humid state is the tests' own (tests/pe25d_moist_ref.py, NumPy only):
the tool reads it from there so that what is timed is what is tested.

One JSON line per sample and one summary line.

  python3 tools/tools_moist_time.py [--rounds 5] [--steps 50] [--warmup 5] [--dtype f64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("plain", "moist", "moist_evap", "kernel_adjusted", "kernel_condensing", "hs_kernel")


def moist_bytes(H, W, L, itemsize=8):
    """the most one launch moves: p once, theta and q read and written, two float64 sums per column read and written"""
    return (1 + 4 * L) * H * W * itemsize + 4 * H * W * 8


def adjusted_bytes(H, W, L, itemsize=8):
    """what a launch moves where nothing condenses: p, theta and q read once, the two float64 sums read and written"""
    return (1 + 2 * L) * H * W * itemsize + 4 * H * W * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--shape", default="720,1440,24", help="H,W,L")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    import pe25d_moist_ref as ref
    from tools_held_suarez_time import friction_levels, held_suarez_bytes
    H, W, L = (int(x) for x in a.shape.split(","))
    dt = 60.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = ref.humid_state(geom, a.dtype)
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    esz = 8 if a.dtype == "f64" else 4
    nbytes = dict(kernel_adjusted=adjusted_bytes(H, W, L, esz), kernel_condensing=moist_bytes(H, W, L, esz),
                  hs_kernel=held_suarez_bytes(H, W, L, friction_levels(list(geom.sig.reshape(-1))), esz))
    samples = {m: [] for m in MODES}
    for rnd in range(a.rounds):
        for mode in MODES:
            core.set_moist(None)
            core.set_state(*st)
            if mode == "moist":
                core.set_moist()
            elif mode == "moist_evap":
                core.set_moist(tau_e=86400.0)
            if mode == "kernel_condensing":
                core.moist_step(dt)
                took = []
                for _ in range(4):
                    core.set_state(*st)
                    core.sync()
                    t0 = time.perf_counter()
                    core.moist_step(dt)
                    core.sync()
                    took.append((time.perf_counter() - t0) * 1e3)
                ms = statistics.median(took)
            elif mode in ("kernel_adjusted", "hs_kernel"):
                call = (lambda: core.moist_step(dt)) if mode == "kernel_adjusted" else (lambda: core.held_suarez_step(geom, dt))
                for _ in range(a.warmup):
                    call()                       # (the first call adjusts the state)
                core.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call()
                core.sync()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
            else:
                core.step(a.warmup, dt)
                core.set_state(*st)
                total, _ = core.time_steps(a.steps, dt, per_kernel=False)
                ms = total / a.steps
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, ms=ms)), flush=True)
    core.close()
    med = {m: statistics.median(v) for m, v in samples.items()}
    out = dict(summary=True, shape=[H, W, L], dtype=a.dtype, steps=a.steps, rounds=a.rounds, median_ms=med,
               spread_ms={m: max(v) - min(v) for m, v in samples.items()},
               added_ms_per_step=dict(moist=med["moist"] - med["plain"], moist_evap=med["moist_evap"] - med["plain"]),
               bytes=nbytes, gb_per_s={m: nbytes[m] / (med[m] * 1e-3) / 1e9 for m in nbytes})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
