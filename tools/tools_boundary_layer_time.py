#!/usr/bin/env python3
"""The surface fluxes and the boundary-layer mixing on the C4 grid (1440x720x24), the tests' windy humid state over a
ground with warmer and colder cells: what the phase adds to a step, and its two launches alone against the bytes they
must move.

One process, one handle per real type, the modes alternated round after round (the state is set again before every
sample), medians over the rounds:

  plain     the step without a registration (the launches of a handle that never heard of the phase)
  boundary  the step with set_boundary_layer()
  launches  --steps explicit gcm_boundary_layer_step calls between two synchronisations: the two launches back to back
  parent    (--parent-root <checkout of the parent commit, library built>) the parent commit's step, which has no such
            phase, by its own library and package in a child process of its own, alternated with the others

Bytes, counted from shapes (phase_bytes): theta, q, u and v read and written once, e written once and read three times
(once from the lane's own column by each wind plane and once from a neighbouring column: the other plane's neighbour is
served by the same lines), p, the ground and cd, r a few times, the two float64 sums read and written.  e, cd, r and the
sums are float64 for either storage type.  The state is the tests' own (tests/pe25d_boundary_layer_ref.py, NumPy only),
so that what is timed is what is tested.

One JSON line per sample and one summary line.

  python3 tools/tools_boundary_layer_time.py [--rounds 5] [--steps 50] [--warmup 5] [--dtype f64] [--parent-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("plain", "boundary", "launches")


def phase_bytes(H, W, L, itemsize=8):
    """what the two launches move: four fields read and written, p once, e written once and read three times, the
    ground, cd and r (written once, read four times) and the two sums read and written"""
    return (8 * L + 1) * H * W * itemsize + (4 * (L - 1) + 1 + 2 * 5 + 4) * H * W * 8


def parent_step_ms(root, shape, dtype, steps, warmup):
    """the step of the library under `root` on the same state, in a child process of its own -> ms per step"""
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import gcmiipy_amd as g\nfrom gcmiipy_amd import _lib, geometry\nimport pe25d_boundary_layer_ref as ref\n"
            "H, W, L = %r\ngeom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)\n"
            "st = ref.windy_state(geom, %r)\n"
            "c = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=%r)\nc.set_ground(ref.ground(geom, st))\n"
            "c.set_state(*st)\nc.step(%d, 60.0)\nc.set_state(*st)\n"
            "total, _ = c.time_steps(%d, 60.0, per_kernel=False)\nprint(json.dumps(total / %d))\n"
            % (root, os.path.join(ROOT, "tests"), tuple(shape), dtype, dtype, warmup, steps, steps))
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=600).stdout
    return float(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--shape", default="720,1440,24", help="H,W,L")
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    import pe25d_boundary_layer_ref as ref
    H, W, L = (int(x) for x in a.shape.split(","))
    dt = 60.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = ref.windy_state(geom, a.dtype)
    gt = ref.ground(geom, st)
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    core.set_ground(gt)
    nbytes = phase_bytes(H, W, L, 8 if a.dtype == "f64" else 4)
    modes = MODES + (("parent",) if a.parent_root else ())
    samples = {m: [] for m in modes}
    for rnd in range(a.rounds):
        for mode in modes:
            if mode == "parent":
                ms = parent_step_ms(a.parent_root, (H, W, L), a.dtype, a.steps, a.warmup)
                samples[mode].append(ms)
                print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, ms=ms)), flush=True)
                continue
            core.set_boundary_layer(None)
            core.set_state(*st)
            if mode == "boundary":
                core.set_boundary_layer()
            if mode == "launches":
                for _ in range(a.warmup):
                    core.boundary_layer_step(dt)
                core.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    core.boundary_layer_step(dt)
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
               added_ms_per_step=med["boundary"] - med["plain"],
               added_ms_over_parent=(med["boundary"] - med["parent"]) if a.parent_root else None, bytes=nbytes,
               gb_per_s=nbytes / (med["launches"] * 1e-3) / 1e9)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
