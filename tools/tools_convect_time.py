#!/usr/bin/env python3
"""The convective adjustment on the C4 grid (1440x720x24): what the phase adds to a step, on an all-stable state (the
price every step pays) and on a state with a documented share of unstable columns, and the kernel alone.

One process, one handle per real type, the modes alternated round after round (the state is set again before every
sample, so every sample starts from the same state), medians over the rounds:

  plain_stable / convect_stable      the step without and with set_convect(gamma=6.5e-3) on the quiet state
                                     (tests/pe25d_convect_ref.unstable_state(..., stable=True): no column is unstable
                                     when the run starts; what the dynamics make unstable on the way is adjusted)
  plain_unstable / convect_unstable  the same on the unstable state: 6 of 7 columns carry 3 K of noise on a 40 K
                                     profile, about 85 % of all columns are adjusted by the first application (the share
                                     the summary prints is counted by the handle: convect_sums().frequency after one step)
  kernel_stable     --steps explicit gcm_convect_step calls on the quiet state between two synchronisations: every wave
                    leaves after pass 1, the launch reads p and theta once (stable_bytes)
  kernel_unstable   four single gcm_convect_step calls, each on the freshly set unstable state and between two
                    synchronisations of its own (a host clock around one launch: it includes that launch's overhead)
  kernel_dry_stable the same as kernel_stable with the dry adjustment (no exp and log per cell in pass 1)

Bytes, counted from shapes: a stable wave reads p and theta once, (L + 1) H W elements (stable_bytes); an unstable wave
reads theta again (from L2 where it still is) with q, and writes theta and q of its merged blocks, plus two float64 words
per adjusted column read and written: at most (5 L + 1) H W elements and the sums (unstable_bytes).

The parent commit has no such phase: its step is this tree's plain step, the same launches from the same kernels.
--parent-root <checkout of the parent commit, library built> adds the modes parent_stable / parent_unstable, that
library's step in a child process of its own per round, alternated with this tree's.

One JSON line per sample and one summary line.

  python3 tools/tools_convect_time.py [--rounds 5] [--steps 50] [--warmup 5] [--dtype f64] [--parent-root DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 6.5e-3
MODES = ("plain_stable", "convect_stable", "plain_unstable", "convect_unstable", "kernel_stable", "kernel_dry_stable",
         "kernel_unstable")


def stable_bytes(H, W, L, itemsize=8):
    """what a launch moves where no wave has an unstable lane: p and theta read once"""
    return (1 + L) * H * W * itemsize


def unstable_bytes(H, W, L, itemsize=8):
    """the most one launch moves: p once, theta read twice, q read once, theta and q written, two float64 sums per
    column read and written"""
    return (1 + 5 * L) * H * W * itemsize + 4 * H * W * 8


def plain_step_ms(root, shape, dtype, stable, steps, warmup):
    """the plain step of the library under `root`, in a child process of its own -> ms per step"""
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import gcmiipy_amd as g\nfrom gcmiipy_amd import _lib, geometry\nimport pe25d_convect_ref as ref\n"
            "H, W, L = %r\ngeom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)\n"
            "st = ref.unstable_state(geom, ref.kappa_of(%r), %r, stable=%r)\n"
            "c = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=%r)\nc.set_state(*st)\nc.step(%d, 60.0)\nc.set_state(*st)\n"
            "total, _ = c.time_steps(%d, 60.0, per_kernel=False)\nprint(json.dumps(total / %d))\n"
            % (root, os.path.join(ROOT, "tests"), tuple(shape), GAMMA, dtype, stable, dtype, warmup, steps, steps))
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
    import pe25d_convect_ref as ref
    H, W, L = (int(x) for x in a.shape.split(","))
    dt = 60.0
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    kc = ref.kappa_of(GAMMA)
    states = dict(stable=ref.unstable_state(geom, kc, a.dtype, stable=True), unstable=ref.unstable_state(geom, kc, a.dtype),
                  dry_stable=ref.unstable_state(geom, 0.0, a.dtype, stable=True))
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    esz = 8 if a.dtype == "f64" else 4
    nbytes = dict(kernel_stable=stable_bytes(H, W, L, esz), kernel_dry_stable=stable_bytes(H, W, L, esz),
                  kernel_unstable=unstable_bytes(H, W, L, esz))
    modes = MODES + (("parent_stable", "parent_unstable") if a.parent_root else ())
    samples = {m: [] for m in modes}
    share = {}
    for which in ("stable", "unstable"):
        core.set_state(*states[which])
        core.set_convect(gamma=GAMMA)
        core.convect_step(gamma=GAMMA)
        share[which] = float(core.convect_sums().frequency.mean())
        core.set_convect(None)
    for rnd in range(a.rounds):
        for mode in modes:
            kind, _, which = mode.partition("_")
            core.set_convect(None)
            if kind == "parent":
                ms = plain_step_ms(a.parent_root, (H, W, L), a.dtype, which == "stable", a.steps, a.warmup)
            elif mode == "kernel_unstable":
                took = []
                for _ in range(4):
                    core.set_state(*states["unstable"])
                    core.sync()
                    t0 = time.perf_counter()
                    core.convect_step(gamma=GAMMA)
                    core.sync()
                    took.append((time.perf_counter() - t0) * 1e3)
                ms = statistics.median(took)
            elif kind == "kernel":
                par = dict(gamma=None if which == "dry_stable" else GAMMA)
                core.set_state(*states[which])
                for _ in range(a.warmup):
                    core.convect_step(**par)
                core.sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    core.convect_step(**par)
                core.sync()
                ms = (time.perf_counter() - t0) * 1e3 / a.steps
            else:
                core.set_state(*states[which])
                if kind == "convect":
                    core.set_convect(gamma=GAMMA)
                core.step(a.warmup, dt)
                core.set_state(*states[which])
                total, _ = core.time_steps(a.steps, dt, per_kernel=False)
                ms = total / a.steps
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, ms=ms)), flush=True)
    core.close()
    med = {m: statistics.median(v) for m, v in samples.items()}
    out = dict(summary=True, shape=[H, W, L], dtype=a.dtype, steps=a.steps, rounds=a.rounds, median_ms=med,
               spread_ms={m: max(v) - min(v) for m, v in samples.items()},
               added_ms_per_step=dict(stable=med["convect_stable"] - med["plain_stable"],
                                      unstable=med["convect_unstable"] - med["plain_unstable"]),
               adjusted_share_first_application=share,
               bytes=nbytes, gb_per_s={m: nbytes[m] / (med[m] * 1e-3) / 1e9 for m in nbytes})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
