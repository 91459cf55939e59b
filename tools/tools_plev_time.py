#!/usr/bin/env python3
"""The pressure-level climatology on the C4 grid (1440x720x24): what a sample costs beside the sigma climatology's, and
that it costs nothing when it is not registered.

(a) the step WITHOUT a registration, this tree against a checkout of the parent commit (--parent-root DIR, its library
    built), alternated A/B in one call on one box: every sample is a fresh process that loads one of the two libraries,
    warms up and times --steps steps through gcm_time_steps.  The spread is what the parent's own repeated samples
    show (max - min over their median); the two trees are "the same" when the medians differ by less than that.
(b) the sample alone, this tree, per real type: --steps explicit gcm_plev_climate_sample calls between two
    synchronisations at the 17 standard levels 1000 .. 10 hPa, and in the same process --steps gcm_climate_sample calls,
    the yardstick.  Beside the times: the bytes one full pass over the state would read, counted from shapes (u, v,
    theta and q of every level and p, once), and the number of target segments of the plan.  A segment reads only the
    levels that bracket its targets, so segments x pass bytes is an upper bound of what a sample requests, and the
    fraction of 8 TB/s it comes to over the sample's time is an upper bound too (above 1: less was read).  The kernel's own time
    comes from a kernel trace of the same child, in a run of its own (rocprofv3 --kernel-trace --stats -- python3
    tools/tools_plev_time.py --child kernel): pe_plev_climate_kernel's row.

One JSON line per sample and one summary line per part.

  python3 tools/tools_plev_time.py [--parent-root DIR] [--rounds 4] [--steps 100] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12                                            # bytes / s
STANDARD_HPA = (1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 20, 10)


def pass_bytes(H, W, L, itemsize=8):
    """what one pass over the state reads at least: u, v, theta and q of every level and p, once"""
    return (4 * L + 1) * H * W * itemsize


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=4, help="samples per tree of part (a)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"], help=argparse.SUPPRESS)
    ap.add_argument("--child", default=None, choices=["plain", "kernel"], help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    return ap


def child(a):
    """one sample in this process, with the package and the library of the tree at a.root"""
    sys.path.insert(0, a.root)
    import bench
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, _, _, _, dt = bench.WORKLOADS["c4"]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    core = g.Core(_lib.PE25D, W, H, L, geom=geom, dtype=a.dtype)
    core.set_state(**st)
    out = {"mode": a.child, "root": a.root, "grid": [W, H, L], "dtype": a.dtype, "steps": a.steps}
    if a.child == "kernel":
        core.set_climate(10 ** 9)
        core.set_plev_climate(10 ** 9, [100.0 * h for h in STANDARD_HPA])
        out["plan"] = core.plev_climate_plan()
        for name, call in (("climate", core.climate_sample), ("plev", core.plev_climate_sample)):
            call()
            core.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            core.sync()
            out[name + "_ms_per_sample"] = (time.perf_counter() - t0) * 1e3 / a.steps
        out["coverage_min_max"] = [float(x) for x in (core.plev_climate().coverage.min(), core.plev_climate().coverage.max())]
    else:
        core.step(a.warmup, dt)
        ms, _ = core.time_steps(a.steps, dt, per_kernel=False)
        out["ms_per_step"] = ms / a.steps
    core.close()
    print(json.dumps(out), flush=True)


def sample(a, root, mode, dtype="f64"):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--dtype", dtype]
    env = dict(os.environ)
    env.pop("GCMCORE_LIB", None)                           # (each tree loads its own library)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, check=True, timeout=600)
    line = r.stdout.decode().strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    a = parser().parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    import bench
    _, H, W, L, _, _, _, _ = bench.WORKLOADS["c4"]
    med = statistics.median
    new, old = [], []
    for _ in range(a.rounds):                              # alternated: parent, this tree, parent, ...
        if a.parent_root:
            old.append(sample(a, os.path.abspath(a.parent_root), "plain")["ms_per_step"])
        new.append(sample(a, ROOT, "plain")["ms_per_step"])
    part_a = {"part": "a", "what": "fp64 step without a registration, this tree against the parent",
              "this_ms_per_step": new, "this_median": med(new)}
    if old:
        spread = (max(old) - min(old)) / med(old)
        diff = (med(new) - med(old)) / med(old)
        part_a.update({"parent_ms_per_step": old, "parent_median": med(old), "parent_spread_rel": spread,
                       "median_difference_rel": diff, "same_within_spread": abs(diff) <= spread})
    else:
        part_a["note"] = "no --parent-root: the parent was not measured"
    print(json.dumps(part_a), flush=True)
    for dtype in ("f64", "f32"):
        k = sample(a, ROOT, "kernel", dtype)
        nb = pass_bytes(H, W, L, 8 if dtype == "f64" else 4)
        passes = k["plan"]["nseg"]
        print(json.dumps({"part": "b", "what": "one sample at the 17 standard levels beside the sigma climatology's", "dtype": dtype,
                          "plev_sample_ms": k["plev_ms_per_sample"], "climate_sample_ms": k["climate_ms_per_sample"],
                          "pass_bytes": nb, "passes": passes, "targets_per_pass": k["plan"]["targets"],
                          "passes_bytes_over_time_fraction_of_8_TB_per_s": passes * nb / (k["plev_ms_per_sample"] * 1e-3) / HBM_PEAK}),
              flush=True)


if __name__ == "__main__":
    main()
