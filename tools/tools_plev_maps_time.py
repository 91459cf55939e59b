#!/usr/bin/env python3
"""The pressure-level maps on the C4 grid (1440x720x24): what a sample costs beside the pressure-level climatology's,
and that it costs nothing when it is not registered.

(a) the step WITHOUT a registration, this tree against a checkout of the parent commit (--parent-root DIR, its library
    built), alternated A/B in one call on one box: every sample is a fresh process that loads one of the two libraries,
    warms up and times --steps steps through gcm_time_steps.  The spread is what the parent's own repeated samples
    show (max - min over their median); the two trees are "the same" when the medians differ by less than that.
(b) the sample alone, this tree, per real type: --steps explicit gcm_plev_maps_sample calls between two
    synchronisations at 850, 500 and 250 hPa, and in the same process --steps gcm_plev_climate_sample calls at the
    same three targets and at the 17 standard levels, the yardsticks.  Beside the times, the bytes a sample needs,
    counted from shapes and from the record's coverage (the fraction of valid (target, column) pairs):
      p                         H W elements
      theta                     L H W elements, once from memory (the second read is the cache's)
      bracket cells             per valid pair two levels of u, of v in rows j and j - 1, and of q: 8 elements
                                (u[i - 1] comes with the lines of u[i]; theta of the bracket is in registers)
      sums                      2 x 8 x (13 valid pairs + 2 H W) bytes: read and written, float64 on either handle
    and what fraction of 8 TB/s those bytes over the sample's time come to.  The kernel's own time comes from a kernel
    trace of the same child, in a run of its own (rocprofv3 --kernel-trace --stats -- python3
    tools/tools_plev_maps_time.py --child kernel): pe_plev_height_kernel's row.

One JSON line per sample and one summary line per part.

  python3 tools/tools_plev_maps_time.py [--parent-root DIR] [--rounds 4] [--steps 100] [--warmup 10]
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
MAP_HPA = (850, 500, 250)
STANDARD_HPA = (1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 20, 10)


def sample_bytes(H, W, L, valid_pairs, itemsize=8):
    """what one sample of the maps needs: the state it reads (in the handle's real type) and the sums it reads and
    writes (float64); valid_pairs: the number of (target, column) pairs in which the target is valid"""
    state = (H * W + L * H * W + 8 * valid_pairs) * itemsize
    sums = 2 * 8 * (13 * valid_pairs + 2 * H * W)
    return {"state_bytes": int(state), "sums_bytes": int(sums), "bytes": int(state + sums)}


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
        targets = [100.0 * h for h in MAP_HPA]
        core.set_plev_maps(10 ** 9, targets)
        out["plan"] = core.plev_maps_plan()

        def timed(name, call):
            call()
            core.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            core.sync()
            out[name + "_ms_per_sample"] = (time.perf_counter() - t0) * 1e3 / a.steps
        timed("maps", core.plev_maps_sample)
        rec = core.plev_maps()
        out["valid_pairs"] = float(rec.coverage.sum())
        out["coverage_per_target"] = [float(rec.coverage[n].mean()) for n in range(len(targets))]
        core.set_plev_climate(10 ** 9, targets)
        timed("plev_climate_same_targets", core.plev_climate_sample)
        core.set_plev_climate(10 ** 9, [100.0 * h for h in STANDARD_HPA])
        timed("plev_climate_17_levels", core.plev_climate_sample)
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
        nb = sample_bytes(H, W, L, k["valid_pairs"], 8 if dtype == "f64" else 4)
        line = {"part": "b", "what": "one sample at 850 / 500 / 250 hPa beside the pressure-level climatology's", "dtype": dtype,
                "maps_sample_ms": k["maps_ms_per_sample"], "plev_climate_same_targets_ms": k["plev_climate_same_targets_ms_per_sample"],
                "plev_climate_17_levels_ms": k["plev_climate_17_levels_ms_per_sample"], "coverage_per_target": k["coverage_per_target"]}
        line.update(nb)
        line["bytes_over_time_fraction_of_8_TB_per_s"] = nb["bytes"] / (k["maps_ms_per_sample"] * 1e-3) / HBM_PEAK
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
