#!/usr/bin/env python3
"""The zonal-mean climatology on the C4 grid (1440x720x24): what a sample costs, and that it costs nothing when it is
not registered.

(a) the step WITHOUT a registration, this tree against a checkout of the parent commit (--parent-root DIR, its library
    built), alternated A/B in one call on one box: every sample is a fresh process that loads one of the two libraries,
    warms up and times --steps steps through gcm_time_steps.  The spread is what the parent's own repeated samples
    show (max - min over their median); the two trees are "the same" when the medians differ by less than that.
(b) the step WITH the climatology registered (this tree), every = 1 and every = 8: the added time per step; and the
    sample alone (--steps explicit gcm_climate_sample calls between two synchronisations) against the bytes it must
    read, counted from shapes (climate_bytes: u, v and theta once per level, p once), as a fraction of 8 TB/s.  The
    kernel's own time comes from a kernel trace of the same child (rocprofv3 --kernel-trace --stats -- python3
    tools/tools_climate_time.py --child kernel): pe_climate_kernel's row.

One JSON line per sample and one summary line per part.

  python3 tools/tools_climate_time.py [--parent-root DIR] [--rounds 4] [--steps 100] [--warmup 10] [--dtype f64]
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


def climate_bytes(H, W, L, itemsize=8):
    """the least one sample reads: u, v and theta of every level and p, once"""
    return (3 * L + 1) * H * W * itemsize


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=4, help="samples per tree and mode")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--child", default=None, choices=["plain", "every1", "every8", "kernel"], help=argparse.SUPPRESS)
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
        core.climate_sample()
        core.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            core.climate_sample()
        core.sync()
        out["ms_per_sample"] = (time.perf_counter() - t0) * 1e3 / a.steps
    else:
        if a.child != "plain":
            core.set_climate(1 if a.child == "every1" else 8)
        core.step(a.warmup, dt)
        ms, _ = core.time_steps(a.steps, dt, per_kernel=False)
        out["ms_per_step"] = ms / a.steps
    core.close()
    print(json.dumps(out), flush=True)


def sample(a, root, mode):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--dtype", a.dtype]
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
    isz = 8 if a.dtype == "f64" else 4
    med = statistics.median
    new, old = [], []
    for _ in range(a.rounds):                              # alternated: parent, this tree, parent, ...
        if a.parent_root:
            old.append(sample(a, os.path.abspath(a.parent_root), "plain")["ms_per_step"])
        new.append(sample(a, ROOT, "plain")["ms_per_step"])
    part_a = {"part": "a", "what": "step without a registration, this tree against the parent", "dtype": a.dtype,
              "this_ms_per_step": new, "this_median": med(new)}
    if old:
        spread = (max(old) - min(old)) / med(old)
        diff = (med(new) - med(old)) / med(old)
        part_a.update({"parent_ms_per_step": old, "parent_median": med(old), "parent_spread_rel": spread,
                       "median_difference_rel": diff, "same_within_spread": abs(diff) <= spread})
    else:
        part_a["note"] = "no --parent-root: the parent was not measured"
    print(json.dumps(part_a), flush=True)
    e1 = [sample(a, ROOT, "every1")["ms_per_step"] for _ in range(a.rounds)]
    e8 = [sample(a, ROOT, "every8")["ms_per_step"] for _ in range(a.rounds)]
    kern = [sample(a, ROOT, "kernel")["ms_per_sample"] for _ in range(max(1, a.rounds // 2))]
    nb = climate_bytes(H, W, L, isz)
    print(json.dumps({"part": "b", "what": "step with the climatology registered", "dtype": a.dtype,
                      "every1_ms_per_step": e1, "every1_median": med(e1), "every1_added_ms_per_step": med(e1) - med(new),
                      "every8_ms_per_step": e8, "every8_median": med(e8), "every8_added_ms_per_step": med(e8) - med(new),
                      "sample_ms": kern, "sample_median_ms": med(kern), "sample_bytes_budget": nb,
                      "sample_fraction_of_8_TB_per_s": nb / (med(kern) * 1e-3) / HBM_PEAK}), flush=True)


if __name__ == "__main__":
    main()
