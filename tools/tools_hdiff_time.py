#!/usr/bin/env python3
"""The horizontal diffusion on the C4 grid (1440x720x24): what it costs, and that it costs nothing when it is off.

(a) the step WITHOUT a registration, this tree against a checkout of the parent commit (--parent-root DIR, its library
    built), alternated A/B in one call on one box: every sample is a fresh process that loads one of the two libraries,
    warms up and times --steps steps through gcm_time_steps.  The spread is what the parent's own repeated samples
    show (max - min over their median); the two trees are "the same" when the medians differ by less than that.
(b) the step WITH the phase registered (this tree; order 1 and order 2, fields "uvt"): the added time per step, and one
    application alone (--steps explicit gcm_hdiff_step calls between two synchronisations: the kernel and the copies of
    the landing fields back into the state), against the bytes counted from shapes: the kernel reads each selected
    field once and writes it once (kernel_bytes), the copies read and write each once more (copy_bytes).  The
    registered step also sums the winds' columns again (pe_colsum_kernel reads u and v once: colsum_bytes), because the
    sums the update kernel left belong to the winds before the diffusion.  The kernel alone comes from a kernel trace
    of the `apply` child (see profiles/hdiff/README.md).

One JSON line per sample and one summary line per part.

  python3 tools/tools_hdiff_time.py [--parent-root DIR] [--rounds 4] [--steps 100] [--warmup 10] [--dtype f64]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = "uvt"
NU = {1: 1.0e5, 2: 1.0e15}                               # m^2/s, m^4/s (the kernel has no data-dependent path: the time does not depend on them)


def kernel_bytes(H, W, L, nfields, itemsize=8):
    """bytes one launch must move: every selected field read once and written once"""
    return 2 * H * W * L * nfields * itemsize


def copy_bytes(H, W, L, nfields, itemsize=8):
    """the landing fields' way back into the state: read once, written once"""
    return 2 * H * W * L * nfields * itemsize


def colsum_bytes(H, W, L, itemsize=8):
    """what the next stage's column sums read again: u and v, every level"""
    return 2 * H * W * L * itemsize


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=4, help="samples per tree and mode")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--child", default=None, choices=["plain", "hd1", "hd2", "apply1", "apply2"], help=argparse.SUPPRESS)
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
    order = int(a.child[-1]) if a.child != "plain" else 0
    if a.child.startswith("apply"):
        par = dict(order=order, nu=NU[order], fields=FIELDS)
        core.horizontal_diffusion_step(dt, **par)
        core.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            core.horizontal_diffusion_step(dt, **par)
        core.sync()
        out["ms_per_application"] = (time.perf_counter() - t0) * 1e3 / a.steps
        out["plan"] = core.horizontal_diffusion_plan()
    else:
        if order:
            core.set_horizontal_diffusion(order=order, nu=NU[order], fields=FIELDS)
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
    nf = len(FIELDS)
    kb, cb, sb = kernel_bytes(H, W, L, nf, isz), copy_bytes(H, W, L, nf, isz), colsum_bytes(H, W, L, isz)
    for order in (1, 2):
        hd = [sample(a, ROOT, "hd%d" % order)["ms_per_step"] for _ in range(a.rounds)]
        app = [sample(a, ROOT, "apply%d" % order)["ms_per_application"] for _ in range(max(1, a.rounds // 2))]
        print(json.dumps({"part": "b", "what": "step with the phase registered", "dtype": a.dtype, "order": order,
                          "fields": FIELDS, "nu": NU[order], "hd_ms_per_step": hd, "hd_median": med(hd),
                          "added_ms_per_step": med(hd) - med(new), "application_ms": app, "application_median_ms": med(app),
                          "kernel_bytes": kb, "copy_bytes": cb, "colsum_bytes_per_step": sb,
                          "application_counted_TB_per_s": (kb + cb) / (med(app) * 1e-3) / 1e12}), flush=True)


if __name__ == "__main__":
    main()
