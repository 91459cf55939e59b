#!/usr/bin/env python3
"""The passive tracers' device monitor (gcm_tracer_stats) on the C4 grid, 1440 x 720 x 24 with 4 tracers, fp64 and
fp32: one JSON line per real type with

  stats_ms        Core.tracer_stats(), end to end (the join, two launches, 48 bytes a tracer back, one synchronisation):
                  median of --rounds calls after a warm-up
  host_ms         what the call replaces: get_tracers() (a transpose on the device, n L H W float64 over PCIe) and the
                  same reductions in NumPy on the host (min, max, sum c p dsig, the two counts)
  stage_ms        one tracer stage of the step, as context: (a step with the tracers - a step without) / 2, from
                  --steps steps each, host clock around the steps and one synchronisation
  bytes           n L H W esz + n H W esz: each tracer byte once, p once per field
  copy_rate_frac  (bytes / the read-only rate of tools/micro/copy_width.hip, --rate, 5.9 TB/s in round 3) / stats_ms:
                  1.0 = the call takes what reading its bytes takes; the call also pays a launch boundary, the fold, the
                  copy back and the synchronisation, which at this size are of the same order as the kernel itself

  python3 tools/tools_tracer_stats_time.py [--grid 1440 720 24] [--tracers 4] [--rounds 15] [--steps 10] [--rate 5.9e12]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 1.0


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", nargs=3, type=int, default=[1440, 720, 24], metavar=("W", "H", "L"))
    ap.add_argument("--tracers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rate", type=float, default=5.9e12, help="read-only bytes per second (tools/micro/copy_width.hip)")
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"], choices=["f64", "f32"])
    return ap


def stats_bytes(W, H, L, n, esz):
    """what pe_tracer_stats_kernel reads: every tracer once, p once per field"""
    return n * L * H * W * esz + n * H * W * esz


def host_stats(c, dsig):
    import numpy as np
    tr = c.get_tracers()
    p = c.get_state(fields=(0,))[0]
    w = p[None] * dsig
    return [(x.min(), x.max(), float(np.sum(x * w)), float(np.sum(w)), int(np.sum(x < 0)), int(np.sum(np.isnan(x))))
            for x in tr]


def median_ms(fn, rounds):
    import numpy as np
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def steps_ms(c, steps):
    c.sync()
    t0 = time.perf_counter()
    c.step(steps, DT)
    c.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    import numpy as np
    import gcmiipy_amd as g
    from gcmiipy_amd import geometry
    a = parser().parse_args()
    W, H, L = a.grid
    n = a.tracers
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    dsig = np.asarray(geom.dsig, dtype=np.float64).reshape(L, 1, 1)
    rng = np.random.default_rng(0)
    p = 1e5 + 10 * rng.standard_normal((H, W))
    u, v = rng.standard_normal((L, H, W)), rng.standard_normal((L, H, W))
    v[:, -1, :] = 0
    t = (300 + rng.standard_normal((L, H, W))) * ((1e5 / (p * geom.sig + geom.ptop)) ** (287.0 / 1004.0))
    q = 3e-6 * (1 + 0.1 * rng.random((L, H, W)))
    trs = 1.0 + rng.random((n, L, H, W))
    for dtype in a.dtypes:
        esz = 8 if dtype == "f64" else 4
        c = g.Core(g._lib.PE25D, W, H, L, geom=geom, dtype=dtype)
        c.set_state(p, u, v, t, q)
        steps_ms(c, 2)
        bare = min(steps_ms(c, a.steps) for _ in range(3))
        c.set_state(p, u, v, t, q)
        c.set_tracers(trs)
        steps_ms(c, 2)
        with_tr = min(steps_ms(c, a.steps) for _ in range(3))
        c.set_state(p, u, v, t, q)
        c.set_tracers(trs)
        for _ in range(3):
            s = c.tracer_stats()
        stats_ms = median_ms(c.tracer_stats, a.rounds)
        host_stats(c, dsig)
        host_ms = median_ms(lambda: host_stats(c, dsig), max(3, a.rounds // 5))
        nbytes = stats_bytes(W, H, L, n, esz)
        print(json.dumps({"case": "tracer_stats", "grid": [W, H, L], "dtype": dtype, "tracers": n,
                          "stats_ms": round(stats_ms, 4), "host_ms": round(host_ms, 2),
                          "host_over_stats": round(host_ms / stats_ms, 1),
                          "stage_ms": round((with_tr - bare) / 2, 4), "step_ms": round(with_tr, 4),
                          "step_without_tracers_ms": round(bare, 4), "bytes": nbytes, "rate_bps": a.rate,
                          "bytes_at_rate_ms": round(nbytes / a.rate * 1e3, 4),
                          "copy_rate_frac": round(nbytes / a.rate * 1e3 / stats_ms, 3),
                          "mass": [float(x) for x in s.mass], "negative": [int(x) for x in s.negative]}), flush=True)
        c.close()


if __name__ == "__main__":
    main()
