#!/usr/bin/env python3
"""Ensembles of the 2-D models (gcm_config.members): time per member-step of one M-member handle against M
separate one-member handles stepped in turn, and against the HBM roofline, one JSON line per case.

  sweep  SW2D (48 B per cell-update) and SW2D_TEMP + van Leer (80 B) at 360x180 and
         720x360, M = 1, 2, 4, ..., 64.  Both sides are timed the same way: a host clock around the steps and
         one synchronisation, after a warm-up of every handle.  The separate handles each take all their steps
         in one call, one handle after the other, on the same stream: the fewest host calls they can need.
  ab     32 x 720x360 SW2D_TEMP + van Leer against C3 (4096x2048, same model) in the same process, alternating
         A and B `--rounds` times so that both see the same clock; medians of ms per step.

  rows   the rows-per-band choice checked: the ensemble alone at each GCM_FUSED_ROWS in --rows and at the
         library's own choice ("auto"), M >= 8 of --members.

roofline_frac = (member cells x bytes per cell-update / 8.0 TB/s) / measured time per step.

  python3 tools/tools_ensemble_time.py [--steps 100] [--warmup 10] [--members 1 2 4 8 16 32 64] [--rounds 7]
                                      [--only sweep|ab|rows] [--rows 4 8 16 24 32 48 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8.0e12
DX, DT = 300e3, 300.0


def state(model, M, H, W, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    s = {"u": rng.standard_normal((M, H, W)), "v": rng.standard_normal((M, H, W))}
    if model == "SW2D":
        s["p"] = 8000 + rng.standard_normal((M, H, W))
    else:
        s["p"] = 101325 + rng.standard_normal((M, H, W))
        s["t"] = 273.16 + rng.standard_normal((M, H, W))
        s["q"] = rng.random((M, H, W))
    return {k: (a[0] if M == 1 else a) for k, a in s.items()}


def make(model, W, H, M, st):
    import gcmiipy_amd as g
    L = g._lib
    c = g.Core(L.SW2D if model == "SW2D" else L.SW2D_TEMP, W, H, dx=DX, members=M,
               tracer=L.TRACER_NONE if model == "SW2D" else L.TRACER_VANLEER)
    c.set_state(**st)
    return c


def timed(cores, steps):
    """ms for `steps` steps of every core in turn, host clock, ended by one synchronisation"""
    cores[-1].sync()
    t0 = time.perf_counter()
    for c in cores:
        c.step(steps, DT)
    for c in cores:
        c.sync()
    return (time.perf_counter() - t0) * 1e3


def sweep(a):
    for model, bpc in (("SW2D", 48.0), ("SW2D_TEMP_VANLEER", 80.0)):
        for W, H in ((360, 180), (720, 360)):
            for M in a.members:
                st = state("SW2D" if model == "SW2D" else "TEMP", M, H, W)
                ens = make(model, W, H, M, st)
                sep = [make(model, W, H, 1, {k: (x[m] if M > 1 else x) for k, x in st.items()}) for m in range(M)]
                timed([ens], a.warmup)
                timed(sep, a.warmup)
                ms_e = min(timed([ens], a.steps) for _ in range(3))
                ms_s = min(timed(sep, a.steps) for _ in range(3))
                floor_ms = W * H * bpc / PEAK_BPS * 1e3
                per_e, per_s = ms_e / (a.steps * M), ms_s / (a.steps * M)
                print(json.dumps({"case": "sweep", "model": model, "grid": [W, H], "members": M, "steps": a.steps,
                                  "us_per_member_step": round(per_e * 1e3, 4),
                                  "separate_us_per_member_step": round(per_s * 1e3, 4),
                                  "speedup_vs_separate": round(per_s / per_e, 3),
                                  "roofline_frac": round(floor_ms / per_e, 3),
                                  "separate_roofline_frac": round(floor_ms / per_s, 3)}), flush=True)
                ens.close()
                for c in sep:
                    c.close()


def ab(a):
    import numpy as np
    import bench
    _, H3, W3, _, _, _, bpc, _ = bench.WORKLOADS["c3"]
    c3 = make("TEMP", W3, H3, 1, bench.synth("c3", H3, W3))
    ens = make("TEMP", 720, 360, 32, state("TEMP", 32, 360, 720))
    timed([c3], a.warmup)
    timed([ens], a.warmup)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed([ens], a.steps) / a.steps)
        tb.append(timed([c3], a.steps) / a.steps)
    ma, mb = float(np.median(ta)), float(np.median(tb))
    cells_a, cells_b = 32 * 720 * 360, W3 * H3
    print(json.dumps({"case": "ab", "a": "32 x 720x360 SW2D_TEMP + van Leer", "b": "C3 4096x2048 SW2D_TEMP + van Leer",
                      "steps": a.steps, "rounds": a.rounds, "a_ms_per_step": round(ma, 4), "b_ms_per_step": round(mb, 4),
                      "a_over_b": round(ma / mb, 3), "a_cells": cells_a, "b_cells": cells_b,
                      "a_ns_per_cell": round(ma * 1e6 / cells_a, 4), "b_ns_per_cell": round(mb * 1e6 / cells_b, 4),
                      "a_roofline_frac": round(cells_a * bpc / PEAK_BPS * 1e3 / ma, 3),
                      "b_roofline_frac": round(cells_b * bpc / PEAK_BPS * 1e3 / mb, 3),
                      "a_ms_all": [round(x, 4) for x in ta], "b_ms_all": [round(x, 4) for x in tb]}), flush=True)
    ens.close()
    c3.close()


def rows(a):
    for model, bpc in (("SW2D", 48.0), ("SW2D_TEMP_VANLEER", 80.0)):
        for W, H in ((360, 180), (720, 360)):
            for M in [m for m in a.members if m >= 8]:
                st = state("SW2D" if model == "SW2D" else "TEMP", M, H, W)
                res = {}
                for r in [None] + a.rows:
                    if r is None:
                        os.environ.pop("GCM_FUSED_ROWS", None)
                    else:
                        os.environ["GCM_FUSED_ROWS"] = str(r)     # read when the handle is created
                    ens = make(model, W, H, M, st)
                    timed([ens], a.warmup)
                    res["auto" if r is None else r] = min(timed([ens], a.steps) for _ in range(3)) / (a.steps * M)
                    ens.close()
                os.environ.pop("GCM_FUSED_ROWS", None)
                best = min((k for k in res if k != "auto"), key=lambda k: res[k])
                print(json.dumps({"case": "rows", "model": model, "grid": [W, H], "members": M, "steps": a.steps,
                                  "us_per_member_step": {str(k): round(v * 1e3, 4) for k, v in res.items()},
                                  "best_rows": best, "auto_over_best": round(res["auto"] / res[best], 3),
                                  "auto_roofline_frac": round(W * H * bpc / PEAK_BPS / res["auto"] * 1e3, 3)}),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--members", nargs="+", type=int, default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["sweep", "ab", "rows"], default=None)
    ap.add_argument("--rows", nargs="+", type=int, default=[4, 8, 16, 24, 32, 48, 64])
    a = ap.parse_args()
    if a.only in (None, "sweep"):
        sweep(a)
    if a.only in (None, "ab"):
        ab(a)
    if a.only == "rows":
        rows(a)


if __name__ == "__main__":
    main()
