#!/usr/bin/env python3
"""The wave pair of GCM_SW2D_TEMP (two steps per launch, sw2d_pair_kernel) against single deep steps on C3 (4096x2048,
van Leer, float64) IN ONE PROCESS: one handle per setting, all created up front (GCM_SW2D_PAIR and GCM_SW2D_PAIR_ROWS
are read when a handle is created), stepped in turn `--rounds` times so that every setting sees the same clock; host
clock around `--steps` steps and one synchronisation, medians of ms per step, one JSON line.

  off      GCM_SW2D_PAIR=0: one deep single-step launch per step
  pair     GCM_SW2D_PAIR=1 at the library's own band length (one resident round of workgroups)
  pairN    GCM_SW2D_PAIR=1 at GCM_SW2D_PAIR_ROWS = ceil(H / N) for every N of --bands (bands per strip)

  python3 tools/tools_sw2d_pair_time.py [--steps 200] [--warmup 20] [--rounds 5] [--bands 12 14]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DX, DT = 300e3, 300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bands", nargs="*", type=int, default=[12, 14])
    a = ap.parse_args()
    import numpy as np
    import bench
    import gcmiipy_amd as g
    _, H, W, _, _, _, _, _ = bench.WORKLOADS["c3"]
    st = bench.synth("c3", H, W)
    settings = [("off", "0", None), ("pair", "1", None)] + [("pair%d" % n, "1", -(-H // n)) for n in a.bands]
    cores, info = {}, {}
    for name, pair, rows in settings:
        os.environ["GCM_SW2D_PAIR"] = pair
        os.environ.pop("GCM_SW2D_PAIR_ROWS", None)
        if rows is not None:
            os.environ["GCM_SW2D_PAIR_ROWS"] = str(rows)
        c = g.Core(g._lib.SW2D_TEMP, W, H, dx=DX, tracer=g._lib.TRACER_VANLEER)
        c.set_state(**st)
        c.snapshot()
        cores[name], info[name] = c, dict(c.sw2d_pair(), plan=c.sw2d_plan(a.steps))
    os.environ.pop("GCM_SW2D_PAIR", None)
    os.environ.pop("GCM_SW2D_PAIR_ROWS", None)

    def timed(c, n):
        c.restore()                       # the noise initial state lives for some hundred steps only (bench.py)
        c.sync()
        t0 = time.perf_counter()
        c.step(n, DT)
        c.sync()
        return (time.perf_counter() - t0) * 1e3 / n

    for c in cores.values():
        timed(c, a.warmup)
    ms = {name: [] for name in cores}
    for _ in range(a.rounds):
        for name, c in cores.items():
            ms[name].append(timed(c, a.steps))
    out = {"case": "sw2d_pair", "grid": [W, H], "steps": a.steps, "rounds": a.rounds}
    for name in cores:
        out[name] = {"ms_per_step": round(float(np.median(ms[name])), 4), "all": [round(x, 4) for x in ms[name]],
                     "pair_rows": info[name]["rows_per_band"], "active": info[name]["active"],
                     "two_step_launches": info[name]["plan"]["two_step_launches"]}
    for name in cores:
        if name != "off":
            out[name]["over_off"] = round(out[name]["ms_per_step"] / out["off"]["ms_per_step"], 4)
    print(json.dumps(out), flush=True)
    for c in cores.values():
        c.close()


if __name__ == "__main__":
    main()
