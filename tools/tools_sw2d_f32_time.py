#!/usr/bin/env python3
"""fp32 2-D handles (gcm_config.dtype = GCM_F32 on GCM_SW2D / GCM_SW2D_TEMP) against fp64, one JSON line per case.

  time   ms per step of the fp64 and the fp32 handle of one workload in the same process, alternating the two
         `--rounds` times so that both see the same clock (medians; each round restores the initial state first:
         the noise initial state lives a few hundred steps only).  Workloads: C2 (720x360 SW2D), C3 (4096x2048
         SW2D_TEMP + van Leer) and the 32 x 720x360 SW2D_TEMP + van Leer ensemble of tools_ensemble_time.py.
         TB/s on the counted bytes: 2 x fields x element size per cell-update.
  cols   A/B of the fp32 fused kernel's request width on the same workloads: one column per lane (60-column
         strips, 240-B row segments) against two (120-column strips of 8-byte requests, 480-B segments), both
         handles in one process (GCM_SW2D_F32_COLS at creation), alternated `--rounds` times, medians.
  sweep  error of fp32 and of fp64 against the float64 oracle run on the same (float32-rounded) inputs after
         1, 10 and 100 steps (--sweep-steps), C2 and C3 recipes (bench.synth, SURVEY section 8 inputs):
         rel_err = L-inf over max|oracle| per field.

  python3 tools/tools_sw2d_f32_time.py [--only time|cols|sweep] [--steps 100] [--warmup 10] [--rounds 7]
                                       [--sweep-steps 1 10 100] [--sweep-cases c2 c3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DX, DT = 300e3, 300.0


def workloads():
    import numpy as np
    import bench
    rng = np.random.default_rng(0)
    M, H, W = 32, 360, 720
    ens = {"u": rng.standard_normal((M, H, W)), "v": rng.standard_normal((M, H, W)),
           "p": 101325 + rng.standard_normal((M, H, W)), "t": 273.16 + rng.standard_normal((M, H, W)),
           "q": rng.random((M, H, W))}
    return [("c2", "SW2D", 720, 360, 1, bench.synth("c2", 360, 720)),
            ("c3", "SW2D_TEMP", 4096, 2048, 1, bench.synth("c3", 2048, 4096)),
            ("ens32_720x360", "SW2D_TEMP", W, H, M, ens)]


def make(model, W, H, M, st, dtype, cols=None):
    import gcmiipy_amd as g
    if cols is None:
        os.environ.pop("GCM_SW2D_F32_COLS", None)
    else:
        os.environ["GCM_SW2D_F32_COLS"] = str(cols)          # read when the handle is created
    L = g._lib
    c = g.Core(L.SW2D if model == "SW2D" else L.SW2D_TEMP, W, H, dx=DX, members=M, dtype=dtype,
               tracer=L.TRACER_NONE if model == "SW2D" else L.TRACER_VANLEER)
    c.set_state(**st)
    c.snapshot()
    return c


def timed(c, steps):
    c.restore()
    c.sync()
    t0 = time.perf_counter()
    c.step(steps, DT)
    c.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def run_time(a):
    import numpy as np
    for name, model, W, H, M, st in workloads():
        nf = 3 if model == "SW2D" else 5
        c64, c32 = make(model, W, H, M, st, "f64"), make(model, W, H, M, st, "f32")
        for c in (c64, c32):
            timed(c, a.warmup)
        t64, t32 = [], []
        for _ in range(a.rounds):
            t64.append(timed(c64, a.steps))
            t32.append(timed(c32, a.steps))
        m64, m32 = float(np.median(t64)), float(np.median(t32))
        cells = W * H * M
        print(json.dumps({"case": name, "model": model + ("" if model == "SW2D" else " + van Leer"), "grid": [W, H],
                          "members": M, "steps": a.steps, "rounds": a.rounds,
                          "f64_ms_per_step": round(m64, 5), "f32_ms_per_step": round(m32, 5),
                          "f32_over_f64": round(m32 / m64, 3),
                          "f64_tbps": round(cells * 2 * nf * 8 / (m64 * 1e-3) / 1e12, 3),
                          "f32_tbps": round(cells * 2 * nf * 4 / (m32 * 1e-3) / 1e12, 3),
                          "f64_ms_all": [round(x, 5) for x in t64], "f32_ms_all": [round(x, 5) for x in t32]}),
              flush=True)
        c64.close()
        c32.close()


def run_cols(a):
    import numpy as np
    for name, model, W, H, M, st in workloads():
        nf = 3 if model == "SW2D" else 5
        c1, c2 = make(model, W, H, M, st, "f32", cols=1), make(model, W, H, M, st, "f32", cols=2)
        os.environ.pop("GCM_SW2D_F32_COLS", None)
        for c in (c1, c2):
            timed(c, a.warmup)
        t1, t2 = [], []
        for _ in range(a.rounds):
            t1.append(timed(c1, a.steps))
            t2.append(timed(c2, a.steps))
        m1, m2 = float(np.median(t1)), float(np.median(t2))
        cells = W * H * M
        print(json.dumps({"case": "cols_" + name, "model": model + ("" if model == "SW2D" else " + van Leer"),
                          "grid": [W, H], "members": M, "steps": a.steps, "rounds": a.rounds,
                          "cols1_ms_per_step": round(m1, 5), "cols2_ms_per_step": round(m2, 5),
                          "cols2_over_cols1": round(m2 / m1, 3),
                          "cols1_tbps": round(cells * 2 * nf * 4 / (m1 * 1e-3) / 1e12, 3),
                          "cols2_tbps": round(cells * 2 * nf * 4 / (m2 * 1e-3) / 1e12, 3),
                          "cols1_ms_all": [round(x, 5) for x in t1], "cols2_ms_all": [round(x, 5) for x in t2]}),
              flush=True)
        c1.close()
        c2.close()


def run_sweep(a):
    import numpy as np
    import bench
    import gcmiipy_amd as g
    from oracle import sw2d, sw2d_temp, tracer as otr
    L = g._lib
    for name in a.sweep_cases:
        _, H, W, _, model, _, _, _ = bench.WORKLOADS[name]
        st = {k: v.astype(np.float32).astype(np.float64) for k, v in bench.synth(name, H, W).items()}
        temp = model == "SW2D_TEMP"
        cores = {d: g.Core(L.SW2D_TEMP if temp else L.SW2D, W, H, dx=DX, dtype=d,
                           tracer=L.TRACER_VANLEER if temp else L.TRACER_NONE) for d in ("f64", "f32")}
        for c in cores.values():
            c.set_state(**st)
        ref = (st["u"], st["v"], st["p"]) + ((st["t"],) if temp else ())
        q = st.get("q")
        done = 0
        for n in sorted(a.sweep_steps):
            t0 = time.perf_counter()
            for _ in range(n - done):
                if temp:
                    q = otr.limited_advection(DT, (DX, DX), np.stack([ref[1], ref[0]]), q, limiter=True)
                    ref = sw2d_temp.matsumo_scheme(*ref, DX, DT)
                else:
                    ref = sw2d.matsumo_scheme(*ref, DX, DT)
            oracle_s = time.perf_counter() - t0
            want = dict(zip("uvpt", ref))
            if temp:
                want["q"] = q
            rec = {"case": "sweep", "workload": name, "grid": [W, H], "steps": n, "oracle_s": round(oracle_s, 1)}
            for d, c in cores.items():
                c.step(n - done, DT)
                got = dict(zip("puvtq", c.get_state()))
                rec[d] = {k: float(np.max(np.abs(got[k] - b)) / np.max(np.abs(b))) for k, b in want.items()}
            done = n
            print(json.dumps(rec), flush=True)
        for c in cores.values():
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["time", "cols", "sweep"], default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sweep-steps", nargs="+", type=int, default=[1, 10, 100])
    ap.add_argument("--sweep-cases", nargs="+", default=["c2", "c3"])
    a = ap.parse_args()
    if a.only in (None, "time"):
        run_time(a)
    if a.only in (None, "cols"):
        run_cols(a)
    if a.only in (None, "sweep"):
        run_sweep(a)


if __name__ == "__main__":
    main()
