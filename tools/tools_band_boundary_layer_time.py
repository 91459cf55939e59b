#!/usr/bin/env python3
"""The boundary layer on a latitude band: what the phase and its third exchange add to the step of one band of the 8-way
split of the C4 grid (1440 x 720 x 24: H = 90), stepped by gcm_band_run on ONE GPU with the loopback exchange (the band is
its own neighbour: device-local copies, no xGMI).  Every figure for N > 1 is therefore EMULATED on one GPU.

Held-Suarez, the convective adjustment and the moist physics are registered in every mode; the state is the tests' windy
humid state over a ground with warmer and colder cells (tests/pe25d_boundary_layer_ref.py), the band's rows of it.

  plain     the band has opted in, the boundary layer is not registered: two exchanges per step
  boundary  with set_boundary_layer(): the phase over the own rows and the third exchange

GCM_BAND_EXCHANGE_DELAY_US (the stand-in for a transfer between two devices) is read once per process and the
orchestration when the exchange is registered, so every (dtype, delay, orchestration) is a child process of its own; in
it the two modes alternate round after round (the state is set again before every sample), medians over the rounds.
How much of the delay shows in the step -- step(delay) - step(0), per exchange -- says whether the third exchange hides
behind the own rows' convective adjustment and moist physics.

  --parent-root DIR   a checkout of the parent commit with its library built: a band WITHOUT the opt-in by this library
                      and by the parent's, child processes alternated, for "nothing changed for those who do not opt in"

One JSON line per sample, one per child, and one summary.

  python3 tools/tools_band_boundary_layer_time.py [--rounds 5] [--steps 100] [--warmup 10] [--dtypes f64,f32]
                                                   [--delays 0,40] [--parent-root DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, L, NB, RANK = 720, 1440, 24, 8, 4
DT = 60.0
ORCH = {"default": {}, "comm_stream": {"GCM_BAND_COMM_STREAM": "1"}}


def child(a):
    """one process: the band under one (dtype, delay, orchestration); --modes alternated over --rounds"""
    sys.path[:0] = [a.root, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange, split_rows
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    d = np.load(a.state)
    st, gt = [d[k] for k in "puvtq"], d["gt"]
    if a.dtype == "f32":
        st = [x.astype(np.float32).astype(np.float64) for x in st]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    row0, n = split_rows(H, NB)[RANK]
    kw = dict(band_boundary_layer=True) if a.opt_in else {}
    c = g.Core(_lib.PE25D, W, n, L, geom=geom, nranks=NB, rank=RANK, global_height=H, row0=row0, dtype=a.dtype,
               stream=torch.cuda.current_stream().cuda_stream, **kw)
    eng = HipBandEngine(c, torch)
    c.set_ground(gt)
    eng.set_held_suarez(geom)
    eng.set_convect(gamma=6.5e-3)
    eng.set_moist(tau_e=0.0)
    runner = BandRunner(eng, RANK, NB, LoopbackExchange(), north=RANK, south=RANK)
    assert runner.native
    samples, nans = {m: [] for m in a.modes.split(",")}, False
    for rnd in range(a.rounds):
        for mode in samples:
            if a.opt_in:
                c.set_boundary_layer(None)
                if mode == "boundary":
                    c.set_boundary_layer()
            c.set_state(*st)
            runner.run(a.warmup, DT)
            c.set_state(*st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runner.run(a.steps, DT)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            nan = c.diag(_lib.DIAG_ANY_NAN) != 0.0
            nans = nans or nan                                   # (reported: such a timing is not one of the model's step)
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, delay_us=a.delay, orch=a.orch, ms=ms, nan=nan)), flush=True)
    c.close()
    print(json.dumps(dict(child=True, nan=nans, dtype=a.dtype, delay_us=a.delay, orch=a.orch, opt_in=bool(a.opt_in), root=a.root,
                          median_ms={m: statistics.median(v) for m, v in samples.items()},
                          spread_ms={m: max(v) - min(v) for m, v in samples.items()})), flush=True)


def run_child(a, root, dtype, delay, orch, modes, opt_in, rounds):
    env = dict(os.environ)
    for k in ("GCM_BAND_COMM_STREAM", "GCM_PE_SINGLE_STREAM", "GCM_BAND_HOST_LOOP", "GCM_BAND_OVERLAP", "GCMCORE_LIB"):
        env.pop(k, None)
    env.update(ORCH[orch])
    env["GCM_BAND_EXCHANGE_DELAY_US"] = str(delay)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--dtype", dtype, "--delay", str(delay),
           "--orch", orch, "--modes", modes, "--opt-in", str(int(opt_in)), "--rounds", str(rounds), "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--state", a.state]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("the child process of (%s, %s, %s) failed: %d" % (dtype, delay, orch, r.returncode))
    out = r.stdout
    sys.stdout.write(out)
    sys.stdout.flush()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--delays", default="0,40")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--delay", type=float, default=0.0)
    ap.add_argument("--orch", default="default", choices=list(ORCH))
    ap.add_argument("--modes", default="plain,boundary")
    ap.add_argument("--opt-in", type=int, default=1)
    ap.add_argument("--state", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    from gcmiipy_amd import geometry
    from gcmiipy_amd.bands import split_rows
    import pe25d_boundary_layer_ref as ref
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = ref.windy_state(geom)
    gt = ref.ground(geom, st)
    row0, n = split_rows(H, NB)[RANK]
    sl = slice(row0, row0 + n)
    tmp = tempfile.mkdtemp()
    a.state = os.path.join(tmp, "band_state.npz")
    np.savez(a.state, gt=gt[sl], **{k: np.ascontiguousarray(x[..., sl, :]) for k, x in zip("puvtq", st)})
    t0 = time.time()
    children, unchanged = [], []
    for dtype in a.dtypes.split(","):
        for orch in ORCH:
            for delay in (float(x) for x in a.delays.split(",")):
                children.append(run_child(a, ROOT, dtype, delay, orch, "plain,boundary", True, a.rounds))
        if a.parent_root:
            # a band that has not opted in, by this library and by the parent's, one process each, alternated
            for rnd in range(a.rounds):
                for who, root in (("this", ROOT), ("parent", a.parent_root)):
                    r = run_child(a, root, dtype, 0.0, "default", "plain", False, 1)
                    unchanged.append(dict(round=rnd, who=who, dtype=dtype, ms=r["median_ms"]["plain"]))
    os.remove(a.state)
    os.rmdir(tmp)
    summary = dict(summary=True, grid=[H, W, L], split=NB, band_rows=n, steps=a.steps, rounds=a.rounds, dt=DT,
                   note="one band of the 8-way split on ONE GPU, loopback exchange: emulated, no xGMI",
                   children=children, seconds=time.time() - t0)
    if unchanged:
        summary["no_opt_in_ms"] = {
            dtype: {who: dict(median=statistics.median(v), min=min(v), max=max(v))
                    for who in ("this", "parent")
                    for v in [[u["ms"] for u in unchanged if u["who"] == who and u["dtype"] == dtype]]}
            for dtype in a.dtypes.split(",")}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
