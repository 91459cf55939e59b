#!/usr/bin/env python3
"""The horizontal diffusion on a latitude band: what the phase and the exchange behind it add to the step of one band of
the 8-way split of the C4 grid (1440 x 720 x 24: H = 90), stepped by gcm_band_run on ONE GPU with the loopback exchange
(the band is its own neighbour: device-local copies, no xGMI).  Every exchange figure is therefore EMULATED on one GPU.

(a) the band step WITHOUT a registration and without the opt-in, this tree against a checkout of the parent commit
    (--parent-root DIR, its library built), fresh processes alternated A/B.  "The same" means that the medians differ by
    less than the parent's own spread, max - min over its median.
(b) the band step with order 1 and order 2 registered (fields "uvt") on a band that has opted in, fp64 and fp32, with
    GCM_BAND_EXCHANGE_DELAY_US (the stand-in for a transfer between two devices) 0 and 40: in one child process per
    (dtype, delay) the modes plain / hd1 / hd2 alternate round after round, medians over the rounds.  Figures to record.
(c) the message bytes per step, counted from shapes: a message is gcm_halo_bytes per neighbour, two without the phase,
    three with it.

One JSON line per sample, one per child, and one summary.

  python3 tools/tools_band_hdiff_time.py [--rounds 4] [--steps 100] [--warmup 10] [--dtypes f64,f32] [--delays 0,40]
                                          [--parent-root DIR] [--out FILE]
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
FIELDS = "uvt"
NU = {1: 1.0e5, 2: 1.0e15}                               # m^2/s, m^4/s (the kernel has no data-dependent path)


def child(a):
    """one process: the band under one (dtype, delay); --modes alternated over --rounds"""
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    from gcmiipy_amd.bands import BandRunner, HipBandEngine, LoopbackExchange, split_rows
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    d = np.load(a.state)
    st, dt = [d[k] for k in "puvtq"], float(d["dt"])
    if a.dtype == "f32":
        st = [x.astype(np.float32).astype(np.float64) for x in st]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    row0, n = split_rows(H, NB)[RANK]
    kw = dict(band_horizontal_diffusion=True) if a.opt_in else {}
    c = g.Core(_lib.PE25D, W, n, L, geom=geom, nranks=NB, rank=RANK, global_height=H, row0=row0, dtype=a.dtype,
               stream=torch.cuda.current_stream().cuda_stream, **kw)
    eng = HipBandEngine(c, torch)
    runner = BandRunner(eng, RANK, NB, LoopbackExchange(), north=RANK, south=RANK)
    assert runner.native
    samples, nans = {m: [] for m in a.modes.split(",")}, False
    for rnd in range(a.rounds):
        for mode in samples:
            if a.opt_in:
                c.set_horizontal_diffusion(None)
                if mode != "plain":
                    order = int(mode[-1])
                    c.set_horizontal_diffusion(order=order, nu=NU[order], fields=FIELDS)
            c.set_state(*st)
            runner.run(a.warmup, dt)
            c.set_state(*st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runner.run(a.steps, dt)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            nan = c.diag(_lib.DIAG_ANY_NAN) != 0.0
            nans = nans or nan                                   # (reported: such a timing is not one of the model's step)
            samples[mode].append(ms)
            print(json.dumps(dict(round=rnd, mode=mode, dtype=a.dtype, delay_us=a.delay, ms=ms, nan=nan)), flush=True)
    halo = c.halo_bytes()
    c.close()
    print(json.dumps(dict(child=True, nan=nans, dtype=a.dtype, delay_us=a.delay, opt_in=bool(a.opt_in), root=a.root,
                          halo_bytes=halo, median_ms={m: statistics.median(v) for m, v in samples.items()},
                          spread_ms={m: max(v) - min(v) for m, v in samples.items()})), flush=True)


def run_child(a, root, dtype, delay, modes, opt_in, rounds):
    env = dict(os.environ)
    for k in ("GCM_BAND_COMM_STREAM", "GCM_PE_SINGLE_STREAM", "GCM_BAND_HOST_LOOP", "GCM_BAND_OVERLAP", "GCMCORE_LIB"):
        env.pop(k, None)
    env["GCM_BAND_EXCHANGE_DELAY_US"] = str(delay)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--dtype", dtype, "--delay", str(delay),
           "--modes", modes, "--opt-in", str(int(opt_in)), "--rounds", str(rounds), "--steps", str(a.steps),
           "--warmup", str(a.warmup), "--state", a.state]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("the child process of (%s, %s, %s) failed: %d" % (root, dtype, delay, r.returncode))
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
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
    ap.add_argument("--modes", default="plain,hd1,hd2")
    ap.add_argument("--opt-in", type=int, default=1)
    ap.add_argument("--state", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from gcmiipy_amd import geometry
    from gcmiipy_amd.bands import split_rows
    dt = bench.WORKLOADS["c4"][-1]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig)
    st = bench.synth("c4", H, W, L, geom=geom)
    row0, n = split_rows(H, NB)[RANK]
    sl = slice(row0, row0 + n)
    tmp = tempfile.mkdtemp()
    a.state = os.path.join(tmp, "band_state.npz")
    np.savez(a.state, dt=dt, **{k: np.ascontiguousarray(st[k][..., sl, :]) for k in "puvtq"})
    t0 = time.time()
    children, unchanged = [], []
    for dtype in a.dtypes.split(","):
        for delay in (float(x) for x in a.delays.split(",")):
            children.append(run_child(a, ROOT, dtype, delay, "plain,hd1,hd2", True, a.rounds))
        if a.parent_root:
            # (a): a band that has not opted in, by this library and by the parent's, one process each, alternated
            for rnd in range(a.rounds):
                for who, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                    r = run_child(a, root, dtype, 0.0, "plain", False, 1)
                    unchanged.append(dict(round=rnd, who=who, dtype=dtype, ms=r["median_ms"]["plain"]))
    os.remove(a.state)
    os.rmdir(tmp)
    summary = dict(summary=True, grid=[H, W, L], split=NB, band_rows=n, steps=a.steps, rounds=a.rounds, dt=dt, fields=FIELDS,
                   note="one band of the 8-way split on ONE GPU, loopback exchange: emulated, no xGMI",
                   children=children, seconds=time.time() - t0)
    # (c) from shapes, the formula of gcm_halo_bytes: two rows of p and of the L levels of u, v, theta, q in the handle's
    # type, and two rows of the float64 ground temperature (the children report gcm_halo_bytes itself: halo_bytes)
    summary["message_bytes"] = {
        dtype: dict(per_message=(8 if dtype == "f64" else 4) * 2 * W * (1 + 4 * L) + 8 * 2 * W,
                    messages_per_neighbour_and_step=dict(plain=2, hd=3))
        for dtype in a.dtypes.split(",")}
    if unchanged:
        part_a = {}
        for dtype in a.dtypes.split(","):
            v = {who: [u["ms"] for u in unchanged if u["who"] == who and u["dtype"] == dtype] for who in ("this", "parent")}
            med = {who: statistics.median(x) for who, x in v.items()}
            spread = (max(v["parent"]) - min(v["parent"])) / med["parent"]
            diff = (med["this"] - med["parent"]) / med["parent"]
            part_a[dtype] = dict(this_ms=v["this"], parent_ms=v["parent"], this_median=med["this"], parent_median=med["parent"],
                                 parent_spread_rel=spread, median_difference_rel=diff, same_within_spread=abs(diff) < spread)
        summary["part_a_no_opt_in"] = part_a
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
