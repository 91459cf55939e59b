"""bench.py --dump-outputs: what the last timed step computed, against a fresh handle stepped from the same seeded
inputs as many times as the bench stepped them before the dump (2-D: W + K after the restore that follows the settle
phase, whose length depends on the box's speed; GCM_PE25D: settle_steps + W + K).  Equal to rounding only if the timed
region is exactly K steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh_run(bench, name, nsteps):
    """the workload's handle built and stepped directly, one domain -> name -> global field"""
    import gcmiipy_amd as g
    from gcmiipy_amd import _lib, geometry
    _, H, W, L, model, tracer, _, dt = bench.WORKLOADS[name]
    geom = geometry.gen_geometry(H, W, L, sig_func=geometry.manabe_sig) if model == "PE25D" else None
    core = g.Core(getattr(_lib, model), W, H, L, dx=bench.DX, geom=geom, variant=_lib.VARIANT_FUSED,
                  tracer={None: _lib.TRACER_NONE, "van_leer": _lib.TRACER_VANLEER}[tracer])
    core.set_state(**bench.synth(name, H, W, L, geom=geom))
    if "phys" in name:
        core.set_ground(np.full((H, W), 288.0))
        core.set_physics(geom, bench.PHYS_UTC0)
    core.step(nsteps, dt)
    out = {f: a for f, a in zip("puvtq", core.get_state()) if a is not None}
    if "phys" in name:
        out["gt"] = core.get_ground()
    core.close()
    return out


def _assert_same(bench, got_dir, want, tmp_path):
    ref = str(tmp_path / "fresh")
    bench.write_outputs(ref, want, np.float64)
    assert sorted(os.listdir(got_dir)) == sorted(os.listdir(ref)) == sorted(f + ".npy" for f in want)
    assert sum(os.path.getsize(os.path.join(got_dir, f)) for f in os.listdir(got_dir)) <= bench.DUMP_BYTES
    for f in want:
        a, b = np.load(os.path.join(got_dir, f + ".npy")), np.load(os.path.join(ref, f + ".npy"))
        assert a.dtype == np.float64 and a.shape == b.shape, f
        assert rel_err(a, b) < 1e-12, (f, rel_err(a, b))


@pytest.mark.parametrize("name", ["c4", "c5_phys"])
def test_run_workload_dumps_the_last_timed_step(monkeypatch, tmp_path, name):
    """PE25D: c4 at its size (sampled: 0.8 GB of state), the physics workload on a small grid"""
    import torch
    import bench
    monkeypatch.setattr(bench, "SETTLE_S", 0.05)
    if name == "c5_phys":
        monkeypatch.setitem(bench.WORKLOADS, name, bench.WORKLOADS[name][:1] + (48, 96, 8) + bench.WORKLOADS[name][4:])
    cx = bench.Ctx()
    cx.torch, cx.dist = torch, None
    cx.rank, cx.world, cx.local, cx.backend = 0, 1, 0, "nccl"
    cx.ring, cx.exchange, cx.stuck, cx.exchange_fallback = None, None, False, None
    torch.cuda.set_device(0)
    res = bench.run_workload(cx, name, 5, 2, want_kernel=False, dump=str(tmp_path / "dump"))
    assert res["steps"] == 5 and res["settle_steps"] == 2 + bench.SETTLE_STEPS_PE
    _assert_same(bench, str(tmp_path / "dump"), _fresh_run(bench, name, res["settle_steps"] + 2 + 5), tmp_path)


def _bench(args, out, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--only", "--no-cpu", "--dump-outputs", out]
                       + args, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_cli_dumps_the_last_timed_step(tmp_path):
    """the command line on one GPU: c2 (whole fields, 6 MB), an odd step count for the two-steps-per-launch kernel"""
    import bench
    d = _bench(["--workload", "c2", "--steps", "7", "--warmup", "3"], str(tmp_path / "dump"))
    assert d["steps"] == 7 and d["warmup"] == 3 and d["n_gpus"] == 1
    _assert_same(bench, str(tmp_path / "dump"), _fresh_run(bench, "c2", 3 + 7), tmp_path)
    assert np.load(str(tmp_path / "dump" / "p.npy")).shape == (360, 720)


def test_bench_two_ranks_dump_the_whole_grid(tmp_path):
    """--gpus 2 (gloo rehearsal on one GPU): the two latitude bands gathered on rank 0 are the single-domain state"""
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GCM_BENCH_BACKEND="gloo", GCM_BENCH_SETTLE_S="0.01")
    d = _bench(["--gpus", "2", "--steps", "8", "--warmup", "4"], str(tmp_path / "dump"), env)
    assert d["n_gpus"] == 2 and d["steps"] == 8
    _assert_same(bench, str(tmp_path / "dump"), _fresh_run(bench, "c3", 4 + 8), tmp_path)
