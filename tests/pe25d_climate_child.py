"""One loopback band of gcm_band_run with the Held-Suarez forcing and the climatology registered (every = 1), in a
process of its own: tests/test_pe25d_climate_gpu.py starts it once per orchestration switch, which the library reads
from the environment when the handle is made.  argv: the file with the single domain's sums, the steps, dt.  Exit status
0: both real types gave the single domain's bits; 1: they did not (the difference is printed).  TEST INFRASTRUCTURE."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]


def main(path, steps, dt):
    import torch
    import gcmiipy_amd as g
    import gpu_setups as su
    import pe25d_inputs as inp
    want = np.load(path)
    H, L, W = want["u_f64"].shape[1], want["u_f64"].shape[0], want["u_f64"].shape[2]
    geom = su.geom_of(H, W, L)
    bad = 0
    for dtype in ("f64", "f32"):
        c, eng, runner = su.loopback_band(g, torch, geom, dtype=dtype, hs={}, every=1)
        assert runner.native
        c.set_state(*inp.state_of(geom, dtype))
        runner.run(steps, dt)
        torch.cuda.synchronize()
        n, m3, m2 = c.climate_sums()
        u = c.get_state()[1]
        c.close()
        same = (n == int(want["n_" + dtype]) and np.array_equal(m3, want["m3_" + dtype]) and
                np.array_equal(m2, want["m2_" + dtype]) and np.array_equal(u, want["u_" + dtype]))
        words = [w for w in range(10) if not np.array_equal(m3[w], want["m3_" + dtype][w])]
        print(dtype, "same" if same else "DIFFERENT: n %d, m3 words %s, m2 %s, u %s" % (
            n, words, np.array_equal(m2, want["m2_" + dtype]), np.array_equal(u, want["u_" + dtype])))
        bad += not same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), float(sys.argv[3])))
