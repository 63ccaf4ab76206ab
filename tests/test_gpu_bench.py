"""bench.py's plain run (pytest -m gpu): the headline figure alone, and the outputs of its last timed step
(--dump-outputs) against the CPU oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_dumps_its_last_step(tmp_path):
    import bench
    from oracle import gp_oracle as O
    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["unit"] == "updates/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    for key in ("strong_scaling", "roofline", "update_latency", "next_rows", "batched_updates", "config4", "cpu_baseline"):
        assert out[key] is None, key                                  # measured with --full only

    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {"logpdf", "acq", "acq_argmax", "acq_max", "factor_z", "factor_L_sample"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the last timed step is step steps-1: its noise level, on the seeded inputs of rank 0
    X, y, Xs = bench.problem(1)
    lam = np.full(bench.D, 0.5)
    post = O.gp_fit(X, y, bench.KERNEL, lam, 1.0, 0.05 + 1e-4 * ((steps - 1) % 7))
    assert abs(got["logpdf"][0] - post.logpdf) <= 1e-9 * (1 + abs(post.logpdf))
    rows, cols = bench.factor_sample_index(bench.N_OBS)
    assert np.allclose(got["factor_L_sample"], post.L[rows, cols], rtol=0, atol=1e-9 * np.abs(post.L).max())
    z_o = O.sla.solve_triangular(post.L, post.delta, lower=True)
    assert np.allclose(got["factor_z"], z_o, rtol=0, atol=1e-9 * (1 + np.abs(z_o).max()))
    acq = got["acq"]
    assert acq.shape == (bench.M_CAND,)
    sl = slice(1000, 1512)
    assert np.allclose(acq[sl], O.ei_acquisition([post], Xs[:, sl], [1.0], None, float(y.max())), rtol=0, atol=1e-10)
    am = int(got["acq_argmax"][0])
    assert am == int(np.argmax(acq)) and got["acq_max"][0] == acq[am]
