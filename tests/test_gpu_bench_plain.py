"""A plain `bench.py` run (no --full) on the GPU: the result line carries the headline figures only, and --dump-outputs
writes the factors the timed loop computed -- from the seeded start, settle + warm-up + timed steps -- the same in every
run and equal to the float64 oracle's after as many iterations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from conftest import ROOT, rel_fro

pytestmark = pytest.mark.gpu


def _plain_run(out_dir, m, steps, warmup, settle):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--rows", str(m), "--preroll-ms", "20", "--settle-iters", str(settle), "--dump-outputs", out_dir]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [json.loads(l) for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()
    return lines[0]


def test_plain_bench_line_and_its_dumped_factors(tmp_path):
    m, n, k, steps, warmup, settle = 4096, 256, 64, 6, 2, 10
    runs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in runs:
        j = _plain_run(d, m, steps, warmup, settle)
        assert j["full"] is False and j["steps"] == steps and j["warmup"] == warmup and j["n_gpus"] == 1
        assert j["settle_iters"] == settle and j["preroll_iters"] > 0
        assert j["metric"] == "factorize_iters_per_sec" and j["unit"] == "iter/s" and j["higher_is_better"] is True
        assert abs(j["ms_per_step"] * j["value"] - 1e3) < 1e-6 * 1e3
        assert j["cold_iters_per_sec"] is None and "cpu_baseline" not in j and "parity_full_size" not in j
        assert j["config"]["class_factorize"] is None and j["config"]["compute_err_true_iters_per_sec"] is None
    Wa, Ha = np.load(os.path.join(runs[0], "W.npy")), np.load(os.path.join(runs[0], "H.npy"))
    assert Wa.dtype == np.float32 and Wa.shape == (m, k) and Ha.dtype == np.float64 and Ha.shape == (k, n)
    np.testing.assert_array_equal(Wa, np.load(os.path.join(runs[1], "W.npy")))
    np.testing.assert_array_equal(Ha, np.load(os.path.join(runs[1], "H.npy")))
    # the oracle from bench.py's seeded start (float32 V and W0 rows, float64 H0), settle + warm-up + timed iterations
    V = bench.gen_rows(np.random.RandomState(1234), m, n, 0, m)
    np.random.seed(42)
    W = bench.gen_rows(np.random.mtrand._rand, m, k, 0, m).astype(np.float64)
    H = np.random.random((k, n))
    for _ in range(settle + warmup + steps):
        oracle.nmf_update_w(V, W, H)
        oracle.nmf_update_h(V, W, H)
    assert rel_fro(Wa, W, what="dumped W") < 2e-5
    assert rel_fro(Ha, H, what="dumped H") < 2e-5
