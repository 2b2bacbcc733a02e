"""bench.py's command line: what a plain run prints and --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_output_is_float32_and_a_fixed_sample_above_the_cap(tmp_path):
    """A buffer within DUMP_MAX_VALUES is written whole (complex as (re, im) pairs); a
    larger one as DUMP_MAX_VALUES values at ascending positions that do not change from
    call to call."""
    import bench

    z = torch.arange(12, dtype=torch.float32).reshape(2, 3, 2)
    bench.dump_output(torch.view_as_complex(z.clone()), str(tmp_path), "z")
    got = np.load(tmp_path / "z.npy")
    assert got.dtype == np.float32 and np.array_equal(got, z.numpy())

    n = bench.DUMP_MAX_VALUES + 4096  # below 2^24: every index is exact in float32
    big = torch.arange(n, dtype=torch.float32).reshape(2, n // 2)
    bench.dump_output(big, str(tmp_path), "a")
    bench.dump_output(big, str(tmp_path), "b")
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_VALUES,) and a.nbytes <= 64_000_000
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n and len(np.unique(a)) > n // 2


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(gpu_lib, tmp_path):
    """One plain run (C2 at 2^16 samples, 1 warm-up + 3 timed steps): the line carries the
    headline fields and none of the --full figures, and DIR/out.npy is bit for bit what a
    fresh chain returns from its fourth call over the same seeded input."""
    import bench

    n, warmup, steps = 1 << 16, 1, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--samples", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["warmup"] == warmup
    ms = line["ms_per_step"]  # printed to 1e-4 ms: that rounding bounds the agreement with `value`
    assert ms > 0 and line["value"] == pytest.approx(n / ms / 1e3, rel=1e-3 + 5e-5 / ms)
    assert line["cpu_baseline"] is None and "host_fed" not in line and "per_launch_ms" not in line["roofline"]
    assert os.listdir(tmp_path) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")

    dev = torch.device("cuda", 0)
    x = bench.wbfm_iq(n, bench.OFFSETS[0], dev, 0x1234)
    chain = gpu_lib.WbfmChain(f_off=bench.OFFSETS[0])
    for _ in range(warmup + steps):
        ref = chain.process_device(x).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref)
