"""bench.py's command line: a plain run (`--gpus 1 --steps N --warmup W`) times exactly N steps and prints the headline
line without the measurements that live behind `--full`; `--dump-outputs DIR` writes what the last timed step left in
the sampler as float32 `DIR/<name>.npy`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FULL_ONLY = ("roofline", "roofline_all", "roofline_frac_at_sclk", "side_legs", "cpu_baseline", "cpu_baseline_throughput",
             "ess_steps", "sustained_steps")


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, cuda_device):
    steps, warm, C, K = 3, 1, 16, 17240
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warm), "--dump-outputs", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warm and d["full"] is False
    assert d["unit"] == "leapfrog-steps/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: C chains x L leapfrog steps per timed step
    assert d["value"] == pytest.approx(C * d["config"]["L"] / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    shapes = {"theta": (C, K), "grad": (C, K), "logp": (C,), "accepted": (C, steps), "logp_trace": (C, steps)}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    arr = {n: np.load(out / (n + ".npy")) for n in shapes}
    for n, a in arr.items():
        assert a.dtype == np.float32 and a.shape == shapes[n] and np.isfinite(a).all(), n
    assert sum(a.nbytes for a in arr.values()) <= 64 * 2 ** 20
    assert np.isin(arr["accepted"], (0.0, 1.0)).all()
    # the state after the last timed step is the last entry of the trace, and the chains have moved apart
    assert np.array_equal(arr["logp"], arr["logp_trace"][:, -1])
    assert np.unique(arr["theta"], axis=0).shape[0] == C
