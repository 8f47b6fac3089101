"""GPU: a plain `bench.py` run (no --full) prints the headline fields only, times exactly --steps steps, and
--dump-outputs writes the logits of its last timed step -- the same ones the hot path computes in this process on the
same seeded pairs and weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from pcr_amd import testing as T

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_logits_of_its_last_step(tmp_path):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--workload", "pt128", "--pairs", "16", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] in ("f32", "bf16x3", "bf16")
    for k in ("roofline", "also", "cpu_baseline", "max_abs_dlogit_vs_f32_path"):
        assert k not in d, k
    got = np.load(out / "logits.npy")
    assert got.dtype == np.float32 and np.isfinite(got).all()

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from pcr_amd import engine
    model, _ = bench.build_model("pt", bench.WORKLOADS["pt128"][3])
    s1, s2 = [t.cuda() for t in T.synthetic_pairs(16, 128, seed=1234, kind="randn")]
    if engine.GUARD and engine.PRECISION == "bf16x3":
        model.calibrate_precision(s1, s2, max_pairs=16)
    with torch.no_grad():
        want = bench.hot_path(model, s1, s2).cpu().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-5
