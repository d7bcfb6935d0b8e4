"""bench.py's command line: a plain run prints the headline line only (no roofline / extras / CPU baseline, which
belong to --full), --steps sets the number of timed steps, and --dump-outputs writes the last timed step's arrays
as float32 / float64 .npy files of at most 64 MB in all."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_and_dump(cuda, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "clips/s" and rec["dtype"] == "bf16"
    assert rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(256 * 1000 / rec["ms_per_step"], rel=1e-3)
    assert not {"roofline", "extras", "cpu_baseline"} & set(rec)
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / "*.npy"))}
    assert {"loss_sums", "audio", "recon", "mu", "logvar", "grad_sample", "params_sample"} <= set(arrays)
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    assert arrays["recon"].shape == arrays["audio"].shape == (256, 1, 128, 128)
    assert arrays["mu"].shape == arrays["logvar"].shape == (256, 128)
