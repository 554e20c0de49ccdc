"""GPU: a plain `python bench.py` run.  It times the steps, prints one short result line
(headline only: what takes runs of its own is behind --full) and, with --dump-outputs DIR,
leaves the last timed step's histogram in DIR/hist.npy -- here checked against the oracle on
config 1's 10,000 codes."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_is_headline_only_and_dumps_the_last_histogram(tmp_path):
    from oracle import oracle as O
    from sctools_amd import synthetic

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--settle-steps", "0", "--config", "1", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "pairs/s" and out["higher_is_better"] is True and out["dtype"] in ("i32", "u32")
    n, L, seed = synthetic.CONFIGS[1]
    P = n * (n - 1) // 2
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(P / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("roofline", "pair_kernel", "paths", "cpu_baseline"):  # --full only
        assert key not in out

    assert sorted(os.listdir(tmp_path / "out")) == ["hist.npy"]
    hist = np.load(tmp_path / "out" / "hist.npy")
    assert hist.dtype == np.float64 and hist.ndim == 1
    ref = O.c_hist_rows(synthetic.whitelist_codes(n, L, seed))
    assert hist.tolist() == [float(x) for x in ref[:hist.size]] and not ref[hist.size:].any()
    assert hist.tolist() == [float(x) for x in out["hist"]] and hist.sum() == P
