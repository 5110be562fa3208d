"""The plain benchmark run (``bench.py --gpus 1 --steps K --warmup W``): it times its steps and prints
the result line without the README workload (that is ``--full``), and ``--dump-outputs DIR`` writes what
the last timed step left - the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_TOTAL = 1200000
STEPS, WARMUP, B = 20, 5, 200


def _bench(tmp_path, name):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=tmp_path,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


@pytest.mark.timeout(240)
def test_plain_run_is_lean_and_dumps_reproducible_outputs(gpu_box, tmp_path):
    j, a = _bench(tmp_path, "a")
    # the headline figure: K timed steps, images/s = B * K / (K * ms_per_step)
    assert j["n_gpus"] == 1 and j["steps"] == STEPS and j["warmup"] == WARMUP and j["unit"] == "images/s"
    assert j["higher_is_better"] is True and j["dtype"] == "bf16" and j["ms_per_step"] > 0
    assert abs(j["value"] - B / (j["ms_per_step"] * 1e-3)) <= 1e-3 * j["value"]
    # nothing of the README workload ran: no child job, no 20 epochs, no evaluation
    for k in ("total_cost_time_s", "reference_script", "wallclock_20ep_s", "final_test_acc"):
        assert j[k] is None, k
    # the dump: flat fp32 parameter / gradient / Adadelta buffers and every timed step's loss
    assert sorted(a) == ["acc_delta", "grad", "loss", "param", "square_avg"]
    for k, v in a.items():
        assert v.dtype == np.float32 and v.shape == ((STEPS,) if k == "loss" else (PARAM_TOTAL,)), k
        assert np.isfinite(v).all(), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert j["dumped_outputs"]["float32"] == {k: list(v.shape) for k, v in a.items()}
    assert np.abs(a["grad"]).max() > 0 and (a["square_avg"] >= 0).all() and np.abs(a["param"]).max() > 0
    assert round(float(a["loss"][-1]), 4) == j["last_train_loss"]
    assert a["loss"][-1] < a["loss"][0]                       # 25 steps from random init: it trains
    # the same arguments give the same inputs and (fixed-order reductions, seeded dropout) the same outputs
    _, b = _bench(tmp_path, "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
