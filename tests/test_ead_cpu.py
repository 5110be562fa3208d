"""EAD on the CPU: ``ead_step_reference`` in float32 against the float64 evaluation of the kernel's formulas,
``Predictor.elastic_net`` (``reference_elastic_net``) on the trained test net, the argument checks and the command
line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import deepfool_ref as D
import ead_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_bits = lambda t: t.contiguous().view(torch.int32)                                          # noqa: E731


@pytest.mark.parametrize("rule", ["en", "l1"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M", [1, 3, 33])
def test_reference_against_float64(M, kind, rule):
    """float32, the sums in the kernel's tree, against float64: the records and every shrinkage decision equal, the
    rows and d_best within 64 float32 ulps of the row's (of d_best's) largest value."""
    for sign in (1, -1):
        for kappa in (0.0, 0.5):
            ops = R.make_case(M, sign, kappa, kind, rule)
            w64, r32 = R.step64(ops, sign, kappa, 4, 2, kind, rule), R.reference32(ops, sign, kappa, 4, 2, kind, rule)
            assert torch.equal(r32["istate"].long(), torch.from_numpy(w64["istate"]))
            assert torch.equal(_bits(r32["fstate"][:, :3]), _bits(torch.from_numpy(w64["fstate"][:, :3]).float()))
            if "branch" in w64:                  # the gap that makes float32 and float64 decide alike: no element left out
                assert w64["gap"].min() >= R.GAP_ULPS
                assert kind == "first" or all((w64["branch"] == b).any() for b in (-1, 0, 1))
                on_clean = torch.from_numpy(w64["branch"] == 0)
                assert torch.equal(_bits(r32["x"])[on_clean], _bits(ops["x0"])[on_clean])
            for k in R.ROWS:
                want = w64[k]
                cap = R.GAP_ULPS * 2.0 ** -23 * np.abs(want).max(axis=1, keepdims=True)
                assert (np.abs(r32[k].double().numpy() - want) <= cap).all(), k
            want, got = w64["fstate"][:, 3], r32["fstate"][:, 3].double().numpy()
            fin = np.isfinite(want)
            assert (got[~fin] == want[~fin]).all() and (np.abs(got[fin] - want[fin]) <= R.GAP_ULPS * 2.0 ** -23 * np.abs(want[fin])).all()


def test_elastic_net_on_the_trained_net():
    imgs, _ = D.trained_case()
    imgs = imgs[:8]
    x = _PIXEL_LUT[imgs.reshape(8, 784).long()]
    pr = Predictor(D.trained_net())
    assert not pr.native
    med = {}
    for rule in ("en", "l1"):
        labels, out = R.cpu_elastic_net(8, rule)
        R.check_invariants(x, labels.long(), out, pr.predict(imgs))
        assert out[0].shape == (8, 1, 28, 28) and out[1][1] == 0 and out[3][1]          # mislabelled: found at radius 0
        med[rule] = float(out[1][out[3]].median())
    print(f"median L1 radius, 8 images, search_steps=3, steps=30: rule en {med['en']:.4f}, rule l1 {med['l1']:.4f}")
    assert med["l1"] <= med["en"]
    # beta = 0, rule en: the objective and the decision are Carlini-Wagner's, by another optimiser
    labels, out = R.cpu_elastic_net(8, "en", 0.0)
    R.check_invariants(x, labels.long(), out, pr.predict(imgs))
    l2 = (out[0].reshape(8, 784).double() - x.double()).square().sum(1).sqrt() * MNIST_STD
    cw = pr.carlini_wagner(imgs, labels, search_steps=3, steps=30)
    both = out[3] & cw[3]
    print(f"median L2 radius: EAD beta=0 {float(l2[both].median()):.4f}, CW {float(cw[1][both].median()):.4f}")
    assert both.sum() >= 6 and abs(float(l2[both].median()) / float(cw[1][both].double().median()) - 1) <= 0.10


@pytest.mark.parametrize("kw", [dict(targeted=True), dict(kappa=-0.5), dict(lr=0.0), dict(search_steps=0), dict(c_init=0.0),
                                dict(beta=-0.01), dict(decision_rule="l2")])
def test_argument_checks(kw):
    imgs, labels = D.trained_case()
    with pytest.raises(ValueError, match="elastic_net"):
        Predictor(D.trained_net()).elastic_net(imgs[:2], None if "targeted" in kw else labels[:2], **kw)


def test_cli(tmp_path):
    torch.manual_seed(5)
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(Net(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    base = [sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size", "16",
            "--checkpoint", ckpt, "--no-cuda"]
    for ead in (True, False):
        log = str(tmp_path / f"log{int(ead)}.jsonl")
        flags = ["--ead", "--ead-count", "8", "--ead-search-steps", "2", "--ead-steps", "5", "--ead-rule", "l1",
                 "--ead-radii", "5"] if ead else []
        r = subprocess.run(base + ["--json-log", log] + flags, cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        with open(log) as f:
            rec = json.loads(f.read())
        keys = {"ead_search_steps", "ead_steps", "ead_lr", "ead_c", "ead_beta", "ead_kappa", "ead_rule", "ead_count",
                "ead_found", "ead_median_radius", "ead_mean_radius", "ead_accuracy_at"}
        if ead:
            assert len(lines) == 3 and lines[1].startswith("EAD set (L1, rule=l1, search=2, steps=5): Found: ") and "/8 (" in lines[1]
            assert lines[2].startswith("Accuracy at radius 5: ") and keys <= set(rec) and rec["ead_count"] == 8
        else:
            assert len(lines) == 1 and not any(k.startswith("ead_") for k in rec) and "EAD set" not in r.stdout
