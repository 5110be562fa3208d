"""Inference on the CPU side: the launch plan of the fused kernel, the Predictor on CPU tensors,
checkpoint round trips and the mnist_predict.py command line."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from pytorch_mnist_ddp_amd.data.datasets import load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pixel_lut_is_normalize_u8_and_shared_with_inference():
    from pytorch_mnist_ddp_amd import inference
    from pytorch_mnist_ddp_amd.data.datasets import PIXEL_HI, PIXEL_LO, PIXEL_LUT
    assert torch.equal(PIXEL_LUT, normalize_u8(torch.arange(256, dtype=torch.uint8).view(1, 16, 16)).reshape(256))
    assert inference._PIXEL_LUT is PIXEL_LUT
    assert (inference.PIXEL_LO, inference.PIXEL_HI) == (PIXEL_LO, PIXEL_HI) == (float(PIXEL_LUT[0]), float(PIXEL_LUT[255]))


def test_infer_plan_invariants():
    C = native.load()
    assert C.INFER_BANDS == 12
    last_ws = 0
    for B in list(range(1, 601)) + [1000, 8192, 10000]:
        p = C.infer_plan(B)
        ipw, groups, bands = p["images_per_wg"], p["groups"], p["bands"]
        assert bands == C.INFER_BANDS
        assert 1 <= ipw <= 16
        assert groups * ipw >= B > (groups - 1) * ipw
        assert p["grid"] == (bands, groups)                  # documented layout: grid.x = band, grid.y = group
        assert p["workspace_bytes"] >= 4 * bands * groups * ipw * 128
        assert p["workspace_bytes"] >= last_ws               # a buffer made for max_B serves every smaller B
        last_ws = p["workspace_bytes"]
        assert p["ticket_count"] >= groups
    # the grid fills the device at small B and caps the images per workgroup at large B
    assert C.infer_plan(1)["images_per_wg"] == 1 and C.infer_plan(21)["images_per_wg"] == 1
    assert C.infer_plan(10000)["images_per_wg"] == 16
    for bad in (0, -1):
        with pytest.raises(Exception):
            C.infer_plan(bad)


def test_predictor_cpu_matches_net_eval_bitwise():
    torch.manual_seed(3)
    net = Net()
    imgs, _ = generate(9, seed=5)
    x = normalize_u8(imgs)
    with torch.no_grad():
        want = net.eval()(x)
    net.train()                                              # the predictor must not depend on the mode ...
    pr = Predictor(net)
    assert not pr.native and pr.device.type == "cpu"
    got_f = pr.log_probs(x)
    assert net.training                                      # ... nor change it
    assert torch.equal(got_f, want)
    assert torch.equal(pr.log_probs(imgs), want)                       # uint8 [B,28,28]
    assert torch.equal(pr.log_probs(imgs.reshape(9, 784)), want)       # uint8 [B,784]
    assert torch.equal(pr.predict(imgs), want.argmax(1))
    assert not got_f.requires_grad
    with pytest.raises(ValueError):
        pr.log_probs(torch.zeros(2, 3, 28, 28))


class _Wrapped(nn.Module):                                   # state_dict keys as DistributedDataParallel's
    def __init__(self, module):
        super().__init__()
        self.module = module


@pytest.mark.parametrize("variant", ["mnist_cnn.pt bare", "mnist_cnn.pt module.", "mnist_cnn_.pt bare"])
def test_from_checkpoint_round_trip(tmp_path, variant):
    torch.manual_seed(4)
    net = Net()
    name, keys = variant.split()
    path = str(tmp_path / name)
    save_state_dict(_Wrapped(net) if keys == "module." else net, path)
    sd = torch.load(path, weights_only=True)
    assert all(k.startswith("module.") for k in sd) == (keys == "module.")
    pr = Predictor.from_checkpoint(path, device="cpu")
    for (n, a), (_, b) in zip(net.named_parameters(), pr.net.named_parameters()):
        assert torch.equal(a, b), n
    imgs, _ = generate(5, seed=6)
    with torch.no_grad():
        assert torch.equal(pr.log_probs(imgs), net.eval()(normalize_u8(imgs)))


def test_predict_cli_on_cpu(tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", "64", "--checkpoint", ckpt, "--batch-size", "24",
                        "--json-log", log],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Test set:")]
    assert len(lines) == 1, r.stdout
    m = re.fullmatch(r"Test set: Average loss: (\d+\.\d{4}), Accuracy: (\d+)/(\d+) \((\d+)%\)", lines[0])
    assert m, lines[0]
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=64, verbose=False)
    loss_sum, correct, n = Predictor(net).evaluate(data.images, data.targets, batch_size=24)
    assert n == 64 and int(m.group(3)) == 64 and int(m.group(2)) == correct
    assert m.group(1) == "{:.4f}".format(loss_sum / n)
    assert m.group(4) == "{:.0f}".format(100. * correct / n)
    import json
    rec = json.loads(open(log).read().strip())
    assert rec["n"] == 64 and rec["correct"] == correct and rec["device"] == "cpu"
