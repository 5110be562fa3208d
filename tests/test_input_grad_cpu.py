"""Input gradients on the CPU side: ``Predictor.input_gradient`` against plain torch autograd, the
native entry point's presence, the launch plan of ``input_grad.hip`` and the ``--saliency`` option."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import _build
from pytorch_mnist_ddp_amd.data.datasets import load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, build_predict_parser
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd_reference(net, x, labels=None):
    """Plain torch autograd over forward_reference in eval mode: (d sum-NLL / dx, log-probs)."""
    was = net.training
    net.eval()
    x = x.clone().requires_grad_()
    lp = net.forward_reference(x)
    target = lp.detach().argmax(1) if labels is None else labels.long()
    F.nll_loss(lp, target, reduction='sum').backward()
    net.train(was)
    return x.grad, lp.detach()


def test_predictor_input_gradient_cpu_is_torch_autograd_bitwise():
    torch.manual_seed(3)
    net = Net()
    imgs, labels = generate(9, seed=5)
    x = normalize_u8(imgs)
    want_g, want_lp = _autograd_reference(net, x, labels)
    want_gp, _ = _autograd_reference(net, x)                 # against the predicted class
    net.zero_grad(set_to_none=True)                          # (the reference's backward filled them)
    net.train()                                              # inference semantics whatever the mode ...
    pr = Predictor(net)
    assert not pr.native
    for inp in (x, imgs, imgs.reshape(9, 784)):              # float [B,1,28,28], uint8 [B,28,28] / [B,784]
        g, lp = pr.input_gradient(inp, labels)
        assert g.shape == (9, 1, 28, 28) and g.dtype == torch.float32 and lp.shape == (9, 10)
        assert torch.equal(g, want_g) and torch.equal(lp, want_lp)
        assert not g.requires_grad and not lp.requires_grad
        g, lp = pr.input_gradient(inp)
        assert torch.equal(g, want_gp) and torch.equal(lp, want_lp)
    assert net.training and (net.dropout1.p, net.dropout2.p) == (0.25, 0.5)   # ... and the mode is left alone
    assert all(p.grad is None for p in net.parameters())     # no parameter gradient is accumulated
    assert want_g.abs().sum() > 0 and not torch.equal(want_g, want_gp)
    with pytest.raises(ValueError):
        pr.input_gradient(torch.zeros(2, 3, 28, 28))
    with pytest.raises(ValueError):
        pr.input_gradient(x, labels[:5])


def test_native_extension_has_input_grad():
    _build.build()
    C = native.load(build_if_missing=False)
    assert callable(C.input_grad) and callable(C.input_grad_plan)


def test_input_grad_plan_invariants():
    C = native.load()
    for cus in (1, 64, 256, 304):
        for B in list(range(1, 300)) + [511, 512, 513, 1000, 8192, 65536]:
            p = C.input_grad_plan(B, cus)
            items, rounds, grid = p["items"], p["rounds"], p["grid"]
            assert items == 4 * B                            # 4 strips of 7 rows cover the 28 dx rows
            assert 1 <= grid <= min(items, 2 * cus)          # two workgroups per CU fit by LDS
            assert grid * rounds >= items > grid * (rounds - 1)          # every item once, no idle round
            assert rounds == -(-items // (2 * cus))          # as few rounds as the full grid would need
            assert grid * rounds - items < rounds            # ... on the fewest workgroups that keep them
    assert C.input_grad_plan(1)["grid"] == 4
    assert C.input_grad_plan(64, 256) == {"items": 256, "rounds": 1, "grid": 256}
    assert C.input_grad_plan(200, 256) == {"items": 800, "rounds": 2, "grid": 400}   # > 1 item per workgroup
    for bad in ((0, 256), (-3, 256), (5, 0)):
        with pytest.raises(Exception):
            C.input_grad_plan(*bad)


def test_predict_parser_saliency_option():
    ap = build_predict_parser()
    assert ap.parse_args([]).saliency is None
    assert ap.parse_args(["--saliency", "out.npy"]).saliency == "out.npy"


def test_predict_cli_writes_saliency_on_cpu(tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    out = str(tmp_path / "sal.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", "40", "--checkpoint", ckpt, "--batch-size", "24",
                        "--saliency", out],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("Test set:")]) == 1
    sal = np.load(out)
    assert sal.shape == (40, 28, 28) and sal.dtype == np.float32
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    want = torch.cat([_autograd_reference(net, normalize_u8(data.images[i:i + 24]), data.targets[i:i + 24])[0]
                      for i in (0, 24)])
    assert torch.equal(torch.from_numpy(sal), want.reshape(40, 28, 28))
