"""L-inf FGSM / PGD on the CPU side: ``Predictor.adversarial`` / ``robust_evaluate`` against the attack
written out in plain torch, the box conditions, the loss it gains on the reference, the native entry
point's presence and the ``mnist_predict.py --attack-eps`` option."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import _build
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, adversarial_line, build_predict_parser
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plain_pgd(net, x0, labels, eps, steps, step_size=None):
    """FGSM / PGD in plain torch over forward_reference in eval mode; ``eps`` in pixel units.  Returns
    (x_adv, log-probs of x_adv, the last step's gradient)."""
    was = net.training
    net.eval()
    eps_n = eps / MNIST_STD
    alpha = (eps if steps == 1 else 2.5 * eps / steps) / MNIST_STD if step_size is None else step_size / MNIST_STD
    lo, hi = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten().tolist()
    with torch.no_grad():
        target = net.forward_reference(x0).argmax(1) if labels is None else labels.long()
    x = x0.clone()
    for _ in range(steps):
        xg = x.clone().requires_grad_()
        g, = torch.autograd.grad(F.nll_loss(net.forward_reference(xg), target, reduction='sum'), xg)
        t = x + alpha * torch.sign(g)
        t = torch.min(torch.max(t, x0 - eps_n), x0 + eps_n)
        x = torch.clamp(t, lo, hi)
    with torch.no_grad():
        lp = net.forward_reference(x)
    net.train(was)
    return x, lp, g


@functools.lru_cache(maxsize=None)
def _case64():
    """The seeded net and the 64 synthetic images of the loss figures below; never modified."""
    torch.manual_seed(3)
    net = Net().train()
    imgs, labels = generate(64, seed=5)
    return net, imgs, labels


@pytest.mark.parametrize("steps", [1, 4])
def test_predictor_adversarial_cpu_is_plain_torch_bitwise(steps):
    torch.manual_seed(3)
    net = Net().train()                                      # inference semantics whatever the mode
    imgs, labels = generate(9, seed=5)
    x = normalize_u8(imgs)
    pr = Predictor(net)
    assert not pr.native
    for lab in (labels, None):
        want_x, want_lp, _ = plain_pgd(net, x, lab, 0.1, steps)
        assert not torch.equal(want_x, x)
        for inp in (x, imgs, imgs.reshape(9, 784)):          # float [B,1,28,28], uint8 [B,28,28] / [B,784]
            xa, lp = pr.adversarial(inp, lab, eps=0.1, steps=steps)
            assert xa.shape == (9, 1, 28, 28) and xa.dtype == torch.float32 and lp.shape == (9, 10)
            assert torch.equal(xa, want_x) and torch.equal(lp, want_lp)
            assert not xa.requires_grad and not lp.requires_grad
    want_x, want_lp, _ = plain_pgd(net, x, labels, 0.2, steps, step_size=0.03)   # an explicit step size
    xa, lp = pr.adversarial(imgs, labels, eps=0.2, steps=steps, step_size=0.03)
    assert torch.equal(xa, want_x) and torch.equal(lp, want_lp)
    assert net.training and (net.dropout1.p, net.dropout2.p) == (0.25, 0.5)      # the mode is left alone
    assert all(p.grad is None for p in net.parameters())     # no parameter gradient is accumulated


@pytest.mark.parametrize("steps,random_start", [(1, False), (4, False), (3, True)])
def test_adversarial_box_conditions_exact(steps, random_start):
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x0 = normalize_u8(imgs)
    for eps in (0.1, 0.3):
        gen = torch.Generator().manual_seed(7)
        xa, _ = pr.adversarial(imgs, labels, eps=eps, steps=steps, random_start=random_start, generator=gen)
        eps_n = eps / MNIST_STD
        assert (xa >= x0 - eps_n).all() and (xa <= x0 + eps_n).all()     # the bounds as fp32 tensors
        lo, hi = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten()
        assert (xa >= lo).all() and (xa <= hi).all()                     # exactly: pixels 0 and 255 normalised
        assert not torch.equal(xa, x0)
        if random_start:                                     # the same generator state, the same start
            again, _ = pr.adversarial(imgs, labels, eps=eps, steps=steps, random_start=True,
                                      generator=torch.Generator().manual_seed(7))
            plain, _ = pr.adversarial(imgs, labels, eps=eps, steps=steps)
            assert torch.equal(again, xa) and not torch.equal(plain, xa)
    xa, lp = pr.adversarial(imgs, labels, eps=0.0, steps=steps)
    assert torch.equal(xa, x0)                               # eps = 0: the clean images, exactly
    assert torch.equal(lp, pr.log_probs(imgs))


def test_reference_attack_raises_the_loss():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    y = labels.long()
    rows = lambda lp: F.nll_loss(lp, y, reduction='none')
    clean = rows(pr.log_probs(imgs))
    _, _, g = plain_pgd(net, normalize_u8(imgs), labels, 0.1, 1)
    assert (g != 0).all()                                    # no gradient element is exactly zero
    adv = {k: rows(pr.adversarial(imgs, labels, eps=0.1, steps=k)[1]) for k in (1, 4)}
    print(f"mean NLL clean {clean.mean():.4f}, 1 step {adv[1].mean():.4f}, 4 steps {adv[4].mean():.4f}")
    assert abs(clean.mean().item() - 2.3066) < 5e-4 and abs(adv[1].mean().item() - 2.4158) < 5e-4
    assert abs(adv[4].mean().item() - 2.4655) < 5e-4
    assert adv[1].mean() > clean.mean() and adv[4].mean() > adv[1].mean()
    assert (adv[1] > clean).all() and (adv[4] > clean).all()           # all 64 rows go up


def test_robust_evaluate_cpu():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    assert pr.robust_evaluate(imgs, labels, 0.0)[1:] == pr.evaluate(imgs, labels)[1:]
    assert pr.robust_evaluate(imgs, labels, 0.0)[0] == pytest.approx(pr.evaluate(imgs, labels)[0], rel=1e-6)
    one = pr.robust_evaluate(imgs, labels, 0.1, steps=2, batch_size=64)
    parts = pr.robust_evaluate(imgs.reshape(64, 784), labels, 0.1, steps=2, batch_size=24)
    assert one[1:] == parts[1:] and one[2] == 64
    assert one[0] == pytest.approx(parts[0], rel=1e-5)
    _, lp = pr.adversarial(imgs, labels, eps=0.1, steps=2)
    assert one[0] == pytest.approx(F.nll_loss(lp, labels.long(), reduction='sum').item(), rel=1e-5)
    assert one[1] == int((lp.argmax(1) == labels).sum())
    assert one[0] > pr.evaluate(imgs, labels)[0]


def test_adversarial_value_errors():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x = imgs[:4]
    for kw in (dict(eps=-0.1), dict(eps=float("nan")), dict(steps=0), dict(steps=-2), dict(step_size=0.0),
               dict(step_size=-0.01)):
        with pytest.raises(ValueError):
            pr.adversarial(x, labels[:4], **kw)
    with pytest.raises(ValueError):
        pr.adversarial(torch.zeros(2, 3, 28, 28))
    with pytest.raises(ValueError):
        pr.adversarial(x, labels[:3])
    with pytest.raises(ValueError):
        pr.adversarial(x, torch.tensor([0, 1, 2, 10]))
    with pytest.raises(ValueError):
        pr.robust_evaluate(normalize_u8(x), labels[:4], 0.1)           # not uint8
    with pytest.raises(ValueError):
        pr.robust_evaluate(x, labels[:4], 0.1, batch_size=0)


def test_native_extension_has_input_grad_step():
    _build.build()
    C = native.load(build_if_missing=False)
    assert callable(C.input_grad_step)
    with pytest.raises(Exception):                           # the launcher's own checks come before any launch
        C.input_grad_step(0, 0, 0, 0, 0, 0, 0, 0.1, 0.1, 0.0, 1.0, 4, 0)
    with pytest.raises(Exception):
        C.input_grad_step(8, 8, 8, 8, 8, 8, 8, 0.1, 0.1, 0.0, 1.0, 0, 0)


def test_predict_parser_attack_options():
    ap = build_predict_parser()
    a = ap.parse_args([])
    assert a.attack_eps is None and a.attack_steps == 1 and a.attack_step_size is None
    a = ap.parse_args(["--attack-eps", "0.3", "--attack-steps", "7", "--attack-step-size", "0.05"])
    assert (a.attack_eps, a.attack_steps, a.attack_step_size) == (0.3, 7, 0.05)
    assert adversarial_line(0.1, 2, 0.12344, 9876, 10000) == \
        "Adversarial set (Linf eps=0.1, steps=2): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"


def _run_predict(tmp_path, *extra):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", "40", "--checkpoint", ckpt, "--batch-size", "24",
                        "--json-log", log, *extra],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(log) as f:
        return net, [ln for ln in r.stdout.splitlines() if ln.strip()], json.loads(f.read())


def test_predict_cli_attack_line_on_cpu(tmp_path):
    net, lines, rec = _run_predict(tmp_path, "--attack-eps", "0.1", "--attack-steps", "2")
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    pr = Predictor(net)
    loss, correct, n = pr.robust_evaluate(data.images, data.targets, 0.1, steps=2, batch_size=24)
    assert len(lines) == 2 and lines[0].startswith("Test set:")
    assert lines[1] == adversarial_line(0.1, 2, loss / n, correct, n)
    assert lines[1].startswith("Adversarial set (Linf eps=0.1, steps=2): Average loss: ")
    assert (rec["adv_eps"], rec["adv_steps"], rec["adv_correct"]) == (0.1, 2, correct)
    assert rec["adv_loss"] == pytest.approx(loss / n, rel=1e-6)
    clean = pr.evaluate(data.images, data.targets)
    assert rec["correct"] == clean[1] and rec["adv_loss"] > rec["test_loss"]


def test_predict_cli_without_attack_is_unchanged(tmp_path):
    _, lines, rec = _run_predict(tmp_path)
    assert len([ln for ln in lines if ln.startswith("Test set:")]) == 1
    assert not any("Adversarial" in ln for ln in lines) and len(lines) == 1
    assert sorted(rec) == ["checkpoint", "correct", "device", "n", "source", "test_loss"]
