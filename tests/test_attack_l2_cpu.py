"""L2 and targeted PGD on the CPU side: ``Predictor.adversarial(norm="l2", targeted=...)`` /
``robust_evaluate(norm="l2")`` against the attack written out in plain torch, the ball and box conditions, the
loss it gains or removes on the reference, the native entry point's presence and ``mnist_predict.py
--attack-norm``."""
import functools
import inspect
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
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor, adversarial_line, build_predict_parser
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.attack import fused_adversarial
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 1e-12
LO, HI = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten().tolist()


def ball_slack(eps_n: float) -> float:
    """Upper bound of ||x_adv - x0||_2 (evaluated in float64) after an fp32 L2 projection to radius eps_n,
    with u = 2^-24 the fp32 unit roundoff and n = 784:
      * the norm m the scale is made from is sqrt of an fp32 sum of n squares: any summation order is within
        (1 + u)^n of the exact sum of the rounded squares, each square within (1 + u), the root halves the
        relative error and adds one rounding: m_hat >= m (1 - (n / 2 + 2) u);
      * the scale's TWO roundings: s = fl(eps / m_hat) and d_i' = fl(d_i s), (1 + u) each - also when the
        scale is clamped to 1 because fl(eps / m_hat) >= 1 only says m_hat <= eps (1 + u);
      * d_i itself is the fp32 t - x0 the norm was taken of (no further error), and x_adv_i = fl(x0_i + d_i')
        is off by at most u max(|lo|, |hi|) per element, sqrt(n) = 28 times that in the norm;
      * the last clamp moves x_adv_i towards x0_i (x0 is inside [lo, hi]): it only shrinks.
    Together: eps_n (1 + (n / 2 + 4) u) (to first order; doubled to cover the higher-order terms: 4 * 2^-23 *
    (n / 8 + 1)) + 28 u max(|lo|, |hi|)."""
    u = 2.0 ** -24
    return eps_n * (1.0 + 4 * 2.0 ** -23 * (784 / 8 + 1)) + 28 * u * max(abs(LO), abs(HI))


def plain_l2_pgd(net, x0, labels, eps, steps, step_size=None, targeted=False, x_init=None):
    """L2 PGD in plain torch over forward_reference in eval mode; ``eps`` in pixel units.  Returns (x_adv,
    log-probs of x_adv)."""
    was = net.training
    net.eval()
    B = x0.shape[0]
    eps_n = eps / MNIST_STD
    alpha = (eps if steps == 1 else 2.5 * eps / steps) / MNIST_STD if step_size is None else step_size / MNIST_STD
    if targeted:
        alpha = -alpha
    with torch.no_grad():
        target = net.forward_reference(x0).argmax(1) if labels is None else labels.long()
    c = x0.reshape(B, 784)
    x = c.clone() if x_init is None else x_init.clone()
    for _ in range(steps):
        xg = x.clone().requires_grad_()
        g, = torch.autograd.grad(F.nll_loss(net.forward_reference(xg.view(B, 1, 28, 28)), target, reduction='sum'), xg)
        n = torch.sqrt(torch.sum(g * g, dim=1, keepdim=True))
        t = x + (alpha / torch.clamp(n, min=TINY)) * g
        d = t - c
        m = torch.sqrt(torch.sum(d * d, dim=1, keepdim=True))
        d = d * torch.clamp(eps_n / torch.clamp(m, min=TINY), max=1.0)
        x = torch.clamp(c + d, LO, HI)
    x = x.view(B, 1, 28, 28)
    with torch.no_grad():
        lp = net.forward_reference(x)
    net.train(was)
    return x, lp


@functools.lru_cache(maxsize=None)
def _case64():
    """The seeded net and 64 synthetic images (those of test_attack_cpu.py); never modified."""
    torch.manual_seed(3)
    net = Net().train()
    imgs, labels = generate(64, seed=5)
    return net, imgs, labels


def _targets(labels):
    return (labels.long() + 3) % 10


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("steps", [1, 3])
def test_predictor_l2_cpu_is_plain_torch_bitwise(steps, targeted):
    torch.manual_seed(3)
    net = Net().train()
    imgs, labels = generate(9, seed=5)
    x = normalize_u8(imgs)
    pr = Predictor(net)
    assert not pr.native and Fk.PGD_L2_TINY == TINY
    lab = _targets(labels) if targeted else labels
    want_x, want_lp = plain_l2_pgd(net, x, lab, 2.0, steps, targeted=targeted)
    assert not torch.equal(want_x, x)
    for inp in (x, imgs, imgs.reshape(9, 784)):
        xa, lp = pr.adversarial(inp, lab, eps=2.0, steps=steps, norm="l2", targeted=targeted)
        assert xa.shape == (9, 1, 28, 28) and xa.dtype == torch.float32 and lp.shape == (9, 10)
        assert torch.equal(xa, want_x) and torch.equal(lp, want_lp)
        assert not xa.requires_grad and not lp.requires_grad
    want_x, want_lp = plain_l2_pgd(net, x, lab, 1.5, steps, step_size=0.4, targeted=targeted)
    xa, lp = pr.adversarial(imgs, lab, eps=1.5, steps=steps, step_size=0.4, norm="l2", targeted=targeted)
    assert torch.equal(xa, want_x) and torch.equal(lp, want_lp)
    if not targeted:                                         # labels None: the class predicted on the clean input
        want_x, _ = plain_l2_pgd(net, x, None, 2.0, steps)
        assert torch.equal(pr.adversarial(imgs, None, eps=2.0, steps=steps, norm="l2")[0], want_x)
    assert net.training and (net.dropout1.p, net.dropout2.p) == (0.25, 0.5)
    assert all(p.grad is None for p in net.parameters())


def test_targeted_linf_cpu_descends_bitwise():
    """``targeted`` with the default norm: the signed-gradient step with its sign turned."""
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x0 = normalize_u8(imgs[:9]).reshape(9, 784)
    tgt = _targets(labels[:9])
    eps_n, alpha = 0.1 / MNIST_STD, 2.5 * 0.1 / 2 / MNIST_STD
    net.eval()
    x = x0.clone()
    for _ in range(2):
        xg = x.clone().requires_grad_()
        g, = torch.autograd.grad(F.nll_loss(net.forward_reference(xg.view(9, 1, 28, 28)), tgt, reduction='sum'), xg)
        t = x - alpha * torch.sign(g)
        x = torch.clamp(torch.min(torch.max(t, x0 - eps_n), x0 + eps_n), LO, HI)
    net.train()
    xa, lp = pr.adversarial(imgs[:9], tgt, eps=0.1, steps=2, targeted=True)
    assert torch.equal(xa.reshape(9, 784), x)
    rows = lambda q: F.nll_loss(q, tgt, reduction='none')
    assert (rows(lp) < rows(pr.log_probs(imgs[:9]))).all()


@pytest.mark.parametrize("steps,random_start,targeted", [(1, False, False), (3, False, False), (3, True, False),
                                                         (3, False, True)])
def test_l2_ball_and_box_conditions(steps, random_start, targeted):
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x0 = normalize_u8(imgs)
    lab = _targets(labels) if targeted else labels
    for eps in (0.5, 2.0):
        gen = torch.Generator().manual_seed(7)
        xa, _ = pr.adversarial(imgs, lab, eps=eps, steps=steps, random_start=random_start, generator=gen,
                               norm="l2", targeted=targeted)
        eps_n = eps / MNIST_STD
        dist = (xa.double() - x0.double()).reshape(64, 784).norm(dim=1)
        print(f"eps_n {eps_n:.6f} largest distance {float(dist.max()):.9f} bound {ball_slack(eps_n):.9f}")
        assert (dist <= ball_slack(eps_n)).all()
        assert (dist > 0).all()                              # every image moved
        assert (xa >= LO).all() and (xa <= HI).all()         # exactly: pixels 0 and 255 normalised
        assert (LO, HI) == (PIXEL_LO, PIXEL_HI)
        if random_start:                                     # the same generator state, the same start
            again, _ = pr.adversarial(imgs, lab, eps=eps, steps=steps, random_start=True,
                                      generator=torch.Generator().manual_seed(7), norm="l2")
            plain, _ = pr.adversarial(imgs, lab, eps=eps, steps=steps, norm="l2")
            assert torch.equal(again, xa) and not torch.equal(plain, xa)
    xa, lp = pr.adversarial(imgs, lab, eps=0.0, steps=steps, norm="l2", targeted=targeted)
    assert torch.equal(xa, x0)                               # eps = 0: the clean images, exactly
    assert torch.equal(lp, pr.log_probs(imgs))


def test_l2_attacks_move_the_loss_on_the_reference():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    y, tgt = labels.long(), _targets(labels)
    clean_lp = pr.log_probs(imgs)
    rows = lambda lp, t: F.nll_loss(lp, t, reduction='none')
    adv = {k: rows(pr.adversarial(imgs, labels, eps=2.0, steps=k, norm="l2")[1], y) for k in (1, 3)}
    clean = rows(clean_lp, y)
    print(f"untargeted: summed NLL clean {clean.sum():.4f}, 1 step {adv[1].sum():.4f}, 3 steps {adv[3].sum():.4f}")
    assert adv[1].sum() > clean.sum() and adv[3].sum() > adv[1].sum()
    assert (adv[1] > clean).all() and (adv[3] > clean).all()
    tclean = rows(clean_lp, tgt)
    tadv = {k: rows(pr.adversarial(imgs, tgt, eps=2.0, steps=k, norm="l2", targeted=True)[1], tgt) for k in (1, 3)}
    print(f"targeted: summed target NLL clean {tclean.sum():.4f}, 1 step {tadv[1].sum():.4f}, "
          f"3 steps {tadv[3].sum():.4f}")
    assert tadv[1].sum() < tclean.sum() and tadv[3].sum() < tadv[1].sum()
    assert (tadv[1] < tclean).all() and (tadv[3] < tclean).all()


def test_l2_step_reference_rows():
    """The torch form of the step on hand-made rows: a zero gradient stays put (projected), a NaN stays in
    its row, a negative step descends."""
    gen = torch.Generator().manual_seed(2)
    x0 = torch.rand(4, 784, generator=gen) * (HI - LO) + LO
    x = (x0 + 0.01 * torch.randn(4, 784, generator=gen)).clamp(LO, HI)
    g = torch.randn(4, 784, generator=gen)
    g[1] = 0.0
    g[2, 5] = float("nan")
    out = Fk.pgd_l2_step_reference(g, x, x0, 3.0, 0.5, LO, HI)
    # t = x exactly; inside the ball and the box the projection is x0 + (x - x0): x up to that rounding
    assert torch.equal(out[1], (x0[1] + (x[1] - x0[1])).clamp(LO, HI))
    assert (out[1] - x[1]).abs().max() <= 2.0 ** -23 * max(abs(LO), abs(HI))
    assert torch.isnan(out[2]).all() and torch.isfinite(out[[0, 1, 3]]).all()
    down = Fk.pgd_l2_step_reference(g, x, x0, 3.0, -0.5, LO, HI)
    assert ((out[0] - x[0]) * g[0]).sum() > 0 and ((down[0] - x[0]) * g[0]).sum() < 0
    assert not torch.equal(out[0], down[0])
    far = Fk.pgd_l2_step_reference(torch.zeros(4, 784), x0 + 1.0, x0, 3.0, 0.5, -1e9, 1e9)   # |d| = 28 > eps
    assert ((far - x0).double().norm(dim=1) <= ball_slack(3.0)).all()
    assert ((far - x0).double().norm(dim=1) > 2.99).all()


def test_zero_gradient_image_stays_put():
    """A net whose output does not depend on the input (conv1 zeroed: every gradient is exactly zero)."""
    torch.manual_seed(3)
    net = Net()
    with torch.no_grad():
        net.conv1.weight.zero_()
    imgs, labels = generate(5, seed=5)
    pr = Predictor(net)
    g, _ = pr.input_gradient(imgs, labels)
    assert not g.any()
    for targeted in (False, True):
        xa, _ = pr.adversarial(imgs, labels, eps=2.0, steps=3, norm="l2", targeted=targeted)
        assert torch.equal(xa, normalize_u8(imgs))


def test_l2_value_errors():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x = imgs[:4]
    for kw in (dict(norm="l1"), dict(norm="L2"), dict(norm=None), dict(norm="l2", eps=-0.1), dict(norm="l2", steps=0),
               dict(norm="l2", step_size=0.0)):
        with pytest.raises(ValueError):
            pr.adversarial(x, labels[:4], **kw)
    for norm in ("linf", "l2"):
        with pytest.raises(ValueError):
            pr.adversarial(x, None, norm=norm, targeted=True)             # a targeted attack needs its targets
    with pytest.raises(ValueError):
        pr.adversarial(x, torch.tensor([0, 1, 2, 10]), norm="l2", targeted=True)
    with pytest.raises(ValueError):
        pr.robust_evaluate(x, labels[:4], 0.5, norm="l0")
    with pytest.raises(ValueError):
        fused_adversarial(net, normalize_u8(x).reshape(4, 784), labels[:4], 1.0, 1, 1.0, LO, HI, norm="l1")


def test_new_keywords_come_last_with_the_old_defaults():
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(Predictor.adversarial)[-2:] == ["norm", "targeted"]
    assert names(Predictor.adversarial)[:-2] == ["self", "x", "labels", "eps", "steps", "step_size", "random_start",
                                                 "generator"]
    assert names(Predictor.robust_evaluate)[-2:] == ["batch_size", "norm"]
    assert names(fused_adversarial)[-3:] == ["x_init", "norm", "targeted"]
    d = inspect.signature(Predictor.adversarial).parameters
    assert d["norm"].default == "linf" and d["targeted"].default is False
    assert inspect.signature(Predictor.robust_evaluate).parameters["norm"].default == "linf"


def test_no_norm_keyword_is_todays_linf():
    """Without ``norm=`` / ``targeted=`` the calls give the L-inf attack written out here, byte for byte (the
    formula of test_attack_cpu.py), random start included."""
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x0 = normalize_u8(imgs[:9]).reshape(9, 784)
    y = labels[:9].long()
    eps_n, alpha = 0.1 / MNIST_STD, 2.5 * 0.1 / 3 / MNIST_STD
    u = torch.rand(9, 784, generator=torch.Generator().manual_seed(11), dtype=torch.float32)
    net.eval()
    for start in (None, (x0 + (2.0 * u - 1.0) * eps_n).clamp_(LO, HI)):
        x = x0.clone() if start is None else start
        for _ in range(3):
            xg = x.clone().requires_grad_()
            g, = torch.autograd.grad(F.nll_loss(net.forward_reference(xg.view(9, 1, 28, 28)), y, reduction='sum'), xg)
            t = x + alpha * torch.sign(g)
            x = torch.clamp(torch.min(torch.max(t, x0 - eps_n), x0 + eps_n), LO, HI)
        net.train()
        kw = lambda: {} if start is None else dict(random_start=True, generator=torch.Generator().manual_seed(11))
        xa, lp = pr.adversarial(imgs[:9], labels[:9], 0.1, 3, **kw())
        xb, lpb = pr.adversarial(imgs[:9], labels[:9], 0.1, 3, norm="linf", targeted=False, **kw())
        assert xa.numpy().tobytes() == x.view(9, 1, 28, 28).numpy().tobytes()
        assert xb.numpy().tobytes() == xa.numpy().tobytes() and lpb.numpy().tobytes() == lp.numpy().tobytes()
        net.eval()
    net.train()
    a = pr.robust_evaluate(imgs, labels, 0.1, 2, None, 24)
    assert a == pr.robust_evaluate(imgs, labels, 0.1, 2, None, 24, norm="linf")
    assert a != pr.robust_evaluate(imgs, labels, 0.1, 2, None, 24, norm="l2")


def test_robust_evaluate_l2_cpu():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    one = pr.robust_evaluate(imgs, labels, 2.0, steps=2, batch_size=64, norm="l2")
    parts = pr.robust_evaluate(imgs.reshape(64, 784), labels, 2.0, steps=2, batch_size=24, norm="l2")
    assert one[1:] == parts[1:] and one[2] == 64
    assert one[0] == pytest.approx(parts[0], rel=1e-5)
    _, lp = pr.adversarial(imgs, labels, eps=2.0, steps=2, norm="l2")
    assert one[0] == pytest.approx(F.nll_loss(lp, labels.long(), reduction='sum').item(), rel=1e-5)
    assert one[1] == int((lp.argmax(1) == labels).sum())
    assert one[0] > pr.evaluate(imgs, labels)[0]
    zero, clean = pr.robust_evaluate(imgs, labels, 0.0, norm="l2"), pr.evaluate(imgs, labels)
    assert zero[1:] == clean[1:] and zero[0] == pytest.approx(clean[0], rel=1e-6)


def test_native_extension_has_pgd_l2_step():
    _build.build()
    C = native.load(build_if_missing=False)
    assert callable(C.pgd_l2_step)
    assert C.PGD_L2_TINY == float(torch.tensor(Fk.PGD_L2_TINY, dtype=torch.float32))   # one constant, fp32 on the device
    # the launcher's own checks come before any launch: null pointers, B = 0, B past the limit, eps < 0 / NaN
    for ptrs in ((0, 16, 16, 16), (16, 0, 16, 16), (16, 16, 0, 16), (16, 16, 16, 0)):
        with pytest.raises(RuntimeError):
            C.pgd_l2_step(*ptrs, 0.1, 0.1, 0.0, 1.0, 4, 0)
    for B in (0, -1, (1 << 20) + 1):
        with pytest.raises(RuntimeError):
            C.pgd_l2_step(16, 16, 16, 16, 0.1, 0.1, 0.0, 1.0, B, 0)
    for eps in (-0.1, float("nan")):
        with pytest.raises(RuntimeError):
            C.pgd_l2_step(16, 16, 16, 16, 0.1, eps, 0.0, 1.0, 4, 0)
    with pytest.raises(RuntimeError):
        C.pgd_l2_step(16, 16, 20, 16, 0.1, 0.1, 0.0, 1.0, 4, 0)          # not 16-byte aligned
    with pytest.raises(ValueError):                          # the functional wrapper wants GPU tensors
        Fk.pgd_l2_step(torch.zeros(2, 784), torch.zeros(2, 784), torch.zeros(2, 784), 1.0, 1.0, 0.0, 1.0)


def test_predict_parser_attack_norm_and_line():
    ap = build_predict_parser()
    assert ap.parse_args([]).attack_norm == "linf"
    assert ap.parse_args(["--attack-norm", "l2"]).attack_norm == "l2"
    with pytest.raises(SystemExit):
        ap.parse_args(["--attack-norm", "l1"])
    assert adversarial_line(2, 5, 0.12344, 9876, 10000, "l2") == \
        "Adversarial set (L2 eps=2, steps=5): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"
    assert adversarial_line(0.1, 2, 0.12344, 9876, 10000, norm="linf") == adversarial_line(0.1, 2, 0.12344, 9876, 10000)
    assert adversarial_line(0.1, 2, 0.12344, 9876, 10000) == \
        "Adversarial set (Linf eps=0.1, steps=2): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"


def test_predict_cli_l2_line_on_cpu(tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", "40", "--checkpoint", ckpt, "--batch-size", "24",
                        "--json-log", log, "--attack-eps", "1.5", "--attack-steps", "2", "--attack-norm", "l2"],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    with open(log) as f:
        rec = json.loads(f.read())
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    pr = Predictor(net)
    loss, correct, n = pr.robust_evaluate(data.images, data.targets, 1.5, steps=2, batch_size=24, norm="l2")
    assert len(lines) == 2 and lines[0].startswith("Test set:")
    assert lines[1] == adversarial_line(1.5, 2, loss / n, correct, n, "l2")
    assert lines[1].startswith("Adversarial set (L2 eps=1.5, steps=2): Average loss: ")
    assert (rec["adv_eps"], rec["adv_steps"], rec["adv_correct"], rec["adv_norm"]) == (1.5, 2, correct, "l2")
    assert rec["adv_loss"] == pytest.approx(loss / n, rel=1e-6)
    assert rec["adv_loss"] > rec["test_loss"]
