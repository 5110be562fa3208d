"""L1 Auto-PGD on the CPU side: the float64 projection against a bisection, schedule, k_sel, refusals, CLI, Predictor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import apgd_l1_ref as R
from attr_ref import trained_net
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, auto_pgd_l1_line, build_predict_parser
from pytorch_mnist_ddp_amd.ops import functional as Fk

LO, HI = R.LO, R.HI


@pytest.mark.parametrize("eps", [0.0, 0.5, 10.0 / MNIST_STD, 200.0])
def test_projection_against_the_bisection(eps):
    case = R.make_case(20, seed=11, eps=eps)                 # free and binding caps, a flat background, zeros, ties
    x0 = case["x0"].double()
    z = (case["x"].double() - x0) * 3.0 + case["dx"].double().sign() * torch.linspace(0, 2, 20).view(20, 1).double()
    z[0] = (case["x"][0].double() - x0[0]) * 0.2             # well inside for eps >= 0.5
    delta, lam = Fk.l1_box_projection_reference(z, x0, eps, LO, HI)
    for i in range(20):
        want, lam_w = R.project(z[i].numpy(), x0[i].numpy(), eps)
        assert np.abs(delta[i].numpy() - want).max() <= 1e-12 and abs(float(lam[i]) - lam_w) <= 1e-12, i
    p = x0 + delta
    assert (delta.abs().sum(dim=1) <= eps * (1 + 1e-12)).all() and (p >= LO).all() and (p <= HI).all()
    assert torch.equal(p, x0) if eps == 0.0 else (float(lam[0]) == 0.0 and torch.equal(delta[0], z[0]))  # inside: untouched


def test_checkpoints_and_k_sel():
    assert Fk.apgd_l1_checkpoints(100) == tuple((i, 4) for i in range(4, 101, 4))
    assert Fk.apgd_l1_checkpoints(50) == tuple((i, 2) for i in range(2, 51, 2))
    assert Fk.apgd_l1_checkpoints(10)[0] == (1, 1) and Fk.apgd_l1_checkpoints(110)[-1] == (108, 4)
    assert [Fk.apgd_l1_k_sel(sp) for sp in (0, 1, 2, 3, 784)] == [1, 1, 2, 2, 523]


def test_refusals_of_the_new_entry_points():
    z, f, n = torch.zeros(2, 784), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    for bad in (dict(sign=0), dict(eps=-1.0), dict(first=True, last=True), dict(window=-1)):
        with pytest.raises(ValueError):
            Fk.apgd_l1_step_reference(z, torch.zeros(2), z, z, z, z, f, n, **dict(dict(sign=1, eps=1.0, lo=LO, hi=HI), **bad))
    pr, x = Predictor(trained_net()), torch.zeros(2, 1, 28, 28)
    for kw in (dict(eps=-1.0), dict(steps=0), dict(loss="l1"), dict(targeted=True), dict(labels=torch.tensor([0]))):
        with pytest.raises(ValueError):
            pr.auto_pgd_l1(x, **kw)


def test_predict_parser_and_line():
    d = build_predict_parser().parse_args([])
    assert (d.apgd_eps, d.apgd_steps, d.apgd_norm, d.apgd_restarts, d.apgd_seed, d.apgd_loss) == (None, 100, "linf", 1, 0, "ce")
    assert (d.apgd_l1_eps, d.apgd_l1_steps, d.apgd_l1_loss) == (None, 100, "ce")
    assert auto_pgd_l1_line(10, 100, 0.12344, 9876, 10000, 23.5) == \
        "Auto-PGD set (L1 eps=10, steps=100): Average loss: 0.1234, Accuracy: 9876/10000 (99%), median pixels changed: 23.5"
    line = auto_pgd_l1_line(5, 3, 1.0, 1, 2, None, "cw")
    assert line.startswith("Auto-PGD set (L1 eps=5, steps=3, loss=cw): ") and line.endswith("median pixels changed: n/a")


def test_predictor_auto_pgd_l1_cpu():
    imgs, labels = generate(64, seed=5)
    x0, y = normalize_u8(imgs).reshape(64, 784)[:8], labels[:8].long()
    pr = Predictor(trained_net())
    x_adv, lp, loss_best = pr.auto_pgd_l1(x0.view(8, 1, 28, 28), y, eps=10.0, steps=10)
    xa = x_adv.reshape(8, 784)
    mass = (xa.double() - x0.double()).abs().sum(dim=1)
    assert (xa >= LO).all() and (xa <= HI).all() and (mass <= 10.0 / MNIST_STD * (1 + 1e-5)).all()
    start = F.nll_loss(pr.log_probs(x0.view(8, 1, 28, 28)), y, reduction='none')
    assert (loss_best >= start).all() and float(mass.max()) > 1.0
    assert torch.allclose(F.nll_loss(lp, y, reduction='none'), loss_best, atol=1e-5)
