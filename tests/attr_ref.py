"""Shared by the attribution tests (tests/test_attribute_cpu.py, tests/test_gpu_attribute.py): the trained test
net (the recipe of test_gpu_input_grad.py), the sixteen completeness images and the completeness gap G(n)."""
import functools

import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import PIXEL_LO, Predictor
from pytorch_mnist_ddp_amd.models.net import Net

# The completeness images: fixed indices into generate(64, seed=5), chosen once so that the CPU reference satisfies
# G(64) <= G(1) / 2 and G(256) <= G(16) (tests/test_attribute_cpu.py checks that it does).
COMPLETENESS_INDEX = tuple(range(16))


@functools.lru_cache(maxsize=None)
def trained_net():
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(1024, seed=11)
    x, y = normalize_u8(imgs), labels.long()
    opt = torch.optim.Adadelta(net.parameters(), lr=1.0)
    net.train()
    with torch.enable_grad():
        for step in range(32):
            i = (step * 64) % 1024
            opt.zero_grad()
            F.nll_loss(net.forward_reference(x[i:i + 64]), y[i:i + 64]).backward()
            opt.step()
    net.zero_grad(set_to_none=True)
    return net.eval()


@functools.lru_cache(maxsize=None)
def completeness_case():
    """(uint8 images [16, 28, 28], labels [16]): never modified."""
    imgs, labels = generate(64, seed=5)
    idx = torch.tensor(COMPLETENESS_INDEX)
    return imgs[idx].contiguous(), labels[idx].contiguous()


def completeness_gaps(pr: Predictor, n: int) -> torch.Tensor:
    """float64 [16]: per image |sum attr - (log p_y(x) - log p_y(black))| of ``pr``'s integrated gradients with
    ``n`` steps against the true labels, both log-probabilities from ``pr.log_probs``."""
    imgs, labels = completeness_case()
    attr, _ = pr.attribute(imgs, labels, "integrated_gradients", steps=n)
    y = labels.long().view(-1, 1)
    lp_x = pr.log_probs(imgs).cpu().gather(1, y)[:, 0].double()
    lp_b = pr.log_probs(torch.full((1, 1, 28, 28), PIXEL_LO)).cpu()[0][y[:, 0]].double()
    return (attr.cpu().reshape(16, 784).double().sum(dim=1) - (lp_x - lp_b)).abs()


def G(pr: Predictor, n: int) -> float:
    return float(completeness_gaps(pr, n).sum())
