"""Host-side references shared by the adversarial-training tests (CPU and GPU): the numpy emulation of the
``adv_init`` kernel (csrc/kernels/adv_train.hip) on ``refmodel.philox4x32``, and the L-inf PGD formula
written out in plain torch."""
import numpy as np
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO

import refmodel as R

ADV_PHILOX_DOMAIN = 0x41445631          # csrc/include/kernels.h
LUT = _PIXEL_LUT.numpy().astype(np.float32)
F32 = np.float32


def adv_uniform_words(B: int, seed: int, step: int) -> np.ndarray:
    """uint32 [B, 784]: element e of row b is word e % 4 of philox4x32((b * 196 + e // 4, DOMAIN, step, 0), seed)."""
    c0 = np.arange(B * 196, dtype=np.uint64)
    w = R.philox4x32((c0, ADV_PHILOX_DOMAIN, int(step) & R.MASK, 0), (seed & R.MASK, (seed >> 32) & R.MASK))
    w = np.stack([np.broadcast_to(np.asarray(x, dtype=np.uint64), c0.shape) for x in w], axis=1)   # [B*196, 4]
    return (w & np.uint64(R.MASK)).astype(np.uint32).reshape(B, 784)


def adv_init_emulation(u8_rows: np.ndarray, seed: int, step: int, eps: float, lo: float, hi: float,
                       random_start: bool):
    """(x0, x, u) float32 [B, 784] as ``adv_init`` computes them for the rows ``u8_rows`` (uint8 [B, 784], already
    resolved): every operation in float32, rounded on its own."""
    x0 = LUT[u8_rows.astype(np.int64)]
    B = x0.shape[0]
    u = (adv_uniform_words(B, seed, step) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    if not random_start:
        return x0, x0.copy(), u
    t = x0 + (F32(2.0) * u - F32(1.0)) * F32(eps)
    x = np.minimum(np.maximum(t, F32(lo)), F32(hi))
    return x0, x.astype(F32), u


def plain_pgd(net, x0: torch.Tensor, labels: torch.Tensor, eps: float, steps: int, step_size=None) -> torch.Tensor:
    """L-inf FGSM / PGD in plain torch over ``forward_reference`` in eval mode (the formula of
    tests/test_attack_cpu.py); ``x0`` float32 [B,1,28,28] normalised, ``eps`` / ``step_size`` in pixel units."""
    was = net.training
    net.eval()
    eps_n = eps / MNIST_STD
    alpha = (eps if steps == 1 else 2.5 * eps / steps) / MNIST_STD if step_size is None else step_size / MNIST_STD
    x = x0.clone()
    for _ in range(steps):
        xg = x.clone().requires_grad_()
        g, = torch.autograd.grad(F.nll_loss(net.forward_reference(xg), labels.long(), reduction='sum'), xg)
        t = x + alpha * torch.sign(g)
        t = torch.min(torch.max(t, x0 - eps_n), x0 + eps_n)
        x = torch.clamp(t, PIXEL_LO, PIXEL_HI)
    net.train(was)
    return x.detach()
