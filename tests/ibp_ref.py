"""Shared by the IBP tests: a float64 oracle in the lower / upper formulation (l' = W+ l + W- u + b, u' = W+ u + W- l +
b: independent of the centre / radius form under test), the two nets and the case maker."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT
from pytorch_mnist_ddp_amd.models.net import Net

from attr_ref import trained_net
from deepfool_ref import trained_case

EPS_ROWS = (0.0, 0.002, 0.05, 1.0)            # per-row eps of the stage cases, cycled (1.0: the whole pixel range)
f32 = lambda v: float(np.float32(v))          # noqa: E731
ulp = lambda v: float(np.spacing(np.float32(v)))   # noqa: E731


@functools.lru_cache(maxsize=None)
def net(kind):
    """"random": a seeded Net with non-zero biases; "trained": ``attr_ref.trained_net()``.  Never modified."""
    if kind == "trained":
        return trained_net()
    torch.manual_seed(3)
    n = Net().eval()
    with torch.no_grad():
        for p in n.parameters():
            if p.dim() == 1:
                p.uniform_(-0.2, 0.2)
    return n


def _affine(op, l, u, W, b):
    Wp, Wn = W.clamp(min=0), W.clamp(max=0)
    return op(l, Wp) + op(u, Wn) + b, op(u, Wp) + op(l, Wn) + b


def _P(n):
    return {k: v.detach().double() for k, v in n.named_parameters()}


def oracle(n, x, y, eps):
    """float64 IBP of ``n`` at the rows ``x`` [M, 784], labels ``y``, eps [M] (float32 values): a dict of every stage's
    bounds - pl, pu, z1c, z1r (fc1 without its bias, as the kernels split it) and lb."""
    P = _P(n)
    M = x.shape[0]
    e = (torch.as_tensor(eps, dtype=torch.float32).expand(M).double() / f32(MNIST_STD))[:, None]
    x = x.double().reshape(M, 784)
    l, u = (x - e).clamp(min=f32(PIXEL_LO)).view(M, 1, 28, 28), (x + e).clamp(max=f32(PIXEL_HI)).view(M, 1, 28, 28)
    for name in ("conv1", "conv2"):
        l, u = _affine(F.conv2d, l, u, P[name + ".weight"], P[name + ".bias"].view(1, -1, 1, 1))
        l, u = l.relu(), u.relu()
    pl, pu = F.max_pool2d(l, 2).flatten(1), F.max_pool2d(u, 2).flatten(1)
    return dict(from_pool(n, pl, pu, y), pl=pl, pu=pu)


def from_pool(n, pl, pu, y):
    """The oracle from the pooled bounds on (float64 of whatever ``pl``, ``pu`` hold): z1c, z1r, lb."""
    zl, zu = _affine(lambda a, W: a @ W.t(), pl.double(), pu.double(), _P(n)["fc1.weight"], 0.0)
    return {"z1c": (zl + zu) / 2, "z1r": (zu - zl) / 2, "lb": from_fc1(n, (zl + zu) / 2, (zu - zl) / 2, y)}


def from_fc1(n, z1c, z1r, y):
    P, y = _P(n), y.long()
    b1 = P["fc1.bias"]
    l, u = (z1c.double() - z1r.double() + b1).relu(), (z1c.double() + z1r.double() + b1).relu()
    C = P["fc2.weight"][y][:, None, :] - P["fc2.weight"][None]
    lb = (C.clamp(min=0) * l[:, None] + C.clamp(max=0) * u[:, None]).sum(dim=2) + (P["fc2.bias"][y][:, None] - P["fc2.bias"])
    lb[torch.arange(len(y)), y] = float("inf")
    return lb


@functools.lru_cache(maxsize=None)
def case(M):
    """(x float32 [M, 784] normalised, labels [M], eps float32 [M]): the first M images of ``trained_case`` with the
    per-row eps ``EPS_ROWS`` cycled.  Never modified."""
    imgs, labels = trained_case()
    x = _PIXEL_LUT[imgs[:M].reshape(M, 784).long()].contiguous()
    return x, labels[:M].long(), torch.tensor([EPS_ROWS[i % 4] for i in range(M)], dtype=torch.float32)


def worst(got, want):
    """(largest |got - want| over the finite entries of the float64 ``want``, its largest finite |value|); infinite
    entries must agree exactly."""
    got, fin = got.double().cpu(), torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin])
    return float((got[fin] - want[fin]).abs().max()), float(want[fin].abs().max())
