"""What the Carlini-Wagner tests share: ``cw_step`` evaluated in numpy float64, the operand cases of the kernel tests
and the CPU reference run of the end-to-end comparison (computed once, never modified)."""
import functools

import numpy as np
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk

import deepfool_ref as D

LO, HI = PIXEL_LO, PIXEL_HI
LR, C_INIT = 0.05, 1.0
KINDS = ("first", "plain", "search_end", "last")
ROWS = ("w", "m1", "v", "x", "x_best")
_f = lambda s: float(np.float32(s))                                                              # noqa: E731


def step64(ops, sign, kappa, t, search, kind):
    """The header block of csrc/kernels/cw.hip on the float32 operands ``ops`` in float64: a dict of the new w, m1, v,
    x, x_best [M, 784], fstate [M, 4] (float64) and istate [M, 4]."""
    a = {k: np.asarray(v.numpy(), dtype=np.float64) for k, v in ops.items() if k != "istate"}
    lo, hi, kap = _f(LO), _f(HI), _f(kappa)
    x0, x, M = a["x0"], a["x"], a["x"].shape[0]
    L = sign * a["loss"]
    w0 = np.arctanh((((x0 - lo) / (hi - lo)) * 2 - 1) * _f(Fk.CW_SHRINK))
    if kind == "first":
        c, c_lo, c_hi = np.full(M, _f(C_INIT)), np.zeros(M), np.full(M, _f(Fk.CW_C_INF))
        d_best, xb = np.full(M, np.inf), x0.copy()
        succ, found, iters, spare = (np.zeros(M, dtype=np.int64) for _ in range(4))
        w, m1, v = w0, np.zeros_like(x0), np.zeros_like(x0)
    else:
        c, c_lo, c_hi, d_best = a["fstate"].T.copy()
        succ, found, iters, spare = ops["istate"].numpy().astype(np.int64).T.copy()
        w, m1, v, xb = a["w"], a["m1"], a["v"], a["x_best"].copy()
    Dn = ((x - x0) ** 2).sum(axis=1)
    ok = (L > 0) & (L >= kap)
    imp = ok & (Dn < d_best)
    succ, d_best, found = np.where(ok, 1, succ), np.where(imp, Dn, d_best), np.where(imp, search + 1, found)
    xb[imp] = x[imp]
    if kind == "search_end":
        s, big = succ > 0, _f(Fk.CW_C_BIG)
        hi_s, lo_f = np.minimum(c_hi, c), np.maximum(c_lo, c)
        c_s = np.where(hi_s < big, (c_lo + hi_s) * 0.5, c)
        c_f = np.where(c_hi < big, (lo_f + c_hi) * 0.5, c * 10)
        c, c_lo, c_hi, succ = np.where(s, c_s, c_f), np.where(s, c_lo, lo_f), np.where(s, hi_s, c_hi), 0 * succ
        w, m1, v, x = w0, np.zeros_like(x0), np.zeros_like(x0), x0
    elif kind != "last":
        b1, b2 = _f(Fk.CW_BETA1), _f(Fk.CW_BETA2)
        bc1, bc2 = Fk.cw_bias_corrections(t)
        th = np.tanh(w)
        gx = 2 * _f(MNIST_STD * MNIST_STD) * (x - x0) - (sign * c * (L < kap))[:, None] * a["dx"]
        gw = gx * (0.5 * (hi - lo) * (1 - th * th))
        m1, v = b1 * m1 + (1 - b1) * gw, b2 * v + (1 - b2) * gw * gw
        w = w - _f(LR) * (m1 / bc1) / (np.sqrt(v / bc2) + _f(Fk.CW_ADAM_EPS))
        x = np.clip(lo + (hi - lo) * (0.5 * (np.tanh(w) + 1)), lo, hi)
        iters = iters + 1
    return dict(w=w, m1=m1, v=v, x=x, x_best=xb, fstate=np.stack((c, c_lo, c_hi, d_best), axis=1),
                istate=np.stack((succ, found, iters, spare), axis=1))


def make_case(M, sign, kappa, kind, seed=0):
    """float32 operands of one launch on M images, no decision on a near-tie: about 70 % of x0 exactly at LO (MNIST's
    background, where w0 and 1 - th^2 are extreme); L = sign * loss cycles through values at least 1e-2 from 0 and
    from kappa; the stored d_best is +inf, 0.5 x or 2 x the float64 D; succ and c_hi (CW_C_INF / below CW_C_BIG) both
    ways."""
    g = torch.Generator().manual_seed(1000 * M + seed)
    r = lambda *s: torch.rand(*s, generator=g)                                                # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)                                               # noqa: E731
    i = torch.arange(M)
    x0 = torch.where(r(M, 784) < 0.7, torch.full((), LO), LO + (HI - LO) * r(M, 784))
    w = Fk.cw_w0(x0, LO, HI) + 0.3 * n(M, 784)
    x = x0.clone() if kind == "first" else (LO + (HI - LO) * (0.5 * (torch.tanh(w) + 1))).clamp(LO, HI)
    L = torch.tensor([-1.3, 0.2, 0.9, -0.02])[i % 4] * (1 + 0.01 * r(M))
    D64 = (x.double() - x0.double()).square().sum(1)
    d_best = torch.where(i % 3 == 0, torch.full((), float("inf"), dtype=torch.float64), D64 * torch.where(i % 3 == 1, 0.5, 2.0))
    c = 0.5 + 20 * r(M)
    unset = (i // 8) % 2 == 0
    fstate = torch.stack((c, torch.where(unset, torch.zeros(()), 0.5 * c),
                          torch.where(unset, torch.full((), Fk.CW_C_INF), 2 * c), d_best.float()), dim=1)
    istate = torch.stack(((i // 4) % 2, i % 3, 7 + i, torch.full_like(i, 5)), dim=1).to(torch.int32)
    return dict(dx=0.05 * n(M, 784), loss=(sign * L).float(), x0=x0, w=w, m1=0.01 * n(M, 784), v=1e-4 * r(M, 784), x=x,
                x_best=LO + (HI - LO) * r(M, 784), fstate=fstate.contiguous(), istate=istate.contiguous())


def reference32(ops, sign, kappa, t, search, kind):
    """``cw_step_reference`` (torch float32, on the device of ``ops``) on a case: the same dict as ``step64``."""
    st = (None,) * 3 + (ops["x"],) + (None,) * 3 if kind == "first" else \
        (ops["w"], ops["m1"], ops["v"], ops["x"], ops["x_best"], ops["fstate"], ops["istate"])
    out = Fk.cw_step_reference(ops["dx"], ops["loss"], ops["x0"], *st, sign, kappa, LR, C_INIT, t, search, LO, HI,
                               first=kind == "first", search_end=kind == "search_end", last=kind == "last")
    return dict(zip(ROWS + ("fstate", "istate"), out))


@functools.lru_cache(maxsize=None)
def cpu_carlini_wagner(search_steps=3, steps=30):
    """``Predictor.carlini_wagner`` of the CPU reference on ``deepfool_ref.trained_case`` with image 1 given a wrong
    label (outside its label on entry): ``(labels, (x_adv, radii, log_probs, found))``, computed once."""
    imgs, labels = D.trained_case()
    labels = labels.clone()
    labels[1] = (labels[1] + 1) % 10
    return labels, Predictor(D.trained_net()).carlini_wagner(imgs, labels, search_steps=search_steps, steps=steps)


def check_invariants(x, labels, out, clean_pred):
    """What every ``carlini_wagner`` result satisfies exactly (``x``: the float32 [B, 784] clean rows)."""
    xa, radii, lp, found = (q.cpu() for q in out)
    B = x.shape[0]
    xa = xa.reshape(B, 784)
    assert (xa >= LO).all() and (xa <= HI).all()
    want = (xa.double() - x.double()).square().sum(1).sqrt() * MNIST_STD
    fin = torch.isfinite(radii)
    assert ((radii.double() - want).abs()[fin] <= 1e-5 * want[fin]).all()
    assert torch.equal(xa[~fin], x[~fin]) and not found[~fin].any() and (radii[~fin] == float("inf")).all()
    assert (radii[clean_pred != labels] == 0).all()
    assert torch.equal(found, lp.argmax(1) != labels) and found[fin].all()
