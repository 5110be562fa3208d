"""What the EAD tests share: ``ead_step`` evaluated in numpy float64, the operand cases of the kernel tests and the
CPU reference run of the end-to-end comparison (computed once, never modified)."""
import functools

import numpy as np
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk

import deepfool_ref as D

LO, HI = PIXEL_LO, PIXEL_HI
LR, C_INIT, BETA, STEPS = 0.01, 1.0, 0.01, 30
KINDS = ("first", "plain", "search_end", "last")
ROWS = ("y", "x", "x_best")
GAP_ULPS = 64
_f = lambda s: float(np.float32(s))                                                              # noqa: E731


def _z64(a, c, sign, kappa, k):
    """float64 (z, act) of the ISTA step on the float64 operands ``a`` with the per-image constants ``c``."""
    s2 = _f(MNIST_STD * MNIST_STD)
    lr_k, _ = Fk.ead_schedule(k, STEPS, LR)
    act = sign * a["loss"][:c.shape[0]] < _f(kappa)
    gx = 2 * s2 * (a["y"] - a["x0"]) - (sign * c * act)[:, None] * a["dx"]
    return a["y"] - (lr_k / s2) * gx, act


def step64(ops, sign, kappa, k, search, kind, rule):
    """The header block of csrc/kernels/ead.hip on the float32 operands ``ops`` in float64: a dict of the new y, x,
    x_best [M, 784], fstate [M, 4] (float64), istate [M, 4], and for a plain launch ``branch`` [M, 784] (1 / -1: shrunk
    from above / below, 0: back on the clean pixel) and ``gap`` [M, 784]: ||z - x0| - beta_n| in float32 ulps of |z|."""
    a = {n: np.asarray(v.numpy(), dtype=np.float64) for n, v in ops.items() if n != "istate"}
    lo, hi, kap, std, s2 = _f(LO), _f(HI), _f(kappa), _f(MNIST_STD), _f(MNIST_STD * MNIST_STD)
    beta, bn = _f(BETA), Fk.ead_beta_n(BETA)
    x0, x, y, M = a["x0"], a["x"], a["y"], a["x"].shape[0]
    Lx = sign * a["loss"][M:]
    if kind == "first":
        c, c_lo, c_hi = np.full(M, _f(C_INIT)), np.zeros(M), np.full(M, _f(Fk.CW_C_INF))
        d_best, xb = np.full(M, np.inf), x0.copy()
        succ, found, iters, spare = (np.zeros(M, dtype=np.int64) for _ in range(4))
    else:
        c, c_lo, c_hi, d_best = a["fstate"].T.copy()
        succ, found, iters, spare = ops["istate"].numpy().astype(np.int64).T.copy()
        xb = a["x_best"].copy()
    l1 = std * np.abs(x - x0).sum(axis=1)
    dist = l1 if rule == "l1" else s2 * ((x - x0) ** 2).sum(axis=1) + beta * l1
    ok = (Lx > 0) & (Lx >= kap)
    imp = ok & (dist < d_best)
    succ, d_best, found = np.where(ok, 1, succ), np.where(imp, dist, d_best), np.where(imp, search + 1, found)
    xb[imp] = x[imp]
    extra = {}
    if kind == "search_end":
        s, big = succ > 0, _f(Fk.CW_C_BIG)
        hi_s, lo_f = np.minimum(c_hi, c), np.maximum(c_lo, c)
        c_s = np.where(hi_s < big, (c_lo + hi_s) * 0.5, c)
        c_f = np.where(c_hi < big, (lo_f + c_hi) * 0.5, c * 10)
        c, c_lo, c_hi, succ = np.where(s, c_s, c_f), np.where(s, c_lo, lo_f), np.where(s, hi_s, c_hi), 0 * succ
        x, y = x0, x0
    elif kind != "last":
        z, _ = _z64(a, c, sign, kappa, k)
        d = z - x0
        branch = np.where(d > bn, 1, np.where(d < -bn, -1, 0))
        xn = np.where(branch > 0, np.minimum(z - bn, hi), np.where(branch < 0, np.maximum(z + bn, lo), x0))
        y, x = xn + Fk.ead_schedule(k, STEPS, LR)[1] * (xn - x), xn
        iters = iters + 1
        extra = dict(branch=branch, gap=np.abs(np.abs(d) - bn) / np.spacing(np.abs(z).astype(np.float32)).astype(np.float64))
    return dict(y=y, x=x, x_best=xb, fstate=np.stack((c, c_lo, c_hi, d_best), axis=1),
                istate=np.stack((succ, found, iters, spare), axis=1), **extra)


def make_case(M, sign, kappa, kind, rule, k=4, seed=0):
    """float32 operands of one launch on M images, no decision on a near-tie: 70 % of x0 exactly at LO (MNIST's
    background), 5 % at HI; x = x0 on 70 % of the pixels (the shrinkage's fixed point), y = x plus a momentum-sized
    offset on half of them, not clamped; L_y and L_x (``loss`` [2 M]: the y rows, then the x rows) cycle through values
    at least 1e-2 from 0 and from kappa; the stored d_best is +inf, 0.5 x or 2 x the float64 distance; succ and c_hi
    (CW_C_INF / below CW_C_BIG) both ways.  Elements whose float64 |z - x0| comes within 4 GAP_ULPS float32 ulps of |z|
    of beta_n have their gradient and slack offset redrawn until none is left, so float32 and float64 take the same branch at every element
    and none is excluded."""
    g = torch.Generator().manual_seed(1000 * M + seed)
    r = lambda *s: torch.rand(*s, generator=g)                                                # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)                                               # noqa: E731
    i = torch.arange(M)
    u = r(M, 784)
    x0 = torch.where(u < 0.7, torch.full((), LO), torch.where(u < 0.75, torch.full((), HI), LO + (HI - LO) * r(M, 784)))
    if kind == "first":
        x, y = x0.clone(), x0.clone()
    else:
        x = torch.where(r(M, 784) < 0.7, x0, (x0 + 0.4 * n(M, 784)).clamp(LO, HI))
        y = torch.where(r(M, 784) < 0.5, x, x + 0.05 * n(M, 784))
    Ly = torch.tensor([-1.3, 0.2, 0.9, -0.02])[i % 4] * (1 + 0.01 * r(M))
    Lx = torch.tensor([0.9, -0.4, 0.2, 1.7, -0.02])[i % 5] * (1 + 0.01 * r(M))
    l1 = MNIST_STD * (x.double() - x0.double()).abs().sum(1)
    dist = l1 if rule == "l1" else MNIST_STD ** 2 * (x.double() - x0.double()).square().sum(1) + _f(BETA) * l1
    d_best = torch.where(i % 3 == 0, torch.full((), float("inf"), dtype=torch.float64), dist * torch.where(i % 3 == 1, 0.5, 2.0))
    c = 0.5 + 20 * r(M)
    unset = (i // 8) % 2 == 0
    fstate = torch.stack((c, torch.where(unset, torch.zeros(()), 0.5 * c),
                          torch.where(unset, torch.full((), Fk.CW_C_INF), 2 * c), d_best.float()), dim=1)
    istate = torch.stack(((i // 4) % 2, i % 3, 7 + i, torch.full_like(i, 5)), dim=1).to(torch.int32)
    ops = dict(dx=0.05 * n(M, 784), loss=(sign * torch.cat((Ly, Lx))).float(), x0=x0, y=y, x=x,
               x_best=LO + (HI - LO) * r(M, 784), fstate=fstate.contiguous(), istate=istate.contiguous())
    if kind in ("first", "plain"):
        cc = np.full(M, _f(C_INIT)) if kind == "first" else fstate[:, 0].double().numpy()
        for _ in range(20):
            a = {q: ops[q].double().numpy() for q in ("dx", "loss", "x0", "y")}
            z, _ = _z64(a, cc, sign, kappa, k)
            near = np.abs(np.abs(z - a["x0"]) - Fk.ead_beta_n(BETA)) < 4 * GAP_ULPS * np.spacing(np.abs(z).astype(np.float32))
            if not near.any():
                break
            near = torch.from_numpy(near)
            ops["dx"][near] = 0.05 * n(int(near.sum()))
            if kind == "plain":                  # (an image whose hinge is off does not see its gradient)
                ops["y"][near] = ops["x"][near] + 0.05 * n(int(near.sum()))
    return ops


def reference32(ops, sign, kappa, k, search, kind, rule):
    """``ead_step_reference`` (torch float32, on the device of ``ops``) on a case: the same dict as ``step64``."""
    st = (ops["y"], ops["x"]) + ((None,) * 3 if kind == "first" else (ops["x_best"], ops["fstate"], ops["istate"]))
    out = Fk.ead_step_reference(ops["dx"], ops["loss"], ops["x0"], *st, sign, kappa, LR, C_INIT, BETA, k, STEPS, search,
                                LO, HI, rule, first=kind == "first", search_end=kind == "search_end", last=kind == "last")
    return dict(zip(ROWS + ("fstate", "istate"), out))


@functools.lru_cache(maxsize=None)
def cpu_elastic_net(n=64, rule="l1", beta=BETA, search_steps=3, steps=30):
    """``Predictor.elastic_net`` of the CPU reference on the first ``n`` images of ``deepfool_ref.trained_case`` with
    image 1 given a wrong label (outside its label on entry): ``(labels, (x_adv, radii, log_probs, found))``."""
    imgs, labels = D.trained_case()
    labels = labels[:n].clone()
    labels[1] = (labels[1] + 1) % 10
    return labels, Predictor(D.trained_net()).elastic_net(imgs[:n], labels, search_steps=search_steps, steps=steps,
                                                          beta=beta, decision_rule=rule)


def check_invariants(x, labels, out, clean_pred):
    """What every ``elastic_net`` result satisfies exactly (``x``: the float32 [B, 784] clean rows)."""
    xa, radii, lp, found = (q.cpu() for q in out)
    B = x.shape[0]
    xa = xa.reshape(B, 784)
    assert (xa >= LO).all() and (xa <= HI).all()
    want = (xa.double() - x.double()).abs().sum(1) * MNIST_STD
    fin = torch.isfinite(radii)
    assert ((radii.double() - want).abs()[fin] <= 1e-5 * want[fin]).all()
    assert torch.equal(xa[~fin], x[~fin]) and not found[~fin].any() and (radii[~fin] == float("inf")).all()
    assert (radii[clean_pred != labels] == 0).all()
    assert torch.equal(found, lp.argmax(1) != labels) and found[fin].all()
