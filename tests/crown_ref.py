"""Shared by the CROWN-IBP tests: a float64 oracle in the W+ / W- and conv_transpose2d formulation (independent of the
centre / radius, gather-form reference under test), from (x, y, eps) or from a given relaxation record."""
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO

import ibp_ref as R

CONTINUOUS = ("lam", "fcb", "v", "vb", "sp", "lb_crown", "lb")
# Per-row eps of the stage cases.  ibp_ref.EPS_ROWS' last row, 1.0, makes the box the whole pixel range: every window's
# four pixels are then equal in real arithmetic, i* is decided by rounding noise in the oracle itself, and far more than
# 1 % of the units fall under the near-tie rule - 0.3 keeps a wide box without that.
EPS_ROWS = R.EPS_ROWS[:3] + (0.3,)
SKIP = 64 * R.ulp(1.0)                      # a unit whose ``gap`` is below this may choose differently


def case(M):
    x, y, _ = R.case(M)
    return x, y, torch.tensor([EPS_ROWS[i % 4] for i in range(M)], dtype=torch.float32)


def margins64(n, x, y):
    """z_y - z_j of the float64 forward (inference semantics) at the rows ``x``."""
    P = R._P(n)
    h = F.relu(F.conv2d(x.double().view(-1, 1, 28, 28), P["conv1.weight"], P["conv1.bias"]))
    h = F.max_pool2d(F.relu(F.conv2d(h, P["conv2.weight"], P["conv2.bias"])), 2).flatten(1)
    z = F.relu(h @ P["fc1.weight"].t() + P["fc1.bias"]) @ P["fc2.weight"].t() + P["fc2.bias"]
    return z.gather(1, y[:, None]) - z


def check_record(got, want, M):
    """The discrete fields agree off the near-tie units, which are at most 1 % of a case; returns the units held."""
    hold = ~(want["gap"] < SKIP)
    assert int((~hold).sum()) <= 0.01 * M * 9216, int((~hold).sum())
    for k in ("istar", "sL"):
        assert torch.equal(got[k].cpu()[hold].double(), want[k][hold].double()), k
    return hold


def relax(l, u):
    """(sL, sU, bU) of relu over [l, u], float64."""
    un = (l < 0) & (u > 0)
    d = torch.where(un, u - l, torch.ones_like(l))
    return ((l >= 0) | (un & (u > -l))).double(), torch.where(un, u / d, (l >= 0).double()), torch.where(un, -l * u / d, 0 * l)


def windows(t):
    M = t.shape[0]
    return t.reshape(M, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(M, 9216, 4)


def forward(n, x, y, eps):
    """IBP in the lower / upper form: the box, the pre-activation bounds of conv1, conv2 and fc1, and lb_ibp."""
    P, M = R._P(n), x.shape[0]
    e = (torch.as_tensor(eps, dtype=torch.float32).expand(M).double() / R.f32(MNIST_STD))[:, None]
    x = x.double().reshape(M, 784)
    xl, xu = (x - e).clamp(min=R.f32(PIXEL_LO)).view(M, 1, 28, 28), (x + e).clamp(max=R.f32(PIXEL_HI)).view(M, 1, 28, 28)
    l1, u1 = R._affine(F.conv2d, xl, xu, P["conv1.weight"], P["conv1.bias"].view(1, -1, 1, 1))
    l2, u2 = R._affine(F.conv2d, l1.relu(), u1.relu(), P["conv2.weight"], P["conv2.bias"].view(1, -1, 1, 1))
    pl, pu = F.max_pool2d(l2.relu(), 2).flatten(1), F.max_pool2d(u2.relu(), 2).flatten(1)
    l3, u3 = R._affine(lambda a, W: a @ W.t(), pl, pu, P["fc1.weight"], P["fc1.bias"])
    return dict(xl=xl, xu=xu, l1=l1, u1=u1, l2=l2, u2=u2, pl=pl, pu=pu, l3=l3, u3=u3,
                lb_ibp=R.from_pool(n, pl, pu, y)["lb"])


def record(l2, u2):
    """The pooled relaxation record, and ``gap``: per unit the oracle's smallest deciding difference (i*, dominant,
    the sign tests and u > -l of pixel i*) over the window's largest |bound| - a unit below 64 ulps may differ."""
    lw, uw = windows(l2), windows(u2)
    top = lw.topk(2, dim=2).values
    istar = (lw == top[..., :1]).double().argmax(dim=2)                         # the first argmax
    hot = F.one_hot(istar, 4).bool()
    ls, us, U = lw.gather(2, istar[..., None])[..., 0], uw.gather(2, istar[..., None])[..., 0], uw.max(dim=2).values
    others = (ls[..., None] - uw).masked_fill(hot, float("inf"))
    dom = (others >= 0).all(dim=2)
    sL, sU, bU = relax(ls, us)
    sU, bU = torch.where(dom, sU, 0 * sU), torch.where(dom, bU, U)
    sL, sU, bU = (torch.where(U <= 0, 0 * t, t) for t in (sL, sU, bU))
    tie = top[..., 0] - top[..., 1]
    tie = tie.masked_fill(tie == 0, float("inf"))       # an exact tie (equal inputs, equal arithmetic): the first wins
    gap = torch.stack((tie, others.abs().min(dim=2).values, ls.abs(), us.abs(), (us + ls).abs(),
                       U.abs())).min(dim=0).values / torch.maximum(lw.abs(), uw.abs()).max(dim=2).values
    return dict(sL=sL, sU=sU, bU=bU, istar=istar, gap=gap)


split = lambda A: (A.clamp(min=0), A.clamp(max=0))                                             # noqa: E731


def fc_part(n, l3, u3, y):
    """(lam [M, 16, 128], fcb [M, 10]) from fc1's pre-activation bounds."""
    P, y = R._P(n), y.long()
    keep = torch.ones(len(y), 10, dtype=torch.bool)
    keep[torch.arange(len(y)), y] = False
    Ap, An = split((P["fc2.weight"][y][:, None, :] - P["fc2.weight"][None]) * keep[..., None])
    sL, sU, bU = (t[:, None].double() for t in relax(l3.double(), u3.double()))
    lam = Ap * sL + An * sU
    return F.pad(lam, (0, 0, 0, 6)), (P["fc2.bias"][y][:, None] - P["fc2.bias"]) * keep + (An * bU).sum(dim=2) + lam @ P["fc1.bias"]


def pool_part(n, lam, rec):
    """(v [M, 10, 9216], vb [M, 576, 10]) from lam and the pooled record (of any dtype)."""
    P, M = R._P(n), lam.shape[0]
    Ap, An = split(lam.double()[:, :10] @ P["fc1.weight"])
    sL, sU, bU = (rec[k].double()[:, None] for k in ("sL", "sU", "bU"))
    v = Ap * sL + An * sU
    tb = An * bU + v * P["conv2.bias"].repeat_interleave(144)
    return v, tb.view(M, 10, 576, 16).sum(dim=3).transpose(1, 2)


def trunk_part(n, f, v, istar):
    """sp [M, 7, 10, 2] from the rows v, each window's i*, the box and conv1's bounds of ``f``."""
    P, M = R._P(n), v.shape[0]
    dense = (v.double()[..., None] * F.one_hot(istar.long(), 4)[:, None]).reshape(M * 10, 64, 12, 12, 2, 2)
    dense = dense.permute(0, 1, 2, 4, 3, 5).reshape(M * 10, 64, 24, 24)
    Ap, An = split(F.conv_transpose2d(dense, P["conv2.weight"]).view(M, 10, 32, 26, 26))
    sL, sU, bU = (t[:, None] for t in relax(f["l1"], f["u1"]))
    A1 = Ap * sL + An * sU
    t1 = (An * bU + A1 * P["conv1.bias"].view(1, 1, 32, 1, 1)).sum(dim=(2, 4))                   # by conv1 row
    Ap, An = split(F.conv_transpose2d(A1.view(M * 10, 32, 26, 26), P["conv1.weight"]).view(M, 10, 28, 28))
    t0 = (Ap * f["xl"] + An * f["xu"]).sum(dim=3)                                                # by input row
    return torch.stack((t0.view(M, 10, 7, 4).sum(dim=3), F.pad(t1, (0, 2)).view(M, 10, 7, 4).sum(dim=3)), dim=3).transpose(1, 2)


def head_part(fcb, vb, sp, lb_ibp, y):
    lbc = fcb.double() + vb.double().sum(dim=1) + sp.double().sum(dim=(1, 3))
    lbc[torch.arange(len(y)), y.long()] = float("inf")
    return lbc, torch.maximum(lbc, lb_ibp.double())


def backward(n, f, rec, y):
    """The backward pass from the forward bounds ``f`` and the record ``rec``: the stages of ``crown_ibp_reference``."""
    lam, fcb = fc_part(n, f["l3"], f["u3"], y)
    v, vb = pool_part(n, lam, rec)
    sp = trunk_part(n, f, v, rec["istar"])
    lbc, lb = head_part(fcb, vb, sp, f["lb_ibp"], y)
    return dict(lam=lam, fcb=fcb, v=v, vb=vb, sp=sp, lb_crown=lbc, lb=lb)


def oracle(n, x, y, eps, rec=None):
    """The whole float64 bound at (x, y, eps): every stage, the record and its ``gap``; ``rec``: the backward pass
    from this record instead of the oracle's own."""
    f = forward(n, x, y, eps)
    own = record(f["l2"], f["u2"])
    return dict(f, **own, **backward(n, f, own if rec is None else rec, y))
