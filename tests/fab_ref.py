"""Shared by the FAB tests (tests/test_fab_cpu.py, tests/test_gpu_fab.py): the float64 numpy oracle of the projection
and of the step, written per image from the definitions (a loop over the sorted breakpoints - not the torch reference's
sort / cumsum form) with its deliberate mistakes, the operands, the hand-made images and the comparator."""
import functools

import numpy as np
import torch

from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk

from attr_ref import trained_net
from deepfool_ref import trained_case

f32 = lambda v: float(np.float32(v))                                                  # noqa: E731
LO, HI, ALPHA_MAX, ETA, BETA = PIXEL_LO, PIXEL_HI, 0.1, 1.05, 0.9
PAR = (ALPHA_MAX, ETA, BETA, LO, HI)
ULP = 2.0 ** -23
NORMS = ("linf", "l2")
STEPS = 20                                                   # iterations of the end-to-end runs
MUTATIONS = ("no_sort", "wrong_room", "swapped_c", "r2_no_shift", "alpha_uncapped", "best_on_ge", "back_towards_x")
KEYS = ("x", "x_best", "norm_best", "status", "iters", "proj")


def pnorm(t, norm):
    return np.abs(t).max() if norm == "linf" else np.sqrt(np.square(t).sum())


def project(w, v, r, norm, variant=None, lo=LO, hi=HI):
    """(delta, g_inf): P(v, r) of one image in float64 and g(inf) = sum a room, walking the sorted breakpoints."""
    lo, hi = f32(lo), f32(hi)
    a, d = np.abs(w), -np.sign(r) * np.sign(w)
    up = (d < 0) if variant == "wrong_room" else (d > 0)
    room = np.maximum(np.where(up, hi - v, v - lo), 0.0)
    c = a if (norm == "l2") != (variant == "swapped_c") else np.ones_like(a)
    act = np.flatnonzero(a > 0)
    order = act if variant == "no_sort" else act[np.argsort(room[act] / c[act], kind="stable")]
    S = np.cumsum((a * c)[order][::-1])[::-1]
    R, tau = 0.0, np.inf
    for k, e in enumerate(order):
        if R + (room[e] / c[e]) * S[k] >= abs(r):
            tau = (abs(r) - R) / S[k]
            break
        R += a[e] * room[e]
    delta = np.zeros_like(w)
    delta[act] = d[act] * np.minimum(tau * c[act], room[act])
    return delta, float((a * room).sum())


def step_one(g, loss, y, x0, x, x_best, norm_best, status, iters, norm, last=False, variant=None):
    """One image's FAB round in float64: the dict of ``KEYS`` plus ``l`` (the chosen class or -1) and ``g_inf`` (the
    g(inf) of the two projections)."""
    am, eta, beta, lo, hi = (f32(v) for v in PAR)
    out = dict(x=x, x_best=x_best, norm_best=norm_best, status=status, iters=iters, proj=np.zeros((2, 784)), l=-1)
    if status != 0:
        return out
    others = [k for k in range(10) if k != y]
    if any(loss[k] < loss[y] or (loss[k] == loss[y] and k < y) for k in others):
        u = pnorm(x - x0, norm)
        if u < norm_best or (variant == "best_on_ge" and u >= norm_best):
            out.update(x_best=x, norm_best=u)
        if u == 0:
            out["status"] = 1
        elif not last:
            moved = x + beta * (x0 - x) if variant == "back_towards_x" else x0 + beta * (x - x0)
            out.update(x=np.clip(moved, lo, hi), iters=iters + 1)
        return out
    if last:
        return out
    w = g[y][None, :] - g
    n = np.abs(w).sum(axis=1) if norm == "linf" else np.sqrt(np.square(w).sum(axis=1))
    with np.errstate(all="ignore"):
        ratio = (np.abs(loss[y] - loss) + f32(Fk.DF_SLACK)) / n
    l = -1
    for k in others:
        if not np.isnan(ratio[k]) and not n[k] < Fk.PGD_L2_TINY and (l < 0 or ratio[k] < ratio[l]):
            l = k
    if l < 0:
        if np.isnan(ratio[others]).any():
            out.update(x=np.full(784, np.nan), proj=np.full((2, 784), np.nan), iters=iters + 1)
        else:
            out["status"] = 2
        return out
    r1 = loss[y] - loss[l]
    r2 = r1 if variant == "r2_no_shift" else r1 + float((w[l] * (x0 - x)).sum())
    (d1, g1), (d2, g2) = project(w[l], x, r1, norm, variant), project(w[l], x0, r2, norm, variant)
    n1, n2 = pnorm(d1, norm), pnorm(d2, norm)
    al = n1 / (n1 + n2) if n1 + n2 > 0 else 0.0
    al = al if variant == "alpha_uncapped" else min(al, am)
    x_new = np.clip((1 - al) * (x + eta * d1) + al * (x0 + eta * d2), lo, hi)
    out.update(x=x_new, iters=iters + 1, proj=np.stack([d1, d2]), l=l, g_inf=(g1, g2), r=(r1, r2))
    return out


def step_images(ops, norm, last=False, variant=None):
    """``step_one`` over the images of the operand dict: float64 tensors of ``KEYS`` plus ``l`` and the list ``raw``."""
    M = ops["y"].numel()
    n64 = lambda k: ops[k].double().numpy()                                          # noqa: E731
    g, loss = n64("dx").reshape(M, 10, 784), n64("loss").reshape(M, 10)
    raw = [step_one(g[i], loss[i], int(ops["y"][i]), n64("x0")[i], n64("x")[i], n64("x_best")[i],
                    float(ops["norm_best"][i]), int(ops["status"][i]), int(ops["iters"][i]), norm, last, variant)
           for i in range(M)]
    out = {k: torch.from_numpy(np.stack([np.asarray(o[k], dtype=np.float64) for o in raw])) for k in KEYS}
    out.update(l=torch.tensor([o["l"] for o in raw]), raw=raw)
    return out


def reference_step(ops, norm, dtype=torch.float32, last=False):
    """``ops.functional.fab_step_reference`` on the operand dict, as a dict of ``KEYS``."""
    t = lambda k: ops[k].to(dtype)                                                    # noqa: E731
    got = Fk.fab_step_reference(t("dx"), t("loss"), ops["y"], t("x0"), t("x"), t("x_best"), t("norm_best"),
                                ops["status"], ops["iters"], *PAR, norm, last=last)
    return dict(zip(KEYS, got))


def _blank(M, x0, x):
    return {"x0": x0, "x": x, "x_best": torch.zeros(M, 784), "norm_best": torch.full((M,), float("inf")),
            "status": torch.zeros(M, dtype=torch.int32), "iters": torch.arange(M, dtype=torch.int32) % 5}


@functools.lru_cache(maxsize=None)
def operands(M):
    """Random operands of one ``fab_step`` launch of ``M`` images in mid-run, none crossed: gradient scales 1e-6 ..
    1e2 per image, class k's gradient m_k times the scale with m a permutation of 1 .. 9 and every |f_k| = 30 x the
    scale (the ratios of an image are an eighth apart at least, and |r| stays far below g(inf) / 2); a third of x's
    pixels exactly on lo, a twentieth on hi, the rest within 0.05 of x0; 40 pixels where every w is exactly 0."""
    rng = np.random.default_rng(2000 + M)
    scale = 10.0 ** rng.uniform(-6, 2, M)
    if M >= 2:
        scale[0], scale[-1] = 1e-6, 1e2
    y = np.arange(M) % 10
    dx = np.empty((M, 10, 784), dtype=np.float32)
    loss = np.empty((M, 10), dtype=np.float32)
    for i in range(M):
        m = np.ones(10)
        m[np.arange(10) != y[i]] = rng.permutation(9) + 1.0
        dx[i] = rng.standard_normal((10, 784)) * (scale[i] * m[:, None])
        dx[i, y[i]] *= 0.1
        dx[i][:, rng.choice(784, 40, replace=False)] = 0.0
        loss[i] = 0.1 + 30.0 * scale[i]
        loss[i, y[i]] = 0.1
    x0 = rng.uniform(LO, HI, (M, 784)).astype(np.float32)
    x = np.clip(x0 + rng.uniform(-0.05, 0.05, (M, 784)), LO, HI).astype(np.float32)
    where = rng.uniform(size=(M, 784))
    x[where < 1 / 3], x0[where < 1 / 6] = np.float32(LO), np.float32(LO)
    x[where > 0.95] = np.float32(HI)
    ops = _blank(M, torch.from_numpy(x0), torch.from_numpy(x))
    ops.update(dx=torch.from_numpy(dx).view(10 * M, 784), loss=torch.from_numpy(loss).view(10 * M),
               y=torch.from_numpy(y.astype(np.int32)))
    return ops


HAND = ("crossed_nearer", "crossed_farther", "clean_misclassified", "misses_box", "x_is_x0", "r_zero", "zero_class",
        "all_zero", "both_clamps", "nan_in_g_y", "nan_in_unchosen", "frozen", "plain")


@functools.lru_cache(maxsize=None)
def hand_cases():
    """One launch of len(HAND) hand-made images (image i is the case HAND[i]) on a coarse binary grid: many w are
    exactly 0 and many breakpoints equal.  y = 3 throughout.  Never modified."""
    M, y, at = len(HAND), 3, HAND.index
    rng = np.random.default_rng(78)
    grid = lambda *shape: (rng.integers(-8, 9, shape) / 16.0).astype(np.float32)      # noqa: E731
    dx = np.stack([grid(10, 784) for _ in range(M)])
    loss = np.tile(np.float32(1.0) + np.arange(10, dtype=np.float32) * np.float32(0.25), (M, 1))
    loss[:, y] = 0.5                                                     # y is the smallest: not crossed
    x0 = np.float32(0.5) + grid(M, 784) / 8
    x = x0 + grid(M, 784) / 16
    ops = _blank(M, torch.from_numpy(x0), torch.from_numpy(x))
    ops["iters"][:] = 0
    for name in ("crossed_nearer", "crossed_farther", "clean_misclassified"):
        loss[at(name), 1] = 0.25                                         # loss_1 < loss_y
    ops["norm_best"][at("crossed_farther")] = 2.0 ** -10
    ops["x_best"][at("crossed_farther")] = 0.25
    x[at("clean_misclassified")] = x0[at("clean_misclassified")]
    dx[at("misses_box")] /= 65536.0                                      # g(inf) far below |f|: every element to its bound
    x[at("x_is_x0")] = x0[at("x_is_x0")]
    loss[at("r_zero"), 7] = 0.5                                          # == with k > y: not crossed, f_7 = 0, l = 7
    i = at("zero_class")                                                 # w_0 = 0 with the smallest |f|: skipped
    dx[i, 0], loss[i, 0] = dx[i, y], 0.5625
    dx[at("all_zero")] = dx[at("all_zero"), y]                           # every w_k = 0: stuck
    dx[at("both_clamps")] /= 896.0                                       # g(inf) just above |f|: both clamps bind
    dx[at("nan_in_g_y"), y, 100] = np.nan
    i = at("nan_in_unchosen")                                            # class 9 has the largest |f|: never chosen
    dx[i], x0[i], x[i] = dx[at("plain")], x0[at("plain")], x[at("plain")]
    dx[i, 9, 5] = np.nan
    i = at("frozen")
    ops["status"][i], ops["iters"][i], ops["norm_best"][i] = 1, 4, 0.0
    ops.update(dx=torch.from_numpy(dx).view(10 * M, 784), loss=torch.from_numpy(loss).view(10 * M),
               y=torch.full((M,), y, dtype=torch.int32))
    return ops


def check_step(got, ops, norm, last=False):
    """Hold the results ``got`` (a dict of ``KEYS``, CPU tensors) to the float64 oracle: status and iters equal, the
    same NaN / inf pattern, every other element of x, x_best, norm_best and proj within the launch's cap of that
    output - 8 x the largest deviation of the float32 CPU reference from the oracle, not below 4 float32 ulps of the
    largest oracle value.  Returns the largest deviation / cap per output.  Raises AssertionError."""
    want, ref = step_images(ops, norm, last), reference_step(ops, norm, torch.float32, last)
    worst = {}
    for k in KEYS:
        a, b, c = got[k].double(), want[k], ref[k].double()
        if k in ("status", "iters"):
            assert torch.equal(a, b), (k, a, b)
            continue
        fin = torch.isfinite(b)
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~fin & ~torch.isnan(b)], b[~fin & ~torch.isnan(b)]), k
        if fin.any():
            eps = max(8.0 * float((c - b)[fin].abs().max()), 4.0 * ULP * float(b[fin].abs().max()))
            dev = float((a - b)[fin].abs().max())
            assert dev <= eps, (k, dev, eps)
            worst[k] = dev / eps if eps > 0 else 0.0
    return worst


@functools.lru_cache(maxsize=None)
def cpu_fab(norm):
    """``Predictor.fab`` of the CPU reference on ``deepfool_ref.trained_case``, ``STEPS`` iterations: computed once."""
    imgs, labels = trained_case()
    return Predictor(trained_net()).fab(imgs, labels, norm, steps=STEPS)
