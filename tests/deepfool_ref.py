"""Shared by the DeepFool tests (tests/test_deepfool_cpu.py, tests/test_gpu_deepfool.py): the step written out per
image (the torch stand-in for the kernel, with its deliberate mistakes), the random operands, the hand-made images,
the comparator that holds a result to the float64 oracle, and the sixty-four images of the end-to-end tests."""
import functools

import numpy as np
import torch

from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk

from attr_ref import trained_net

LO, HI, OVERSHOOT = PIXEL_LO, PIXEL_HI, 0.02
ULP = 2.0 ** -23
MUTATIONS = ("last_minimum", "no_slack", "n_not_n2", "w_sign", "overshoot_on_step", "frozen_rewritten", "tie_k_gt_y",
             "zero_norm_kept")
KEYS = ("r_tot", "x", "status", "iters", "norm")


def step_one(g, loss, y, x0, r_tot, x, status, iters, norm, overshoot=OVERSHOOT, lo=LO, hi=HI, variant=None):
    """One image's DeepFool step, spelled out with a Python loop over the classes, in the dtype of ``g`` ([10, 784]).
    Returns ``(r_tot, x, status, iters, norm, l)``, ``l`` the chosen class or -1.  ``variant`` names a deliberate
    mistake (``MUTATIONS``)."""
    dt = g.dtype
    keep = (r_tot, x, status, iters, norm, -1)
    if status != 0:
        if variant == "frozen_rewritten":
            return (r_tot, x0.clone(), status, iters + 1, norm, -1)
        return keep
    slack = torch.tensor(0.0 if variant == "no_slack" else float(np.float32(Fk.DF_SLACK)), dtype=dt)
    for k in range(10):
        tie = (k > y) if variant == "tie_k_gt_y" else (k < y)
        if k != y and (loss[k] < loss[y] or (loss[k] == loss[y] and tie)):
            return (r_tot, x, 1, iters, norm, -1)
    l, l_nan, best, w_all = -1, -1, None, (g[y][None, :] - g) if variant != "w_sign" else (g - g[y][None, :])
    n2_all = w_all.square().sum(dim=1)
    for k in range(10):
        if k == y:
            continue
        n = n2_all[k].sqrt()
        ratio = ((loss[y] - loss[k]).abs() + slack) / n
        if ratio != ratio:
            l_nan = k if l_nan < 0 else l_nan
        elif (variant == "zero_norm_kept" or not n < Fk.PGD_L2_TINY) and \
                (l < 0 or (ratio <= best if variant == "last_minimum" else ratio < best)):
            l, best = k, ratio
    l = l_nan if l < 0 else l
    if l < 0:
        return (r_tot, x, 2, iters, norm, -1)
    num = (loss[y] - loss[l]).abs() + slack
    scale = num / (n2_all[l].sqrt() if variant == "n_not_n2" else n2_all[l])
    os1 = torch.tensor(1.0, dtype=dt) + torch.tensor(float(np.float32(overshoot)), dtype=dt)
    if variant == "overshoot_on_step":
        r_new = r_tot + os1 * (scale * w_all[l])
        x_new = (x0 + r_new).clamp(float(np.float32(lo)), float(np.float32(hi)))
    else:
        r_new = r_tot + scale * w_all[l]
        x_new = (x0 + os1 * r_new).clamp(float(np.float32(lo)), float(np.float32(hi)))
    return (r_new, x_new, 0, iters + 1, (x_new - x0)[None, :].square().sum(dim=1).sqrt()[0], l)


def step_images(ops, dtype=torch.float32, variant=None):
    """``step_one`` over the images of the operand dict ``ops`` (``operands`` / ``hand_cases``): a dict of the
    five results (``KEYS``) plus ``l`` [M]."""
    M = ops["y"].numel()
    g, loss = ops["dx"].to(dtype).view(M, 10, 784), ops["loss"].to(dtype).view(M, 10)
    out = [step_one(g[i], loss[i], int(ops["y"][i]), ops["x0"][i].to(dtype), ops["r_tot"][i].to(dtype),
                    ops["x"][i].to(dtype), int(ops["status"][i]), int(ops["iters"][i]), ops["norm"][i].to(dtype),
                    variant=variant) for i in range(M)]
    return {"r_tot": torch.stack([o[0] for o in out]), "x": torch.stack([o[1] for o in out]),
            "status": torch.tensor([o[2] for o in out], dtype=torch.int32),
            "iters": torch.tensor([o[3] for o in out], dtype=torch.int32),
            "norm": torch.stack([torch.as_tensor(o[4], dtype=dtype) for o in out]),
            "l": torch.tensor([o[5] for o in out])}


def reference_step(ops, dtype=torch.float32):
    """``ops.functional.deepfool_step_reference`` on the operand dict, as a dict of the five results."""
    got = Fk.deepfool_step_reference(ops["dx"].to(dtype), ops["loss"].to(dtype), ops["y"], ops["x0"].to(dtype),
                                     ops["r_tot"].to(dtype), ops["x"].to(dtype), ops["status"], ops["iters"],
                                     ops["norm"].to(dtype), OVERSHOOT, LO, HI)
    return dict(zip(KEYS, got))


def _blank(M, x0):
    return {"x0": x0, "r_tot": torch.zeros(M, 784), "x": x0.clone(), "status": torch.zeros(M, dtype=torch.int32),
            "iters": torch.zeros(M, dtype=torch.int32), "norm": torch.zeros(M)}


@functools.lru_cache(maxsize=None)
def operands(M, seed=0):
    """Random operands of one ``deepfool_step`` launch of ``M`` images in mid-run: gradient scales 1e-6 .. 1e2 (log
    uniform per image), y = (i + seed) % 10 with loss_y the smallest (not crossed), the other losses 0.5 + 0.3 * a
    permutation of 0 .. 8 above it (the ratios of an image are then far apart: ``ratio_gap``), a non-zero r_tot of
    the size of a step, x0 uniform in the box.  Never modified."""
    rng = np.random.default_rng(1000 * M + seed)
    scale = 10.0 ** rng.uniform(-6, 2, (M, 1, 1))
    if M >= 2:
        scale[0], scale[-1] = 1e-6, 1e2
    dx = (rng.standard_normal((M, 10, 784)) * scale).astype(np.float32)
    y = (np.arange(M) + seed) % 10
    loss = np.empty((M, 10), dtype=np.float32)
    for i in range(M):
        base = rng.uniform(0.01, 0.2)
        loss[i, y[i]] = base
        loss[i, np.arange(10) != y[i]] = base + 0.5 + 0.3 * rng.permutation(9) + rng.uniform(0, 0.05, 9)
    x0 = rng.uniform(LO, HI, (M, 784)).astype(np.float32)
    r = (rng.standard_normal((M, 784)) / (40.0 * 28.0 * scale[:, 0])).astype(np.float32)
    ops = _blank(M, torch.from_numpy(x0))
    ops.update(dx=torch.from_numpy(dx).view(10 * M, 784), loss=torch.from_numpy(loss).view(10 * M),
               y=torch.from_numpy(y.astype(np.int32)), r_tot=torch.from_numpy(r),
               iters=torch.arange(M, dtype=torch.int32) % 5, norm=torch.full((M,), 0.25))
    return ops


def ratio_gap(ops):
    """float64 [M]: (second smallest - smallest) / smallest of the float64 oracle's ratios of each image."""
    M = ops["y"].numel()
    g, loss = ops["dx"].double().view(M, 10, 784), ops["loss"].double().view(M, 10)
    gaps = []
    for i in range(M):
        y = int(ops["y"][i])
        w = g[i, y][None, :] - g[i]
        r = ((loss[i, y] - loss[i]).abs() + float(np.float32(Fk.DF_SLACK))) / w.square().sum(dim=1).sqrt()
        r = r[torch.arange(10) != y].sort().values
        gaps.append(float((r[1] - r[0]) / r[0]))
    return torch.tensor(gaps, dtype=torch.float64)


HAND = ("crossed", "equal_loss_k_below_y", "equal_loss_k_above_y", "identical_twins", "mirrored_tie", "zero_class",
        "all_unselectable", "both_clamps", "nan_in_g_y", "nan_in_unchosen", "frozen", "plain")


@functools.lru_cache(maxsize=None)
def hand_cases():
    """One launch of len(HAND) hand-made images (image i is the case HAND[i]); values on a coarse binary grid where
    a case needs exact arithmetic.  y = 3 throughout.  Never modified."""
    M, y = len(HAND), 3
    rng = np.random.default_rng(77)
    grid = lambda *shape: (rng.integers(-8, 9, shape) / 16.0).astype(np.float32)      # noqa: E731
    dx = np.stack([grid(10, 784) for _ in range(M)])
    loss = np.tile(np.float32(1.0) + np.arange(10, dtype=np.float32) * np.float32(0.25), (M, 1))
    loss[:, y] = 0.5                                                     # y is the smallest: not crossed
    x0 = np.full((M, 784), 0.5, dtype=np.float32) + grid(M, 784) / 8
    ops = _blank(M, torch.from_numpy(x0))
    at = HAND.index
    loss[at("crossed"), 1] = 0.25                                        # loss_1 < loss_y
    loss[at("equal_loss_k_below_y"), 1] = 0.5                            # == with k < y: crossed
    loss[at("equal_loss_k_above_y"), 7] = 0.5                            # == with k > y: not crossed; f_7 = 0 exactly
    i = at("identical_twins")                                            # classes 2 and 6 alike and nearest: 2 wins
    dx[i, 6], loss[i, 2], loss[i, 6] = dx[i, 2], 0.625, 0.625
    i = at("mirrored_tie")                                               # w_6 = -w_2 exactly: the same n2, the same
    dx[i, 6], loss[i, 2], loss[i, 6] = 2 * dx[i, y] - dx[i, 2], 0.625, 0.625      # ratio, opposite steps: 2 wins
    i = at("zero_class")                                                 # w_0 = 0 with the smallest |f|: skipped
    dx[i, 0], loss[i, 0] = dx[i, y], 0.5625
    dx[at("all_unselectable")] = dx[at("all_unselectable"), y]           # every w_k = 0: stuck
    i = at("both_clamps")                                                # a long step: both clamps bind
    dx[i] /= 1024.0
    i = at("nan_in_g_y")
    dx[i, y, 100] = np.nan
    i = at("nan_in_unchosen")                                            # class 9 has the largest |f|: never chosen
    dx[i] = dx[at("plain")]
    dx[i, 9, 5] = np.nan
    x0[i] = x0[at("plain")]
    i = at("frozen")
    ops["status"][i], ops["iters"][i], ops["norm"][i] = 1, 4, 0.75
    ops["r_tot"][i] = torch.from_numpy(grid(784))
    ops["x"][i] = ops["x0"][i] + ops["r_tot"][i]
    ops["x0"] = torch.from_numpy(x0)
    ops["x"] = torch.where((ops["status"] == 0)[:, None], ops["x0"], ops["x"])
    ops.update(dx=torch.from_numpy(dx).view(10 * M, 784), loss=torch.from_numpy(loss).view(10 * M),
               y=torch.full((M,), y, dtype=torch.int32))
    return ops


def tolerances(ops):
    """(oracle, eps, eps_image): the float64 oracle's results and the caps of r_tot / x / norm by the project's
    rule: 8 x the largest deviation of the same formula in torch float32 on the CPU from the oracle, not below 4
    float32 ulps of the largest oracle value - ``eps`` taken over the whole launch (one number per output),
    ``eps_image`` over each image's elements alone ([M] per output)."""
    want, f32 = reference_step(ops, torch.float64), reference_step(ops, torch.float32)
    eps, eps_image = {}, {}
    for k in ("r_tot", "x", "norm"):
        a, b = want[k].reshape(want[k].shape[0], -1), f32[k].double().reshape(want[k].shape[0], -1)
        dev = torch.nan_to_num((a - b).abs(), nan=0.0, posinf=0.0).max(dim=1).values
        top = torch.nan_to_num(a.abs(), nan=0.0, posinf=0.0).max(dim=1).values
        eps_image[k] = torch.maximum(8.0 * dev, 4.0 * ULP * top)
        eps[k] = max(8.0 * float(dev.max()), 4.0 * ULP * float(top.max()))
    return want, eps, eps_image


def check_step(got, ops):
    """Hold the results ``got`` (a dict of ``KEYS``, CPU tensors) of the launch ``ops`` to the float64 oracle: status
    and iters equal, the same NaN pattern, and every other element of r_tot, x and norm within the launch's cap of
    that output (``tolerances``).  r_tot and norm are held to their image's own cap as well.  x is not: where a long
    step and r_tot cancel, an element of x is the small remainder of operands a thousand times its size, a few
    elements of an image escape both clamps, and what the CPU's float32 run deviates on those few says little about
    another float32 summation order - the per-image figure of x is returned, not asserted.  Returns the largest
    deviation / cap per output: ``r_tot``, ``x``, ``norm`` over the launch, and ``r_tot_image``, ``x_image``,
    ``norm_image`` against the images' own caps.  Raises AssertionError."""
    want, eps, eps_image = tolerances(ops)
    M = ops["y"].numel()
    worst = {}
    for i in range(M):
        assert int(got["status"][i]) == int(want["status"][i]), ("status", i, int(got["status"][i]))
        assert int(got["iters"][i]) == int(want["iters"][i]), ("iters", i, int(got["iters"][i]))
        for k in ("r_tot", "x", "norm"):
            a, b = got[k][i].double().reshape(-1), want[k][i].reshape(-1)
            nan = b != b
            assert torch.equal(a != a, nan), (k, i, "NaN pattern")
            dev = float((a - b)[~nan].abs().max()) if (~nan).any() else 0.0
            assert dev <= eps[k], (k, i, dev, eps[k])
            cap = float(eps_image[k][i])
            assert k == "x" or dev <= cap, (k, i, dev, cap, "the image's own cap")
            worst[k] = max(worst.get(k, 0.0), dev / eps[k] if eps[k] > 0 else 0.0)
            worst[k + "_image"] = max(worst.get(k + "_image", 0.0), dev / cap if cap > 0 else 0.0)
    return worst


@functools.lru_cache(maxsize=None)
def trained_case():
    """(uint8 images [64, 28, 28], labels [64]): the first 64 images of generate(256, seed=5) that the trained test
    net classifies correctly on the CPU.  Never modified."""
    imgs, labels = generate(256, seed=5)
    idx = (Predictor(trained_net()).predict(imgs) == labels.long()).nonzero()[:64, 0]
    assert idx.numel() == 64
    return imgs[idx].contiguous(), labels[idx].contiguous()


@functools.lru_cache(maxsize=None)
def cpu_minimum_norm():
    """``Predictor.minimum_norm`` of the CPU reference on ``trained_case``, steps = 50: computed once."""
    imgs, labels = trained_case()
    return Predictor(trained_net()).minimum_norm(imgs, labels, steps=50)
