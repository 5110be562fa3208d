"""Inference with a trained ``Net``: ``Predictor`` and the ``mnist_predict.py`` command line.

``Predictor.from_checkpoint("mnist_cnn.pt")`` loads any of the three checkpoint variants the
reference writes (``utils/checkpoint.py``; weights-only loading); ``Predictor(net)`` wraps a live
``Net`` and follows its parameters (the bf16 shadows the kernels read are refreshed whenever a
parameter's version counter moved, as ``Net.forward`` on the GPU does).

Dispatch of one batch of B images:

* GPU, ``dtype="bf16"``, B <= ``INFER_FUSED_MAX_B``: the single-launch fused forward
  (``csrc/kernels/infer_fwd.hip`` through ``ops.functional.infer_forward``; the constant is 0 as
  measured, see below);
* GPU, ``dtype="bf16"``, larger B: the three-launch eval chain (``ops.chain.EvalChain``), as the
  trainer's per-epoch eval runs it;
* CPU, or ``dtype="fp32"``: ``Net.forward_reference`` (stock torch ops) in eval mode under ``no_grad``.

``Predictor.input_gradient`` (saliency, adversarial examples) returns the gradient of the summed NLL
wrt the normalised image, in the same inference semantics (no dropout):

* GPU, ``dtype="bf16"``: the fused forward in its training form with dropout switched off by flag,
  ``head_train`` + ``fc_bwd`` for the dy records, then one launch of ``csrc/kernels/input_grad.hip``
  (``ops.fused_net.fused_input_gradient``); no conv weight gradient is computed;
* CPU, or ``dtype="fp32"``: torch autograd over ``Net.forward_reference`` in eval mode.

The other methods split the same way.  On the GPU with ``dtype="bf16"`` each runs a native loop over the launch
chains of ``ops/chain.py`` (no autograd, no per-step allocation, no host sync; the loop's module lists its launches);
on the CPU, or with ``dtype="fp32"``, the same formula in torch ops over autograd through ``Net.forward_reference``
in eval mode (where noise is drawn: the same distribution, not the same bits):

* ``adversarial`` / ``robust_evaluate`` (L-inf or L2 FGSM / PGD, untargeted or targeted; ``eps`` and ``step_size`` in
  pixel units on the [0, 1] scale): ``ops.attack.fused_adversarial`` / ``reference_adversarial``; the returned
  log-probabilities are the predictor's own forward (above) of the adversarial images;
* ``auto_pgd`` / ``robust_evaluate_apgd`` (Auto-PGD, Croce & Hein 2020: PGD without a step size to tune; the same
  norms, units and targeted form): ``ops.apgd.fused_auto_pgd`` / ``reference_auto_pgd``; it takes
  ``loss="cw"`` / ``"dlr"`` (the CW margin, the DLR loss and its targeted form) in the NLL's place, and
  ``robust_evaluate_ensemble`` counts the images that survive APGD-CE, targeted APGD-DLR and the Square Attack;
* ``square_attack`` / ``robust_evaluate_square`` (the L-inf Square Attack, Andriushchenko et al. 2020: score-based and
  black-box, it reads log-probabilities only; the same units; here both paths draw the same Philox bits):
  ``ops.square.fused_square_attack`` / ``reference_square_attack``;
* ``smoothed_counts`` / ``certify`` (randomized smoothing: the class counts of Gaussian-noised copies of an image and
  the certified L2 radius they give; ``sigma`` in pixel units): ``ops.smooth.fused_smooth_counts`` / ``torch.randn``
  over the reference forward; the certificate itself (``ops.smooth.certify_from_counts``) is host code on either path;
* ``minimum_norm`` (L2 DeepFool: the smallest perturbation that leaves the class, per image; radii in pixel units):
  ``ops.deepfool.fused_minimum_norm`` / ``reference_minimum_norm``;
* ``attribute`` (integrated gradients and SmoothGrad of log p_y(x): n gradient rows per image, reduced; ``sigma`` and
  scalar baselines in pixel units): ``ops.attribute.fused_attribution`` / ``reference_attribution``.

There is no fallback between them: a GPU predictor without the native extension raises.
"""
from __future__ import annotations

import argparse
import contextlib
import json

import torch
import torch.nn.functional as F

from .data.datasets import MNIST_MEAN, MNIST_STD, PIXEL_HI, PIXEL_LO, load_mnist  # noqa: F401
from .data.datasets import PIXEL_LUT as _PIXEL_LUT
from .models.net import Net
from .ops.chain import chain_loss
from .ops.functional import (APGD_LOSS_BEST, DF_CLASSES, PGD_L2_TINY, SQUARE_DONE, SQUARE_QUERIES, apgd_checkpoints,
                             apgd_step_reference, attr_path_reference, attr_reduce_reference, deepfool_step_reference,
                             margin_loss_reference, pgd_l2_step_reference, square_init_reference, square_sides,
                             square_state_margin, square_step_reference)
from .utils.checkpoint import load_state_dict
from .utils.logging import test_line

# Largest batch the fused single-launch kernel serves; above it the three-launch path runs.  Taken
# from tools/infer_bench.py's table (profiles/infer/infer_bench.txt, docs/PERF_NOTES.md): as measured,
# the three-launch path is faster at every batch size, B = 1 included (16.9 against 21.1 us), so the
# Predictor never dispatches to the fused kernel until that changes.
INFER_FUSED_MAX_B = 0


@contextlib.contextmanager
def _eval_mode(net: Net):
    """``net`` in eval mode (no dropout) inside the block; its mode is restored afterwards."""
    was_training = net.training
    net.eval()
    try:
        yield
    finally:
        net.train(was_training)


def _loss_rows_fn(name: str, loss: str, targeted: bool, labels: torch.Tensor, true_labels):
    """log-probs [B, 10] -> the per-row loss [B] ``reference_auto_pgd`` ascends (``targeted``: descend): the NLL of
    ``labels``, or the margin loss ``chain_loss`` names - targeted "dlr": of ``true_labels`` towards ``labels``."""
    kind = chain_loss(name, loss, targeted)
    if kind == "ce":
        return lambda lp: F.nll_loss(lp, labels.long(), reduction='none')
    if kind == "dlr_t":
        if true_labels is None:
            raise ValueError(f"{name}: the targeted DLR loss needs true_labels")
        return lambda lp: margin_loss_reference(lp, true_labels.to(lp.device), "dlr_t", labels)
    return lambda lp: margin_loss_reference(lp, labels, kind)


def reference_adversarial(net: Net, x0: torch.Tensor, labels: torch.Tensor, eps: float, steps: int,
                          step_size: float, lo: float, hi: float, x_init: torch.Tensor | None = None,
                          norm: str = "linf", targeted: bool = False) -> torch.Tensor:
    """``ops.attack.fused_adversarial`` in torch ops on any device: ``steps`` projected gradient steps on the
    summed NLL of ``labels`` through autograd over ``Net.forward_reference`` in eval mode (no dropout; the
    net's mode is restored afterwards), from ``x_init`` (default ``x0``).  Same arguments (float32 [B, 784]
    normalised images, normalised units), same formula, same return.  The CPU / fp32 path of
    ``Predictor.adversarial`` and of adversarial training on the module engine."""
    B = x0.shape[0]
    x_adv = x0 if x_init is None else x_init
    alpha_s = -step_size if targeted else step_size
    with _eval_mode(net):
        for _ in range(int(steps)):
            xg = x_adv.clone().requires_grad_()
            with torch.enable_grad():
                lp = net.forward_reference(xg.view(B, 1, 28, 28))
                loss = F.nll_loss(lp, labels, reduction='sum')
                g, = torch.autograd.grad(loss, xg)
            if norm == "l2":
                x_adv = pgd_l2_step_reference(g, x_adv, x0, eps, alpha_s, lo, hi)
            else:
                t = x_adv + alpha_s * g.sign()
                t = torch.min(torch.max(t, x0 - eps), x0 + eps)
                x_adv = t.clamp(lo, hi)
    return x_adv


def reference_auto_pgd(net: Net, x0: torch.Tensor, labels: torch.Tensor, eps: float, steps: int, lo: float,
                       hi: float, x_init: torch.Tensor | None = None, norm: str = "linf", targeted: bool = False,
                       loss: str = "ce", true_labels: torch.Tensor | None = None):
    """``ops.apgd.fused_auto_pgd`` in torch float32 on any device: the same ``steps + 1`` rounds - the per-row NLL of
    ``labels`` and its gradient by autograd over ``Net.forward_reference`` in eval mode (no dropout; the net's mode
    is restored afterwards), then ``apgd_step_reference`` with the same ``first`` / ``last`` flags and the windows
    of ``apgd_checkpoints``.  Same arguments (float32 [B, 784] normalised images, normalised units), same return:
    ``(x_best [B, 784], loss_best [B])``, the loss as the NLL of ``labels`` - with ``loss`` "cw" / "dlr" the margin
    loss of ``margin_loss_reference`` on the log-probs instead, throughout.  The CPU / fp32 path of
    ``Predictor.auto_pgd`` and the reference of its GPU tests."""
    if steps < 1:
        raise ValueError("reference_auto_pgd: steps must be at least 1")
    B, steps = x0.shape[0], int(steps)
    x0 = x0.detach().reshape(B, 784).to(torch.float32)
    y = labels.reshape(B).long().to(x0.device)
    window = dict(apgd_checkpoints(steps))
    sign = -1 if targeted else 1
    loss_of = _loss_rows_fn("reference_auto_pgd", loss, targeted, y, true_labels)
    state = ((x0 if x_init is None else x_init.detach().reshape(B, 784).to(torch.float32)).clone(),
             None, None, None, None, None)
    with _eval_mode(net):
        for j in range(steps + 1):
            xg = state[0].clone().requires_grad_()
            with torch.enable_grad():
                lp = net.forward_reference(xg.view(B, 1, 28, 28))
                g, = torch.autograd.grad(loss_of(lp).sum(), xg)
            loss_rows = loss_of(lp.detach())
            state = apgd_step_reference(g, loss_rows, x0, *state, sign, eps, lo, hi, norm=norm, first=j == 0,
                                        last=j == steps, window=window.get(j, 0))
    loss_best = state[4][:, APGD_LOSS_BEST]
    return state[2], (-loss_best if targeted else loss_best.clone())


def reference_square_attack(net: Net, x0: torch.Tensor, labels: torch.Tensor, eps: float, queries: int, lo: float,
                            hi: float, p_init: float = 0.8, seed: int = 0, ids=None, targeted: bool = False,
                            check_every: int = 64):
    """``ops.square.fused_square_attack`` in torch float32 on any device: the same ``queries`` rounds - the
    log-probabilities of the candidates from ``Net.forward_reference`` in eval mode under ``no_grad`` (the net's mode
    is restored afterwards), then ``square_step_reference`` with the same ``first`` / ``last`` flags, query indices
    and ``square_sides`` - with the same Philox draws (``ops.philox``).  Same arguments (float32 [B, 784] normalised
    images, normalised units), same return: ``(x_best [B, 784], margin_best [B], queries_used int32 [B])``.
    ``check_every`` = k > 0 stops once every image is broken, looked at every k queries; the result does not depend
    on it.  The CPU / fp32 path of ``Predictor.square_attack`` and the reference of its GPU tests."""
    queries, check_every = int(queries), int(check_every)
    if queries < 1 or queries >= 1 << 32:
        raise ValueError("reference_square_attack: queries must be in [1, 2**32)")
    if check_every < 0:
        raise ValueError(f"reference_square_attack: check_every must be >= 0, got {check_every}")
    sides = square_sides(p_init, queries)
    B = x0.shape[0]
    x0 = x0.detach().reshape(B, 784).to(torch.float32)
    y = labels.reshape(B).to(x0.device, torch.int32)
    ids = list(range(B)) if ids is None else [int(v) for v in ids]
    if len(ids) != B:
        raise ValueError(f"reference_square_attack: {len(ids)} ids for {B} images")
    x_cand = square_init_reference(x0, eps, lo, hi, seed, ids)
    x_best = state = None
    with _eval_mode(net), torch.no_grad():
        for j in range(queries):
            last = j == queries - 1
            lp = net.forward_reference(x_cand.view(B, 1, 28, 28))
            x_best, x_cand, state = square_step_reference(lp, y, x0, x_best, x_cand, state, eps, lo, hi, seed, j + 1,
                                                          1 if last else sides[j], ids, first=j == 0, last=last,
                                                          targeted=targeted)
            if check_every and (j + 1) % check_every == 0 and bool((state[:, SQUARE_DONE] != 0).all()):
                break
    return x_best, square_state_margin(state), state[:, SQUARE_QUERIES].clone()


ATTRIBUTION_METHODS = ("integrated_gradients", "smoothgrad")
_REF_ROWS = 1000                   # rows per forward / backward (and per generator draw) of the torch paths


def reference_minimum_norm(net: Net, x0: torch.Tensor, labels: torch.Tensor, steps: int, overshoot: float,
                           lo: float, hi: float):
    """``ops.deepfool.fused_minimum_norm`` in torch float32 on any device: L2 DeepFool with the kernel's formulas
    (``deepfool_step_reference``: the same selection rule, slack, skip rule and freezing), the ten class gradients
    and losses of an image from one autograd pass over ``Net.forward_reference`` in eval mode on its ten rows,
    labelled 0 .. 9 (the net's mode is restored afterwards).  ``x0``: float32 [B, 784] normalised images; same
    return: ``(x_adv [B, 784], norm [B], iters int32 [B], status int32 [B])``.  The images run in chunks of
    ``_REF_ROWS`` // 10, each until no image of it is still running or ``steps`` iterations are made.  The CPU /
    fp32 path of ``Predictor.minimum_norm`` and the reference of its GPU tests."""
    B, dev = x0.shape[0], x0.device
    x0 = x0.detach().reshape(B, 784).to(torch.float32)
    y = labels.reshape(B).long().to(dev)
    x_adv, norm = x0.clone(), torch.zeros(B, dtype=torch.float32, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    mc = _REF_ROWS // DF_CLASSES
    with _eval_mode(net):
        for i0 in range(0, B, mc):
            c0, yc = x0[i0:i0 + mc], y[i0:i0 + mc]
            m = c0.shape[0]
            lab10 = torch.arange(DF_CLASSES, device=dev).repeat(m)
            state = (torch.zeros_like(c0), c0.clone(), status[i0:i0 + m], iters[i0:i0 + m], norm[i0:i0 + m])
            for _ in range(int(steps)):
                rows = state[1].repeat_interleave(DF_CLASSES, dim=0).requires_grad_()
                with torch.enable_grad():
                    lp = net.forward_reference(rows.view(DF_CLASSES * m, 1, 28, 28))
                    g, = torch.autograd.grad(F.nll_loss(lp, lab10, reduction='sum'), rows)
                loss_rows = -lp.detach()[torch.arange(DF_CLASSES * m, device=dev), lab10]
                state = deepfool_step_reference(g, loss_rows, yc, c0, *state, overshoot, lo, hi)
                if not bool((state[2] == 0).any()):
                    break
            x_adv[i0:i0 + m], status[i0:i0 + m], iters[i0:i0 + m], norm[i0:i0 + m] = state[1:]
    return x_adv, norm, iters, status


def _smooth_generator_seed(seed: int, image_id: int) -> int:
    """The seed of an image's ``torch.Generator`` on the torch paths of ``smoothed_counts`` and SmoothGrad."""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(image_id)) & (2 ** 63 - 1)


def reference_attribution(net: Net, x0: torch.Tensor, labels: torch.Tensor, method: str, n: int, base=0.0,
                          sigma_n: float = 0.0, seed: int = 0, ids=None) -> torch.Tensor:
    """``ops.attribute.fused_attribution`` in torch ops on any device: float32 [B, 784] attribution of
    log p_labels(x0), with g = d NLL / d x by autograd over ``Net.forward_reference`` in eval mode (the net's mode
    is restored afterwards):

        "integrated_gradients":  -(x0 - b) * (1/n) * sum_s g(b + alpha_s (x0 - b)),  alpha_s = (s + 1/2) / n
        "smoothgrad":            -(1/n) * sum_s g(x0 + sigma_n z_s)

    ``x0``: float32 [B, 784] normalised images; ``base``: a float or float32 [B, 784] (normalised units).  The
    path rows, the sum in ascending s, the scale float32(-1/n) and the product are ``attr_path_reference`` /
    ``attr_reduce_reference``: the arithmetic of the kernels.  Image j is processed alone, ``_REF_ROWS`` rows at a
    time; its SmoothGrad noise is ``torch.randn`` from a generator seeded by ``seed`` and ``ids[j]`` (default j)
    as ``Predictor.smoothed_counts`` seeds it: the same distribution as the GPU path, not the same bits.  The CPU /
    fp32 path of ``Predictor.attribute`` and the reference of its GPU tests."""
    import numpy as np
    if method not in ATTRIBUTION_METHODS:
        raise ValueError(f"reference_attribution: method must be one of {ATTRIBUTION_METHODS}, got {method!r}")
    path = method == "integrated_gradients"
    B, n, dev = x0.shape[0], int(n), x0.device
    xc = x0.detach().to("cpu", torch.float32).reshape(B, 784)
    bc = base.detach().to("cpu", torch.float32).reshape(B, 784) if isinstance(base, torch.Tensor) else None
    lab = labels.reshape(B).long().to(dev)
    scale = float(np.float32(-1.0) / np.float32(n))
    out = torch.empty(B, 784, dtype=torch.float32)
    gen = torch.Generator()
    with _eval_mode(net):
        for j in range(B):
            bj = float(base) if bc is None else bc[j:j + 1]
            if not path:
                gen.manual_seed(_smooth_generator_seed(seed, j if ids is None else ids[j]))
            acc = None
            for s0 in range(0, n, _REF_ROWS):
                ns = min(_REF_ROWS, n - s0)
                if path:
                    rows = torch.from_numpy(attr_path_reference(xc[j:j + 1], n, s0, ns, bj))
                else:
                    rows = xc[j] + sigma_n * torch.randn(ns, 784, generator=gen, dtype=torch.float32)
                xg = rows.to(dev).requires_grad_()
                with torch.enable_grad():
                    lp = net.forward_reference(xg.view(ns, 1, 28, 28))
                    g, = torch.autograd.grad(F.nll_loss(lp, lab[j].expand(ns), reduction='sum'), xg)
                last = s0 + ns == n
                acc = attr_reduce_reference(g, 1, ns, acc, scale if last else None,
                                            xc[j:j + 1] if path and last else None, bj)
            out[j] = torch.from_numpy(acc[0])
    return out.to(dev)


def normalised_pixel(value: float) -> float:
    """The pixel value ``value`` on the [0, 1] scale in normalised units, in float32 arithmetic (a scalar baseline)."""
    import numpy as np
    return float((np.float32(value) - np.float32(MNIST_MEAN)) / np.float32(MNIST_STD))


def _rows_f32(x: torch.Tensor, B: int, device) -> torch.Tensor:
    """Detached contiguous float32 [B, 784] normalised rows on ``device`` of uint8 images (through the pixel LUT:
    the kernels' normalisation, bit for bit, wherever ``x`` lives) or of float, already-normalised input."""
    if x.dtype == torch.uint8:
        x = _PIXEL_LUT.to(x.device)[x.reshape(B, 784).long()]
    return x.detach().reshape(B, 784).to(device, torch.float32).contiguous()


def _ids(name: str, ids, B: int):
    """``ids`` (None, a tensor or a sequence) as None or a list of ``B`` ints."""
    if ids is None:
        return None
    ids = [int(v) for v in (ids.tolist() if isinstance(ids, torch.Tensor) else ids)]
    if len(ids) != B:
        raise ValueError(f"{name}: {len(ids)} ids for {B} images")
    return ids


def adversarial_units(eps: float, steps: int, step_size: float | None):
    """(eps, step_size, lo, hi) in normalised units from pixel units on the [0, 1] scale, with
    ``Predictor.adversarial``'s default step: ``eps`` for one step, ``2.5 * eps / steps`` otherwise."""
    if step_size is None:
        step_size = eps if steps == 1 else 2.5 * eps / steps
    return eps / MNIST_STD, step_size / MNIST_STD, PIXEL_LO, PIXEL_HI


def _random_start(x0: torch.Tensor, eps_n: float, lo: float, hi: float, norm: str, generator, device) -> torch.Tensor:
    """The random start of ``Predictor.adversarial`` / ``auto_pgd`` around the float32 [B, 784] rows ``x0``, drawn
    with torch from ``generator`` (on its device, or on ``device`` without one) - L-inf: ``x0 + U(-eps, eps)``; L2:
    uniform in the ball (a normal direction scaled to radius ``eps * u^(1/784)``) - clamped to [lo, hi]."""
    B = x0.shape[0]
    draw = dict(generator=generator, dtype=torch.float32,
                device=generator.device if generator is not None else device)
    if norm == "linf":
        u = torch.rand(B, 784, **draw).to(device)
        return (x0 + (2.0 * u - 1.0) * eps_n).clamp_(lo, hi)
    g = torch.randn(B, 784, **draw).to(device)
    u = torch.rand(B, 1, **draw).to(device)
    radius = eps_n * u.pow(1.0 / 784.0)
    return (x0 + g * (radius / g.square().sum(dim=1, keepdim=True).sqrt().clamp_min(PGD_L2_TINY))).clamp_(lo, hi)


class Predictor:
    def __init__(self, net: Net, dtype: str = "bf16"):
        if dtype not in ("bf16", "fp32"):
            raise ValueError(f"dtype must be 'bf16' or 'fp32', got {dtype!r}")
        self.net = net
        self.dtype = dtype
        self.device = next(net.parameters()).device
        self.native = self.device.type == "cuda" and dtype == "bf16"
        self._infer_buf = None            # ops.functional.InferBuffers (fused path)
        self._eval_buf = None             # activation set of the three-launch path, one batch size
        if self.native:
            from .ops.fused_net import fused_state
            self._st = fused_state(net)   # owns the ModelState (flat parameters + bf16 shadows)

    @classmethod
    def from_checkpoint(cls, path: str, device=None, dtype: str = "bf16") -> "Predictor":
        if device is None:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        net = Net()
        load_state_dict(net, path, map_location="cpu")
        return cls(net.to(torch.device(device)), dtype=dtype)

    # ------------------------------------------------------------------ public API
    def log_probs(self, x: torch.Tensor) -> torch.Tensor:
        """float32 [B, 10] log-probabilities of uint8 [B,28,28] / [B,784] images or float
        [B,1,28,28] already-normalised input."""
        return self._forward(x)[0]

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """int64 [B] predicted classes."""
        return self._forward(x)[1]

    def evaluate(self, images_u8: torch.Tensor, labels: torch.Tensor, batch_size: int = 1000):
        """(loss_sum, correct, n) over uint8 images [N,28,28] / [N,784] and their labels."""
        n = int(labels.shape[0])
        if images_u8.dtype != torch.uint8 or images_u8.shape[0] != n:
            raise ValueError("evaluate: images_u8 must be uint8 with one row per label")
        if batch_size < 1:
            raise ValueError("evaluate: batch_size must be positive")
        if not self.native:
            loss_sum, correct = 0.0, 0
            lab = labels.long().to(self.device)
            for i in range(0, n, batch_size):
                lp, pred = self._forward(images_u8[i:i + batch_size])
                loss_sum += F.nll_loss(lp, lab[i:i + batch_size], reduction='sum').item()
                correct += int((pred == lab[i:i + batch_size]).sum().item())
            return loss_sum, correct, n
        u8 = images_u8.reshape(n, 784).contiguous().to(self.device)
        lab = labels.to(torch.int32).to(self.device)
        loss = torch.zeros((), dtype=torch.float64, device=self.device)
        hits = torch.zeros((), dtype=torch.int64, device=self.device)
        for i in range(0, n, batch_size):
            b = min(batch_size, n - i)
            out = self._native(b, u8=u8[i:i + b], labels=lab[i:i + b])
            loss += out.loss_rows[:b].double().sum()
            hits += out.correct[:b].sum()
        return float(loss.item()), int(hits.item()), n

    def input_gradient(self, x: torch.Tensor, labels: torch.Tensor | None = None):
        """(grad, log_probs): float32 [B,1,28,28] gradient of the summed NLL wrt the NORMALISED input
        and the float32 [B,10] log-probabilities, without dropout.  The loss is taken against ``labels``
        ([B] integers), or against the predicted class when ``labels`` is None.  ``x``: uint8
        [B,28,28] / [B,784] images (normalised first) or float [B,1,28,28] already-normalised input."""
        B = self._check_input(x)
        xf = _rows_f32(x, B, self.device)
        if labels is not None:
            labels = self._labels("input_gradient", labels, B, check_range=False)
        if self.native:
            from .ops.fused_net import fused_input_gradient
            grad, lp = fused_input_gradient(self.net, xf, labels)
            return grad.reshape(B, 1, 28, 28), lp
        xf = xf.view(B, 1, 28, 28).clone().requires_grad_()
        with _eval_mode(self.net):
            with torch.enable_grad():
                lp = self.net.forward_reference(xf)
                target = lp.detach().argmax(dim=1) if labels is None else labels
                grad, = torch.autograd.grad(F.nll_loss(lp, target, reduction='sum'), xf)
        return grad, lp.detach()

    def adversarial(self, x: torch.Tensor, labels: torch.Tensor | None = None, eps: float = 0.1, steps: int = 1,
                    step_size: float | None = None, random_start: bool = False, generator=None,
                    norm: str = "linf", targeted: bool = False):
        """(x_adv, log_probs): FGSM (``steps`` = 1) / PGD adversarial examples of ``x`` and the
        predictor's float32 [B,10] log-probabilities of them.  ``x_adv`` is float32 [B,1,28,28] in
        NORMALISED units, inside both the ``eps`` ball around ``x`` and the valid pixel range [0, 1].

        ``norm``: ``"linf"`` (signed-gradient steps, the ball is a box) or ``"l2"`` (steps of length
        ``step_size`` along the gradient, the ball is Euclidean per image).  ``eps``, ``step_size``: pixel
        units on the [0, 1] scale (L-inf: 0.1, 0.3 are usual for MNIST; L2: 1.5 to 2.0); ``step_size``
        None: ``eps`` for one step, ``2.5 * eps / steps`` otherwise.  The summed NLL against ``labels``
        ([B] integers) is ascended, or against the class predicted on the clean input when ``labels`` is
        None; ``targeted``: ``labels`` (required) are the classes to reach and their NLL is descended.
        ``random_start``: start from a point drawn with torch from ``generator`` - L-inf: ``x + U(-eps,
        eps)``; L2: uniform in the ball (a normal direction scaled to radius ``eps * u^(1/784)``) - clamped
        to the valid range.  Inference semantics as ``input_gradient``: no dropout, the net's mode,
        dropout modules and parameter gradients are untouched.  ``x``: uint8 [B,28,28] / [B,784] images
        or float [B,1,28,28] already-normalised input."""
        B = self._check_input(x)
        if norm not in ("linf", "l2"):
            raise ValueError(f"adversarial: norm must be 'linf' or 'l2', got {norm!r}")
        if targeted and labels is None:
            raise ValueError("adversarial: a targeted attack needs labels (the target classes)")
        if not eps >= 0:
            raise ValueError(f"adversarial: eps must be >= 0, got {eps}")
        if steps != int(steps) or steps < 1:
            raise ValueError(f"adversarial: steps must be a positive integer, got {steps}")
        if step_size is not None and not step_size > 0:
            raise ValueError(f"adversarial: step_size must be > 0, got {step_size}")
        x0 = _rows_f32(x, B, self.device)
        if labels is None:
            labels = self._forward(x0.view(B, 1, 28, 28))[1]
        else:
            labels = self._labels("adversarial", labels, B, check_range=True)
        eps_n, alpha_n, lo, hi = adversarial_units(eps, steps, step_size)
        x_init = _random_start(x0, eps_n, lo, hi, norm, generator, self.device) if random_start else None
        if self.native:
            from .ops.attack import fused_adversarial
            x_adv = fused_adversarial(self.net, x0, labels, eps_n, int(steps), alpha_n, lo, hi, x_init,
                                      norm=norm, targeted=targeted)
        else:
            x_adv = reference_adversarial(self.net, x0, labels, eps_n, int(steps), alpha_n, lo, hi, x_init,
                                          norm=norm, targeted=targeted)
        x_adv = x_adv.view(B, 1, 28, 28)
        return x_adv, self._forward(x_adv)[0]

    def robust_evaluate(self, images_u8: torch.Tensor, labels: torch.Tensor, eps: float, steps: int = 1,
                        step_size: float | None = None, batch_size: int = 1000, norm: str = "linf"):
        """(loss_sum, correct, n) as ``evaluate``, of the images after an untargeted L-inf or L2 (``norm``)
        attack against their true labels (``adversarial`` without a random start), ``batch_size`` images at
        a time."""
        if norm not in ("linf", "l2"):
            raise ValueError(f"robust_evaluate: norm must be 'linf' or 'l2', got {norm!r}")
        n = int(labels.shape[0])
        if images_u8.dtype != torch.uint8 or images_u8.shape[0] != n:
            raise ValueError("robust_evaluate: images_u8 must be uint8 with one row per label")
        if batch_size < 1:
            raise ValueError("robust_evaluate: batch_size must be positive")
        lab = labels.long().to(self.device)
        loss = torch.zeros((), dtype=torch.float64, device=self.device)
        hits = torch.zeros((), dtype=torch.int64, device=self.device)
        for i in range(0, n, batch_size):
            y = lab[i:i + batch_size]
            _, lp = self.adversarial(images_u8[i:i + batch_size], y, eps, steps, step_size, norm=norm)
            loss += F.nll_loss(lp, y, reduction='none').double().sum()
            hits += (lp.argmax(dim=1) == y).sum()
        return float(loss.item()), int(hits.item()), n

    def auto_pgd(self, x: torch.Tensor, labels: torch.Tensor | None = None, eps: float = 0.1, steps: int = 100,
                 norm: str = "linf", targeted: bool = False, random_start: bool = False, restarts: int = 1,
                 generator=None, loss: str = "ce", true_labels: torch.Tensor | None = None):
        """(x_adv, log_probs, loss_best): Auto-PGD (Croce & Hein 2020, the gradient attack of AutoAttack) adversarial
        examples of ``x`` - PGD with a momentum step, a per-image step size that starts at ``2 eps`` and is halved at
        scheduled checkpoints when the loss stops rising, and a restart from the best point found so far; there is
        no step size to choose.  ``x_adv``: float32 [B,1,28,28] in NORMALISED units, the point of the highest loss
        among the ``steps + 1`` iterates (``targeted``: the lowest), inside both the ``eps`` ball around ``x`` and
        the valid pixel range [0, 1]; ``log_probs``: the predictor's own float32 [B,10] forward of ``x_adv``;
        ``loss_best``: float32 [B], the chosen loss (``loss``: the NLL of ``labels`` by default) at ``x_adv`` as the
        attack's own forward computed it.

        Whether an image was broken is read from ``log_probs`` (``log_probs.argmax(1) != labels``): the attack keeps
        the highest-loss point, it has no arg-max of the iterates and so does not keep "the first misclassified
        point" apart as the authors' code does.  ``loss``: "ce" (the NLL, cross-entropy), "cw" (the CW margin
        max_{j != y} z_j - z_y on the logits) or "dlr" (the DLR loss of Croce & Hein 2020: that margin over z_pi1 -
        z_pi3, invariant to a rescaling of the logits), ascended against ``labels`` or, ``targeted``, descended towards
        them; ``targeted`` with "dlr" is the authors' APGD-T: the targeted DLR loss (z_y - z_t) / (z_pi1 - (z_pi3 +
        z_pi4) / 2), which reads ``true_labels`` ([B] integers; None: the class predicted on the clean input; no row's
        target may equal its true label), is descended (it is the negative of their objective).
        ``ops.functional.margin_loss_reference`` has the exact forms and the tie rules.

        ``norm``, ``eps`` (pixel units on the [0, 1] scale), ``labels`` (None: the class predicted on the clean
        input), ``targeted`` (``labels`` required: the classes to reach, their NLL is descended), ``random_start``
        and ``generator``: as ``adversarial``, the same draw.  ``restarts`` > 1 (needs ``random_start``): that many
        runs from consecutive draws; per image the run with the highest ``loss_best`` (``targeted``: the lowest) is
        kept, the first of equals.  Inference semantics as ``input_gradient``: no dropout; the net's mode, dropout
        modules, parameters and gradients are untouched.  GPU with ``dtype="bf16"``: the native loop
        ``ops.apgd.fused_auto_pgd``; CPU, or ``dtype="fp32"``: ``reference_auto_pgd``.  ``x``: uint8 [B,28,28] /
        [B,784] images or float [B,1,28,28] already-normalised input."""
        B = self._check_input(x)
        if norm not in ("linf", "l2"):
            raise ValueError(f"auto_pgd: norm must be 'linf' or 'l2', got {norm!r}")
        if loss not in ("ce", "cw", "dlr"):
            raise ValueError(f"auto_pgd: loss must be 'ce', 'cw' or 'dlr', got {loss!r}")
        if targeted and labels is None:
            raise ValueError("auto_pgd: a targeted attack needs labels (the target classes)")
        if not eps >= 0:
            raise ValueError(f"auto_pgd: eps must be >= 0, got {eps}")
        if isinstance(steps, bool) or steps != int(steps) or steps < 1:
            raise ValueError(f"auto_pgd: steps must be a positive integer, got {steps}")
        if isinstance(restarts, bool) or restarts != int(restarts) or restarts < 1:
            raise ValueError(f"auto_pgd: restarts must be a positive integer, got {restarts}")
        if restarts > 1 and not random_start:
            raise ValueError("auto_pgd: restarts > 1 needs random_start (every run would be the same)")
        x0 = _rows_f32(x, B, self.device)
        if labels is None:
            labels = self._forward(x0.view(B, 1, 28, 28))[1]
        else:
            labels = self._labels("auto_pgd", labels, B, check_range=True)
        true_labels = self._true_labels("auto_pgd", loss, targeted, labels, true_labels, x0, B)
        eps_n, _, lo, hi = adversarial_units(eps, int(steps), None)
        if self.native:
            from .ops.apgd import fused_auto_pgd as attack
        else:
            attack = reference_auto_pgd
        x_adv = loss_best = None
        for _ in range(int(restarts)):
            x_init = _random_start(x0, eps_n, lo, hi, norm, generator, self.device) if random_start else None
            xr, lr = attack(self.net, x0, labels, eps_n, int(steps), lo, hi, x_init, norm=norm, targeted=targeted,
                            loss=loss, true_labels=true_labels)
            if x_adv is None:
                x_adv, loss_best = xr, lr
            else:
                better = (lr < loss_best) if targeted else (lr > loss_best)
                x_adv = torch.where(better[:, None], xr, x_adv)
                loss_best = torch.where(better, lr, loss_best)
        x_adv = x_adv.view(B, 1, 28, 28)
        return x_adv, self._forward(x_adv)[0], loss_best

    def robust_evaluate_apgd(self, images_u8: torch.Tensor, labels: torch.Tensor, eps: float, steps: int = 100,
                             batch_size: int = 1000, norm: str = "linf", restarts: int = 1, generator=None,
                             loss: str = "ce"):
        """(loss_sum, correct, n) as ``robust_evaluate``, with Auto-PGD as the attack: the images after an untargeted
        ``auto_pgd`` against their true labels, ``batch_size`` images at a time; ``restarts`` > 1: that many runs
        from random starts drawn from ``generator``, else one run from the clean image.  There is no step size.
        ``loss``: the loss the attack ascends (``auto_pgd``); ``loss_sum`` is the NLL of the attacked images."""
        if norm not in ("linf", "l2"):
            raise ValueError(f"robust_evaluate_apgd: norm must be 'linf' or 'l2', got {norm!r}")
        n = int(labels.shape[0])
        if images_u8.dtype != torch.uint8 or images_u8.shape[0] != n:
            raise ValueError("robust_evaluate_apgd: images_u8 must be uint8 with one row per label")
        if batch_size < 1:
            raise ValueError("robust_evaluate_apgd: batch_size must be positive")
        lab = labels.long().to(self.device)
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        hits = torch.zeros((), dtype=torch.int64, device=self.device)
        for i in range(0, n, batch_size):
            y = lab[i:i + batch_size]
            _, lp, _ = self.auto_pgd(images_u8[i:i + batch_size], y, eps, steps, norm=norm,
                                     random_start=restarts > 1, restarts=restarts, generator=generator, loss=loss)
            total += F.nll_loss(lp, y, reduction='none').double().sum()
            hits += (lp.argmax(dim=1) == y).sum()
        return float(total.item()), int(hits.item()), n

    def square_attack(self, x: torch.Tensor, labels: torch.Tensor | None = None, eps: float = 0.3, queries: int = 1000,
                      p_init: float = 0.8, seed: int = 0, ids=None, targeted: bool = False, check_every: int = 64):
        """(x_adv, log_probs, margin, queries_used): the L-inf Square Attack (Andriushchenko, Croce, Flammarion, Hein
        2020, the score-based black-box attack of AutoAttack) on ``x`` - a random search that reads only the
        log-probabilities of its candidates, never a gradient: the cross-check of ``adversarial`` / ``auto_pgd`` on
        a net whose gradients may be masked.  ``x_adv``: float32 [B,1,28,28] in NORMALISED units, the queried point
        of the lowest margin, every pixel of it clamp(x + eps) or clamp(x - eps) into the valid range [0, 1];
        ``log_probs``: the predictor's own float32 [B,10] forward of ``x_adv``; ``margin``: float32 [B], the margin at
        ``x_adv`` as the attack's own forward gave it (log p_y - max_{j != y} log p_j; ``targeted``: the negative;
        < 0: broken); ``queries_used``: int32 [B], the forwards spent on the image until it broke (``queries`` when
        it did not).

        ``eps``: pixel units on the [0, 1] scale; ``labels``: [B] integers, or the class predicted on the clean
        input when None; ``targeted``: ``labels`` (required) are the classes to reach.  At most ``queries`` queries per
        image: query 0 is a start of vertical stripes of +-eps, every later one moves one square of the image to
        +eps or -eps and is kept when the margin drops; the square's side follows ``functional.square_sides`` from
        the share ``p_init`` of the image.  Image j draws under the id ``ids[j]`` (default j) from the Philox stream
        keyed by ``seed``: its squares depend on (seed, id, query index) alone, on the GPU and on the CPU alike.
        ``check_every``: look every that many queries whether every image is broken (0: never; the result does not
        depend on it).  The margin loss serves the targeted form too (the paper uses cross-entropy there), and the
        paper's resampling of a square that changes nothing is not made.  Inference semantics: no dropout; the
        net's mode, parameters and gradients are untouched.  GPU with ``dtype="bf16"``: the native loop
        ``ops.square.fused_square_attack``; CPU, or ``dtype="fp32"``: ``reference_square_attack``.  ``x``: uint8
        [B,28,28] / [B,784] images or float [B,1,28,28] already-normalised input."""
        B = self._check_input(x)
        if targeted and labels is None:
            raise ValueError("square_attack: a targeted attack needs labels (the target classes)")
        if not eps >= 0:
            raise ValueError(f"square_attack: eps must be >= 0, got {eps}")
        if isinstance(queries, bool) or queries != int(queries) or queries < 1:
            raise ValueError(f"square_attack: queries must be a positive integer, got {queries}")
        if not 0.0 < p_init <= 1.0:
            raise ValueError(f"square_attack: p_init must be in (0, 1], got {p_init}")
        if isinstance(check_every, bool) or check_every != int(check_every) or check_every < 0:
            raise ValueError(f"square_attack: check_every must be a non-negative integer, got {check_every}")
        ids = _ids("square_attack", ids, B)
        x0 = _rows_f32(x, B, self.device)
        if labels is None:
            labels = self._forward(x0.view(B, 1, 28, 28))[1]
        else:
            labels = self._labels("square_attack", labels, B, check_range=True)
        eps_n, _, lo, hi = adversarial_units(eps, 1, None)
        if self.native:
            from .ops.square import fused_square_attack as attack
        else:
            attack = reference_square_attack
        x_adv, margin, used = attack(self.net, x0, labels, eps_n, int(queries), lo, hi, float(p_init), int(seed), ids,
                                     targeted, int(check_every))
        x_adv = x_adv.view(B, 1, 28, 28)
        return x_adv, self._forward(x_adv)[0], margin, used

    def robust_evaluate_square(self, images_u8: torch.Tensor, labels: torch.Tensor, eps: float, queries: int = 1000,
                               batch_size: int = 1000, p_init: float = 0.8, seed: int = 0):
        """(loss_sum, correct, n, median_queries): the first three as ``robust_evaluate``, with the untargeted
        ``square_attack`` against the true labels as the attack, ``batch_size`` images at a time; an image's id is its
        row index, so its squares do not depend on ``batch_size``.  ``median_queries``: the median of
        ``queries_used`` over the images that are correct on the clean input and broken after the attack (None when
        there is none; the median of an even count is the mean of the middle two)."""
        n = int(labels.shape[0])
        if images_u8.dtype != torch.uint8 or images_u8.shape[0] != n:
            raise ValueError("robust_evaluate_square: images_u8 must be uint8 with one row per label")
        if batch_size < 1:
            raise ValueError("robust_evaluate_square: batch_size must be positive")
        lab = labels.long().to(self.device)
        loss = torch.zeros((), dtype=torch.float64, device=self.device)
        hits = torch.zeros((), dtype=torch.int64, device=self.device)
        spent = []
        for i in range(0, n, batch_size):
            y = lab[i:i + batch_size]
            clean = self._forward(images_u8[i:i + batch_size])[1] == y
            _, lp, _, used = self.square_attack(images_u8[i:i + batch_size], y, eps, queries, p_init, seed,
                                                ids=range(i, i + y.shape[0]))
            right = lp.argmax(dim=1) == y
            loss += F.nll_loss(lp, y, reduction='none').double().sum()
            hits += right.sum()
            spent.append(used[clean & ~right].double().cpu())
        spent = torch.cat(spent)
        median = float(spent.quantile(0.5)) if spent.numel() else None
        return float(loss.item()), int(hits.item()), n, median

    def robust_evaluate_ensemble(self, images_u8: torch.Tensor, labels: torch.Tensor, eps: float, steps: int = 100,
                                 n_targets: int = 9, queries: int = 5000, batch_size: int = 1000,
                                 p_init: float = 0.8, seed: int = 0):
        """(correct, n, after): the worst case over an ensemble of L-inf attacks of radius ``eps`` - how many of the
        ``n`` images are still classified correctly after all of them.  Per batch of ``batch_size`` images, each
        stage runs only on the images that are still correct (a batch with none left skips the stage):

            clean    the predictor's forward of the clean images;
            apgd_ce  ``auto_pgd`` with ``loss="ce"`` and ``steps`` updates, from the clean point;
            apgd_t   for k = 1 .. ``n_targets``: ``auto_pgd(targeted=True, loss="dlr")`` towards the k-th most likely
                     class other than the label at the clean point (ties: the lower class);
            square   ``square_attack`` with up to ``queries`` queries, ``p_init`` and ``seed``, an image's id its row
                     index in ``images_u8`` (its squares do not depend on the batch or on what broke before).

        An image is broken when the predictor's own forward of the returned point misses the label.  ``after``: a
        dict of the survivors after each stage, in the order above.  ``n_targets`` in 0..9 and ``queries`` >= 0; 0
        skips the stage.  This is not AutoAttack's standard set: FAB-T is not built, and APGD starts from the clean
        point, not from random starts."""
        n = int(labels.shape[0])
        if images_u8.dtype != torch.uint8 or images_u8.shape[0] != n:
            raise ValueError("robust_evaluate_ensemble: images_u8 must be uint8 with one row per label")
        if batch_size < 1:
            raise ValueError("robust_evaluate_ensemble: batch_size must be positive")
        if isinstance(n_targets, bool) or n_targets != int(n_targets) or not 0 <= n_targets <= 9:
            raise ValueError(f"robust_evaluate_ensemble: n_targets must be an integer in 0..9, got {n_targets}")
        if isinstance(queries, bool) or queries != int(queries) or queries < 0:
            raise ValueError(f"robust_evaluate_ensemble: queries must be a non-negative integer, got {queries}")
        if isinstance(steps, bool) or steps != int(steps) or steps < 1:
            raise ValueError(f"robust_evaluate_ensemble: steps must be a positive integer, got {steps}")
        if not eps >= 0:
            raise ValueError(f"robust_evaluate_ensemble: eps must be >= 0, got {eps}")
        lab = labels.long().to(self.device)
        after = {"clean": 0, "apgd_ce": 0, "apgd_t": 0, "square": 0}
        for i in range(0, n, batch_size):
            xb, y = images_u8[i:i + batch_size], lab[i:i + batch_size]
            rows = torch.arange(i, i + y.shape[0], device=self.device)
            lp0 = self._forward(xb)[0]
            alive = lp0.argmax(dim=1) == y
            after["clean"] += int(alive.sum())
            # the k-th most likely class other than the label: a stable descending sort with the label pushed last
            order = lp0.clone().scatter_(1, y[:, None], float("-inf")).sort(dim=1, descending=True, stable=True)[1]

            def stage(attack):
                at = alive.nonzero()[:, 0]
                if at.numel():
                    lp = attack(at)
                    alive[at] = lp.argmax(dim=1) == y[at]

            stage(lambda at: self.auto_pgd(xb[at.to(xb.device)], y[at], eps, steps, loss="ce")[1])
            after["apgd_ce"] += int(alive.sum())
            for k in range(int(n_targets)):
                stage(lambda at: self.auto_pgd(xb[at.to(xb.device)], order[at, k], eps, steps, targeted=True, loss="dlr",
                                               true_labels=y[at])[1])
            after["apgd_t"] += int(alive.sum())
            if queries > 0:
                stage(lambda at: self.square_attack(xb[at.to(xb.device)], y[at], eps, queries, p_init, seed,
                                                    ids=rows[at])[1])
            after["square"] += int(alive.sum())
        return after["square"], n, after

    def minimum_norm(self, x: torch.Tensor, labels: torch.Tensor | None = None, steps: int = 50,
                     overshoot: float = 0.02, check_every: int = 8):
        """(x_adv, radii, log_probs, found): minimum-norm adversarial examples of ``x`` by L2 DeepFool
        (Moosavi-Dezfooli, Fawzi, Frossard 2016) - how far the decision boundary is from each image.  ``x_adv``:
        float32 [B,1,28,28] in NORMALISED units, inside the valid pixel range [0, 1]; ``radii``: float32 [B], the L2
        norm of ``x_adv - x`` in pixel units on the [0, 1] scale (as every ``eps`` here); ``log_probs``: the
        predictor's own float32 [B,10] forward of ``x_adv``; ``found``: bool [B], whether that forward no longer
        gives ``labels``.  An image already misclassified on entry keeps ``x_adv = x``, radius 0 and is found.

        ``labels`` ([B] integers): the class each image is to leave, or the class predicted on the clean input when
        None.  At most ``steps`` iterations per image: each steps to the nearest boundary of the classifier
        linearised at the iterate, x_adv = clamp(x + (1 + ``overshoot``) * (the sum of the steps)); an image stops
        once the iterate has left its class.  ``check_every``: on the GPU, look every that many iterations whether
        every image has stopped (0: never; the result does not depend on it).  Inference semantics as
        ``input_gradient``: no dropout; the net's mode, parameters and gradients are untouched.  GPU with
        ``dtype="bf16"``: the native loop ``ops.deepfool.fused_minimum_norm``; CPU, or ``dtype="fp32"``:
        ``reference_minimum_norm``.  ``x``: uint8 [B,28,28] / [B,784] images or float [B,1,28,28] normalised input."""
        B = self._check_input(x)
        if isinstance(steps, bool) or steps != int(steps) or steps < 1:
            raise ValueError(f"minimum_norm: steps must be a positive integer, got {steps}")
        if not overshoot >= 0:
            raise ValueError(f"minimum_norm: overshoot must be >= 0, got {overshoot}")
        if isinstance(check_every, bool) or check_every != int(check_every) or check_every < 0:
            raise ValueError(f"minimum_norm: check_every must be a non-negative integer, got {check_every}")
        if labels is None:
            labels = self._forward(x)[1]
        else:
            labels = self._labels("minimum_norm", labels, B, check_range=True)
        if self.native:
            from .ops.deepfool import fused_minimum_norm
            x_adv, norm, _, _ = fused_minimum_norm(self.net, self._rows_native(x, B), labels, int(steps),
                                                   float(overshoot), PIXEL_LO, PIXEL_HI, int(check_every))
        else:
            x_adv, norm, _, _ = reference_minimum_norm(self.net, _rows_f32(x, B, self.device), labels, int(steps),
                                                       float(overshoot), PIXEL_LO, PIXEL_HI)
        x_adv = x_adv.view(B, 1, 28, 28)
        lp = self._forward(x_adv)[0]
        return x_adv, norm * MNIST_STD, lp, lp.argmax(dim=1) != labels

    # ------------------------------------------------------------------ randomized smoothing
    def smoothed_counts(self, x: torch.Tensor, sigma: float, n: int, seed: int = 0, ids=None,
                        sample_base: int = 0) -> torch.Tensor:
        """int32 [B, 10]: how many of ``n`` copies ``x + N(0, sigma^2 I)`` of each image the net classifies as
        each class (no clamp, no dropout; the net's mode, parameters and gradients are untouched).  ``sigma`` in
        pixel units on the [0, 1] scale; ``x``: uint8 [B,28,28] / [B,784] images or float [B,1,28,28]
        already-normalised input.

        * GPU, ``dtype="bf16"``: the native loop ``ops.smooth.fused_smooth_counts``.  Image j draws the samples
          [``sample_base``, ``sample_base`` + n) of the in-kernel Philox stream keyed by ``seed`` under the id
          ``ids[j]`` (default j): the noised rows of an image do not depend on the batch it arrives in, bit for bit.
          Its counts follow except on an exact near-tie: ``fc1_fwd`` splits K 32 ways below 512 rows a launch
          and 4 ways from there, which can move a log-probability's last bits, so the size of a launch - the
          batch, and its last, smaller chunk - can flip such a vote.
        * CPU, or ``dtype="fp32"``: the same algorithm with ``torch.randn`` from a generator seeded by ``seed``
          and the image's id (advanced past the samples [0, ``sample_base``)), over ``forward_reference`` in eval
          mode: the same distribution, NOT the same bits as the GPU path."""
        B = self._check_input(x)
        if not sigma > 0:
            raise ValueError(f"smoothed_counts: sigma must be > 0, got {sigma}")
        if n != int(n) or n < 1:
            raise ValueError(f"smoothed_counts: n must be a positive integer, got {n}")
        if sample_base < 0:
            raise ValueError(f"smoothed_counts: sample_base must be >= 0, got {sample_base}")
        ids = _ids("smoothed_counts", ids, B)
        n, sigma_n = int(n), sigma / MNIST_STD
        if self.native:
            from .ops.smooth import fused_smooth_counts
            return fused_smooth_counts(self.net, self._rows_native(x, B), sigma_n, n, seed, ids, sample_base)
        x0 = _rows_f32(x, B, "cpu")
        gen = torch.Generator()
        counts = torch.zeros(B, 10, dtype=torch.int32)
        with _eval_mode(self.net), torch.no_grad():
            for j in range(B):                                   # per image: a generator run of its own
                gen.manual_seed(_smooth_generator_seed(seed, j if ids is None else ids[j]))
                for s0 in range(0, sample_base, _REF_ROWS):      # past the samples [0, sample_base)
                    torch.randn(min(_REF_ROWS, sample_base - s0), 784, generator=gen, dtype=torch.float32)
                for s0 in range(0, n, _REF_ROWS):
                    ns = min(_REF_ROWS, n - s0)
                    z = torch.randn(ns, 784, generator=gen, dtype=torch.float32)
                    rows = (x0[j] + sigma_n * z).view(ns, 1, 28, 28).to(self.device)
                    pred = self.net.forward_reference(rows).argmax(dim=1).cpu()
                    counts[j] += torch.bincount(pred, minlength=10).to(torch.int32)
        return counts.to(self.device)

    def certify(self, x: torch.Tensor, sigma: float, n0: int = 100, n: int = 1000, alpha: float = 0.001,
                seed: int = 0, ids=None):
        """Randomized-smoothing certificate (Cohen, Rosenfeld, Kolter 2019) of each image: ``(classes int64 [B],
        radii float64 [B], counts int32 [B,10])``, all on the CPU.  The smoothed classifier's class is selected
        from the samples [0, ``n0``); its vote share is estimated from the disjoint samples [``n0``, ``n0`` + n)
        (``counts``); ``ops.smooth.certify_from_counts`` turns both into the class and the L2 radius, in pixel
        units as ``sigma``, within which that class is returned with probability >= 1 - ``alpha`` - or into
        class -1 and radius 0 (abstain).  Paths, ``seed`` and ``ids`` as ``smoothed_counts``."""
        from .ops.smooth import certify_from_counts
        B = self._check_input(x)
        if not sigma > 0:
            raise ValueError(f"certify: sigma must be > 0, got {sigma}")
        if n0 != int(n0) or n0 < 1 or n != int(n) or n < 1:
            raise ValueError(f"certify: n0 and n must be positive integers, got {n0}, {n}")
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"certify: alpha must be in (0, 1), got {alpha}")
        ids = _ids("certify", ids, B)
        counts0 = self.smoothed_counts(x, sigma, int(n0), seed, ids, sample_base=0).cpu()
        counts = self.smoothed_counts(x, sigma, int(n), seed, ids, sample_base=int(n0)).cpu()
        classes = torch.empty(B, dtype=torch.int64)
        radii = torch.empty(B, dtype=torch.float64)
        for j in range(B):
            classes[j], radii[j] = certify_from_counts(counts0[j].tolist(), counts[j].tolist(), sigma, alpha)
        return classes, radii, counts

    # ------------------------------------------------------------------ attribution
    def attribute(self, x: torch.Tensor, labels: torch.Tensor | None = None, method: str = "integrated_gradients",
                  steps: int = 32, baseline=None, sigma: float = 0.15, seed: int = 0, ids=None):
        """(attr, log_probs): float32 [B,1,28,28] attribution of log p_y(x) to the NORMALISED input and the float32
        [B,10] log-probabilities of the clean input.  y is ``labels`` ([B] integers), or the class predicted on the
        clean input when ``labels`` is None.  With g = d NLL_y / d x (what ``input_gradient`` returns):

        * ``"integrated_gradients"`` (Sundararajan et al. 2017), midpoint rule over ``steps`` points from the
          baseline b: ``-(x - b) * mean_s g(b + (s + 1/2) / steps * (x - b))``; its sum over the pixels approaches
          log p_y(x) - log p_y(b) as ``steps`` grows (completeness).  ``baseline``: None = the black image, a float
          in pixel units on the [0, 1] scale, or a tensor in any form ``x`` may take.
        * ``"smoothgrad"`` (Smilkov et al. 2017): ``-mean_s g(x + N(0, sigma^2 I))`` over ``steps`` noised copies,
          no clamp; ``sigma`` in pixel units, ``seed`` and ``ids`` as ``smoothed_counts`` takes them (image j draws
          the samples [0, steps) under the id ``ids[j]``, default j).  ``baseline`` is not used; ``sigma``, ``seed``
          and ``ids`` are used by this method only.

        Inference semantics (no dropout); the net's mode, parameters and gradients are untouched.  GPU with
        ``dtype="bf16"``: the native loop ``ops.attribute.fused_attribution``; CPU, or ``dtype="fp32"``:
        ``reference_attribution``.  ``x``: uint8 [B,28,28] / [B,784] images or float [B,1,28,28] normalised input."""
        B = self._check_input(x)
        if method not in ATTRIBUTION_METHODS:
            raise ValueError(f"attribute: method must be one of {ATTRIBUTION_METHODS}, got {method!r}")
        if isinstance(steps, bool) or steps != int(steps) or steps < 1:
            raise ValueError(f"attribute: steps must be a positive integer, got {steps}")
        steps, path = int(steps), method == "integrated_gradients"
        base = 0.0
        if path:
            if baseline is None:
                base = PIXEL_LO
            elif isinstance(baseline, torch.Tensor):
                if baseline.numel() != B * 784:
                    raise ValueError(f"attribute: the baseline must hold {B} images, got {tuple(baseline.shape)}")
                base = _rows_f32(baseline, B, self.device)
            elif isinstance(baseline, (int, float)) and baseline == baseline:
                base = normalised_pixel(baseline)
            else:
                raise ValueError("attribute: baseline must be None, a float in pixel units or a tensor of images")
        else:
            if not sigma > 0:
                raise ValueError(f"attribute: sigma must be > 0, got {sigma}")
            ids = _ids("attribute", ids, B)
        lp, pred = self._forward(x)
        labels = pred if labels is None else self._labels("attribute", labels, B, check_range=True)
        sigma_n = sigma / MNIST_STD
        if self.native:
            from .ops.attribute import fused_attribution
            attr = fused_attribution(self.net, self._rows_native(x, B), labels, method, steps, base, sigma_n, seed, ids)
        else:
            attr = reference_attribution(self.net, _rows_f32(x, B, self.device), labels, method, steps, base,
                                         sigma_n, seed, ids)
        return attr.view(B, 1, 28, 28), lp

    # ------------------------------------------------------------------ dispatch
    def _check_input(self, x: torch.Tensor) -> int:
        B = int(x.shape[0])
        if x.numel() != B * 784 or B < 1:
            raise ValueError(f"Predictor expects [B,28,28] / [B,784] / [B,1,28,28] input, got {tuple(x.shape)}")
        return B

    def _true_labels(self, name: str, loss: str, targeted: bool, labels: torch.Tensor, true_labels, x0: torch.Tensor,
                     B: int):
        """The true classes the targeted DLR loss reads beside the targets ``labels`` (None for every other loss):
        ``true_labels`` checked, or the class predicted on the clean rows ``x0``; no row's target may equal it."""
        if not (targeted and loss == "dlr"):
            return None
        if true_labels is None:
            true_labels = self._forward(x0.view(B, 1, 28, 28))[1]
        else:
            true_labels = self._labels(name, true_labels, B, check_range=True)
        if bool((true_labels == labels).any()):
            raise ValueError(f"{name}: the targeted DLR loss needs every target to differ from its row's true label")
        return true_labels

    def _rows_native(self, x: torch.Tensor, B: int) -> torch.Tensor:
        """The rows the native loops take, contiguous [B, 784] on the predictor's device: uint8 images stay uint8
        (the kernels normalise them), float input becomes detached float32."""
        if x.dtype == torch.uint8:
            return x.reshape(B, 784).contiguous().to(self.device)
        return x.detach().reshape(B, 784).to(self.device, torch.float32).contiguous()

    def _labels(self, name: str, labels: torch.Tensor, B: int, check_range: bool) -> torch.Tensor:
        """int64 [B] labels on the predictor's device; ``check_range``: each in [0, 10)."""
        if labels.numel() != B:
            raise ValueError(f"{name}: {labels.numel()} labels for {B} images")
        labels = labels.reshape(B).long().to(self.device)
        if check_range and (int(labels.min()) < 0 or int(labels.max()) > 9):
            raise ValueError(f"{name}: labels must be in [0, 10)")
        return labels

    def _forward(self, x: torch.Tensor):
        B = self._check_input(x)
        if not self.native:
            xf = _rows_f32(x, B, self.device).view(B, 1, 28, 28)
            with _eval_mode(self.net), torch.no_grad():
                lp = self.net.forward_reference(xf)
            return lp, lp.argmax(dim=1)
        src = self._rows_native(x, B)
        out = self._native(B, u8=src) if src.dtype == torch.uint8 else self._native(B, x=src)
        lp = out.logp[:B].clone()
        pred = out.pred[:B].long() if out.pred is not None else lp.argmax(dim=1)
        return lp, pred

    def _native(self, B: int, u8=None, x=None, labels=None):
        """One batch through the HIP kernels; returns the buffer set holding rows [0, B)."""
        from .ops import functional as Fk
        from .ops.chain import EvalChain
        self._st.sync()
        ms = self._st.ms
        if B <= INFER_FUSED_MAX_B:
            if self._infer_buf is None or self._infer_buf.max_B < B:
                self._infer_buf = Fk.InferBuffers.allocate(max(B, INFER_FUSED_MAX_B), self.device)
            Fk.infer_forward(ms, self._infer_buf, B, u8=u8, x=x, labels=labels)
            return self._infer_buf
        buf = self._eval_buf
        if buf is None or buf.rows != B:
            buf = self._eval_buf = Fk.EvalBuffers.allocate(B, self.device)
        p = Fk.native.ptr
        EvalChain(ms, buf).run(B, u8=p(u8), xin=p(x), labels=p(labels))
        return buf


# ---------------------------------------------------------------------------- mnist_predict.py
def build_predict_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Evaluate a saved MNIST checkpoint on the test split")
    ap.add_argument('--checkpoint', default='mnist_cnn.pt', help='state_dict file written by --save-model')
    ap.add_argument('--batch-size', type=int, default=1000, metavar='N',
                    help='images per forward (default: 1000)')
    ap.add_argument('--no-cuda', action='store_true', default=False, help='run on the CPU')
    ap.add_argument('--json-log', default=None, help='append the result as one JSON line to this file')
    ap.add_argument('--data-root', default='./data', help='MNIST root (torchvision layout)')
    ap.add_argument('--synthetic', action='store_true', default=None,
                    help='use deterministic synthetic 28x28 data (auto when MNIST files are absent)')
    ap.add_argument('--synthetic-test-size', type=int, default=None)
    ap.add_argument('--saliency', default=None, metavar='OUT.npy',
                    help='also write d NLL / d (normalised image) against the true labels for the evaluated '
                         'split as a float32 [N,28,28] .npy file (default: off)')
    ap.add_argument('--saliency-method', choices=('gradient',) + ATTRIBUTION_METHODS, default='gradient',
                    help='what --saliency writes: the raw gradient, or the integrated-gradients / SmoothGrad '
                         'attribution of log p(true label) (default: gradient)')
    ap.add_argument('--saliency-steps', type=int, default=32, metavar='N',
                    help='path points (integrated gradients) or noised copies (SmoothGrad) per image (default: 32)')
    ap.add_argument('--saliency-sigma', type=float, default=0.15, metavar='S',
                    help='SmoothGrad noise standard deviation in pixel units on the [0, 1] scale (default: 0.15)')
    ap.add_argument('--saliency-baseline', type=float, default=None, metavar='V',
                    help='integrated-gradients baseline: a constant image of pixel value V (default: 0, black)')
    ap.add_argument('--saliency-seed', type=int, default=0, help='seed of the SmoothGrad noise (default: 0)')
    ap.add_argument('--attack-eps', type=float, default=None, metavar='E',
                    help='also report loss and accuracy under an L-inf FGSM / PGD attack of radius E, in pixel '
                         'units on the [0, 1] scale (default: off)')
    ap.add_argument('--attack-steps', type=int, default=1, metavar='K',
                    help='attack iterations: 1 = FGSM, more = PGD (default: 1)')
    ap.add_argument('--attack-step-size', type=float, default=None, metavar='A',
                    help='attack step in pixel units (default: E for one step, 2.5 * E / K otherwise)')
    ap.add_argument('--attack-norm', choices=('linf', 'l2'), default='linf',
                    help='norm of the attack radius E and of its steps (default: linf)')
    ap.add_argument('--apgd-eps', type=float, default=None, metavar='E',
                    help='also report loss and accuracy under an Auto-PGD attack (no step size to tune) of radius E, '
                         'in pixel units on the [0, 1] scale (default: off)')
    ap.add_argument('--apgd-steps', type=int, default=100, metavar='N', help='Auto-PGD iterations (default: 100)')
    ap.add_argument('--apgd-norm', choices=('linf', 'l2'), default='linf',
                    help='norm of the Auto-PGD radius E (default: linf)')
    ap.add_argument('--apgd-restarts', type=int, default=1, metavar='R',
                    help='Auto-PGD runs per image; more than one: each from a random start (default: 1, from the '
                         'clean image)')
    ap.add_argument('--apgd-seed', type=int, default=0, help='seed of the random starts (default: 0)')
    ap.add_argument('--apgd-loss', choices=('ce', 'cw', 'dlr'), default='ce',
                    help='loss Auto-PGD ascends: cross-entropy, the CW margin or the DLR loss (default: ce)')
    ap.add_argument('--ensemble-eps', type=float, default=None, metavar='E',
                    help='also report the accuracy of the images that survive every attack of an L-inf ensemble of '
                         'radius E, in pixel units on the [0, 1] scale: Auto-PGD on the cross-entropy, targeted '
                         'Auto-PGD on the DLR loss towards the T most likely other classes, the Square Attack; not '
                         "AutoAttack's standard set: no FAB-T, no random starts (default: off)")
    ap.add_argument('--ensemble-steps', type=int, default=100, metavar='N',
                    help='Auto-PGD iterations of the ensemble (default: 100)')
    ap.add_argument('--ensemble-targets', type=int, default=9, metavar='T',
                    help='target classes of the targeted stage, 0..9 (default: 9)')
    ap.add_argument('--ensemble-queries', type=int, default=5000, metavar='Q',
                    help='most queries per image of the Square Attack stage; 0: skip it (default: 5000)')
    ap.add_argument('--ensemble-seed', type=int, default=0, help='seed of the squares (default: 0)')
    ap.add_argument('--square-eps', type=float, default=None, metavar='E',
                    help='also report loss and accuracy under the L-inf Square Attack (score-based, black-box: no '
                         'gradient is read) of radius E, in pixel units on the [0, 1] scale (default: off)')
    ap.add_argument('--square-queries', type=int, default=1000, metavar='N',
                    help='most queries (forwards) per image of the Square Attack (default: 1000)')
    ap.add_argument('--square-p-init', type=float, default=0.8, metavar='P',
                    help='share of the image the first squares cover (default: 0.8)')
    ap.add_argument('--square-seed', type=int, default=0, help='seed of the squares (default: 0)')
    ap.add_argument('--certify-sigma', type=float, default=None, metavar='S',
                    help='also report certified accuracy under randomized smoothing with Gaussian noise of standard '
                         'deviation S, in pixel units on the [0, 1] scale (default: off)')
    ap.add_argument('--certify-n', type=int, default=1000, metavar='N',
                    help='noise samples per image that estimate the vote share (default: 1000)')
    ap.add_argument('--certify-n0', type=int, default=100, metavar='N0',
                    help='noise samples per image that select the class (default: 100)')
    ap.add_argument('--certify-alpha', type=float, default=0.001, metavar='A',
                    help='failure probability of the certificate (default: 0.001)')
    ap.add_argument('--certify-radii', type=_radii, default=(0.0, 0.25, 0.5), metavar='R1,R2,...',
                    help='L2 radii, in pixel units, at which certified accuracy is reported (default: 0,0.25,0.5)')
    ap.add_argument('--certify-count', type=int, default=None, metavar='M',
                    help='certify the first M images of the split (default: all)')
    ap.add_argument('--certify-seed', type=int, default=0, help='seed of the noise (default: 0)')
    ap.add_argument('--min-norm', action='store_true', default=False,
                    help='also report the minimum-norm (L2 DeepFool) adversarial radius of the images against their '
                         'true labels: how many are found, the median and mean radius in pixel units (default: off)')
    ap.add_argument('--min-norm-steps', type=int, default=50, metavar='K',
                    help='most DeepFool iterations per image (default: 50)')
    ap.add_argument('--min-norm-overshoot', type=float, default=0.02, metavar='O',
                    help='overshoot past the linearised boundary (default: 0.02)')
    ap.add_argument('--min-norm-count', type=int, default=None, metavar='M',
                    help='attack the first M images of the split (default: all)')
    ap.add_argument('--min-norm-radii', type=_radii, default=(), metavar='R1,R2,...',
                    help='L2 radii, in pixel units, at which accuracy is read off the per-image radii (default: none)')
    return ap


def _radii(text: str) -> tuple:
    vals = tuple(float(t) for t in text.split(',') if t.strip())
    if not vals or any(not v >= 0 for v in vals):
        raise argparse.ArgumentTypeError(f"expected non-negative radii R1,R2,..., got {text!r}")
    return vals


def certified_line(sigma: float, n: int, alpha: float, radius: float, correct: int, m: int, abstained: int) -> str:
    """One ``Certified set`` line: ``correct`` of ``m`` images are classified correctly, not abstained on and
    certified at an L2 radius >= ``radius``."""
    return (f"Certified set (L2 sigma={sigma:g}, n={n}, alpha={alpha:g}, radius={radius:g}): "
            f"Accuracy: {correct}/{m} ({100.0 * correct / m:.0f}%), abstained {abstained}")


def _loss_tag(loss_name: str) -> str:
    return "" if loss_name == "ce" else f", loss={loss_name}"


def adversarial_line(eps: float, steps: int, loss: float, correct: int, n: int, norm: str = "linf") -> str:
    """The ``Test set:`` line's figures (``utils.logging.test_line``) for the attacked split."""
    figures = test_line(loss, correct, n).split(": ", 1)[1].rstrip("\n")
    return f"Adversarial set ({'L2' if norm == 'l2' else 'Linf'} eps={eps:g}, steps={steps}): {figures}"


def auto_pgd_line(eps: float, steps: int, restarts: int, loss: float, correct: int, n: int, norm: str = "linf",
                  loss_name: str = "ce") -> str:
    """The ``Auto-PGD set`` line of ``mnist_predict.py --apgd-eps``, in the number formats of ``adversarial_line``;
    ``loss_name``: the loss the attack ascended, named in the line when it is not the cross-entropy."""
    figures = test_line(loss, correct, n).split(": ", 1)[1].rstrip("\n")
    return (f"Auto-PGD set ({'L2' if norm == 'l2' else 'Linf'} eps={eps:g}, steps={steps}, restarts={restarts}"
            f"{_loss_tag(loss_name)}): {figures}")


def ensemble_line(eps: float, targets: int, correct: int, n: int) -> str:
    """The ``Ensemble set`` line of ``mnist_predict.py --ensemble-eps``."""
    return (f"Ensemble set (Linf eps={eps:g}: apgd-ce, apgd-t x {targets}, square): "
            f"Accuracy: {correct}/{n} ({100.0 * correct / n:.0f}%)")


def square_line(eps: float, queries: int, p_init: float, loss: float, correct: int, n: int, median) -> str:
    """The ``Square set`` line of ``mnist_predict.py --square-eps``, in the number formats of ``adversarial_line``;
    ``median``: the median queries of the broken images, None when none broke."""
    figures = test_line(loss, correct, n).split(": ", 1)[1].rstrip("\n")
    return (f"Square set (Linf eps={eps:g}, queries={queries}, p_init={p_init:g}): {figures}, "
            f"median queries: {'n/a' if median is None else format(median, 'g')}")


def minimum_norm_stats(radii: torch.Tensor, found: torch.Tensor, clean: torch.Tensor, at=()):
    """``(found, median, mean, accuracy_at)`` of per-image DeepFool results: how many images were found; the median
    and mean radius over the found images that were correct on the clean input (None when there is none; the median
    of an even count is the mean of the middle two); and per radius R of ``at`` how many images are correct on the
    clean input and either not found or found only at a radius > R."""
    r = radii[found & clean].double()
    median = float(r.quantile(0.5)) if r.numel() else None
    mean = float(r.mean()) if r.numel() else None
    return int(found.sum()), median, mean, [int((clean & (~found | (radii > R))).sum()) for R in at]


def minimum_norm_line(steps: int, overshoot: float, m: int, found: int, median, mean) -> str:
    """The ``Minimum-norm set`` line of ``mnist_predict.py --min-norm``."""
    fmt = lambda v: "n/a" if v is None else f"{v:.4f}"   # noqa: E731
    return (f"Minimum-norm set (L2 DeepFool, steps={steps}, overshoot={overshoot:g}): "
            f"Found: {found}/{m} ({100.0 * found / m:.0f}%), median radius: {fmt(median)}, mean radius: {fmt(mean)}")


def completeness_gap(predictor: "Predictor", attr: torch.Tensor, lp: torch.Tensor, labels: torch.Tensor,
                     baseline: float | None = None) -> float:
    """sum over the images of |sum attr - (log p_y(x) - log p_y(b))| for integrated gradients ``attr`` of images
    with clean log-probabilities ``lp``, against the constant baseline of pixel value ``baseline`` (None: black);
    log p_y(b) from ``predictor.log_probs``."""
    B = attr.shape[0]
    b = PIXEL_LO if baseline is None else normalised_pixel(baseline)
    y = labels.reshape(B, 1).long().to(lp.device)
    lp_b = predictor.log_probs(torch.full((1, 1, 28, 28), b, dtype=torch.float32))[0].to(lp.device)
    delta = lp.gather(1, y)[:, 0].double() - lp_b[y[:, 0]].double()
    return float((attr.reshape(B, 784).double().sum(dim=1) - delta).abs().sum())


def predict_main(argv=None) -> int:
    args = build_predict_parser().parse_args(argv)
    use_cuda = not args.no_cuda and torch.cuda.is_available()
    device = torch.device("cuda", 0) if use_cuda else torch.device("cpu")
    predictor = Predictor.from_checkpoint(args.checkpoint, device=device)
    data = load_mnist(args.data_root, False, args.synthetic, args.synthetic_test_size)
    images = data.device_images(device) if use_cuda else data.images
    loss_sum, correct, n = predictor.evaluate(images, data.targets, args.batch_size)
    print(test_line(loss_sum / n, correct, n))
    attribution = {}
    if args.saliency:
        import numpy as np
        method = args.saliency_method
        out = np.empty((n, 28, 28), dtype=np.float32)
        gap = 0.0
        for i in range(0, n, args.batch_size):
            xb, yb = images[i:i + args.batch_size], data.targets[i:i + args.batch_size]
            if method == "gradient":
                g, _ = predictor.input_gradient(xb, yb)
            else:
                g, lp = predictor.attribute(xb, yb, method, args.saliency_steps, args.saliency_baseline,
                                            args.saliency_sigma, args.saliency_seed, ids=range(i, i + xb.shape[0]))
                if method == "integrated_gradients":
                    gap += completeness_gap(predictor, g, lp, yb, args.saliency_baseline)
            out[i:i + g.shape[0]] = g.reshape(-1, 28, 28).cpu().numpy()
        with open(args.saliency, "wb") as f:      # (np.save on a name would append ".npy")
            np.save(f, out)
        if method != "gradient":
            attribution = {"saliency_method": method, "saliency_steps": args.saliency_steps}
            if method == "smoothgrad":
                attribution.update(saliency_sigma=args.saliency_sigma, saliency_seed=args.saliency_seed)
            else:
                attribution.update(saliency_baseline=0.0 if args.saliency_baseline is None else args.saliency_baseline,
                                   saliency_completeness_gap=gap / n)
    record = {"checkpoint": args.checkpoint, "device": str(device), "source": data.source,
              "test_loss": loss_sum / n, "correct": correct, "n": n}
    record.update(attribution)
    if args.attack_eps is not None:
        adv_loss, adv_correct, _ = predictor.robust_evaluate(images, data.targets, args.attack_eps, args.attack_steps,
                                                             args.attack_step_size, args.batch_size,
                                                             norm=args.attack_norm)
        print(adversarial_line(args.attack_eps, args.attack_steps, adv_loss / n, adv_correct, n, args.attack_norm))
        record.update(adv_eps=args.attack_eps, adv_steps=args.attack_steps, adv_loss=adv_loss / n,
                      adv_correct=adv_correct, adv_norm=args.attack_norm)
    if args.certify_sigma is not None:
        m = n if args.certify_count is None else max(1, min(n, args.certify_count))
        classes = torch.empty(m, dtype=torch.int64)
        radii = torch.empty(m, dtype=torch.float64)
        for i in range(0, m, args.batch_size):
            j = min(m, i + args.batch_size)
            classes[i:j], radii[i:j], _ = predictor.certify(images[i:j], args.certify_sigma, args.certify_n0,
                                                            args.certify_n, args.certify_alpha, args.certify_seed,
                                                            ids=range(i, j))
        right = classes == data.targets[:m].long().cpu()
        abstained = int((classes < 0).sum())
        certified = [int((right & (radii >= r)).sum()) for r in args.certify_radii]
        for r, c in zip(args.certify_radii, certified):
            print(certified_line(args.certify_sigma, args.certify_n, args.certify_alpha, r, c, m, abstained))
        record.update(certify_sigma=args.certify_sigma, certify_n=args.certify_n, certify_n0=args.certify_n0,
                      certify_alpha=args.certify_alpha, certify_seed=args.certify_seed, certify_count=m,
                      certify_radii=list(args.certify_radii), certify_correct=certified,
                      certify_abstained=abstained)
    if args.min_norm:
        m = n if args.min_norm_count is None else max(1, min(n, args.min_norm_count))
        found = torch.empty(m, dtype=torch.bool)
        clean = torch.empty(m, dtype=torch.bool)
        radii = torch.empty(m, dtype=torch.float32)
        for i in range(0, m, args.batch_size):
            j = min(m, i + args.batch_size)
            yb = data.targets[i:j]
            clean[i:j] = (predictor.predict(images[i:j]).cpu() == yb.long().cpu())
            _, r, _, fnd = predictor.minimum_norm(images[i:j], yb, args.min_norm_steps, args.min_norm_overshoot)
            radii[i:j], found[i:j] = r.cpu(), fnd.cpu()
        stats = minimum_norm_stats(radii, found, clean, args.min_norm_radii)
        print(minimum_norm_line(args.min_norm_steps, args.min_norm_overshoot, m, *stats[:3]))
        for r, c in zip(args.min_norm_radii, stats[3]):
            print(f"Accuracy at radius {r:g}: {c}/{m} ({100.0 * c / m:.0f}%)")
        record.update(min_norm_steps=args.min_norm_steps, min_norm_overshoot=args.min_norm_overshoot,
                      min_norm_count=m, min_norm_found=stats[0], min_norm_median_radius=stats[1],
                      min_norm_mean_radius=stats[2],
                      min_norm_accuracy_at={f"{r:g}": c for r, c in zip(args.min_norm_radii, stats[3])})
    if args.apgd_eps is not None:
        gen = torch.Generator().manual_seed(args.apgd_seed) if args.apgd_restarts > 1 else None
        ap_loss, ap_correct, _ = predictor.robust_evaluate_apgd(images, data.targets, args.apgd_eps, args.apgd_steps,
                                                                args.batch_size, norm=args.apgd_norm,
                                                                restarts=args.apgd_restarts, generator=gen,
                                                                loss=args.apgd_loss)
        print(auto_pgd_line(args.apgd_eps, args.apgd_steps, args.apgd_restarts, ap_loss / n, ap_correct, n,
                            args.apgd_norm, args.apgd_loss))
        record.update(apgd_eps=args.apgd_eps, apgd_steps=args.apgd_steps, apgd_norm=args.apgd_norm,
                      apgd_restarts=args.apgd_restarts, apgd_loss=ap_loss / n, apgd_correct=ap_correct)
        if args.apgd_loss != "ce":
            record.update(apgd_loss_name=args.apgd_loss)
    if args.square_eps is not None:
        sq_loss, sq_correct, _, sq_median = predictor.robust_evaluate_square(
            images, data.targets, args.square_eps, args.square_queries, args.batch_size, args.square_p_init,
            args.square_seed)
        print(square_line(args.square_eps, args.square_queries, args.square_p_init, sq_loss / n, sq_correct, n,
                          sq_median))
        record.update(square_eps=args.square_eps, square_queries=args.square_queries,
                      square_p_init=args.square_p_init, square_seed=args.square_seed, square_loss=sq_loss / n,
                      square_correct=sq_correct, square_median_queries=sq_median)
    if args.ensemble_eps is not None:
        en_correct, _, en_after = predictor.robust_evaluate_ensemble(
            images, data.targets, args.ensemble_eps, args.ensemble_steps, args.ensemble_targets, args.ensemble_queries,
            args.batch_size, seed=args.ensemble_seed)
        print(ensemble_line(args.ensemble_eps, args.ensemble_targets, en_correct, n))
        record.update(ensemble_eps=args.ensemble_eps, ensemble_steps=args.ensemble_steps,
                      ensemble_targets=args.ensemble_targets, ensemble_queries=args.ensemble_queries,
                      ensemble_seed=args.ensemble_seed, ensemble_correct=en_correct, ensemble_after=en_after)
    if args.json_log:
        with open(args.json_log, "a") as f:
            f.write(json.dumps(record) + "\n")
    return 0
