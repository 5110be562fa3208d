"""Auto-PGD (Croce & Hein, ICML 2020: the gradient attack of AutoAttack) on the fused MI355X kernels: the native
loop behind ``Predictor.auto_pgd``.

Auto-PGD has no step size to tune: a momentum step, a per-image step that is halved at scheduled checkpoints when
progress stalls, and a restart from the best point found so far.  All of that is per-image state - iterate, previous
iterate, best point, best gradient, best loss, step, counters - and one row kernel, ``apgd_step``
(csrc/kernels/apgd.hip, one workgroup per image), keeps and updates it.  One iteration is six launches on the current
stream, with no autograd ``Function``, no allocation and no host sync:

    trunk_fwd -> fc1_fwd -> head_train -> fc_bwd (role B)      ``ops.chain.GradChain``: the NLL of the iterate per row
    -> input_grad (plain form: d NLL / d x into one dx buffer)
    -> apgd_step (counters and best point, checkpoint, momentum step: the next iterate, in place)

``steps`` updates take ``steps + 1`` rounds: round 0 has ``first`` (it sets the state up and makes update 1), round
``steps`` has ``last`` (it only brings the best point up to date with the loss of the last iterate), and the rounds
``functional.apgd_checkpoints`` names close a window.

``loss="cw"`` / ``"dlr"`` put ``head_margin`` in ``head_train``'s place (``GradChain(loss=...)``): ``apgd_step`` only
sees a loss per row and dx, so the CW margin and the DLR loss (targeted: the APGD-T objective) take the same six
launches.
"""
from __future__ import annotations

import torch

from . import native
from .chain import GradChain, chain_loss, margin_operands
from .functional import APGD_LOSS_BEST, apgd_checkpoints
from .fused_net import fused_state


def fused_auto_pgd(net, x0: torch.Tensor, labels: torch.Tensor, eps: float, steps: int, lo: float, hi: float,
                   x_init: torch.Tensor | None = None, norm: str = "linf", targeted: bool = False, loss: str = "ce",
                   true_labels: torch.Tensor | None = None):
    """``(x_best, loss_best)``: Auto-PGD with ``steps`` updates on the NLL of ``labels``, in inference semantics (no
    dropout), starting from ``x_init`` (default ``x0``), inside the ``norm`` ball of radius ``eps`` around ``x0`` and
    the range [lo, hi] (``functional.apgd_step_reference`` has the exact form).  ``targeted``: ``labels`` are the
    targets and their NLL is descended.  ``loss``: "ce", or "cw" / "dlr" (``functional.margin_loss_reference``) in the
    NLL's place throughout, the returned loss included; targeted "dlr" is the "dlr_t" form (the negative of the APGD-T
    objective, descended), which also reads ``true_labels`` ([B], required).

    ``x0`` / ``x_init``: float32 [B, 784] normalised images on the net's device; ``labels``: [B] integers in [0, 10)
    (not checked here: ``Predictor.auto_pgd`` does); ``eps``, ``lo``, ``hi`` in normalised units.  Returns the float32
    [B, 784] point of the highest loss (targeted: the lowest) among the ``steps + 1`` iterates and float32 [B] its
    NLL of ``labels`` as ``head_train`` computed it.  Every buffer is allocated before the loop.  One activation set
    is taken from and returned to the fused state's pool; ``net.training``, the dropout modules, the dropout counter
    stream and every parameter and ``.grad`` are left as they were."""
    if steps < 1:
        raise ValueError("fused_auto_pgd: steps must be at least 1")
    if norm not in ("linf", "l2"):
        raise ValueError(f"fused_auto_pgd: norm must be 'linf' or 'l2', got {norm!r}")
    kind = chain_loss("fused_auto_pgd", loss, targeted)
    st = fused_state(net)
    st.sync()                                   # once: the bf16 shadows follow the parameters
    dev = st.ms.device
    if x0.dim() != 2 or x0.shape[1] != 784 or x0.dtype != torch.float32 or x0.device != dev:
        raise ValueError("fused_auto_pgd: x0 must be float32 [B, 784] on the net's device")
    B = x0.shape[0]
    if labels.numel() != B:
        raise ValueError(f"fused_auto_pgd: {labels.numel()} labels for {B} images")
    if x_init is not None and (x_init.shape != x0.shape or x_init.dtype != x0.dtype or x_init.device != dev):
        raise ValueError("fused_auto_pgd: x_init must match x0")
    x0 = x0.contiguous()
    x = (x0 if x_init is None else x_init).clone(memory_format=torch.contiguous_format)   # the iterate
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    # every element of these is written by launch 0 (dx: by every input_grad) before it is read
    dx, x_old, x_best, g_best = (torch.empty(B, 784, dtype=torch.float32, device=dev) for _ in range(4))
    fstate = torch.empty(B, 4, dtype=torch.float32, device=dev)
    istate = torch.empty(B, 4, dtype=torch.int32, device=dev)
    window = dict(apgd_checkpoints(steps))
    sign = -1.0 if targeted else 1.0
    l2 = norm == "l2"
    lab, tgt = margin_operands("fused_auto_pgd", kind, lab, true_labels, B, dev)
    chain = GradChain(st, B, kind)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px, plab, ptgt, pdx, ploss = p(x), p(lab), p(tgt), p(dx), chain.loss_rows
    rest = (p(x0), px, p(x_old), p(x_best), p(g_best), p(fstate), p(istate), sign, eps, lo, hi, l2)
    run, grad, step = chain.run, chain.input_grad, C.apgd_step
    for j in range(steps + 1):
        run(px, plab, B, ptgt)
        grad(pdx, B)
        step(pdx, ploss, *rest, j == 0, j == steps, window.get(j, 0), B, s)
    chain.release()                             # last use enqueued: the next taker is stream ordered after it
    loss_best = fstate[:, APGD_LOSS_BEST]
    return x_best, (-loss_best if targeted else loss_best.clone())
