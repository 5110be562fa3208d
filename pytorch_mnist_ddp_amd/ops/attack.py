"""L-inf and L2 FGSM / PGD on the fused MI355X kernels: the native attack loop behind
``Predictor.adversarial``.

One L-inf iteration is five launches on the current stream, with no autograd ``Function``, no allocation
and no host sync: the four of the gradient chain (``ops.chain.GradChain``: the summed NLL of the iterate, as
``fused_input_gradient``), then ``input_grad`` in its step form (csrc/kernels/input_grad.hip), which updates
the iterate in place.

One L2 iteration is six: the step needs the norm of an image's whole gradient, which four workgroups of
``input_grad`` write, so ``input_grad`` runs in its plain form into one ``dx`` buffer (allocated once per
call) and ``pgd_l2_step`` (csrc/kernels/attack_step.hip, one workgroup per image) updates the iterate in
place.  A targeted attack is the same loop with the step negated: the loss of the target is descended.
"""
from __future__ import annotations

import torch

from . import native
from .chain import GradChain
from .fused_net import fused_state


def fused_adversarial(net, x0: torch.Tensor, labels: torch.Tensor, eps: float, steps: int, step_size: float,
                      lo: float, hi: float, x_init: torch.Tensor | None = None, norm: str = "linf",
                      targeted: bool = False) -> torch.Tensor:
    """``steps`` projected gradient steps on the summed NLL of ``labels``, in inference semantics (no
    dropout), starting from ``x_init`` (default ``x0``); with g = d NLL / d x and a = ``step_size``
    (``targeted``: a = -``step_size``, ``labels`` are the targets and their loss is descended):

        "linf":  x <- clamp(clamp(x + a * sign(g), x0 - eps, x0 + eps), lo, hi)
        "l2":    x <- clamp(x0 + proj(x + a * g / |g| - x0), lo, hi),  proj(d) = d * min(1, eps / |d|)

    per image, with |.| the L2 norm (``functional.pgd_l2_step`` has the exact form).

    ``x0`` / ``x_init``: float32 [B, 784] normalised images on the net's device; ``labels``: [B] integers
    in [0, 10) (not checked here: ``Predictor.adversarial`` does); ``eps``, ``step_size``, ``lo``, ``hi`` in
    normalised units.  Returns the float32 [B, 784] iterate after the last step (a new tensor, the one
    buffer the loop updates in place).  One activation set is taken from and returned to the fused
    state's pool; ``net.training``, the dropout modules, the dropout counter stream and every parameter
    and ``.grad`` are left as they were."""
    if steps < 1:
        raise ValueError("fused_adversarial: steps must be at least 1")
    if norm not in ("linf", "l2"):
        raise ValueError(f"fused_adversarial: norm must be 'linf' or 'l2', got {norm!r}")
    st = fused_state(net)
    st.sync()                                   # once: the bf16 shadows follow the parameters
    dev = st.ms.device
    if x0.dim() != 2 or x0.shape[1] != 784 or x0.dtype != torch.float32 or x0.device != dev:
        raise ValueError("fused_adversarial: x0 must be float32 [B, 784] on the net's device")
    B = x0.shape[0]
    if labels.numel() != B:
        raise ValueError(f"fused_adversarial: {labels.numel()} labels for {B} images")
    if x_init is not None and (x_init.shape != x0.shape or x_init.dtype != x0.dtype or x_init.device != dev):
        raise ValueError("fused_adversarial: x_init must match x0")
    x0 = x0.contiguous()
    x = (x0 if x_init is None else x_init).clone(memory_format=torch.contiguous_format)   # the iterate
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    chain = GradChain(st, B)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px, px0, plab = p(x), p(x0), p(lab)
    alpha = -step_size if targeted else step_size
    # the L2 form's gradient buffer: every element is written by input_grad; held until the last launch is enqueued
    dx = torch.empty(B, 784, dtype=torch.float32, device=dev) if norm == "l2" else None
    pdx = p(dx)
    run, grad, grad_step = chain.run, chain.input_grad, chain.input_grad_step
    for _ in range(steps):
        run(px, plab, B)
        if norm == "linf":
            grad_step(px, px0, px, alpha, eps, lo, hi, B)
        else:
            grad(pdx, B)
            C.pgd_l2_step(pdx, px, px0, px, alpha, eps, lo, hi, B, s)
    chain.release()                             # last use enqueued: the next taker is stream ordered after it
    return x
