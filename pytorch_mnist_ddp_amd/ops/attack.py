"""L-inf and L2 FGSM / PGD on the fused MI355X kernels: the native attack loop behind
``Predictor.adversarial``.

One L-inf iteration is five launches on the current stream, with no autograd ``Function``, no allocation
and no host sync:

    trunk_fwd (xin = the iterate, training form, STEP_FLAG_NO_DROPOUT) -> fc1_fwd
    -> head_train (labels given directly, loss scale 1.0: the summed NLL, as ``fused_input_gradient``)
    -> fc_bwd, role B only (the dy records; no fc weight gradient is formed)
    -> input_grad in its step form (csrc/kernels/input_grad.hip): the iterate is updated in place

One L2 iteration is six: the step needs the norm of an image's whole gradient, which four workgroups of
``input_grad`` write, so ``input_grad`` runs in its plain form into one ``dx`` buffer (allocated once per
call) and ``pgd_l2_step`` (csrc/kernels/attack_step.hip, one workgroup per image) updates the iterate in
place.  A targeted attack is the same loop with the step negated: the loss of the target is descended.

Role B alone is enough at every batch size: it reads ``dz1`` (head_train), ``pmask`` (trunk_fwd), the
``w1t`` shadow and the step flags, and its ceil(B / 16) x 36 tiles write every byte of every image's 144
records (128 B of gradients + 16 B of argmax planes each) - all that ``input_grad`` reads of ``buf.dyc``.
Roles A and C write the fc gradients only (for B > 1024: their split partials), which nothing here reads.
"""
from __future__ import annotations

import torch

from . import native
from .functional import FC_ROLE_B, round_up
from .fused_net import _step_state, fused_state


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
    C, ms = native.load(), st.ms
    dev = ms.device
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
    state = _step_state(st, False, dev, 1)      # zero seed and counter, STEP_FLAG_NO_DROPOUT: nothing is drawn
    buf = st.take(B, dev)
    p, o = native.ptr, ms.offsets
    P, s, Bp = p(ms.param), native.stream_handle(), round_up(B, 32)
    c1w, c1b, c2b = P + 4 * o["conv1.weight"], P + 4 * o["conv1.bias"], P + 4 * o["conv2.bias"]
    f1b, f2w, f2b = P + 4 * o["fc1.bias"], P + 4 * o["fc2.weight"], P + 4 * o["fc2.bias"]
    px, px0, pst, plab = p(x), p(x0), p(state), p(lab)
    a1, pp, pmask, z1part, loss_rows = p(buf.a1), p(buf.p), p(buf.pmask), p(buf.z1part), p(buf.loss_rows)
    dz1, h_bf, dl_bf, dyc, fcpart = p(buf.dz1), p(buf.h_bf), p(buf.dl_bf), p(buf.dyc), p(buf.fcpart)
    w2f, w2d, w1, w1t = p(ms.w2f), p(ms.w2d), p(ms.w1), p(ms.w1t)
    alpha = -step_size if targeted else step_size
    # the L2 form's gradient buffer: every element is written by input_grad; held until the last launch is enqueued
    dx = torch.empty(B, 784, dtype=torch.float32, device=dev) if norm == "l2" else None
    pdx = p(dx)
    for _ in range(steps):
        C.trunk_fwd(0, 0, 0, pst, c1w, c1b, w2f, c2b, a1, pp, pmask, B, True, s, xin=px)
        C.fc1_fwd(pp, w1, z1part, B, s)
        C.head_train(z1part, f1b, f2w, f2b, plab, 0, 0, pst, 1.0, loss_rows, dz1, h_bf, dl_bf, B, Bp, s)
        C.fc_bwd(dz1, pp, pmask, w1t, h_bf, dl_bf, loss_rows, pst, 0, dyc, 0, 1.0, 1.0, B, Bp, s,
                 role=FC_ROLE_B, part=fcpart)
        if norm == "linf":
            C.input_grad_step(dyc, a1, w2d, c1w, px, px0, px, alpha, eps, lo, hi, B, s)
        else:
            C.input_grad(dyc, a1, w2d, c1w, pdx, B, s)
            C.pgd_l2_step(pdx, px, px0, px, alpha, eps, lo, hi, B, s)
    st.give(buf)                                # last use enqueued: the next taker is stream ordered after it
    return x
