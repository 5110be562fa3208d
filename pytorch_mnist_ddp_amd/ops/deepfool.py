"""Minimum-norm adversarial examples (L2 DeepFool, Moosavi-Dezfooli, Fawzi, Frossard 2016) on the fused MI355X
kernels: the native loop behind ``Predictor.minimum_norm``.

An image's ten rows, labelled 0 .. 9, carry every class gradient g_c = d NLL_c / d x (``input_grad``) and every logit
difference (``head_train``'s ``loss_rows`` = -log p_c) of that image.  Per chunk of images ``deepfool_init``
(csrc/kernels/deepfool.hip) writes the rows once; one iteration is then six launches on the current stream, with no
autograd, no allocation and no host sync:

    the four launches of the gradient chain (``ops.chain.GradChain``) on the 10 m rows -> input_grad in its plain form
    -> deepfool_step (one workgroup per image: the nine norms |g_y - g_k|, the nearest linearised boundary, the
       accumulated perturbation, the next iterate into the image's ten rows; crossed and stuck images freeze)

A frozen image stores nothing, so the host may look at ``status`` every ``check_every`` iterations and end a chunk
early without changing a bit of the result.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import native
from .chain import GradChain
from .functional import DF_CLASSES, DF_RUNNING
from .fused_net import fused_state


def _buffers(st, rows: int, dev):
    """The row buffer and the gradient buffer of the loop, kept on the net's fused state and reused while they are
    large enough (as ``ops.attribute`` keeps ``attr_buf``)."""
    buf = getattr(st, "deepfool_buf", None)
    if buf is None or buf.rows < rows or buf.x.device != dev:
        buf = st.deepfool_buf = SimpleNamespace(
            rows=rows,
            x=torch.zeros(rows, 784, dtype=torch.float32, device=dev),
            dx=torch.zeros(rows, 784, dtype=torch.float32, device=dev))
    return buf


def fused_minimum_norm(net, x: torch.Tensor, labels: torch.Tensor, steps: int, overshoot: float, lo: float, hi: float,
                       check_every: int = 8, rows_per_launch: int = 8192):
    """At most ``steps`` DeepFool iterations per image, in inference semantics (no dropout): ``(x_adv float32
    [B, 784], norm float32 [B], iters int32 [B], status int32 [B])`` on the net's device.  ``norm`` = |x_adv - x0| in
    normalised units; ``iters``: the updates made; ``status``: 0 = still running after the last iteration, 1 = the
    gradient chain saw the iterate leave ``labels`` (or start outside it: then x_adv = x0 and norm = 0), 2 = no
    class left to step towards.

    ``x``: uint8 [B, 784] raw rows or float32 [B, 784] normalised rows on the net's device; ``labels``: [B] integers
    in [0, 10), the class each image is to leave (not checked here: ``Predictor.minimum_norm`` does); ``overshoot``
    >= 0; ``lo``, ``hi``: the valid range in normalised units.  The images are independent and run in chunks of at
    most ``rows_per_launch // 10``; the result does not depend on the chunking, bit for bit, while every launch
    stays on one side of fc1_fwd's 512-row split change.  ``check_every`` = k > 0 reads a chunk's ``status`` on the
    host after every k iterations and ends the chunk once no image is still running; 0 never syncs.  The result does
    not depend on it.  One activation set is taken from and given back to the fused state's pool, the row and
    gradient buffers stay on it; the call allocates the labels and the results.  The net's mode, parameters,
    ``.grad`` and dropout counter stream are untouched."""
    steps, check_every, rows_per_launch = int(steps), int(check_every), int(rows_per_launch)
    if steps < 1:
        raise ValueError("fused_minimum_norm: steps must be at least 1")
    if not overshoot >= 0:
        raise ValueError(f"fused_minimum_norm: overshoot must be >= 0, got {overshoot}")
    if check_every < 0:
        raise ValueError(f"fused_minimum_norm: check_every must be >= 0, got {check_every}")
    if rows_per_launch < DF_CLASSES:
        raise ValueError(f"fused_minimum_norm: rows_per_launch must be at least {DF_CLASSES}")
    st = fused_state(net)
    st.sync()
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or x.device != dev:
        raise ValueError("fused_minimum_norm: x must be uint8 or float32 [B, 784] on the net's device")
    B = x.shape[0]
    if B < 1:
        raise ValueError("fused_minimum_norm: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_minimum_norm: {labels.numel()} labels for {B} images")
    x = x.contiguous()
    mc = min(B, rows_per_launch // DF_CLASSES)                          # images per chunk
    y = labels.reshape(B).to(dev, torch.int32).contiguous()
    lab10 = torch.arange(DF_CLASSES, dtype=torch.int32, device=dev).repeat(mc)
    f32 = dict(dtype=torch.float32, device=dev)
    x_adv, r_tot, norm = torch.empty(B, 784, **f32), torch.empty(B, 784, **f32), torch.empty(B, **f32)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    u8 = x.dtype == torch.uint8
    x0 = torch.empty(B, 784, **f32) if u8 else x                        # what the step reads as the clean image
    seen = torch.empty(mc, dtype=torch.int32, pin_memory=True) if check_every else None
    rb = _buffers(st, DF_CLASSES * mc, dev)
    chain = GradChain(st, DF_CLASSES * mc)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    prows, pdx, plab, ploss = p(rb.x), p(rb.dx), p(lab10), chain.loss_rows
    src, row_bytes = p(x), 784 * x.element_size()
    px, px0, pr, py, pst, pit, pn = p(x_adv), p(x0), p(r_tot), p(y), p(status), p(iters), p(norm)
    run, grad, step = chain.run, chain.input_grad, C.deepfool_step
    try:
        for i0 in range(0, B, mc):
            m = min(mc, B - i0)
            rows, o4, o784 = DF_CLASSES * m, 4 * i0, 3136 * i0
            at = src + i0 * row_bytes
            C.deepfool_init(at if u8 else 0, 0 if u8 else at, prows, px + o784, px0 + o784 if u8 else 0, pr + o784,
                            pst + o4, pit + o4, pn + o4, m, s)
            for it in range(1, steps + 1):
                run(prows, plab, rows)
                grad(pdx, rows)
                step(pdx, ploss, py + o4, px0 + o784, pr + o784, px + o784, prows, pst + o4, pit + o4, pn + o4,
                     overshoot, lo, hi, m, s)
                if check_every and it % check_every == 0 and it < steps:
                    seen[:m].copy_(status[i0:i0 + m])                       # the one host sync: every image frozen?
                    if not bool((seen[:m] == DF_RUNNING).any()):
                        break
    finally:
        chain.release()                         # also when a launcher raised; the next taker is stream ordered
    return x_adv, norm, iters, status
