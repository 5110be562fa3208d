"""The Fast Adaptive Boundary attack (Croce & Hein 2020), untargeted, in the L-inf or the L2 norm, on the fused MI355X
kernels: the native loop behind ``Predictor.fab``.

The layout is DeepFool's (``ops.deepfool``): an image's ten rows, labelled 0 .. 9, carry every class gradient and
every logit difference of that image.  Per chunk of images ``deepfool_init`` writes the rows once (its ``r_tot``
output is the best point's buffer); one round is then six launches on the current stream, with no autograd, no
allocation and no host sync:

    the four launches of the gradient chain (``ops.chain.GradChain``) on the 10 m rows -> input_grad in its plain form
    -> fab_step (csrc/kernels/fab.hip, one workgroup per image: an iterate outside its class is recorded when it is
       the nearest so far and pulled back towards the clean image; any other steps along the two box-constrained
       projections onto the nearest linearised boundary)

``steps`` updates are ``steps`` + 1 rounds: the last one only examines the point the last update made.
"""
from __future__ import annotations

import torch

from . import native
from .chain import GradChain
from .deepfool import _buffers
from .functional import DF_CLASSES, FAB_NORMS
from .fused_net import fused_state


def fused_fab(net, x: torch.Tensor, labels: torch.Tensor, norm: str, steps: int, alpha_max: float, eta: float,
              beta: float, lo: float, hi: float, rows_per_launch: int = 8192):
    """``steps`` FAB iterations per image, in inference semantics (no dropout): ``(x_best float32 [B, 784], norm_best
    float32 [B], iters int32 [B], status int32 [B])`` on the net's device.  ``x_best``: the nearest point outside
    ``labels`` that the run examined, the clean image where there is none; ``norm_best`` = |x_best - x0| in the
    chosen norm and normalised units, +inf where there is none; ``iters``: the updates made; ``status``: 0 = ran to
    the end, 1 = the clean point is outside its label already (x_best = x0, norm_best = 0), 2 = no class to step
    towards.

    ``x``: uint8 [B, 784] raw rows or float32 [B, 784] normalised rows on the net's device; ``labels``: [B] integers
    in [0, 10) (not checked here: ``Predictor.fab`` does); ``norm``: "linf" or "l2"; ``alpha_max`` in [0, 1], ``eta``
    >= 1, ``beta`` in (0, 1]; ``lo``, ``hi``: the valid range in normalised units.  The images are independent and run
    in chunks of at most ``rows_per_launch // 10``; the result does not depend on the chunking, bit for bit, while
    every launch stays on one side of fc1_fwd's 512-row split change.  There is no host sync: FAB has no early end.
    One activation set is taken from and given back to the fused state's pool, the row and gradient buffers are
    ``ops.deepfool``'s and stay on the state; the call allocates the labels and the results.  The net's mode,
    parameters, ``.grad`` and dropout counter stream are untouched."""
    steps, rows_per_launch = int(steps), int(rows_per_launch)
    if norm not in FAB_NORMS:
        raise ValueError(f"fused_fab: norm must be 'linf' or 'l2', got {norm!r}")
    if steps < 1:
        raise ValueError("fused_fab: steps must be at least 1")
    if not (eta >= 1 and 0 < beta <= 1 and 0 <= alpha_max <= 1):
        raise ValueError("fused_fab: need eta >= 1, beta in (0, 1] and alpha_max in [0, 1]")
    if rows_per_launch < DF_CLASSES:
        raise ValueError(f"fused_fab: rows_per_launch must be at least {DF_CLASSES}")
    st = fused_state(net)
    st.sync()
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or x.device != dev:
        raise ValueError("fused_fab: x must be uint8 or float32 [B, 784] on the net's device")
    B = x.shape[0]
    if B < 1:
        raise ValueError("fused_fab: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_fab: {labels.numel()} labels for {B} images")
    x = x.contiguous()
    mc = min(B, rows_per_launch // DF_CLASSES)                          # images per chunk
    y = labels.reshape(B).to(dev, torch.int32).contiguous()
    lab10 = torch.arange(DF_CLASSES, dtype=torch.int32, device=dev).repeat(mc)
    f32 = dict(dtype=torch.float32, device=dev)
    x_it, x_best, unused = torch.empty(B, 784, **f32), torch.empty(B, 784, **f32), torch.empty(B, **f32)
    norm_best = torch.full((B,), float("inf"), **f32)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    u8 = x.dtype == torch.uint8
    x0 = torch.empty(B, 784, **f32) if u8 else x                        # what the step reads as the clean image
    rb = _buffers(st, DF_CLASSES * mc, dev)
    chain = GradChain(st, DF_CLASSES * mc)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    prows, pdx, plab, ploss = p(rb.x), p(rb.dx), p(lab10), chain.loss_rows
    src, row_bytes = p(x), 784 * x.element_size()
    px, px0, pb, py, pst, pit, pn, pun = p(x_it), p(x0), p(x_best), p(y), p(status), p(iters), p(norm_best), p(unused)
    run, grad, step, code = chain.run, chain.input_grad, C.fab_step, FAB_NORMS[norm]
    try:
        for i0 in range(0, B, mc):
            m = min(mc, B - i0)
            rows, o4, o784 = DF_CLASSES * m, 4 * i0, 3136 * i0
            at = src + i0 * row_bytes
            C.deepfool_init(at if u8 else 0, 0 if u8 else at, prows, px + o784, px0 + o784 if u8 else 0, pb + o784,
                            pst + o4, pit + o4, pun + o4, m, s)
            for it in range(steps + 1):
                run(prows, plab, rows)
                grad(pdx, rows)
                step(pdx, ploss, py + o4, px0 + o784, px + o784, pb + o784, pn + o4, prows, pst + o4, pit + o4, 0,
                     alpha_max, eta, beta, lo, hi, code, it == steps, m, s)
    finally:
        chain.release()                         # also when a launcher raised; the next taker is stream ordered
    return torch.where(torch.isinf(norm_best)[:, None], x0, x_best), norm_best, iters, status
