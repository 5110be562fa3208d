"""Carlini & Wagner's L2 attack (S&P 2017) on the fused MI355X kernels: the native loop behind
``Predictor.carlini_wagner``.

The attack minimises |x - x0|^2 + c * max(kappa - margin, 0) over a tanh-space variable with Adam, and searches the
trade-off constant c per image by bisection.  All of that is per-image state - the variable, the two Adam moments, the
iterate, the nearest success, c and its bracket - and one row kernel, ``cw_step`` (csrc/kernels/cw.hip, one workgroup
per image), keeps and updates it.  One iteration is six launches on the current stream, with no autograd, no
allocation and no host sync:

    trunk_fwd -> fc1_fwd -> head_margin (CW) -> fc_bwd (role B)   ``ops.chain.GradChain(loss="cw")``: the margin per row
    -> input_grad (plain form: d margin / d x into one dx buffer)
    -> cw_step (success test and nearest success, Adam step: the next iterate, in place)

A search step of ``steps`` updates takes ``steps + 1`` rounds: round ``steps`` has ``search_end`` (it looks at the last
iterate, bisects c in the kernel and puts the image back to the clean point), the last round of the last search step
has ``last`` instead.  The very first round has ``first`` and reads no state.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import native
from .chain import GradChain
from .functional import (CW_ADAM_EPS, CW_BETA1, CW_BETA2, CW_C, CW_D_BEST, CW_FOUND_SEARCH, cw_bias_corrections,
                         cw_dist_scale)
from .fused_net import fused_state


def _buffers(st, rows: int, dev):
    """The five row buffers of the loop (iterate, gradient, tanh-space variable, Adam moments), kept on the net's fused
    state and reused while they are large enough (as ``ops.deepfool`` keeps ``deepfool_buf``)."""
    buf = getattr(st, "cw_buf", None)
    if buf is None or buf.rows < rows or buf.x.device != dev:
        new = lambda: torch.zeros(rows, 784, dtype=torch.float32, device=dev)                 # noqa: E731
        buf = st.cw_buf = SimpleNamespace(rows=rows, x=new(), dx=new(), w=new(), m1=new(), v=new())
    return buf


def fused_carlini_wagner(net, x: torch.Tensor, labels: torch.Tensor, search_steps: int, steps: int, lr: float,
                         c_init: float, kappa: float, sign: float, lo: float, hi: float, rows_per_launch: int = 8192):
    """``search_steps`` bisection steps of ``steps`` Adam updates each, in inference semantics (no dropout): ``(x_adv
    float32 [B, 784], d_best float32 [B], found_search int32 [B], c float32 [B])`` on the net's device.  ``x_adv``: the
    nearest iterate that was a success (margin ``sign * (max_{j != y} z_j - z_y)`` > 0 and >= ``kappa``, as the gradient
    chain computed it), the clean image where there was none; ``d_best`` = |x_adv - x|^2 in normalised units, +inf
    where none; ``found_search``: 1 + the search step that found it, 0 where none; ``c``: the constant of the last
    search step.  ``functional.cw_step_reference`` has the exact form.

    ``x``: float32 [B, 784] normalised rows on the net's device, inside [lo, hi]; ``labels``: [B] integers in [0, 10)
    (not checked here: ``Predictor.carlini_wagner`` does), the class to leave (``sign`` = +1) or to reach (-1);
    ``lo``, ``hi``: the valid range in normalised units.  The images are independent and run in chunks of at most
    ``rows_per_launch``; the result does not depend on the chunking, bit for bit, while every launch stays on one side
    of fc1_fwd's 512-row split change.  ``search_steps * (steps + 1)`` rounds of six launches per chunk, no host sync.
    One activation set is taken from and given back to the fused state's pool, the row buffers stay on it; the call
    allocates the labels and the results.  The net's mode, parameters, ``.grad`` and dropout counter stream are
    untouched."""
    search_steps, steps, rows_per_launch = int(search_steps), int(steps), int(rows_per_launch)
    if search_steps < 1 or steps < 1:
        raise ValueError("fused_carlini_wagner: search_steps and steps must be at least 1")
    if sign not in (1, -1) or not kappa >= 0 or not lr > 0 or not c_init > 0:
        raise ValueError("fused_carlini_wagner: need sign +1 or -1, kappa >= 0, lr > 0 and c_init > 0")
    if rows_per_launch < 1:
        raise ValueError("fused_carlini_wagner: rows_per_launch must be at least 1")
    st = fused_state(net)
    st.sync()                                   # once: the bf16 shadows follow the parameters
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype != torch.float32 or x.device != dev:
        raise ValueError("fused_carlini_wagner: x must be float32 [B, 784] on the net's device")
    B = x.shape[0]
    if B < 1:
        raise ValueError("fused_carlini_wagner: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_carlini_wagner: {labels.numel()} labels for {B} images")
    x0 = x.contiguous()
    mc = min(B, rows_per_launch)                                        # images per chunk
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    x_adv = torch.empty(B, 784, dtype=torch.float32, device=dev)        # every element is written by a first launch
    fstate = torch.empty(B, 4, dtype=torch.float32, device=dev)
    istate = torch.empty(B, 4, dtype=torch.int32, device=dev)
    rb = _buffers(st, mc, dev)
    bc = [cw_bias_corrections(t + 1) for t in range(steps)] + [(1.0, 1.0)]     # (round `steps` makes no Adam step)
    scal = (float(sign), float(kappa), float(lr), float(c_init), CW_BETA1, CW_BETA2, CW_ADAM_EPS)
    tail = (cw_dist_scale(), float(lo), float(hi))
    chain = GradChain(st, mc, "cw")
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px, pdx, ploss = p(rb.x), p(rb.dx), chain.loss_rows
    rows = (p(rb.w), p(rb.m1), p(rb.v), px)
    px0, plab, pbest, pf, pi = p(x0), p(lab), p(x_adv), p(fstate), p(istate)
    run, grad, step = chain.run, chain.input_grad, C.cw_step
    try:
        for i0 in range(0, B, mc):
            m = min(mc, B - i0)
            o4, o16, o784 = 4 * i0, 16 * i0, 3136 * i0
            rb.x[:m].copy_(x0[i0:i0 + m])                               # a first launch reads x = x0
            head = (pdx, ploss, px0 + o784, *rows, pbest + o784, pf + o16, pi + o16, *scal)
            for k in range(search_steps):
                final = k == search_steps - 1
                for j in range(steps + 1):
                    end = j == steps
                    run(px, plab + o4, m)
                    grad(pdx, m)
                    step(*head, *bc[j], *tail, k, k == 0 and j == 0, end and not final, end and final, m, s)
    finally:
        chain.release()                         # also when a launcher raised; the next taker is stream ordered
    return x_adv, fstate[:, CW_D_BEST].clone(), istate[:, CW_FOUND_SEARCH].clone(), fstate[:, CW_C].clone()
