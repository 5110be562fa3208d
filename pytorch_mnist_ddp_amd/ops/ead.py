"""EAD, the elastic-net attack (Chen, Sharma, Zhang, Yi & Hsieh, AAAI 2018), on the fused MI355X kernels: the native
loop behind ``Predictor.elastic_net``.

The attack minimises c * max(kappa - margin, 0) + |x - x0|_2^2 + beta |x - x0|_1 in pixel space by ISTA with FISTA
momentum, and searches the trade-off constant c per image by bisection.  Each image carries two points - the slack
point y, where the gradient is taken, and the shrunk point x, the candidate adversarial example, where success is
judged - and one row kernel, ``ead_step`` (csrc/kernels/ead.hip, one workgroup per image), keeps and updates them with
the nearest success, c and its bracket.  One iteration is six launches on the current stream, with no autograd, no
allocation and no host sync:

    trunk_fwd -> fc1_fwd -> head_margin (CW) -> fc_bwd (role B)   ``ops.chain.GradChain(loss="cw")`` over 2 m rows:
                                                                  rows [0, m) the y points, rows [m, 2 m) the x points
    -> input_grad (plain form, the m y rows only: d margin / d y into one dx buffer)
    -> ead_step (success test and nearest success at x; shrinkage step and momentum: the next x and y, in place)

A search step of ``steps`` updates takes ``steps + 1`` rounds: round ``steps`` has ``search_end`` (it looks at the last
x, bisects c in the kernel and puts both points back to the clean image), the last round of the last search step has
``last`` instead.  The very first round has ``first`` and reads no state.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import native
from .chain import GradChain
from .functional import (CW_C, CW_D_BEST, CW_FOUND_SEARCH, EAD_RULES, cw_dist_scale, ead_beta_n, ead_schedule)
from .fused_net import fused_state


def _buffers(st, rows: int, dev):
    """The loop's row buffers, kept on the net's fused state and reused while they are large enough: ``xin`` [2 rows,
    784], the chain's input (a chunk of m images has its y points in rows [0, m) and its x points in rows [m, 2 m)),
    the gradient ``dx`` [rows, 784] and the doubled labels ``lab`` [2 rows]."""
    buf = getattr(st, "ead_buf", None)
    if buf is None or buf.rows < rows or buf.xin.device != dev:
        buf = st.ead_buf = SimpleNamespace(rows=rows, xin=torch.zeros(2 * rows, 784, dtype=torch.float32, device=dev),
                                           dx=torch.zeros(rows, 784, dtype=torch.float32, device=dev),
                                           lab=torch.zeros(2 * rows, dtype=torch.int32, device=dev))
    return buf


def fused_elastic_net(net, x: torch.Tensor, labels: torch.Tensor, search_steps: int, steps: int, lr: float,
                      c_init: float, beta: float, kappa: float, rule: str, sign: float, lo: float, hi: float,
                      rows_per_launch: int = 4096):
    """``search_steps`` bisection steps of ``steps`` ISTA updates each, in inference semantics (no dropout): ``(x_adv
    float32 [B, 784], d_best float32 [B], found_search int32 [B], c float32 [B])`` on the net's device.  ``x_adv``: the
    nearest shrunk point that was a success (margin ``sign * (max_{j != y} z_j - z_y)`` > 0 and >= ``kappa``, as the
    gradient chain computed it), the clean image where there was none; ``d_best``: its distance by ``rule`` in pixel
    units - "en": |d|_2^2 + beta |d|_1, "l1": |d|_1 - and +inf where none; ``found_search``: 1 + the search step that
    found it, 0 where none; ``c``: the constant of the last search step.  ``functional.ead_step_reference`` has the
    exact form.

    ``x``: float32 [B, 784] normalised rows on the net's device, inside [lo, hi]; ``labels``: [B] integers in [0, 10)
    (not checked here: ``Predictor.elastic_net`` does), the class to leave (``sign`` = +1) or to reach (-1); ``lo``,
    ``hi``: the valid range in normalised units.  The images are independent and run in chunks of at most
    ``rows_per_launch`` images (twice as many chain rows); the result does not depend on the chunking, bit for bit,
    while every chain launch stays on one side of fc1_fwd's 512-row split change.  ``search_steps * (steps + 1)``
    rounds of six launches per chunk, no host sync.  One activation set is taken from and given back to the fused
    state's pool, the row buffers stay on it; the call allocates the results.  The net's mode, parameters, ``.grad``
    and dropout counter stream are untouched."""
    from ..data.datasets import MNIST_STD
    search_steps, steps, rows_per_launch = int(search_steps), int(steps), int(rows_per_launch)
    if search_steps < 1 or steps < 1:
        raise ValueError("fused_elastic_net: search_steps and steps must be at least 1")
    if sign not in (1, -1) or not kappa >= 0 or not lr > 0 or not c_init > 0 or not beta >= 0:
        raise ValueError("fused_elastic_net: need sign +1 or -1, kappa >= 0, lr > 0, c_init > 0 and beta >= 0")
    if rule not in EAD_RULES:
        raise ValueError(f"fused_elastic_net: rule must be 'en' or 'l1', got {rule!r}")
    if rows_per_launch < 1:
        raise ValueError("fused_elastic_net: rows_per_launch must be at least 1")
    st = fused_state(net)
    st.sync()                                   # once: the bf16 shadows follow the parameters
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype != torch.float32 or x.device != dev:
        raise ValueError("fused_elastic_net: x must be float32 [B, 784] on the net's device")
    B = x.shape[0]
    if B < 1:
        raise ValueError("fused_elastic_net: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_elastic_net: {labels.numel()} labels for {B} images")
    x0 = x.contiguous()
    mc = min(B, rows_per_launch)                                        # images per chunk
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    x_adv = torch.empty(B, 784, dtype=torch.float32, device=dev)        # every element is written by a first launch
    fstate = torch.empty(B, 4, dtype=torch.float32, device=dev)
    istate = torch.empty(B, 4, dtype=torch.int32, device=dev)
    rb = _buffers(st, mc, dev)
    sched = [ead_schedule(j, steps, lr) for j in range(steps)] + [(float(lr), 0.0)]      # (round `steps` makes no step)
    head = (float(sign), float(kappa), float(c_init))
    tail = (float(beta), ead_beta_n(beta), float(MNIST_STD), cw_dist_scale(), float(lo), float(hi))
    code = EAD_RULES[rule]
    chain = GradChain(st, 2 * mc, "cw")
    C, s, p = native.load(), native.stream_handle(), native.ptr
    pin, pdx, plab2, ploss = p(rb.xin), p(rb.dx), p(rb.lab), chain.loss_rows
    px0, pbest, pf, pi = p(x0), p(x_adv), p(fstate), p(istate)
    run, grad, step = chain.run, chain.input_grad, C.ead_step
    try:
        for i0 in range(0, B, mc):
            m = min(mc, B - i0)
            o16, o784 = 16 * i0, 3136 * i0
            rb.xin[:m].copy_(x0[i0:i0 + m])                             # a first launch reads x = y = x0
            rb.xin[m:2 * m].copy_(x0[i0:i0 + m])
            rb.lab[:m].copy_(lab[i0:i0 + m])
            rb.lab[m:2 * m].copy_(lab[i0:i0 + m])
            ops = (pdx, ploss, px0 + o784, pin, pin + 3136 * m, pbest + o784, pf + o16, pi + o16, *head)
            for k in range(search_steps):
                final = k == search_steps - 1
                for j in range(steps + 1):
                    end = j == steps
                    run(pin, plab2, 2 * m)
                    grad(pdx, m)                                        # the y rows are the chain's first m
                    step(*ops, *sched[j], *tail, k, code, k == 0 and j == 0, end and not final, end and final, m, s)
    finally:
        chain.release()                         # also when a launcher raised; the next taker is stream ordered
    return x_adv, fstate[:, CW_D_BEST].clone(), istate[:, CW_FOUND_SEARCH].clone(), fstate[:, CW_C].clone()
