"""Integrated gradients (Sundararajan et al. 2017) and SmoothGrad (Smilkov et al. 2017) on the fused MI355X
kernels: the native loop behind ``Predictor.attribute``.

Both methods are "n gradient rows per image, then a reduction" of g(.) = d NLL_y / d x, the gradient the attack
loop's chain computes; both attribute log p_y(x), hence the factor -1:

    integrated gradients:  attr = -(x - b) * (1/n) * sum_{s<n} g(b + alpha_s (x - b)),  alpha_s = (s + 1/2) / n
    SmoothGrad:            attr = -(1/n) * sum_{s<n} g(x + sigma z_s)

One chunk of rows is seven launches on the current stream, with no autograd, no host sync and no allocation:

    attr_path (csrc/kernels/attr.hip: the rows of the path) or smooth_noise (csrc/kernels/smooth.hip: the noised rows)
    -> the four launches of the gradient chain (``ops.chain.GradChain``) -> input_grad in its plain form
    -> attr_reduce (csrc/kernels/attr.hip: the per-image sum in ascending sample order, accumulating over the sample
       chunks of an image; the last one finishes: * -1/n, and * (x - b) for integrated gradients)

The reduction's fixed serial order makes an image's sum the same bits under any chunking of its samples.  (The
gradient rows themselves follow, up to fc1_fwd's split-K: 32-way below 512 rows a launch and 4-way from there, so
launches on either side of 512 rows can differ in the last bits.)
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import native
from .chain import GradChain
from .functional import ATTR_FINISH_NONE, ATTR_FINISH_PATH, ATTR_FINISH_SCALE
from .fused_net import fused_state
from .smooth import smooth_chunks

METHODS = ("integrated_gradients", "smoothgrad")


def _buffers(st, rows: int, dev):
    """The row buffer and the gradient buffer of the loop, kept on the net's fused state and reused while they are
    large enough (as ``ops.smooth`` keeps ``smooth_buf``)."""
    buf = getattr(st, "attr_buf", None)
    if buf is None or buf.rows < rows or buf.x.device != dev:
        buf = st.attr_buf = SimpleNamespace(
            rows=rows,
            x=torch.zeros(rows, 784, dtype=torch.float32, device=dev),
            dx=torch.zeros(rows, 784, dtype=torch.float32, device=dev))
    return buf


def fused_attribution(net, x: torch.Tensor, labels: torch.Tensor, method: str, n: int, base=0.0,
                      sigma_n: float = 0.0, seed: int = 0, ids=None, rows_per_launch: int = 8192) -> torch.Tensor:
    """float32 [B, 784] attribution of log p_labels(x), in inference semantics (no dropout).

    ``x``: uint8 [B, 784] raw rows or float32 [B, 784] normalised rows on the net's device; ``labels``: [B] integers
    in [0, 10) (not checked here: ``Predictor.attribute`` does); ``method``: ``"integrated_gradients"`` with ``n``
    path points from ``base`` (a float in normalised units or a float32 [B, 784] tensor), or ``"smoothgrad"`` with
    ``n`` noised copies of standard deviation ``sigma_n`` > 0 (normalised units), image j drawing the samples [0, n)
    of ``smooth_noise``'s stream under (``seed``, ``ids[j]``; default j).  Per chunk of ``smooth_chunks(B, n, ids,
    rows_per_launch)`` the seven launches of the module docstring run on one activation set taken from and given back
    to the fused state's pool plus the row and gradient buffers kept on it; the call allocates the expanded labels,
    the running sums and the result.  The result does not depend on ``rows_per_launch``, bit for bit, while every
    launch stays on one side of fc1_fwd's 512-row split change.  The net's mode, parameters, ``.grad`` and dropout
    counter stream are untouched."""
    if method not in METHODS:
        raise ValueError(f"fused_attribution: method must be one of {METHODS}, got {method!r}")
    path = method == "integrated_gradients"
    st = fused_state(net)
    st.sync()
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or x.device != dev:
        raise ValueError("fused_attribution: x must be uint8 or float32 [B, 784] on the net's device")
    B, n = x.shape[0], int(n)
    if B < 1 or n < 1:
        raise ValueError("fused_attribution: B and n must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_attribution: {labels.numel()} labels for {B} images")
    ids = list(range(B)) if ids is None else [int(v) for v in ids]
    if len(ids) != B:
        raise ValueError(f"fused_attribution: {len(ids)} ids for {B} images")
    pbase, base_value = 0, 0.0
    if path:
        if isinstance(base, torch.Tensor):
            if base.shape != (B, 784) or base.dtype != torch.float32 or base.device != dev:
                raise ValueError("fused_attribution: a baseline tensor must be float32 [B, 784] on the net's device")
            base = base.contiguous()
            pbase = native.ptr(base)
        else:
            base_value = float(base)
    elif not sigma_n > 0:
        raise ValueError(f"fused_attribution: sigma_n must be > 0, got {sigma_n}")
    x = x.contiguous()
    plan = smooth_chunks(B, n, ids if not path else list(range(B)), rows_per_launch)
    rows_max = max(m * ns for _, m, _, ns in plan)
    lab = labels.reshape(B).to(dev, torch.int32).repeat_interleave(n).contiguous()   # [B * n]: every chunk points into it
    acc = torch.empty(B, 784, dtype=torch.float32, device=dev)
    out = torch.empty(B, 784, dtype=torch.float32, device=dev)
    rb = _buffers(st, rows_max, dev)
    chain = GradChain(st, rows_max)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px, pdx, plab, pacc, pout = p(rb.x), p(rb.dx), p(lab), p(acc), p(out)
    u8 = x.dtype == torch.uint8
    src, row_bytes = p(x), 784 * x.element_size()
    seed = int(seed) & (2 ** 64 - 1)
    scale = float(np.float32(-1.0) / np.float32(n))
    run, grad = chain.run, chain.input_grad
    for i0, m, s0, ns in plan:
        rows = m * ns
        at = src + i0 * row_bytes
        xu8, xf32 = (at, 0) if u8 else (0, at)
        bat = pbase + i0 * 3136 if pbase else 0
        if path:
            C.attr_path(xu8, xf32, bat, base_value, px, s0, n, m, ns, s)
        else:
            C.smooth_noise(xu8, xf32, px, sigma_n, seed, s0, ids[i0], m, ns, s)
        run(px, plab + 4 * (i0 * n + s0), rows)
        grad(pdx, rows)
        last = s0 + ns == n
        finish = (ATTR_FINISH_PATH if path else ATTR_FINISH_SCALE) if last else ATTR_FINISH_NONE
        C.attr_reduce(pdx, pacc + i0 * 3136, pout + i0 * 3136 if last else 0, xu8 if path and last else 0,
                      xf32 if path and last else 0, bat if last else 0, base_value, scale, m, ns, s0 > 0, finish, s)
    chain.release()                             # last use enqueued: the next taker is stream ordered after it
    return out
