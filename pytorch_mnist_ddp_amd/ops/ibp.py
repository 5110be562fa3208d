"""Interval bound propagation on the fused MI355X kernels: the native rounds behind ``Predictor.verify_linf`` and
``Predictor.certified_radius_linf``.

One round bounds the fp32 net's logit differences over each image's L-inf box and is three launches on the current
stream (csrc/kernels/ibp.hip), with no autograd, no allocation and no host sync:

    ibp_trunk (input box, conv1, conv2 on the fp32 MFMA, ReLU, pool) -> ibp_fc1 (split-K partials) -> ibp_head (lb)

Each image's eps lives in its 16-byte record ``(eps, lo, hi, margin)`` on the device; with ``search`` the head bisects
it, so a radius search of ``search_steps`` bisections is ``search_steps + 1`` rounds and never returns to the host.
The parameters are the fp32 ones (``ModelState.param``), whatever the predictor's dtype.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import native
from .functional import IBP_SPLITS, NCLS, NFLAT, NH, _ibp_setup
from .fused_net import fused_state


def _buffers(st, rows: int, dev):
    """The pooled bounds and the fc1 slab of a chunk, kept on the net's fused state and reused while large enough."""
    buf = getattr(st, "ibp_buf", None)
    if buf is None or buf.rows < rows or buf.pl.device != dev:
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)                       # noqa: E731
        buf = st.ibp_buf = SimpleNamespace(rows=rows, pl=new(rows * NFLAT), pu=new(rows * NFLAT),
                                           part=new(IBP_SPLITS * rows * 2 * NH))
    return buf


def _rounds(net, x: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor, rounds: int, search: bool,
            rows_per_launch: int, who: str) -> torch.Tensor:
    """``rounds`` rounds over the images in chunks of at most ``rows_per_launch``; ``lb`` [B, 10] of the last round.
    ``rec`` float32 [B, 4] on the device is read, and updated when ``search``."""
    rows_per_launch = int(rows_per_launch)
    if rows_per_launch < 1:
        raise ValueError(f"{who}: rows_per_launch must be at least 1")
    st = fused_state(net)
    st.sync()                                   # the flat fp32 buffer follows the module's parameters
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype != torch.float32 or x.device != dev:
        raise ValueError(f"{who}: x must be float32 [B, 784] on the net's device")
    B = x.shape[0]
    if B < 1:
        raise ValueError(f"{who}: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"{who}: {labels.numel()} labels for {B} images")
    x0 = x.contiguous()
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    lb = torch.empty(B, NCLS, dtype=torch.float32, device=dev)
    mc = min(B, rows_per_launch, native.load().IBP_MAX_B)
    buf = _buffers(st, mc, dev)
    _, std, lo, hi = _ibp_setup({}, torch.float32, None, None)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    pp, px, plab, plb, prec = p(st.ms.param), p(x0), p(lab), p(lb), p(rec)
    ppl, ppu, ppart = p(buf.pl), p(buf.pu), p(buf.part)
    trunk, fc1, head = C.ibp_trunk, C.ibp_fc1, C.ibp_head
    for i0 in range(0, B, mc):
        m = min(mc, B - i0)
        r = prec + 16 * i0
        for _ in range(rounds):
            trunk(pp, px + 3136 * i0, r, ppl, ppu, std, lo, hi, m, s)
            fc1(pp, ppl, ppu, ppart, m, s)
            head(pp, ppart, plab + 4 * i0, plb + 40 * i0, r, search, m, s)
    return lb


def fused_ibp(net, x: torch.Tensor, labels: torch.Tensor, eps, rows_per_launch: int = 8192) -> torch.Tensor:
    """One round: ``lb`` float32 [B, 10], lower bounds of z_labels - z_j (+inf at j = labels) of the fp32 net over the
    box of radius ``eps`` (pixel units on [0, 1]; a number or [B]) around the normalised float32 rows ``x`` [B, 784] on
    the net's device, clipped to the valid pixel range.  ``functional.ibp_reference`` has the exact form.  An image is
    certified where ``lb.min(dim=1) > 0``."""
    B = x.shape[0]
    e = torch.as_tensor(eps, dtype=torch.float32, device=x.device).expand(B)
    if not bool((e >= 0).all()):
        raise ValueError("fused_ibp: eps must be >= 0")
    rec = torch.zeros(B, 4, dtype=torch.float32, device=x.device)
    rec[:, 0] = e
    return _rounds(net, x, labels, rec, 1, False, rows_per_launch, "fused_ibp")


def fused_ibp_radius(net, x: torch.Tensor, labels: torch.Tensor, eps_max: float, search_steps: int,
                     rows_per_launch: int = 8192) -> torch.Tensor:
    """The per-image bisection of the certified radius in [0, ``eps_max``]: ``search_steps + 1`` rounds, the records
    float32 [B, 4] = (eps, lo, hi, margin) returned.  ``lo`` is an eps at which the bound itself was positive, or 0;
    ``hi`` one at which it was not, or ``eps_max``; ``margin`` = min_j lb_j of the last round.  An image's record does
    not depend on the batch, its row or the chunking, bit for bit."""
    search_steps = int(search_steps)
    if search_steps < 0 or not eps_max >= 0:
        raise ValueError("fused_ibp_radius: need search_steps >= 0 and eps_max >= 0")
    rec = torch.tensor([eps_max, 0.0, eps_max, 0.0], dtype=torch.float32).repeat(x.shape[0], 1).to(x.device)
    _rounds(net, x, labels, rec, search_steps + 1, True, rows_per_launch, "fused_ibp_radius")
    return rec
