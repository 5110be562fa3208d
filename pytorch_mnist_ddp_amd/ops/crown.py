"""CROWN-IBP on the fused MI355X kernels: the native rounds behind ``Predictor.verify_linf`` and
``Predictor.certified_radius_linf`` with ``method="crown-ibp"``.

One round is six launches on the current stream (csrc/kernels/crown.hip, csrc/kernels/ibp.hip), with no autograd, no
allocation and no host sync:

    crown_relax (ibp_trunk + the pooled relaxation record) -> ibp_fc1 -> crown_lambda (fc1 relaxation, lb_ibp)
    -> crown_fc (Lambda fc1.weight, pool relaxation) -> crown_bwd (transposed trunk, concretisation) -> crown_head

The record, the search and the contract are ``ops/ibp.py``'s: an image's bits do not depend on the batch, its row or
the chunking.  A chunk's buffers are about 650 KB an image (``v`` alone 369 KB), so the default chunk is 384 images.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import native
from .functional import CROWN_SLICES, CROWN_SPEC, CROWN_STRIPS, IBP_SPLITS, NCLS, NFLAT, NH, _ibp_setup
from .fused_net import fused_state


def _buffers(st, rows: int, dev):
    """The buffers of a chunk, kept on the net's fused state and reused while large enough."""
    buf = getattr(st, "crown_buf", None)
    if buf is None or buf.rows < rows or buf.pl.device != dev:
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)                       # noqa: E731
        buf = st.crown_buf = SimpleNamespace(
            rows=rows, pl=new(rows * NFLAT), pu=new(rows * NFLAT), relax=new(rows * NFLAT * 4),
            part=new(IBP_SPLITS * rows * 2 * NH), lam=new(rows * CROWN_SPEC * NH), fcb=new(rows * 2 * CROWN_SPEC),
            v=new(rows * NCLS * NFLAT), vb=new(rows * CROWN_SLICES * CROWN_SPEC), sp=new(rows * CROWN_STRIPS * NCLS * 2))
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
    b = _buffers(st, mc, dev)
    _, std, lo, hi = _ibp_setup({}, torch.float32, None, None)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    pp, px, plab, plb, prec = p(st.ms.param), p(x0), p(lab), p(lb), p(rec)
    ppl, ppu, prel, ppart, plam, pfcb, pv, pvb, psp = (p(t) for t in (b.pl, b.pu, b.relax, b.part, b.lam, b.fcb, b.v,
                                                                       b.vb, b.sp))
    for i0 in range(0, B, mc):
        m = min(mc, B - i0)
        r, xi, li = prec + 16 * i0, px + 3136 * i0, plab + 4 * i0
        for _ in range(rounds):
            C.crown_relax(pp, xi, r, ppl, ppu, prel, std, lo, hi, m, s)
            C.ibp_fc1(pp, ppl, ppu, ppart, m, s)
            C.crown_lambda(pp, ppart, li, plam, pfcb, m, s)
            C.crown_fc(pp, prel, plam, pv, pvb, m, s)
            C.crown_bwd(pp, xi, r, prel, pv, li, psp, std, lo, hi, m, s)
            C.crown_head(pfcb, pvb, psp, li, 0, plb + 40 * i0, r, search, m, s)
    return lb


def fused_crown_ibp(net, x: torch.Tensor, labels: torch.Tensor, eps, rows_per_launch: int = 384) -> torch.Tensor:
    """One round: ``lb`` float32 [B, 10] = max(lb_crown, lb_ibp), lower bounds of z_labels - z_j (+inf at j = labels)
    of the fp32 net over the box of ``ops.ibp.fused_ibp``.  ``functional.crown_ibp_reference`` has the exact form."""
    B = x.shape[0]
    e = torch.as_tensor(eps, dtype=torch.float32, device=x.device).expand(B)
    if not bool((e >= 0).all()):
        raise ValueError("fused_crown_ibp: eps must be >= 0")
    rec = torch.zeros(B, 4, dtype=torch.float32, device=x.device)
    rec[:, 0] = e
    return _rounds(net, x, labels, rec, 1, False, rows_per_launch, "fused_crown_ibp")


def fused_crown_ibp_radius(net, x: torch.Tensor, labels: torch.Tensor, eps_max: float, search_steps: int,
                           rows_per_launch: int = 384) -> torch.Tensor:
    """The per-image bisection of the certified radius in [0, ``eps_max``] on the CROWN-IBP bound: ``search_steps + 1``
    rounds, the records float32 [B, 4] = (eps, lo, hi, margin) of ``ops.ibp.fused_ibp_radius`` returned."""
    search_steps = int(search_steps)
    if search_steps < 0 or not eps_max >= 0:
        raise ValueError("fused_crown_ibp_radius: need search_steps >= 0 and eps_max >= 0")
    rec = torch.tensor([eps_max, 0.0, eps_max, 0.0], dtype=torch.float32).repeat(x.shape[0], 1).to(x.device)
    _rounds(net, x, labels, rec, search_steps + 1, True, rows_per_launch, "fused_crown_ibp_radius")
    return rec
