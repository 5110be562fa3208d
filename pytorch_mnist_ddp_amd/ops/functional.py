"""Kernel-level functional API over torch tensors.

Each function launches exactly one of the hand-written kernels on the current torch stream,
with torch-allocated inputs/outputs.  These are the units the numerics tests compare against
fp32 torch references (SURVEY §4 tier T1) and the building blocks of the module-level
``Net.forward`` on GPU.  ``StepBuffers`` allocates every per-batch activation at once.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import native
from .chain import param_ptrs, round_up  # noqa: F401  (round_up: this module's callers import it from here)

NFLAT, NH, NCLS = 9216, 128, 10
DYC_REC = 144                       # compact dy record bytes (csrc/include/kernels.h DYC_REC)


def _C():
    return native.load()


def _s() -> int:
    return native.stream_handle()


@dataclass
class StepBuffers:
    B: int
    a1: torch.Tensor          # bf16 [B,26,26,32]
    p: torch.Tensor           # bf16 [Bp64, 9216]
    pmask: torch.Tensor       # u8 [B, 9216]
    z1part: torch.Tensor      # f32 [KSPLIT, B, 128]
    loss_rows: torch.Tensor   # f32 [B]
    dz1: torch.Tensor         # bf16 [Bp64, 128]
    h_bf: torch.Tensor        # bf16 [Bp64, 128]
    dl_bf: torch.Tensor       # bf16 [Bp64, 16]
    dyc: torch.Tensor         # uint8 [B, 144*144] compact grad wrt conv2 output (pooled grads + argmax planes)
    fcpart: torch.Tensor      # f32 fc-gradient split partials (B > 1024), else a 1-element placeholder
    c1part: torch.Tensor      # f32 [4B, 320]
    w2part: torch.Tensor      # f32 [G, 18496]
    correct: torch.Tensor     # i32 [B]
    logp: torch.Tensor        # f32 [B, 10]

    @staticmethod
    def allocate(B: int, device) -> "StepBuffers":
        C = _C()
        Bp = round_up(B, 64)
        G = C.conv_wgrad_groups(B)
        z = dict(device=device)
        bf = dict(dtype=torch.bfloat16, device=device)
        return StepBuffers(
            B=B,
            a1=torch.zeros(B, 26, 26, 32, **bf),
            p=torch.zeros(Bp, NFLAT, **bf),
            pmask=torch.zeros(B, NFLAT, dtype=torch.uint8, **z),
            z1part=torch.zeros(C.FC1_KSPLIT, B, NH, dtype=torch.float32, **z),
            loss_rows=torch.zeros(B, dtype=torch.float32, **z),
            dz1=torch.zeros(Bp, NH, **bf),
            h_bf=torch.zeros(Bp, NH, **bf),
            dl_bf=torch.zeros(Bp, 16, **bf),
            dyc=torch.zeros(B, 144 * DYC_REC, dtype=torch.uint8, device=device),
            fcpart=torch.zeros(max(1, (C.fc_bwd_splits(B) > 1) * C.fc_bwd_splits(B) * C.FCB_PART_STRIDE),
                               dtype=torch.float32, device=device),
            c1part=torch.zeros(4 * B, 320, dtype=torch.float32, **z),
            w2part=torch.zeros(G, 18432 + 64, dtype=torch.float32, **z),
            correct=torch.zeros(B, dtype=torch.int32, **z),
            logp=torch.zeros(B, NCLS, dtype=torch.float32, **z),
        )


@dataclass
class EvalBuffers:
    """The set of the three-launch eval forward (``chain.EvalChain``); ``rows`` rows serve any launch of fewer."""
    rows: int
    p: torch.Tensor           # bf16 [rows64, 9216]
    z1part: torch.Tensor      # f32 [KSPLIT, rows, 128]
    loss_rows: torch.Tensor   # f32 [rows]
    correct: torch.Tensor     # i32 [rows]
    logp: torch.Tensor        # f32 [rows, 10]
    pred: None = None         # (``InferBuffers`` holds one: the Predictor reads either set)
    x: torch.Tensor | None = None   # f32 [rows, 784] input rows, set by a loop that writes its own (ops.smooth)

    @staticmethod
    def allocate(rows: int, device) -> "EvalBuffers":
        def z(*shape, dtype=torch.float32):
            return torch.zeros(*shape, dtype=dtype, device=device)
        return EvalBuffers(rows, z(round_up(rows, 64), NFLAT, dtype=torch.bfloat16), z(_C().FC1_KSPLIT, rows, NH),
                           z(rows), z(rows, dtype=torch.int32), z(rows, NCLS))


def pmask_flat(pmask: torch.Tensor) -> torch.Tensor:
    """The trunk's pool/dropout flags in torch flatten order [B, 9216] (channel-major) from the device
    layout [B][36][64][4] (pooled position / 4, channel, position % 4; mnist_common.h)."""
    B = pmask.shape[0]
    return pmask.view(B, 36, 64, 4).permute(0, 2, 1, 3).reshape(B, 9216)


def trunk_fwd(ms, data_u8: torch.Tensor | None, idx: torch.Tensor | None, buf: StepBuffers, train: bool,
              idx_stride: int = 0, state: torch.Tensor | None = None, xin: torch.Tensor | None = None) -> None:
    """``xin`` (float32 [B, 784], already normalised) replaces the dataset rows ``data_u8`` / ``idx``."""
    p, w = native.ptr, param_ptrs(ms)
    _C().trunk_fwd(p(data_u8), p(idx), idx_stride, p(state if state is not None else ms.state),
                   w.c1w, w.c1b, w.w2f, w.c2b, p(buf.a1) if train else 0, p(buf.p),
                   p(buf.pmask) if train else 0, buf.B, train, _s(), xin=p(xin))


def fc1_fwd(ms, buf: StepBuffers) -> None:
    p = native.ptr
    _C().fc1_fwd(p(buf.p), p(ms.w1), p(buf.z1part), buf.B, _s())


def head_train(ms, labels: torch.Tensor, idx: torch.Tensor | None, buf: StepBuffers, idx_stride: int = 0,
               state: torch.Tensor | None = None, inv_batch: float | None = None) -> None:
    """``idx`` None: ``labels`` holds one int32 label per batch row.  ``inv_batch``: the loss scale
    (default 1 / B, the mean NLL; 1.0 gives the gradient of the summed NLL)."""
    p, w = native.ptr, param_ptrs(ms)
    B = buf.B
    _C().head_train(p(buf.z1part), w.f1b, w.f2w, w.f2b, p(labels), p(idx), idx_stride,
                    p(state if state is not None else ms.state), 1.0 / B if inv_batch is None else inv_batch,
                    p(buf.loss_rows), p(buf.dz1), p(buf.h_bf), p(buf.dl_bf), B, round_up(B, 32), _s())


MARGIN_KINDS = {"cw": 0, "dlr": 1, "dlr_t": 2}      # head_margin loss codes (csrc/include/kernels.h MarginKind)
DLR_GUARD = 1e-12                                   # added to the DLR denominators (the authors' guard)


def first_max_excluding(z: torch.Tensor, taken: torch.Tensor) -> torch.Tensor:
    """int64 [R]: per row of ``z`` [R, C] the first maximum over the classes whose ``taken`` [R, C] flag is False,
    by explicit > comparisons in ascending class order - the first of equals wins, a NaN never wins over an earlier
    class.  The selection rule of ``head_margin`` (at least one class per row must be free)."""
    R, C = z.shape
    idx = torch.full((R,), -1, dtype=torch.long, device=z.device)
    best = torch.zeros(R, dtype=z.dtype, device=z.device)
    for c in range(C):
        take = ~taken[:, c] & ((idx < 0) | (z[:, c] > best))
        best = torch.where(take, z[:, c], best)
        idx = torch.where(take, torch.full_like(idx, c), idx)
    return idx


def margin_selections(z: torch.Tensor, labels: torch.Tensor):
    """``(o, pi1, pi2, pi3, pi4)``, int64 [R] each, of the logits (or log-probs) ``z`` [R, 10]: ``o`` the first
    maximum over j != label, ``pi1`` the first maximum, ``pi2`` .. ``pi4`` the first maximum over the classes not yet
    taken (``first_max_excluding``)."""
    z = z.detach()
    cls = torch.arange(z.shape[1], device=z.device)[None, :]
    o = first_max_excluding(z, cls == labels.long().reshape(-1, 1))
    taken = torch.zeros_like(z, dtype=torch.bool)
    pis = []
    for _ in range(4):
        pis.append(first_max_excluding(z, taken))
        taken = taken | (cls == pis[-1][:, None])
    return (o, *pis)


def margin_loss_reference(logits_or_logp: torch.Tensor, labels: torch.Tensor, kind: str,
                          targets: torch.Tensor | None = None) -> torch.Tensor:
    """The per-row margin loss [R] of ``head_margin`` in differentiable torch ops on any device, in the dtype of the
    [R, 10] logits - or log-probs: the losses are shift-invariant.  ``kind``, with y = ``labels`` and the selections
    of ``margin_selections`` (explicit, not ``torch.sort``, so ties are defined as in the kernel):

        "cw":     z[o] - z[y]
        "dlr":    (z[o] - z[y]) / ((z[pi1] - z[pi3]) + 1e-12)
        "dlr_t":  (z[y] - z[t]) / ((z[pi1] - 0.5 (z[pi3] + z[pi4])) + 1e-12),  t = ``targets`` (t != y)

    Autograd treats the selections as constants; the gradient it gives is the ``dl`` of the kernel at scale 1."""
    if kind not in MARGIN_KINDS:
        raise ValueError(f"margin_loss_reference: kind must be one of {sorted(MARGIN_KINDS)}, got {kind!r}")
    if kind == "dlr_t" and targets is None:
        raise ValueError("margin_loss_reference: the targeted DLR loss needs targets")
    z = logits_or_logp
    y = labels.long().reshape(-1).to(z.device)
    o, p1, _, p3, p4 = margin_selections(z, y)
    at = lambda i: z.gather(1, i[:, None]).squeeze(1)                                       # noqa: E731
    if kind == "cw":
        return at(o) - at(y)
    if kind == "dlr":
        return (at(o) - at(y)) / ((at(p1) - at(p3)) + DLR_GUARD)
    t = targets.long().reshape(-1).to(z.device)
    return (at(y) - at(t)) / ((at(p1) - 0.5 * (at(p3) + at(p4))) + DLR_GUARD)


def head_margin_reference(z1part: torch.Tensor, b_fc1: torch.Tensor, w_fc2: torch.Tensor, b_fc2: torch.Tensor,
                          labels: torch.Tensor, kind: str, targets: torch.Tensor | None = None, scale: float = 1.0,
                          dtype=None) -> dict:
    """``head_margin`` in torch ops on any device, in ``dtype`` (default: that of ``z1part`` [ksplit, R, 128]): z1 =
    bias + the partials summed in chunk order, h = relu(z1), the logits, the loss rows, ``dl`` [R, 10] with the terms
    added in the kernel's order, and dz1 = (z1 > 0) (dl . w_fc2), all before any rounding to bf16."""
    if kind not in MARGIN_KINDS:
        raise ValueError(f"head_margin_reference: kind must be one of {sorted(MARGIN_KINDS)}, got {kind!r}")
    if kind == "dlr_t" and targets is None:
        raise ValueError("head_margin_reference: the targeted DLR loss needs targets")
    dt = z1part.dtype if dtype is None else dtype
    s = torch.zeros_like(z1part[0], dtype=dt)
    for c in range(z1part.shape[0]):
        s = s + z1part[c].to(dt)
    z1 = b_fc1.to(dt) + s
    h = torch.relu(z1)
    z = h @ w_fc2.to(dt).t() + b_fc2.to(dt)
    y = labels.long().reshape(-1).to(z.device)
    o, p1, _, p3, p4 = margin_selections(z, y)
    at = lambda i: z.gather(1, i[:, None]).squeeze(1)                                       # noqa: E731
    dl = torch.zeros_like(z)
    add = lambda i, v: dl.scatter_add_(1, i[:, None], v[:, None])                           # noqa: E731
    sc = torch.full_like(z[:, 0], float(scale))
    if kind == "cw":
        loss = at(o) - at(y)
        add(o, sc)
        add(y, -sc)
    elif kind == "dlr":
        d = (at(p1) - at(p3)) + DLR_GUARD
        loss = (at(o) - at(y)) / d
        add(o, sc / d)
        add(y, -(sc / d))
        q = (sc * loss) / d
        add(p1, -q)
        add(p3, q)
    else:
        t = targets.long().reshape(-1).to(z.device)
        d = (at(p1) - 0.5 * (at(p3) + at(p4))) + DLR_GUARD
        loss = (at(y) - at(t)) / d
        add(y, sc / d)
        add(t, -(sc / d))
        q = (sc * loss) / d
        add(p1, -q)
        add(p3, 0.5 * q)
        add(p4, 0.5 * q)
    dz1 = (dl @ w_fc2.to(dt)) * (z1 > 0)
    return dict(z1=z1, h=h, logits=z, loss=loss, dl=dl, dz1=dz1, d=None if kind == "cw" else d)


def head_margin(ms, labels: torch.Tensor, buf: StepBuffers, kind: str, targets: torch.Tensor | None = None,
                scale: float = 1.0) -> None:
    """One launch of ``head_margin`` (csrc/kernels/fc_head.hip) on ``buf.z1part``: ``head_train``'s forward without
    dropout and the ``kind`` margin loss (``margin_loss_reference``) of the int32 [B] ``labels`` (``"dlr_t"``: and
    int32 [B] ``targets``) into ``buf.loss_rows``, ``scale`` times its gradient into ``buf.dl_bf`` / ``buf.dz1``,
    relu(z1) into ``buf.h_bf``, under ``head_train``'s padding contract."""
    if kind not in MARGIN_KINDS:
        raise ValueError(f"head_margin: kind must be one of {sorted(MARGIN_KINDS)}, got {kind!r}")
    p, w = native.ptr, param_ptrs(ms)
    B = buf.B
    _C().head_margin(p(buf.z1part), w.f1b, w.f2w, w.f2b, p(labels), p(targets), MARGIN_KINDS[kind], float(scale),
                     p(buf.loss_rows), p(buf.dz1), p(buf.h_bf), p(buf.dl_bf), B, round_up(B, 32), _s())


def head_eval(ms, labels: torch.Tensor | None, idx: torch.Tensor | None, buf: StepBuffers) -> None:
    p, w = native.ptr, param_ptrs(ms)
    _C().head_eval(p(buf.z1part), w.f1b, w.f2w, w.f2b, p(labels), p(idx), p(buf.loss_rows), p(buf.correct),
                   p(buf.logp), buf.B, _s())


# fc_bwd launches other than the whole step's (role = -1): one workgroup role of the kernel, the lean
# fc1 weight-gradient kernel, the role pairs the side schedules launch (B > 1024: split partials, no
# reduce) and fc_grad_reduce alone
FC_ROLE_C, FC_ROLE_A, FC_ROLE_B, FC_DW1, FC_ROLES_CB, FC_ROLES_CA, FC_ROLES_B, FC_REDUCE = range(8)
CONV_DGRAD, CONV_WGRAD, CONV_REDUCE, CONV_ALL = 1, 2, 4, 7      # conv_bwd stage mask


ADA_ALL, ADA_FC, ADA_CONV = 0, 1, 2                             # adadelta_step regions (kernels.h AdadeltaRegion)
ADA_FC_TILES = 577                  # workgroups of the fc region's full grid; fewer walk the tiles grid-stride
RED_W2_PARTS, RED_ALL_PARTS = 289, 309                          # conv reduce parts: conv2, then conv1 (kernels.h)
# conv_bwd(update=...): the reduce stage fused with the Adadelta step (adadelta.hip)
UPD_WHOLE, UPD_C1 = "whole", "c1"                               # or ("parts", lo, hi)


def _ada_args(ms, wt: bool, advance_step: bool) -> dict:
    """AdadeltaArgs of a stand-alone launch (completion holds and start signal null: the engine's)."""
    d = ms.buffers()
    d.pop("state")
    d.update(rho=ms.rho, eps=ms.eps, weight_decay=ms.weight_decay, wt=bool(wt),
             state_inc=native.ptr(ms.state) if advance_step else 0)
    return d


def fc_bwd(ms, buf: StepBuffers, grad_scale: float = 1.0, loss_log: torch.Tensor | None = None,
           role: int = -1, state: torch.Tensor | None = None, update: bool = False, wt: bool = False) -> None:
    """``update``: roles C + A with the fc Adadelta step in their epilogues (``fc_wgrad_update``, the
    OVERLAP step at one split; ``wt``: write-through stores).  The launcher refuses more than one split,
    a grad scale other than 1 and a foreign grad buffer."""
    p = native.ptr
    B = buf.B
    _C().fc_bwd(p(buf.dz1), p(buf.p), p(buf.pmask), param_ptrs(ms).w1t, p(buf.h_bf), p(buf.dl_bf), p(buf.loss_rows),
                p(state if state is not None else ms.state), p(ms.grad), p(buf.dyc), p(loss_log), grad_scale,
                1.0 / B, B, round_up(B, 32), _s(), role=role, part=p(buf.fcpart),
                ada=_ada_args(ms, wt, False) if update else None)


def conv_bwd(ms, data_u8: torch.Tensor, idx: torch.Tensor, buf: StepBuffers, grad_scale: float = 1.0,
             idx_stride: int = 0, stages: int = CONV_ALL, xin: torch.Tensor | None = None,
             c1red: torch.Tensor | None = None, update=None, wt: bool = False,
             advance_step: bool = False) -> None:
    """conv2 dgrad (+ conv1 weight-gradient partials), conv2 wgrad and the partials' reduce; ``stages``
    selects the launches.  ``xin`` (fp32 [B,784]) replaces the dataset rows; with ``c1red`` (f32
    [C1_PRE_SLABS, 320]) the dgrad stage also pre-reduces the conv1 partials and the reduce reads those.
    ``update`` replaces the reduce launch by one fused with the Adadelta step: ``UPD_WHOLE`` (the serial
    step's single launch, which also updates the fc region from ``ms.grad``), ``("parts", lo, hi)`` (reduce
    parts [lo, hi) of the conv bucket only) or ``UPD_C1`` (the conv1 parts on one-wave workgroups)."""
    p, w = native.ptr, param_ptrs(ms)
    form, lo, hi = 0, 0, 0
    if update == UPD_WHOLE:
        form = 1
    elif update == UPD_C1:
        form = 3
    elif update is not None:
        kind, lo, hi = update
        if kind != "parts":
            raise ValueError(f"conv_bwd: unknown update form {update!r}")
        form = 2
    _C().conv_bwd(p(buf.dyc), p(buf.a1), w.w2d, w.c1w, w.c1b, p(data_u8), p(idx), idx_stride, p(ms.state),
                  p(buf.c1part), p(buf.w2part), p(ms.grad), grad_scale, buf.B, _s(), xin=p(xin), stages=stages,
                  c1red=p(c1red), update=form, upd_lo=lo, upd_hi=hi,
                  ada=_ada_args(ms, wt, advance_step) if form else None)


def _grid_kw(name: str, grid: int) -> dict:
    """The ``grid`` keyword of the two input_grad launches: absent for 0 (the plan), refused when negative."""
    if grid < 0:
        raise ValueError(f"{name}: grid must not be negative")
    return {"grid": int(grid)} if grid else {}


def input_grad(ms, buf: StepBuffers, out: torch.Tensor | None = None, grid: int = 0) -> torch.Tensor:
    """Gradient wrt the normalised input, float32 [B, 784], from one launch of ``input_grad.hip`` on
    what the conv backward reads (``buf.dyc`` after ``fc_bwd``, ``buf.a1``, the conv weights).  Every
    element of ``out`` is written; it needs no zeroing.  ``grid`` (the tests'): 0 = the planned grid; a
    positive value only shrinks it - the same bits on any grid."""
    B = buf.B
    kw = _grid_kw("input_grad", grid)
    out = _out_rows("input_grad", "out", out, B, buf.dyc.device)
    p, w = native.ptr, param_ptrs(ms)
    _C().input_grad(p(buf.dyc), p(buf.a1), w.w2d, w.c1w, p(out), B, _s(), **kw)
    return out.view(B, 784)


def _f32_rows(name: str, what: str, t: torch.Tensor, B: int, device, at_least: str | None = None) -> None:
    """``t`` must be contiguous float32 [B, 784] on ``device``; ``at_least`` (the message's name for B): or more rows."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or \
            (t.numel() < B * 784 if at_least else t.numel() != B * 784):
        shape = f"with at least {at_least} rows of 784" if at_least else "[B, 784]"
        raise ValueError(f"{name}: {what} must be contiguous float32 {shape} on the buffers' device")


def _out_rows(name: str, what: str, out: torch.Tensor | None, rows: int, device,
              at_least: str | None = None) -> torch.Tensor:
    """The output ``out`` of a row kernel: a new float32 [rows, 784] when None, else checked as ``_f32_rows`` does."""
    if out is None:
        return torch.empty(rows, 784, dtype=torch.float32, device=device)
    _f32_rows(name, what, out, rows, device, at_least)
    return out


def _src_ptrs(x: torch.Tensor) -> tuple[int, int]:
    """(uint8 pointer, float32 pointer) of the image rows ``x``: the one it is, and 0."""
    return (native.ptr(x), 0) if x.dtype == torch.uint8 else (0, native.ptr(x))


def _check_rows(name: str, expr: str, rows: int) -> None:
    """A launch takes at most ``SMOOTH_MAX_ROWS`` rows; ``expr`` is the caller's name for ``rows``."""
    if rows > SMOOTH_MAX_ROWS:
        raise ValueError(f"{name}: {expr} = {rows} rows exceed SMOOTH_MAX_ROWS = {SMOOTH_MAX_ROWS} a launch")


def input_grad_step(ms, buf: StepBuffers, x: torch.Tensor, x0: torch.Tensor, eps: float, alpha: float,
                    lo: float, hi: float, out: torch.Tensor | None = None,
                    dx: torch.Tensor | None = None, grid: int = 0) -> torch.Tensor:
    """One projected signed-gradient step on the normalised image from one launch of ``input_grad.hip``
    in its step form: with ``g`` what ``input_grad`` returns on the same buffers,

        t = x + alpha * sign(g);  t = min(max(t, x0 - eps), x0 + eps);  out = min(max(t, lo), hi)

    elementwise in float32 (a NaN in ``g`` reaches ``out``).  ``x``, ``x0``, ``out``: float32 [B, 784];
    ``out`` may be ``x`` itself (in place) and is allocated when None.  ``dx`` (optional, float32
    [B, 784], no overlap with the others) also receives ``g``.  ``grid``: as ``input_grad``'s."""
    B, dev = buf.B, buf.dyc.device
    kw = _grid_kw("input_grad_step", grid)
    _f32_rows("input_grad_step", "x", x, B, dev)
    _f32_rows("input_grad_step", "x0", x0, B, dev)
    out = _out_rows("input_grad_step", "out", out, B, dev)
    if out.data_ptr() == x0.data_ptr():
        raise ValueError("input_grad_step: out must not be x0 (the centre of the eps ball is read, not written)")
    if dx is not None:
        _f32_rows("input_grad_step", "dx", dx, B, dev)
        if dx.data_ptr() in (x.data_ptr(), x0.data_ptr(), out.data_ptr()):
            raise ValueError("input_grad_step: dx must not alias x, x0 or out")
    if not (eps >= 0 and alpha >= 0 and lo <= hi):
        raise ValueError("input_grad_step: need eps >= 0, alpha >= 0 and lo <= hi")
    p, w = native.ptr, param_ptrs(ms)
    _C().input_grad_step(p(buf.dyc), p(buf.a1), w.w2d, w.c1w, p(x), p(x0), p(out), alpha, eps, lo, hi, B, _s(),
                         dx=p(dx), **kw)
    return out.view(B, 784)


PGD_L2_TINY = 1e-12                 # floor of both norms of the L2 step (csrc/include/kernels.h PGD_L2_TINY)


def pgd_l2_step_reference(dx: torch.Tensor, x: torch.Tensor, x0: torch.Tensor, eps: float, alpha: float,
                          lo: float, hi: float) -> torch.Tensor:
    """The L2 step of ``pgd_l2_step`` in torch ops, on any device and dtype (the CPU / fp32 path of
    ``Predictor.adversarial``; in float64 the oracle of the kernel's tests).  All [B, 784]."""
    n = dx.square().sum(dim=1, keepdim=True).sqrt()
    t = x + (alpha / n.clamp_min(PGD_L2_TINY)) * dx
    d = t - x0
    m = d.square().sum(dim=1, keepdim=True).sqrt()
    d = d * (eps / m.clamp_min(PGD_L2_TINY)).clamp_max(1.0)
    return (x0 + d).clamp(lo, hi)


def pgd_l2_step(dx: torch.Tensor, x: torch.Tensor, x0: torch.Tensor, eps: float, alpha: float,
                lo: float, hi: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """One L2 projected-gradient step on the normalised image from one launch of ``attack_step.hip``: per
    image, with ``g`` = ``dx`` (what ``input_grad`` returns),

        t = x + alpha * g / max(|g|, TINY);  d = t - x0;  out = min(max(x0 + d * min(1, eps / max(|d|, TINY)), lo), hi)

    in float32 with both L2 norms a fixed-order sum (a NaN in an image's ``g`` makes that image's ``out``
    NaN).  ``alpha`` < 0 descends.  ``dx``, ``x``, ``x0``, ``out``: float32 [B, 784] on the GPU; ``x0`` must
    lie in [lo, hi] for ``out`` to stay in the eps ball; ``out`` may be ``x`` itself (in place) and is
    allocated when None."""
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("pgd_l2_step: x must be a [B, 784] tensor on the GPU")
    B, dev = x.shape[0], x.device
    _f32_rows("pgd_l2_step", "x", x, B, dev)
    _f32_rows("pgd_l2_step", "x0", x0, B, dev)
    _f32_rows("pgd_l2_step", "dx", dx, B, dev)
    out = _out_rows("pgd_l2_step", "out", out, B, dev)
    if out.data_ptr() in (x0.data_ptr(), dx.data_ptr()):
        raise ValueError("pgd_l2_step: out must not be x0 or dx (both are read, not written)")
    if not (eps >= 0 and lo <= hi and alpha == alpha):
        raise ValueError("pgd_l2_step: need eps >= 0, lo <= hi and a step that is not NaN")
    p = native.ptr
    _C().pgd_l2_step(p(dx), p(x), p(x0), p(out), alpha, eps, lo, hi, B, _s())
    return out.view(B, 784)


ADV_PHILOX_DOMAIN = 0x41445631      # Philox counter word 1 of adv_init (csrc/include/kernels.h)


def adv_init(data_u8: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor | None, state: torch.Tensor, B: int,
             idx_stride: int = 0, eps: float = 0.0, lo: float = 0.0, hi: float = 0.0, random_start: bool = False,
             x0: torch.Tensor | None = None, x: torch.Tensor | None = None,
             labels_out: torch.Tensor | None = None):
    """The first launch of an adversarial training step (``csrc/kernels/adv_train.hip``), one launch:
    ``(x0, x, labels_out)`` for the ``B`` rows of the step ``state`` holds (row r = step * ``idx_stride`` + b;
    image and label ``idx[r]`` of ``data_u8`` / ``labels``, or r itself when ``idx`` is None).

        x0 = the normalised image (bit for bit ``data.datasets.PIXEL_LUT[u8]``);  labels_out = its label
        x  = x0, or with ``random_start``  min(max(x0 + (2u - 1) * eps, lo), hi),  u = (w >> 8) * 2**-24

    in float32, each operation rounded on its own, ``w`` one Philox-4x32-10 word per element: word e % 4 of
    ``philox4x32(counter = (b * 196 + e // 4, ADV_PHILOX_DOMAIN, step, 0), key = seed)``.  ``data_u8``: uint8
    [N, 784]; ``labels`` / ``idx``: int32; ``state``: the 24-byte StepState tensor; ``eps``, ``lo``, ``hi`` in
    normalised units.  Outputs: float32 [>= B, 784] / int32 [>= B], allocated when None; rows past ``B`` are
    not written."""
    dev = data_u8.device
    if data_u8.dtype != torch.uint8 or not data_u8.is_contiguous() or data_u8.numel() % 784:
        raise ValueError("adv_init: data_u8 must be contiguous uint8 rows of 784")
    if labels.dtype != torch.int32 or (idx is not None and idx.dtype != torch.int32):
        raise ValueError("adv_init: labels and idx must be int32")
    if B < 1:
        raise ValueError("adv_init: B must be positive")
    x0 = _out_rows("adv_init", "x0", x0, B, dev, at_least="B")
    x = _out_rows("adv_init", "x", x, B, dev, at_least="B")
    if labels_out is None:
        labels_out = torch.empty(B, dtype=torch.int32, device=dev)
    if labels_out.dtype != torch.int32 or labels_out.numel() < B or labels_out.device != dev:
        raise ValueError("adv_init: labels_out must be int32 with at least B entries")
    if x0.data_ptr() == x.data_ptr():
        raise ValueError("adv_init: x must not be x0")
    if random_start and not (eps >= 0 and lo <= hi):
        raise ValueError("adv_init: need eps >= 0 and lo <= hi")
    p = native.ptr
    _C().adv_init(p(data_u8), p(idx), idx_stride, p(labels), p(state), p(x0), p(x), p(labels_out), eps, lo, hi,
                  bool(random_start), B, _s())
    return x0, x, labels_out


SMOOTH_PHILOX_DOMAIN = 0x534D5431   # Philox counter word 1 of smooth_noise (csrc/include/kernels.h)
SMOOTH_MAX_ROWS = 1 << 23           # most rows (M * n, or B) one smooth_noise / smooth_vote launch takes (kernels.h)


def smooth_noise(x: torch.Tensor, sigma: float, n: int, seed: int, sample_base: int = 0, id_base: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """``n`` Gaussian-noised copies of each of the M images ``x`` (``csrc/kernels/smooth.hip``), one launch:

        out[i * n + s] = x0_i + sigma * z          float32 [M * n, 784], no clamp

    ``x``: uint8 [M, 784] raw rows (normalised in the kernel, bit for bit ``data.datasets.PIXEL_LUT[u8]``) or
    float32 [M, 784] already-normalised rows; ``sigma`` >= 0 in normalised units.  ``z``: Box-Muller normals
    from ``philox4x32(counter = (sample_base + s, SMOOTH_PHILOX_DOMAIN, id_base + i, e // 4), key = seed)``:
    words (0, 1) give elements 4v, 4v + 1 (cos, sin), words (2, 3) elements 4v + 2, 4v + 3.  A row depends on
    (seed, image id, sample index, sigma, x0) alone.  ``out``: float32 with at least M * n rows of 784,
    allocated when None; rows past M * n are not written.  One launch takes at most ``SMOOTH_MAX_ROWS`` = 2**23
    rows (one workgroup per row in a 32-bit grid): ``ValueError`` beyond, chunk as ``ops.smooth`` does."""
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous():
        raise ValueError("smooth_noise: x must be contiguous uint8 or float32 [M, 784]")
    M, n = x.shape[0], int(n)
    if M < 1 or n < 1:
        raise ValueError("smooth_noise: M and n must be positive")
    _check_rows("smooth_noise", "M * n", M * n)
    if not sigma >= 0:
        raise ValueError(f"smooth_noise: sigma must be >= 0, got {sigma}")
    if sample_base < 0 or sample_base + n > 1 << 32 or id_base < 0 or id_base + M > 1 << 32:
        raise ValueError("smooth_noise: sample_base + n and id_base + M must not exceed 2**32")
    out = _out_rows("smooth_noise", "out", out, M * n, x.device, at_least="M * n")
    _C().smooth_noise(*_src_ptrs(x), native.ptr(out), float(sigma), int(seed) & (2 ** 64 - 1),
                      int(sample_base), int(id_base), M, n, _s())
    return out


def smooth_noise_step(state: torch.Tensor, x0: torch.Tensor, sigma: float, B: int,
                      x: torch.Tensor | None = None) -> torch.Tensor:
    """The step form of ``smooth_noise``: ``x[b] = x0[b] + sigma * z`` for the ``B`` rows of the step ``state``
    holds, counter ``(low 32 bits of rng_base + 2 * step, SMOOTH_PHILOX_DOMAIN, b, e // 4)``, key the state's
    seed.  ``x`` may be ``x0`` (in place); allocated when None.  Rows past ``B`` are not written.  ``B`` is at
    most ``SMOOTH_MAX_ROWS`` = 2**23 (``ValueError`` beyond)."""
    if x0.dtype != torch.float32 or not x0.is_contiguous() or x0.numel() < B * 784 or B < 1:
        raise ValueError("smooth_noise_step: x0 must be contiguous float32 with at least B >= 1 rows of 784")
    _check_rows("smooth_noise_step", "B", B)
    if not sigma >= 0:
        raise ValueError(f"smooth_noise_step: sigma must be >= 0, got {sigma}")
    x = _out_rows("smooth_noise_step", "x", x, B, x0.device, at_least="B")
    p = native.ptr
    _C().smooth_noise_step(p(state), p(x0), p(x), float(sigma), B, _s())
    return x


def smooth_vote(logp: torch.Tensor, M: int, n: int, counts: torch.Tensor | None = None,
                accumulate: bool = False) -> torch.Tensor:
    """The vote of randomized smoothing, one launch: ``counts[i, c]`` = the number of rows ``s < n`` of
    ``logp[i * n + s]`` (float32 [>= M * n, 10]) whose argmax is class c - the first maximum wins a tie, a row
    holding a NaN votes for nothing.  ``accumulate``: add to ``counts`` (int32 [>= M, 10]; required then)
    instead of overwriting it.  Rows of ``counts`` past ``M`` are not written.  One launch takes at most
    ``SMOOTH_MAX_ROWS`` = 2**23 rows M * n (``ValueError`` beyond; accumulate over several launches)."""
    if logp.dtype != torch.float32 or not logp.is_contiguous() or M < 1 or n < 1 or logp.numel() < M * n * NCLS:
        raise ValueError("smooth_vote: logp must be contiguous float32 with at least M * n >= 1 rows of 10")
    _check_rows("smooth_vote", "M * n", M * n)
    if counts is None:
        if accumulate:
            raise ValueError("smooth_vote: accumulate needs counts")
        counts = torch.empty(M, NCLS, dtype=torch.int32, device=logp.device)
    if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.numel() < M * NCLS \
            or counts.device != logp.device:
        raise ValueError("smooth_vote: counts must be contiguous int32 with at least M rows of 10")
    p = native.ptr
    _C().smooth_vote(p(logp), p(counts), M, int(n), bool(accumulate), _s())
    return counts


ATTR_MAX_STEPS = 1 << 24            # most steps n_total of attr_path: every sample index is an exact float (kernels.h)
ATTR_FINISH_NONE, ATTR_FINISH_SCALE, ATTR_FINISH_PATH = 0, 1, 2     # attr_reduce finish forms (kernels.h AttrFinish)


def _attr_rows(a):
    """float32 numpy [M, 784] normalised rows of a uint8 / float32 tensor or array (uint8: the pixel LUT)."""
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype == np.uint8:
        from ..data.datasets import PIXEL_LUT
        a = PIXEL_LUT.numpy()[a.astype(np.int64)]
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 784)


def _attr_base(base, M: int):
    """float32 numpy baseline that broadcasts against [M, 784]: rows, or one value."""
    import numpy as np
    if isinstance(base, (int, float)):
        return np.float32(base)
    b = _attr_rows(base)
    if b.shape[0] != M:
        raise ValueError(f"attribution: {b.shape[0]} baseline rows for {M} images")
    return b


def attr_path_reference(x, n_total: int, sample_base: int = 0, ns: int | None = None, base=0.0):
    """``attr_path`` in numpy float32, bit for bit: float32 [M * ns, 784] rows ``b + alpha * (x - b)`` with
    ``alpha = (float32(sample_base + s) + 0.5) / float32(n_total)``, every operation rounded on its own.  ``x``:
    uint8 or float32 [M, 784] (tensor or array); ``base``: a float or float32 [M, 784]; normalised units."""
    import numpy as np
    x = _attr_rows(x)
    M = x.shape[0]
    ns = n_total - sample_base if ns is None else int(ns)
    if n_total < 1 or n_total > ATTR_MAX_STEPS or sample_base < 0 or ns < 1 or sample_base + ns > n_total:
        raise ValueError("attr_path: need 0 <= sample_base, ns >= 1 and sample_base + ns <= n_total <= ATTR_MAX_STEPS")
    b = _attr_base(base, M)
    alpha = (np.arange(sample_base, sample_base + ns).astype(np.float32) + np.float32(0.5)) / np.float32(n_total)
    d = (x - b).astype(np.float32)                                           # [M, 784]
    m = (alpha[None, :, None] * d[:, None, :]).astype(np.float32)            # [M, ns, 784]
    bb = b if np.ndim(b) == 0 else b[:, None, :]
    return (bb + m).astype(np.float32).reshape(M * ns, 784)


def attr_reduce_reference(dx, M: int, ns: int, acc=None, scale: float | None = None, x=None, base=0.0):
    """``attr_reduce`` in numpy float32, bit for bit: per element the rows ``dx[i * ns + s]`` are added in
    ascending ``s`` onto ``acc`` (float32 [M, 784]; None: zeros).  ``scale`` None: the running sums (no finish);
    else ``sums * scale``, times ``(x - base)`` when ``x`` is given (as ``attr_path_reference`` reads them)."""
    import numpy as np
    dx = _attr_rows(dx)[:M * ns].reshape(M, ns, 784)
    t = np.zeros((M, 784), dtype=np.float32) if acc is None else _attr_rows(acc)[:M].copy()
    with np.errstate(all="ignore"):
        for s in range(ns):
            t = (t + dx[:, s]).astype(np.float32)
        if scale is None:
            return t
        t = (t * np.float32(scale)).astype(np.float32)
        if x is not None:
            x = _attr_rows(x)
            t = (t * (x - _attr_base(base, M)).astype(np.float32)).astype(np.float32)
    return t


def _attr_image_args(name: str, x: torch.Tensor, base, M: int):
    """(x_u8, x_f32, base pointer, base value) of an image / baseline pair, checked."""
    if x.dim() != 2 or x.shape != (M, 784) or x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous uint8 or float32 [M, 784]")
    if isinstance(base, torch.Tensor):
        if base.shape != (M, 784) or base.dtype != torch.float32 or not base.is_contiguous() or base.device != x.device:
            raise ValueError(f"{name}: a baseline tensor must be contiguous float32 [M, 784] on x's device")
        return (*_src_ptrs(x), native.ptr(base), 0.0)
    if not isinstance(base, (int, float)) or base != base:
        raise ValueError(f"{name}: the baseline must be a float or a float32 [M, 784] tensor")
    return (*_src_ptrs(x), 0, float(base))


def attr_path(x: torch.Tensor, n_total: int, sample_base: int = 0, ns: int | None = None, base=0.0,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """The rows of the integration path of integrated gradients (``csrc/kernels/attr.hip``), one launch:

        out[i * ns + s] = b_i + alpha * (x_i - b_i),  alpha = (float32(sample_base + s) + 0.5) / float32(n_total)

    float32 [M * ns, 784]: the samples [``sample_base``, ``sample_base`` + ``ns``) (default: up to ``n_total``) of
    the midpoints of ``n_total`` equal steps from the baseline to the image, every operation rounded on its own
    (``attr_path_reference`` gives the same bits).  ``x``: uint8 [M, 784] raw rows (normalised in the kernel, bit
    for bit ``data.datasets.PIXEL_LUT[u8]``) or float32 [M, 784] normalised rows; ``base``: a float (normalised units)
    or a float32 [M, 784] tensor.  ``out``: float32 with at least M * ns rows of 784, allocated when None; rows
    past M * ns are not written.  At most ``SMOOTH_MAX_ROWS`` rows a launch (``ValueError`` beyond)."""
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("attr_path: x must be contiguous uint8 or float32 [M, 784] on the GPU")
    M, n_total, sample_base = x.shape[0], int(n_total), int(sample_base)
    ns = n_total - sample_base if ns is None else int(ns)
    if M < 1 or ns < 1:
        raise ValueError("attr_path: M and ns must be positive")
    _check_rows("attr_path", "M * ns", M * ns)
    if n_total > ATTR_MAX_STEPS or sample_base < 0 or sample_base + ns > n_total:
        raise ValueError("attr_path: need 0 <= sample_base and sample_base + ns <= n_total <= ATTR_MAX_STEPS")
    img = _attr_image_args("attr_path", x, base, M)
    out = _out_rows("attr_path", "out", out, M * ns, x.device, at_least="M * ns")
    _C().attr_path(*img, native.ptr(out), sample_base, n_total, M, ns, _s())
    return out


def attr_reduce(dx: torch.Tensor, M: int, ns: int, acc: torch.Tensor | None = None, accumulate: bool = False,
                scale: float | None = None, x: torch.Tensor | None = None, base=0.0,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """The per-image reduction of gradient rows (``csrc/kernels/attr.hip``), one launch: per element
    ``dx[i * ns + s]`` (float32 [>= M * ns, 784]) is added in ascending ``s``, in float32, onto ``acc[i]`` (float32
    [>= M, 784]; ``accumulate``: from what it holds, else from 0).  That fixed order makes the sum of an image's
    rows the same bits under any split of its samples over accumulating launches (``attr_reduce_reference`` gives
    them).  ``scale`` None: the running sums are stored to ``acc``, which is returned.  With ``scale`` (float32
    ``-1 / n``) the launch finishes: ``out = acc * scale``, times ``(x_i - b_i)`` when ``x`` is given (``x`` /
    ``base`` as ``attr_path`` takes them); ``out`` (float32 [>= M, 784], may be ``acc``) is allocated when None and
    returned, ``acc`` is then left as it was (unless it is ``out``).  Rows past M are not written.  At most
    ``SMOOTH_MAX_ROWS`` rows a launch (``ValueError`` beyond)."""
    M, ns = int(M), int(ns)
    _check_rows("attr_reduce", "M * ns", M * ns)
    if dx.dtype != torch.float32 or not dx.is_contiguous() or M < 1 or ns < 1 or dx.numel() < M * ns * 784:
        raise ValueError("attr_reduce: dx must be contiguous float32 with at least M * ns >= 1 rows of 784")
    if dx.device.type != "cuda":
        raise ValueError("attr_reduce: dx must be on the GPU")
    dev = dx.device
    if acc is None and accumulate:
        raise ValueError("attr_reduce: accumulate needs acc")
    acc = _out_rows("attr_reduce", "acc", acc, M, dev, at_least="M")
    if out is not None:
        _f32_rows("attr_reduce", "out", out, M, dev, at_least="M")
    p = native.ptr
    if scale is None:
        if x is not None or out is not None:
            raise ValueError("attr_reduce: x and out belong to a finishing launch (give scale)")
        _C().attr_reduce(p(dx), p(acc), 0, 0, 0, 0, 0.0, 0.0, M, ns, bool(accumulate), ATTR_FINISH_NONE, _s())
        return acc
    if out is None:
        out = torch.empty(M, 784, dtype=torch.float32, device=dev)
    if x is None:
        _C().attr_reduce(p(dx), p(acc), p(out), 0, 0, 0, 0.0, float(scale), M, ns, bool(accumulate),
                         ATTR_FINISH_SCALE, _s())
        return out
    if x.device != dev:
        raise ValueError("attr_reduce: x must be on dx's device")
    img = _attr_image_args("attr_reduce", x, base, M)
    _C().attr_reduce(p(dx), p(acc), p(out), *img, float(scale), M, ns, bool(accumulate), ATTR_FINISH_PATH, _s())
    return out


DF_CLASSES = 10                     # rows per image of the DeepFool kernels (csrc/include/kernels.h)
DF_SLACK = 1e-4                     # added to |f_k| in the ratio and the step (kernels.h DF_SLACK)
DF_MAX_M = SMOOTH_MAX_ROWS // DF_CLASSES     # most images one deepfool_init / deepfool_step launch takes (kernels.h)
DF_RUNNING, DF_CROSSED, DF_STUCK = 0, 1, 2   # the per-image status (kernels.h DfStatus)


def deepfool_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, y: torch.Tensor, x0: torch.Tensor,
                            r_tot: torch.Tensor, x: torch.Tensor, status: torch.Tensor, iters: torch.Tensor,
                            norm: torch.Tensor, overshoot: float, lo: float, hi: float):
    """``deepfool_step`` in torch ops on any device, in the dtype of ``dx`` (float32: the CPU / fp32 path of
    ``Predictor.minimum_norm``; float64: the oracle of the kernel's tests).  Same operands - ``dx`` [10 M, 784],
    ``loss_rows`` [10 M], ``y`` [M] integers, ``x0`` / ``r_tot`` / ``x`` [M, 784], ``status`` / ``iters`` [M]
    integers, ``norm`` [M] - none of them modified; returns the new ``(r_tot, x, status, iters, norm)``.  Per image,
    with f_k = loss_y - loss_k and w_k = g_y - g_k for k != y:

        frozen (status != 0): everything kept;  crossed (some loss_k < loss_y, or == with k < y): status = 1
        l = the first smallest (|f_k| + DF_SLACK) / |w_k| in ascending k, skipping |w_k| < PGD_L2_TINY and NaN ratios;
            none left: the first k with a NaN ratio (its NaN fills the image), else status = 2 (stuck)
        r_tot += ((|f_l| + DF_SLACK) / |w_l|^2) * w_l;  x = clamp(x0 + (1 + overshoot) * r_tot, lo, hi)
        norm = |x - x0|;  iters += 1

    ``overshoot``, ``lo`` and ``hi`` are rounded to float32 first, as the kernel receives them."""
    import numpy as np
    dt, dev = dx.dtype, dx.device
    M = y.numel()
    g = dx.reshape(M, DF_CLASSES, 784)
    loss = loss_rows.reshape(M, DF_CLASSES).to(dt)
    x0, r_tot, x = x0.reshape(M, 784).to(dt), r_tot.reshape(M, 784).to(dt), x.reshape(M, 784).to(dt)
    ar = torch.arange(M, device=dev)
    yl = y.reshape(M).long()
    inside = (yl >= 0) & (yl < DF_CLASSES)
    yc = yl.clamp(0, DF_CLASSES - 1)
    k = torch.arange(DF_CLASSES, device=dev)[None, :]
    other = k != yc[:, None]
    ly = loss[ar, yc][:, None]
    crossed = (other & ((loss < ly) | ((loss == ly) & (k < yc[:, None])))).any(dim=1)
    f = ly - loss
    w = g[ar, yc][:, None, :] - g                                        # [M, 10, 784]
    n2 = w.square().sum(dim=2)
    n = n2.sqrt()
    num = f.abs() + torch.tensor(float(np.float32(DF_SLACK)), dtype=dt, device=dev)
    ratio = num / n
    nan = ratio != ratio
    ok = other & ~nan & ~(n < PGD_L2_TINY)
    l = torch.full((M,), -1, dtype=torch.long, device=dev)
    l_nan = torch.full((M,), -1, dtype=torch.long, device=dev)
    best = torch.zeros(M, dtype=dt, device=dev)
    for c in range(DF_CLASSES):                                          # ascending k, strict <: the first minimum
        take = ok[:, c] & ((l < 0) | (ratio[:, c] < best))
        best = torch.where(take, ratio[:, c], best)
        l = torch.where(take, torch.full_like(l, c), l)
        l_nan = torch.where(other[:, c] & nan[:, c] & (l_nan < 0), torch.full_like(l_nan, c), l_nan)
    l = torch.where(l < 0, l_nan, l)
    active = status.reshape(M).long() == DF_RUNNING
    cross = active & inside & crossed
    upd = active & inside & ~crossed & (l >= 0)
    stuck = active & ~cross & ~upd
    lc = l.clamp_min(0)
    scale = num[ar, lc] / n2[ar, lc]
    r_new = r_tot + scale[:, None] * w[ar, lc]
    os1 = torch.tensor(1.0, dtype=dt, device=dev) + torch.tensor(float(np.float32(overshoot)), dtype=dt, device=dev)
    x_new = (x0 + os1 * r_new).clamp(float(np.float32(lo)), float(np.float32(hi)))
    norm_new = (x_new - x0).square().sum(dim=1).sqrt()
    u = upd[:, None]
    st = status.reshape(M).clone()
    st[cross] = DF_CROSSED
    st[stuck] = DF_STUCK
    return (torch.where(u, r_new, r_tot), torch.where(u, x_new, x), st,
            iters.reshape(M) + upd.to(iters.dtype), torch.where(upd, norm_new, norm.reshape(M).to(dt)))


def _df_vec(name: str, what: str, t: torch.Tensor, dtype, count: int, device, at_least: str) -> None:
    if t.dtype != dtype or not t.is_contiguous() or t.device != device or t.numel() < count:
        raise ValueError(f"{name}: {what} must be contiguous {str(dtype).split('.')[-1]} with at least {at_least} "
                         f"entries on the images' device")


def deepfool_init(x: torch.Tensor, rows: torch.Tensor | None = None, x_out: torch.Tensor | None = None,
                  x0_out: torch.Tensor | None = None, r_tot: torch.Tensor | None = None,
                  status: torch.Tensor | None = None, iters: torch.Tensor | None = None,
                  norm: torch.Tensor | None = None):
    """The start of a DeepFool run (``csrc/kernels/deepfool.hip``), one launch: for each of the M images ``x`` (uint8
    [M, 784] raw rows, normalised in the kernel bit for bit ``data.datasets.PIXEL_LUT[u8]``, or float32 [M, 784]
    normalised rows) the ten rows ``rows[10 i + c]`` and ``x_out[i]`` = the normalised image, ``r_tot[i]`` = 0,
    ``status[i]`` = ``iters[i]`` = 0, ``norm[i]`` = 0, and ``x0_out[i]`` = the normalised image (always written with
    uint8 rows; with float32 rows only when given).  Outputs (float32 [>= 10 M, 784] / [>= M, 784], int32 / float32
    [>= M]) are allocated when None; nothing past M is written.  Returns ``(rows, x_out, x0, r_tot, status, iters,
    norm)`` with ``x0`` the buffer the step reads: ``x0_out``, or ``x`` itself for float32 rows without one."""
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or not x.is_contiguous() \
            or x.device.type != "cuda":
        raise ValueError("deepfool_init: x must be contiguous uint8 or float32 [M, 784] on the GPU")
    M, dev = x.shape[0], x.device
    if M < 1 or M > DF_MAX_M:
        raise ValueError(f"deepfool_init: M = {M} images must be in [1, DF_MAX_M = {DF_MAX_M}] a launch")
    rows = _out_rows("deepfool_init", "rows", rows, DF_CLASSES * M, dev, at_least="10 M")
    x_out = _out_rows("deepfool_init", "x_out", x_out, M, dev, at_least="M")
    r_tot = _out_rows("deepfool_init", "r_tot", r_tot, M, dev, at_least="M")
    if x0_out is not None or x.dtype == torch.uint8:
        x0_out = _out_rows("deepfool_init", "x0_out", x0_out, M, dev, at_least="M")
    status = torch.empty(M, dtype=torch.int32, device=dev) if status is None else status
    iters = torch.empty(M, dtype=torch.int32, device=dev) if iters is None else iters
    norm = torch.empty(M, dtype=torch.float32, device=dev) if norm is None else norm
    _df_vec("deepfool_init", "status", status, torch.int32, M, dev, "M")
    _df_vec("deepfool_init", "iters", iters, torch.int32, M, dev, "M")
    _df_vec("deepfool_init", "norm", norm, torch.float32, M, dev, "M")
    p = native.ptr
    _C().deepfool_init(*_src_ptrs(x), p(rows), p(x_out), p(x0_out), p(r_tot), p(status), p(iters), p(norm), M, _s())
    return rows, x_out, (x0_out if x0_out is not None else x), r_tot, status, iters, norm


def deepfool_step(dx: torch.Tensor, loss_rows: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, r_tot: torch.Tensor,
                  x: torch.Tensor, rows: torch.Tensor, status: torch.Tensor, iters: torch.Tensor, norm: torch.Tensor,
                  overshoot: float, lo: float, hi: float, M: int | None = None) -> None:
    """One L2 DeepFool step per image (``csrc/kernels/deepfool.hip``), one launch, in place: from the ten gradient
    rows ``dx[10 i + c]`` (float32 [>= 10 M, 784], what ``input_grad`` wrote) and losses ``loss_rows[10 i + c]`` =
    -log p_c (float32 [>= 10 M], what ``head_train`` stored), the class ``y[i]`` being left (int32 [>= M]) and the
    clean image ``x0[i]``, the update of ``deepfool_step_reference`` on ``r_tot``, ``x`` (float32 [>= M, 784]), the
    image's ten ``rows`` (float32 [>= 10 M, 784]), ``status``, ``iters`` (int32 [>= M]) and ``norm`` (float32
    [>= M]).  float32 throughout, the sums a fixed tree: the same operands give the same bits.  An image with
    ``status`` != 0 is frozen: nothing of it is stored.  ``M``: the images of the launch (default ``y.numel()``);
    nothing past M is touched."""
    if dx.dim() != 2 or dx.device.type != "cuda":
        raise ValueError("deepfool_step: dx must be a float32 [10 M, 784] tensor on the GPU")
    dev = dx.device
    M = int(y.numel() if M is None else M)
    if M < 1 or M > DF_MAX_M:
        raise ValueError(f"deepfool_step: M = {M} images must be in [1, DF_MAX_M = {DF_MAX_M}] a launch")
    _f32_rows("deepfool_step", "dx", dx, DF_CLASSES * M, dev, at_least="10 M")
    _f32_rows("deepfool_step", "rows", rows, DF_CLASSES * M, dev, at_least="10 M")
    for what, t in (("x0", x0), ("r_tot", r_tot), ("x", x)):
        _f32_rows("deepfool_step", what, t, M, dev, at_least="M")
    _df_vec("deepfool_step", "loss_rows", loss_rows, torch.float32, DF_CLASSES * M, dev, "10 M")
    _df_vec("deepfool_step", "y", y, torch.int32, M, dev, "M")
    _df_vec("deepfool_step", "status", status, torch.int32, M, dev, "M")
    _df_vec("deepfool_step", "iters", iters, torch.int32, M, dev, "M")
    _df_vec("deepfool_step", "norm", norm, torch.float32, M, dev, "M")
    ptrs = [t.data_ptr() for t in (dx, x0, r_tot, x, rows)]
    if len(set(ptrs)) != len(ptrs):
        raise ValueError("deepfool_step: dx, x0, r_tot, x and rows must be five buffers")
    if not (overshoot >= 0 and lo <= hi):
        raise ValueError("deepfool_step: need overshoot >= 0 and lo <= hi")
    p = native.ptr
    _C().deepfool_step(p(dx), p(loss_rows), p(y), p(x0), p(r_tot), p(x), p(rows), p(status), p(iters), p(norm),
                       float(overshoot), float(lo), float(hi), M, _s())


APGD_MOMENTUM = 0.75                # a of the momentum step after the first update (csrc/kernels/apgd.hip)
APGD_RHO = (3, 4)                   # a window of k iterations oscillates when 4 n_up <= 3 k (rho = 0.75, in integers)
APGD_MAX_M = 1 << 20                # most images one apgd_step launch takes (kernels.h INPUT_GRAD_MAX_B)
# columns of the per-image records (kernels.h ApgdStepArgs)
APGD_ETA, APGD_LOSS_BEST, APGD_LOSS_PREV, APGD_LOSS_CHECK = 0, 1, 2, 3        # fstate, float32 [M, 4]
APGD_N_UP, APGD_REDUCED, APGD_ITERS, APGD_RESTARTED = 0, 1, 2, 3              # istate, int32 [M, 4]


def apgd_checkpoints(steps: int) -> tuple:
    """The checkpoint schedule of Auto-PGD (Croce & Hein 2020, the authors' code) for ``steps`` iterations: a tuple
    of ``(iteration, k)`` - after ``iteration`` updates (1-based) a window of ``k`` iterations closes.  k starts at
    max(int(0.22 N), 1) and shrinks by max(int(0.03 N), 1) a window, not below max(int(0.06 N), 1); the last
    checkpoint is <= N.  N = 100: iterations 22, 41, 57, 70, 80, 87, 93, 99."""
    n = int(steps)
    if n < 1:
        raise ValueError("apgd_checkpoints: steps must be at least 1")
    k, k_min, decr = max(int(0.22 * n), 1), max(int(0.06 * n), 1), max(int(0.03 * n), 1)
    out, at = [], 0
    while at + k <= n:
        at += k
        out.append((at, k))
        k = max(k - decr, k_min)
    return tuple(out)


def apgd_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, x: torch.Tensor,
                        x_old: torch.Tensor | None, x_best: torch.Tensor | None, g_best: torch.Tensor | None,
                        fstate: torch.Tensor | None, istate: torch.Tensor | None, sign: float, eps: float,
                        lo: float, hi: float, norm: str = "linf", first: bool = False, last: bool = False,
                        window: int = 0):
    """``apgd_step`` in torch ops on any device, in the dtype of ``dx`` (float32: the CPU / fp32 path of
    ``Predictor.auto_pgd``; float64: the oracle of the kernel's tests).  Same operands - ``dx``, ``x0``, ``x``,
    ``x_old``, ``x_best``, ``g_best`` [M, 784], ``loss_rows`` [M], ``fstate`` [M, 4] (eta, loss_best, loss_prev,
    loss_check), ``istate`` integers [M, 4] (n_up, reduced, iters, restarted) - none of them modified; returns the new
    ``(x, x_old, x_best, g_best, fstate, istate)``.  With ``first`` the last five inputs are not read (None will do).
    Per image, with L = sign * loss and g = sign * dx:

        first:   eta = 2 eps; loss_best = loss_prev = loss_check = L; x_best = x; g_best = dx; n_up = 0; reduced = 1;
                 iters = 0; restarted = 0; a = 1; (src, gs) = (x, g)
        else:    n_up += L > loss_prev; loss_prev = L;  L > loss_best: loss_best = L, x_best = x, g_best = dx
                 last: stop here
                 (src, gs) = (x, g); a = 0.75; restarted = 0
                 window k > 0: r = 4 n_up <= 3 k or (reduced == 0 and loss_check >= loss_best); reduced = r;
                               loss_check = loss_best; n_up = 0; r: eta /= 2, (src, gs) = (x_best, sign g_best),
                               restarted = 1
        linf:    z = C(B(src + eta sgn(gs)));  x = C(B((src + a (z - src)) + (1 - a) (src - x_old)))
        l2:      z = P(src + (eta / max(|gs|, TINY)) gs);  x = P((src + a (z - src)) + (1 - a) (src - x_old))
                 B(t) = min(max(t, x0 - eps), x0 + eps); C = clamp(., lo, hi); P(t) = C(x0 + d min(1, eps / max(|d|, TINY)))
        x_old = src; iters += 1                   (first: no (1 - a) term)

    ``eps``, ``lo`` and ``hi`` are rounded to float32 first, as the kernel receives them."""
    import numpy as np
    if norm not in ("linf", "l2"):
        raise ValueError(f"apgd_step_reference: norm must be 'linf' or 'l2', got {norm!r}")
    if sign not in (1, -1) or (first and last) or window < 0:
        raise ValueError("apgd_step_reference: sign is +1 or -1, window >= 0, and a launch is not first and last")
    dt, dev = dx.dtype, dx.device
    M = dx.shape[0]
    eps, lo, hi = (float(np.float32(v)) for v in (eps, lo, hi))
    tiny = float(np.float32(PGD_L2_TINY))
    sgn = float(sign)
    x0, x = x0.reshape(M, 784).to(dt), x.reshape(M, 784).to(dt)
    L = sgn * loss_rows.reshape(M).to(dt)
    i32 = dict(dtype=torch.int32, device=dev)
    if first:
        eta = torch.full((M,), 2.0 * eps, dtype=dt, device=dev)
        loss_best, loss_prev, loss_check = L.clone(), L.clone(), L.clone()
        n_up, reduced, iters = torch.zeros(M, **i32), torch.ones(M, **i32), torch.zeros(M, **i32)
        restarted = torch.zeros(M, **i32)
        xb, gb = x.clone(), dx.clone()
        improved = torch.ones(M, dtype=torch.bool, device=dev)
    else:
        eta, loss_best, loss_prev, loss_check = fstate.reshape(M, 4).to(dt).unbind(dim=1)
        n_up, reduced, iters, restarted = istate.reshape(M, 4).to(torch.int32).unbind(dim=1)
        n_up = n_up + (L > loss_prev).to(torch.int32)
        loss_prev = L
        improved = L > loss_best
        loss_best = torch.where(improved, L, loss_best)
        xb = torch.where(improved[:, None], x, x_best.reshape(M, 784).to(dt))
        gb = torch.where(improved[:, None], dx, g_best.reshape(M, 784).to(dt))
    pack = lambda: (torch.stack((eta, loss_best, loss_prev, loss_check), dim=1),             # noqa: E731
                    torch.stack((n_up, reduced, iters, restarted), dim=1))
    if last:
        return (x.clone(), x_old.reshape(M, 784).to(dt).clone(), xb, gb, *pack())
    restart = torch.zeros(M, dtype=torch.bool, device=dev)
    if not first:
        restarted = torch.zeros(M, **i32)
        if window > 0:
            osc = APGD_RHO[1] * n_up <= APGD_RHO[0] * int(window)
            stall = (reduced == 0) & (loss_check >= loss_best)
            restart = osc | stall
            restarted = reduced = restart.to(torch.int32)
            loss_check = loss_best.clone()
            n_up = torch.zeros(M, **i32)
            eta = torch.where(restart, 0.5 * eta, eta)
    src = torch.where(restart[:, None], xb, x)
    gs = sgn * torch.where(restart[:, None], gb, dx)
    a = 1.0 if first else APGD_MOMENTUM
    e = eta[:, None]

    def mix(z):
        t = src + a * (z - src)
        return t if first else t + (1.0 - a) * (src - x_old.reshape(M, 784).to(dt))

    if norm == "linf":
        el, eh = x0 - eps, x0 + eps
        box = lambda t: torch.min(torch.max(t, el), eh).clamp(lo, hi)                            # noqa: E731
        sg = torch.where(gs != gs, gs, torch.sign(gs))       # a NaN gradient stays a NaN
        x_new = box(mix(box(src + e * sg)))
    else:
        def proj(t):
            d = t - x0
            m = d.square().sum(dim=1, keepdim=True).sqrt()
            return (x0 + d * (eps / m.clamp_min(tiny)).clamp_max(1.0)).clamp(lo, hi)
        n = gs.square().sum(dim=1, keepdim=True).sqrt()
        x_new = proj(mix(proj(src + (e / n.clamp_min(tiny)) * gs)))
    iters = iters + 1
    return (x_new, src, xb, gb, *pack())


def apgd_step(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, x: torch.Tensor, x_old: torch.Tensor,
              x_best: torch.Tensor, g_best: torch.Tensor, fstate: torch.Tensor, istate: torch.Tensor, sign: float,
              eps: float, lo: float, hi: float, norm: str = "linf", first: bool = False, last: bool = False,
              window: int = 0, M: int | None = None) -> None:
    """One Auto-PGD iteration per image (``csrc/kernels/apgd.hip``), one launch, in place: from the gradient rows
    ``dx`` (float32 [>= M, 784], what ``input_grad`` wrote) and losses ``loss_rows`` (float32 [>= M], what
    ``head_train`` stored) at the iterate ``x``, and the clean images ``x0``, the update of ``apgd_step_reference`` on
    ``x``, ``x_old``, ``x_best``, ``g_best`` (float32 [>= M, 784]), ``fstate`` (float32 [>= M, 4]) and ``istate``
    (int32 [>= M, 4]).  float32 throughout, the L2 sums a fixed tree: the same operands give the same bits.
    ``first``: no state is read, all of it is written; ``last``: only loss_prev, n_up and the best point are brought
    up to date; ``window``: k > 0 when this launch closes a checkpoint window of k iterations.  ``M``: the images of
    the launch (default ``x.shape[0]``); nothing past M is touched."""
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("apgd_step: x must be a float32 [M, 784] tensor on the GPU")
    if norm not in ("linf", "l2"):
        raise ValueError(f"apgd_step: norm must be 'linf' or 'l2', got {norm!r}")
    dev = x.device
    M = int(x.shape[0] if M is None else M)
    if M < 1 or M > APGD_MAX_M:
        raise ValueError(f"apgd_step: M = {M} images must be in [1, APGD_MAX_M = {APGD_MAX_M}] a launch")
    rows = (("dx", dx), ("x0", x0), ("x", x), ("x_old", x_old), ("x_best", x_best), ("g_best", g_best))
    for what, t in rows:
        _f32_rows("apgd_step", what, t, M, dev, at_least="M")
    _df_vec("apgd_step", "loss_rows", loss_rows, torch.float32, M, dev, "M")
    _df_vec("apgd_step", "fstate", fstate, torch.float32, 4 * M, dev, "4 M")
    _df_vec("apgd_step", "istate", istate, torch.int32, 4 * M, dev, "4 M")
    ptrs = [t.data_ptr() for _, t in rows]
    if len(set(ptrs)) != len(ptrs):
        raise ValueError("apgd_step: dx, x0, x, x_old, x_best and g_best must be six buffers")
    if not (eps >= 0 and lo <= hi) or sign not in (1, -1) or int(window) < 0 or (first and last):
        raise ValueError("apgd_step: need eps >= 0, lo <= hi, sign +1 or -1, window >= 0, and not first and last")
    p = native.ptr
    _C().apgd_step(p(dx), p(loss_rows), p(x0), p(x), p(x_old), p(x_best), p(g_best), p(fstate), p(istate),
                   float(sign), float(eps), float(lo), float(hi), norm == "l2", bool(first), bool(last), int(window),
                   M, _s())


SQUARE_PHILOX_DOMAIN = 0x53515231   # Philox counter word 1 of square_init / square_step (csrc/include/kernels.h)
SQUARE_MAX_M = 1 << 20              # most images one square_init / square_step launch takes (kernels.h INPUT_GRAD_MAX_B)
SQUARE_MAX_SIDE = 27
# columns of the per-image record, int32 [M, 4] (kernels.h SquareStepArgs); column 0 holds the bits of a float32
SQUARE_MARGIN, SQUARE_QUERIES, SQUARE_DONE = 0, 1, 2
_SQUARE_SCHEDULE = ((10, 1), (50, 2), (200, 4), (500, 8), (1000, 16), (2000, 32), (4000, 64), (6000, 128), (8000, 256))


def square_sides(p_init: float, queries: int) -> tuple:
    """The side of the square of each proposal of a Square Attack (Andriushchenko et al. 2020) of ``queries``
    queries: entry ``q - 1`` belongs to query index q = 1 .. queries - 1 (query 0 is the stripe start).  The share
    of the image a square covers is ``p_init`` halved on the authors' piecewise-constant schedule, rescaled from
    their 10000 queries: it = int(q / queries * 10000); p = p_init / 1, 2, 4, ... 512 as ``it`` passes 10, 50, 200,
    500, 1000, 2000, 4000, 6000, 8000; side = min(max(floor(sqrt(p * 784) + 0.5), 1), 27) in float64."""
    import math
    queries = int(queries)
    if queries < 1:
        raise ValueError("square_sides: queries must be at least 1")
    if not 0.0 < p_init <= 1.0:
        raise ValueError(f"square_sides: p_init must be in (0, 1], got {p_init}")
    out = []
    for q in range(1, queries):
        it = int(q / queries * 10000)
        div = next((d for top, d in _SQUARE_SCHEDULE if it <= top), 512)
        side = int(math.floor(math.sqrt(float(p_init) / div * 784.0) + 0.5))
        out.append(min(max(side, 1), SQUARE_MAX_SIDE))
    return tuple(out)


def square_state_margin(state: torch.Tensor) -> torch.Tensor:
    """float32 [M]: ``margin_best`` of the int32 [M, 4] records of ``square_step`` (column 0 read as float32)."""
    return state[:, SQUARE_MARGIN].contiguous().view(torch.float32)


def _square_ids(name: str, ids, id_base: int, M: int):
    import numpy as np
    ids = np.arange(M, dtype=np.int64) + int(id_base) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.shape[0] != M:
        raise ValueError(f"{name}: {ids.shape[0]} ids for {M} images")
    if M and (ids.min() < 0 or ids.max() >= 1 << 32):
        raise ValueError(f"{name}: every image id must fit 32 bits")
    return ids


def _square_vertex(x0: torch.Tensor, plus: torch.Tensor, eps: float, lo: float, hi: float) -> torch.Tensor:
    """clamp(x0 + eps) where ``plus`` else clamp(x0 - eps): float32, each operation rounded on its own."""
    import numpy as np
    e = torch.tensor(float(np.float32(eps)), dtype=torch.float32, device=x0.device)
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return torch.where(plus, x0 + e, x0 - e).clamp(lo, hi)


def square_init_reference(x0: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, ids=None,
                          id_base: int = 0) -> torch.Tensor:
    """``square_init`` in torch float32 on any device: the candidate of query 0, vertical stripes - column c of every
    row of image i is clamp(x0 + eps) when bit 0 of word ``c & 3`` of ``philox4x32(counter = (0,
    SQUARE_PHILOX_DOMAIN, id_i, c >> 2), key = seed)`` is set, else clamp(x0 - eps).  ``ids``: the images' ids
    (default ``id_base`` + i).  The same bits as the kernel (``ops.philox`` draws them)."""
    import numpy as np
    from .philox import philox4x32
    M = x0.shape[0]
    x0 = x0.detach().reshape(M, 784).to(torch.float32)
    ids = _square_ids("square_init_reference", ids, id_base, M)
    w = philox4x32(0, SQUARE_PHILOX_DOMAIN, ids[:, None], np.arange(7)[None, :], seed)        # [M, 7, 4]
    plus = torch.from_numpy((w.reshape(M, 28) & 1).astype(np.bool_)).to(x0.device)
    return _square_vertex(x0.view(M, 28, 28), plus[:, None, :], eps, lo, hi).reshape(M, 784)


def square_margin_reference(logp: torch.Tensor, y: torch.Tensor, targeted: bool = False) -> torch.Tensor:
    """float32 [M]: the margin ``square_step`` reads off a row of ten log-probabilities - untargeted lp[y] -
    max_{j != y} lp[j], targeted the negative; < 0: broken.  A NaN anywhere in the row (the maximum lets it through)
    and a y outside [0, 10) give a NaN."""
    M = logp.shape[0]
    lp = logp.detach().reshape(M, NCLS).to(torch.float32)
    y = y.reshape(M).long().to(lp.device)
    valid = (y >= 0) & (y < NCLS)
    yc = y.clamp(0, NCLS - 1)
    own = torch.zeros(M, NCLS, dtype=torch.bool, device=lp.device).scatter_(1, yc[:, None], valid[:, None])
    ly = torch.where(valid, lp.gather(1, yc[:, None])[:, 0], torch.full_like(lp[:, 0], float("nan")))
    mo = lp.masked_fill(own, float("-inf")).max(dim=1).values
    return (mo - ly) if targeted else (ly - mo)


def square_step_reference(logp: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x_best: torch.Tensor | None,
                          x_cand: torch.Tensor, state: torch.Tensor | None, eps: float, lo: float, hi: float,
                          seed: int = 0, q: int = 1, side: int = 1, ids=None, id_base: int = 0, first: bool = False,
                          last: bool = False, targeted: bool = False):
    """``square_step`` in torch float32 on any device (the CPU / fp32 path of ``Predictor.square_attack``): none of
    the operands - ``logp`` [M, 10], ``y`` [M], ``x0`` / ``x_best`` / ``x_cand`` [M, 784], ``state`` int32 [M, 4]
    (margin_best as float32 bits, queries_used, done, spare) - is modified; returns the new ``(x_best, x_cand,
    state)``.  With ``first`` neither ``x_best`` nor ``state`` is read (None will do).  Per image, with L the margin
    (``square_margin_reference``) of ``logp``:

        first:          margin_best = L; x_best = x_cand; queries_used = 1
        done on entry:  nothing changes (frozen)
        else:           queries_used += 1;  L < margin_best (strict): margin_best = L, x_best = x_cand
        done = margin_best < 0
        last:           x_cand stays
        else, done:     x_cand = x_best
        else:           x_cand = x_best with the square of side ``side`` at (row0, col0) set to clamp(x0 + eps) (w2 & 1)
                        or clamp(x0 - eps): w = philox4x32(counter = (q, SQUARE_PHILOX_DOMAIN, id_i, 0), key = seed),
                        row0 = (w0 * (29 - side)) >> 32, col0 = (w1 * (29 - side)) >> 32

    ``q``: the query index of that proposal (round j: j + 1)."""
    import numpy as np
    from .philox import philox4x32
    side, q = int(side), int(q)
    if not 1 <= side <= SQUARE_MAX_SIDE:
        raise ValueError(f"square_step_reference: side must be in [1, {SQUARE_MAX_SIDE}], got {side}")
    if not 0 <= q < 1 << 32:
        raise ValueError("square_step_reference: q must fit 32 bits")
    M = x_cand.shape[0]
    dev = x_cand.device
    x0 = x0.detach().reshape(M, 784).to(torch.float32)
    x_cand = x_cand.detach().reshape(M, 784).to(torch.float32)
    ids = _square_ids("square_step_reference", ids, id_base, M)
    L = square_margin_reference(logp, y, targeted).to(dev)
    if first:
        active = accept = torch.ones(M, dtype=torch.bool, device=dev)
        margin = L
        used = torch.ones(M, dtype=torch.int32, device=dev)
        done_was = spare = torch.zeros(M, dtype=torch.int32, device=dev)
        xb = x_cand
    else:
        state = state.reshape(M, 4).to(torch.int32)
        was = square_state_margin(state)
        done_was, spare = state[:, SQUARE_DONE], state[:, 3]
        active = done_was == 0
        accept = active & (L < was)
        margin = torch.where(accept, L, was)
        used = state[:, SQUARE_QUERIES] + active.to(torch.int32)
        xb = torch.where(accept[:, None], x_cand, x_best.detach().reshape(M, 784).to(torch.float32))
    broken = margin < 0
    done = torch.where(active, broken.to(torch.int32), done_was)
    xc = x_cand
    if not last:
        w = philox4x32(q, SQUARE_PHILOX_DOMAIN, ids, 0, seed).astype(np.uint64)                 # [M, 4]
        span = np.uint64(29 - side)
        row0 = torch.from_numpy(((w[:, 0] * span) >> np.uint64(32)).astype(np.int64)).to(dev)
        col0 = torch.from_numpy(((w[:, 1] * span) >> np.uint64(32)).astype(np.int64)).to(dev)
        plus = torch.from_numpy((w[:, 2] & np.uint64(1)).astype(np.bool_)).to(dev)
        at = torch.arange(28, device=dev)
        rows = (at[None, :] >= row0[:, None]) & (at[None, :] < row0[:, None] + side)
        cols = (at[None, :] >= col0[:, None]) & (at[None, :] < col0[:, None] + side)
        window = (rows[:, :, None] & cols[:, None, :]).reshape(M, 784)
        prop = torch.where(window, _square_vertex(x0, plus[:, None], eps, lo, hi), xb)
        xc = torch.where((active & ~broken)[:, None], prop, torch.where(active[:, None], xb, x_cand))
    margin_bits = torch.where(active, margin, square_state_margin(state) if not first else margin)
    new = torch.stack((margin_bits.contiguous().view(torch.int32), used, done, spare), dim=1)
    return xb, xc, new


def _square_common(name: str, eps: float, lo: float, hi: float, id_base: int, M: int) -> None:
    if M < 1 or M > SQUARE_MAX_M:
        raise ValueError(f"{name}: M = {M} images must be in [1, SQUARE_MAX_M = {SQUARE_MAX_M}] a launch")
    if not (eps >= 0 and lo <= hi):
        raise ValueError(f"{name}: need eps >= 0 and lo <= hi")
    if id_base < 0 or id_base + M > 1 << 32:
        raise ValueError(f"{name}: id_base + M must not exceed 2**32")


def square_init(x0: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, id_base: int = 0,
                out: torch.Tensor | None = None, M: int | None = None) -> torch.Tensor:
    """The start of a Square Attack (``csrc/kernels/square.hip``), one launch: ``out[i]`` = the stripe point of
    ``square_init_reference`` for the M images ``x0`` (float32 [>= M, 784] normalised rows on the GPU), image i under
    the id ``id_base + i``.  ``out``: float32 with at least M rows of 784, allocated when None; nothing past M is
    written.  Bit for bit the reference."""
    if x0.dim() != 2 or x0.device.type != "cuda":
        raise ValueError("square_init: x0 must be a float32 [M, 784] tensor on the GPU")
    M = int(x0.shape[0] if M is None else M)
    _square_common("square_init", eps, lo, hi, int(id_base), M)
    _f32_rows("square_init", "x0", x0, M, x0.device, at_least="M")
    out = _out_rows("square_init", "out", out, M, x0.device, at_least="M")
    if out.data_ptr() == x0.data_ptr():
        raise ValueError("square_init: x0 and out must be two buffers")
    _C().square_init(native.ptr(x0), native.ptr(out), float(eps), float(lo), float(hi), int(seed) & (2 ** 64 - 1),
                     int(id_base), M, _s())
    return out


def square_step(logp: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x_best: torch.Tensor, x_cand: torch.Tensor,
                state: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, q: int = 1, side: int = 1,
                id_base: int = 0, first: bool = False, last: bool = False, targeted: bool = False,
                M: int | None = None) -> None:
    """One Square Attack query per image (``csrc/kernels/square.hip``), one launch, in place: from the
    log-probabilities ``logp`` (float32 [>= M, 10], what ``head_eval`` wrote for the candidates ``x_cand``), the
    labels ``y`` (int32 [>= M]; ``targeted``: the classes to reach) and the clean images ``x0``, the update of
    ``square_step_reference`` on ``x_best``, ``x_cand`` (float32 [>= M, 784]) and ``state`` (int32 [>= M, 4]),
    image i under the id ``id_base + i``.  ``first``: no record and no ``x_best`` is read, both are written;
    ``last``: ``x_cand`` is not written; an image whose record says done is frozen: nothing of it is stored.  ``q``,
    ``side``: the query index and the square's side of the proposal written to ``x_cand``.  ``M``: the images of the
    launch (default ``x_cand.shape[0]``); nothing past M is touched.  Bit for bit the reference."""
    if x_cand.dim() != 2 or x_cand.device.type != "cuda":
        raise ValueError("square_step: x_cand must be a float32 [M, 784] tensor on the GPU")
    dev = x_cand.device
    M = int(x_cand.shape[0] if M is None else M)
    _square_common("square_step", eps, lo, hi, int(id_base), M)
    rows = (("x0", x0), ("x_best", x_best), ("x_cand", x_cand))
    for what, t in rows:
        _f32_rows("square_step", what, t, M, dev, at_least="M")
    _df_vec("square_step", "logp", logp, torch.float32, NCLS * M, dev, "10 M")
    _df_vec("square_step", "y", y, torch.int32, M, dev, "M")
    _df_vec("square_step", "state", state, torch.int32, 4 * M, dev, "4 M")
    if len({t.data_ptr() for _, t in rows}) != len(rows):
        raise ValueError("square_step: x0, x_best and x_cand must be three buffers")
    if not 1 <= int(side) <= SQUARE_MAX_SIDE:
        raise ValueError(f"square_step: side must be in [1, {SQUARE_MAX_SIDE}], got {side}")
    if not 0 <= int(q) < 1 << 32:
        raise ValueError("square_step: q must fit 32 bits")
    p = native.ptr
    _C().square_step(p(logp), p(y), p(x0), p(x_best), p(x_cand), p(state), float(eps), float(lo), float(hi),
                     int(seed) & (2 ** 64 - 1), int(q), int(id_base), int(side), bool(first), bool(last),
                     bool(targeted), M, _s())


def adadelta_step(ms, region: int = 0, advance_step: bool = False, grid: int = 0, wt: bool = False) -> None:
    """``grid`` > 0 (``ADA_FC`` only): that many workgroups; below ``ADA_FC_TILES`` they walk the fc tiles
    grid-stride.  ``wt``: write-through 16-byte stores (the engine's choice at B <= WT_MAX_B)."""
    p = native.ptr
    _C().adadelta(p(ms.param), p(ms.grad), p(ms.square_avg), p(ms.acc_delta), p(ms.lr), ms.rho, ms.eps,
                  ms.weight_decay, p(ms.w2f), p(ms.w2d), p(ms.w1), p(ms.w1t),
                  p(ms.state) if advance_step else 0, region, True, _s(), grid=grid, wt=wt)


def xgmi_allreduce(x, channel: int, offset: int, count: int, ms=None, wt: bool = False,
                   advance_step: bool = False, max_wg: int = 0) -> None:
    """``x.out[offset, offset + count)`` = the rank-ordered sum of every rank's ``x.in`` range (one-shot up to the
    communicator's ``oneshot_max`` floats, two-shot above).  With ``ms`` the Adadelta step of flat elements
    ``[offset, offset + count)`` is fused on the reduced values (the fp32 step's buckets).  ``max_wg`` > 0 shrinks
    the planned grid; every rank passes the same value."""
    x.allreduce(channel, offset, count, _s(), ada=_ada_args(ms, wt, advance_step) if ms is not None else None,
                max_wg=max_wg)


def xgmi_fc_fused(x, channel: int, ms, wt: bool = False, advance_step: bool = False, max_wg: int = 0) -> None:
    """The fc bucket's all-reduce with the fc Adadelta step and the ``w1`` / ``w1t`` shadows fused.  The kernel does
    not advance the step counter even with ``advance_step`` (the conv bucket's launch is the end-of-step marker)."""
    x.allreduce_fc_fused(channel, _s(), _ada_args(ms, wt, advance_step), max_wg=max_wg)


def xgmi_conv_reduce_fused(x, channel: int, ms, data_u8: torch.Tensor, idx: torch.Tensor, buf: StepBuffers,
                           grad_scale: float = 1.0, idx_stride: int = 0, c1red: torch.Tensor | None = None,
                           lo: int = 0, hi: int = RED_ALL_PARTS, wt: bool = False, advance_step: bool = False,
                           max_wg: int = 0) -> None:
    """Reduce parts [lo, hi) of the conv gradient slabs, their all-reduce through the staging slots and the
    Adadelta step with the conv2 shadows, one launch (operands as ``conv_bwd``'s reduce stage)."""
    p, w = native.ptr, param_ptrs(ms)
    x.conv_reduce_fused(channel, p(buf.dyc), p(buf.a1), w.w2d, w.c1w, w.c1b, p(data_u8), p(idx), idx_stride,
                        p(ms.state), p(buf.c1part), p(buf.w2part), p(ms.grad), grad_scale, buf.B, _s(),
                        _ada_args(ms, wt, advance_step), c1red=p(c1red), lo=lo, hi=hi, max_wg=max_wg)


def scale_copy(dst: torch.Tensor, src: torch.Tensor, n: int, s: float) -> None:
    """``dst[:n] = src[:n] * float32(s)`` (the DDP bucket copy-in); fp32 views, any 4-byte alignment."""
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or n < 0 or n > min(dst.numel(), src.numel()):
        raise ValueError("scale_copy: fp32 tensors of at least n elements")
    _C().scale_copy(native.ptr(dst), native.ptr(src), n, float(s), _s())


def fill_bytes(t: torch.Tensor, nbytes: int, value: int) -> None:
    """The first ``nbytes`` bytes of the uint8 view ``t`` = ``value`` (the setup buffers' byte fill)."""
    if t.dtype != torch.uint8 or nbytes < 0 or nbytes > t.numel():
        raise ValueError("fill_bytes: a uint8 tensor of at least nbytes elements")
    _C().fill(native.ptr(t), nbytes, value, _s())


def gather_rows(src_u8: torch.Tensor, src_labels: torch.Tensor, idx: torch.Tensor, start: int, n: int,
                dst_u8: torch.Tensor, dst_labels: torch.Tensor) -> None:
    """Rows [start, start + n) of ``dst_u8`` [., 784] / ``dst_labels`` = the source rows ``idx[start + i]``."""
    if start < 0 or n < 0 or start + n > min(idx.numel(), dst_u8.shape[0], dst_labels.numel()):
        raise ValueError("gather_rows: rows out of range")
    p = native.ptr
    _C().gather_rows(p(src_u8), p(src_labels), p(idx), start, n, p(dst_u8), p(dst_labels), _s())


def train_step(ms, data_u8, labels, idx, buf: StepBuffers, idx_stride: int = 0, grad_scale: float = 1.0,
               loss_log: torch.Tensor | None = None, update: bool = True) -> None:
    """One full fused training step (no DDP): fwd, loss, bwd, optional Adadelta."""
    trunk_fwd(ms, data_u8, idx, buf, True, idx_stride)
    fc1_fwd(ms, buf)
    head_train(ms, labels, idx, buf, idx_stride)
    fc_bwd(ms, buf, grad_scale, loss_log)
    conv_bwd(ms, data_u8, idx, buf, grad_scale, idx_stride)
    if update:
        adadelta_step(ms, 0, advance_step=True)


def eval_forward(ms, data_u8, labels, idx, buf: StepBuffers) -> None:
    trunk_fwd(ms, data_u8, idx, buf, False)
    fc1_fwd(ms, buf)
    head_eval(ms, labels, idx, buf)


def route_codes(planes: torch.Tensor) -> torch.Tensor:
    """[..., 16] uint8 code bit planes of a record (byte 2 c8 + p: bit j = bit p of channel 8 c8 + j's
    argmax code) -> [..., 64] int64 codes 0..3."""
    pl = planes.long().view(*planes.shape[:-1], 8, 2)              # [..., chunk, plane]
    bits = (pl.unsqueeze(-1) >> torch.arange(8, device=planes.device)) & 1   # [..., chunk, plane, j]
    return (bits[..., 0, :] | (bits[..., 1, :] << 1)).reshape(*planes.shape[:-1], 64)


def dense_dy(buf: StepBuffers) -> torch.Tensor:
    """Expand the compact un-pooled gradient records to the dense NHWC bf16 [B,24,24,64] map
    (what the conv backward kernels stage in LDS); for tests and tools."""
    B = buf.B
    rec = buf.dyc.view(B, 12, 12, DYC_REC)
    g = rec[..., :128].contiguous().view(torch.bfloat16).view(B, 12, 12, 64)
    code = route_codes(rec[..., 128:])                              # [B,12,12,64] window position
    dense = torch.zeros(B, 12, 2, 12, 2, 64, dtype=torch.bfloat16, device=g.device)
    for q in range(4):
        sel = (code == q)
        dense[:, :, q >> 1, :, q & 1, :] = torch.where(sel, g, torch.zeros_like(g))
    return dense.view(B, 24, 24, 64)


# ---------------------------------------------------------------------------- fp32 step, one launcher at a time
# launch_f32_forward's stage mask and the backward launchers of csrc/kernels/f32_net.hip (kernels.h F32Stage)
F32_PREP, F32_CONV1, F32_CONV2, F32_POOL, F32_FC1, F32_HEAD, F32_FWD_ALL = 1, 2, 4, 8, 16, 32, 63
F32_FC_SMALL, F32_FC1W, F32_FC1X, F32_CONV2W, F32_CONV2X_CONV1W, F32_CONV_REDUCE = range(6)
F32_MAX_SPLITS, F32_C1W_BLOCKS = 128, 1024      # kernels.h


def f32_fc1_splits(B: int) -> int:
    return 36 if B <= 1024 else 9


@dataclass
class F32Buffers:
    """The workspace of the fp32 step (kernels.h F32Step) for batch ``B``, every tensor with one guard row or
    guard slab beyond what B needs.  ``trunk`` False: no conv activations (a1 / dx1 keep the guard row only)."""
    B: int
    w2fwd: torch.Tensor       # f32 [9+1, 32, 64]
    w2bwd: torch.Tensor       # f32 [9+1, 64, 32]
    w1p: torch.Tensor         # f32 [128+1, 144, 64]
    a1: torch.Tensor          # f32 [B+1, 26, 26, 32]
    dx1: torch.Tensor         # f32 [B+1, 26, 26, 32]
    y2: torch.Tensor          # f32 [B+1, 24, 24, 64]  conv2 pre-activation, then its gradient
    p: torch.Tensor           # f32 [B+1, 9216]
    pm: torch.Tensor          # u8  [B+1, 144, 64]
    z1part: torch.Tensor      # f32 [splits * B + 1, 128]
    h: torch.Tensor           # f32 [B+1, 128]
    dz1: torch.Tensor         # f32 [B+1, 128]
    dl: torch.Tensor          # f32 [B+1, 16]
    loss_rows: torch.Tensor   # f32 [B+2]: a launch may use rows [out_row, out_row + B)
    correct: torch.Tensor     # i32 [B+2]
    c2part: torch.Tensor      # f32 [F32_MAX_SPLITS+1, 64, 289]
    c1part: torch.Tensor      # f32 [F32_C1W_BLOCKS+1, 32, 10]

    @staticmethod
    def allocate(B: int, device, trunk: bool = True) -> "F32Buffers":
        def z(*shape, dtype=torch.float32):
            return torch.zeros(*shape, dtype=dtype, device=device)
        Bt = B if trunk else 0
        return F32Buffers(B, z(10, 32, 64), z(10, 64, 32), z(129, 144, 64), z(Bt + 1, 26, 26, 32), z(Bt + 1, 26, 26, 32),
                          z(B + 1, 24, 24, 64), z(B + 1, NFLAT), z(B + 1, 144, 64, dtype=torch.uint8),
                          z(f32_fc1_splits(B) * B + 1, NH), z(B + 1, NH), z(B + 1, NH), z(B + 1, 16), z(B + 2),
                          z(B + 2, dtype=torch.int32), z(F32_MAX_SPLITS + 1, 64, 289), z(F32_C1W_BLOCKS + 1, 32, 10))

    def tensors(self) -> dict:
        return {k: v for k, v in vars(self).items() if isinstance(v, torch.Tensor)}


def _f32_ptrs(buf: F32Buffers, out_row: int, **ext) -> dict:
    d = {k: native.ptr(v) for k, v in {**buf.tensors(), **ext}.items() if v is not None}
    d["loss_rows"] += 4 * out_row
    d["correct"] += 4 * out_row
    return d


def f32_forward(buf: F32Buffers, param: torch.Tensor, data_u8: torch.Tensor, labels: torch.Tensor,
                idx: torch.Tensor | None = None, idx_stride: int = 0, state: torch.Tensor | None = None,
                inv_batch: float = 0.0, train: bool = True, stages: int = F32_FWD_ALL, out_row: int = 0) -> None:
    """The forward kernels of the fp32 step named by the ``stages`` mask, in order, on caller-owned buffers.
    ``state`` None: the eval form's null StepState (step 0, no dropout).  ``out_row``: first row of
    ``buf.loss_rows`` / ``buf.correct`` the launch uses."""
    ptrs = _f32_ptrs(buf, out_row, param=param, data_u8=data_u8, labels=labels, idx=idx, state=state)
    _C().f32_forward(ptrs, idx_stride, inv_batch, buf.B, bool(train), stages, _s())


def f32_backward(buf: F32Buffers, stage: int, param: torch.Tensor, grad: torch.Tensor, data_u8: torch.Tensor,
                 labels: torch.Tensor, idx: torch.Tensor | None = None, idx_stride: int = 0,
                 state: torch.Tensor | None = None, inv_batch: float = 0.0, loss_log: torch.Tensor | None = None,
                 out_row: int = 0) -> None:
    """One backward launcher of the fp32 step (``F32_FC_SMALL`` .. ``F32_CONV_REDUCE``) on caller-owned buffers."""
    ptrs = _f32_ptrs(buf, out_row, param=param, grad=grad, data_u8=data_u8, labels=labels, idx=idx, state=state,
                     loss_log=loss_log)
    _C().f32_backward(ptrs, idx_stride, inv_batch, buf.B, stage, _s())


# ---------------------------------------------------------------------------- single-launch inference
@dataclass
class InferBuffers:
    """Workspace, tickets and outputs of ``infer_forward`` for any batch size up to ``max_B``.  The
    tickets are zeroed here, once; every completed launch leaves them zero."""
    max_B: int
    z1part: torch.Tensor      # f32 workspace: [INFER_BANDS, B, 128] of the launch's B
    tickets: torch.Tensor     # i32 [max_B] (a launch uses one per group)
    logp: torch.Tensor        # f32 [max_B, 10]
    pred: torch.Tensor        # i32 [max_B]
    loss_rows: torch.Tensor   # f32 [max_B]
    correct: torch.Tensor     # i32 [max_B]

    @staticmethod
    def allocate(max_B: int, device) -> "InferBuffers":
        plan = _C().infer_plan(max_B)            # workspace_bytes grows with B: max_B's serves every B below
        z = dict(device=device)
        return InferBuffers(
            max_B=max_B,
            z1part=torch.zeros(plan["workspace_bytes"] // 4, dtype=torch.float32, **z),
            tickets=torch.zeros(max(max_B, plan["ticket_count"]), dtype=torch.int32, **z),
            logp=torch.zeros(max_B, NCLS, dtype=torch.float32, **z),
            pred=torch.zeros(max_B, dtype=torch.int32, **z),
            loss_rows=torch.zeros(max_B, dtype=torch.float32, **z),
            correct=torch.zeros(max_B, dtype=torch.int32, **z),
        )


def infer_forward(ms, buf: InferBuffers, B: int, *, u8: torch.Tensor | None = None,
                  idx: torch.Tensor | None = None, x: torch.Tensor | None = None,
                  labels: torch.Tensor | None = None) -> None:
    """Rows [0, B) of ``buf.logp`` / ``buf.pred`` (and ``loss_rows`` / ``correct`` with ``labels``) from
    exactly one launch on the current stream.  Input: ``u8`` uint8 [N, 784] rows (row b, or row
    ``idx[b]`` with an int32 ``idx``), or ``x`` float32 [B, 784] already normalised.  ``labels`` int32:
    one per ``u8`` row when ``idx`` is given, else one per batch row."""
    if (u8 is None) == (x is None):
        raise ValueError("infer_forward: pass exactly one of u8 and x")
    if not 1 <= B <= buf.max_B:
        raise ValueError(f"infer_forward: B = {B} outside [1, {buf.max_B}]")
    if x is not None:
        if idx is not None:
            raise ValueError("infer_forward: idx applies to u8 rows only")
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < B * 784:
            raise ValueError("infer_forward: x must be contiguous float32 with at least B rows of 784")
    else:
        if u8.dtype != torch.uint8 or not u8.is_contiguous() or u8.numel() % 784:
            raise ValueError("infer_forward: u8 must be contiguous uint8 rows of 784")
        if idx is None and u8.numel() < B * 784:
            raise ValueError("infer_forward: u8 has fewer than B rows")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < B):
        raise ValueError("infer_forward: idx must be int32 with at least B entries")
    if labels is not None and labels.dtype != torch.int32:
        raise ValueError("infer_forward: labels must be int32")
    p, w = native.ptr, param_ptrs(ms)
    _C().infer_fwd(p(u8), p(idx), p(x), p(labels), w.c1w, w.c1b, w.w2f, w.c2b, w.w1, w.f1b, w.f2w, w.f2b,
                   p(buf.z1part), p(buf.tickets), p(buf.logp), p(buf.pred),
                   p(buf.loss_rows) if labels is not None else 0, p(buf.correct) if labels is not None else 0,
                   B, _s())
