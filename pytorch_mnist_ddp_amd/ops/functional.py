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


FAB_LINF, FAB_L2 = 0, 1             # the norm of a fab_step launch (kernels.h FabNorm)
FAB_NORMS = {"linf": FAB_LINF, "l2": FAB_L2}
FAB_RUNNING, FAB_DONE, FAB_STUCK = 0, 1, 2   # the per-image status (kernels.h FabStatus)


def _f32_scalar(v: float, dt, dev) -> torch.Tensor:
    import numpy as np
    return torch.tensor(float(np.float32(v)), dtype=dt, device=dev)


def fab_projection_reference(w: torch.Tensor, v: torch.Tensor, r: torch.Tensor, lo: float, hi: float,
                             norm: str) -> torch.Tensor:
    """The box-constrained projection P(v, r) of ``fab_step`` in torch ops, in the dtype of ``w``: per row of ``w``
    / ``v`` ([M, 784]) and entry of ``r`` ([M]) the delta of smallest ``norm`` ("linf" / "l2") with r + w . delta = 0
    and lo <= v + delta <= hi.  Per element a = |w|, d = -sgn(r) sgn(w), room = (hi - v if d > 0 else v - lo) floored
    at 0, c = 1 (linf) or a (l2); delta = d min(tau c, room), tau the smallest root of sum a min(tau c, room) = |r|:
    on the stably sorted breakpoints room / c, the first position k with R_k + tau_k S_k >= |r| (R_k: the sum of
    a room before k, S_k: the sum of a c from k on) gives tau = (|r| - R_k) / S_k; none (the hyperplane misses the
    box): tau = inf.  Elements with a = 0 take no part.  ``lo`` and ``hi`` are rounded to float32 first."""
    if norm not in FAB_NORMS:
        raise ValueError(f"fab_projection_reference: norm must be 'linf' or 'l2', got {norm!r}")
    dt, dev = w.dtype, w.device
    w = w.reshape(-1, w.shape[-1])
    v, r = v.reshape(w.shape).to(dt), r.reshape(-1).to(dt)
    lo, hi = _f32_scalar(lo, dt, dev), _f32_scalar(hi, dt, dev)
    a = w.abs()
    d = -(torch.sign(r)[:, None] * torch.sign(w))
    room = torch.where(d > 0, hi - v, v - lo).clamp_min(0)
    act = a > 0
    c = a if norm == "l2" else torch.ones_like(a)
    zero, inf = torch.zeros((), dtype=dt, device=dev), torch.full((), float("inf"), dtype=dt, device=dev)
    taus, order = torch.sort(torch.where(act, room / c, inf), dim=1, stable=True)
    ars = torch.where(act, a * room, zero).gather(1, order)
    acs = torch.where(act, a * c, zero).gather(1, order)
    R = torch.cat([torch.zeros_like(ars[:, :1]), ars.cumsum(1)[:, :-1]], dim=1)
    S = acs.flip(1).cumsum(1).flip(1)
    ra = r.abs()
    ok = (R + taus * S) >= ra[:, None]
    first = ok.to(torch.int8).argmax(dim=1, keepdim=True)               # the first position that reaches |r|
    tau = torch.where(ok.any(dim=1), (ra - R.gather(1, first)[:, 0]) / S.gather(1, first)[:, 0], inf)
    return torch.where(act, d * torch.minimum(tau[:, None] * c, room), zero)


def _fab_norm(t: torch.Tensor, norm: str) -> torch.Tensor:
    return t.abs().amax(dim=-1) if norm == "linf" else t.square().sum(dim=-1).sqrt()


def fab_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x: torch.Tensor,
                       x_best: torch.Tensor, norm_best: torch.Tensor, status: torch.Tensor, iters: torch.Tensor,
                       alpha_max: float, eta: float, beta: float, lo: float, hi: float, norm: str,
                       last: bool = False):
    """``fab_step`` in torch ops on any device, in the dtype of ``dx`` (float32: the CPU / fp32 path of
    ``Predictor.fab``).  Same operands - ``dx`` [10 M, 784], ``loss_rows`` [10 M], ``y`` [M] integers, ``x0`` / ``x`` /
    ``x_best`` [M, 784], ``norm_best`` [M], ``status`` / ``iters`` [M] integers - none of them modified; returns the
    new ``(x, x_best, norm_best, status, iters, proj)``, ``proj`` [M, 2, 784] the two projections of the images that
    made a forward step (zeros elsewhere).  Per image, with f_k = loss_y - loss_k, w_k = g_y - g_k, |.| the norm and q
    its dual exponent:

        frozen (status != 0): everything kept
        crossed (some loss_k < loss_y, or == with k < y): u = |x - x0|; u < norm_best: x_best = x, norm_best = u;
            u == 0: status = 1 (done); else, unless ``last``: x = clamp(x0 + beta (x - x0)), iters += 1
        not crossed and ``last``: everything kept
        l = the first smallest (|f_k| + DF_SLACK) / |w_k|_q in ascending k, skipping |w_k|_q < PGD_L2_TINY and NaN
            ratios; none left: a NaN ratio fills x and proj with NaN (iters += 1), else status = 2 (stuck)
        r1 = f_l, r2 = f_l + sum w_l (x0 - x); d1 = P(x, r1), d2 = P(x0, r2) (``fab_projection_reference``);
        alpha = min(|d1| / (|d1| + |d2|), alpha_max), 0 / 0 = 0;
        x = clamp((1 - alpha) (x + eta d1) + alpha (x0 + eta d2), lo, hi); iters += 1

    The scalars are rounded to float32 first, as the kernel receives them."""
    if norm not in FAB_NORMS:
        raise ValueError(f"fab_step_reference: norm must be 'linf' or 'l2', got {norm!r}")
    dt, dev = dx.dtype, dx.device
    M = y.numel()
    g = dx.reshape(M, DF_CLASSES, 784)
    loss = loss_rows.reshape(M, DF_CLASSES).to(dt)
    x0, x, x_best = x0.reshape(M, 784).to(dt), x.reshape(M, 784).to(dt), x_best.reshape(M, 784).to(dt)
    norm_best = norm_best.reshape(M).to(dt)
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
    n = w.abs().sum(dim=2) if norm == "linf" else w.square().sum(dim=2).sqrt()
    ratio = (f.abs() + _f32_scalar(DF_SLACK, dt, dev)) / n
    nan = ratio != ratio
    ok = other & ~nan & ~(n < PGD_L2_TINY)
    l = torch.full((M,), -1, dtype=torch.long, device=dev)
    best = torch.zeros(M, dtype=dt, device=dev)
    for c in range(DF_CLASSES):                                          # ascending k, strict <: the first minimum
        take = ok[:, c] & ((l < 0) | (ratio[:, c] < best))
        best = torch.where(take, ratio[:, c], best)
        l = torch.where(take, torch.full_like(l, c), l)
    active = status.reshape(M).long() == FAB_RUNNING
    cross = active & inside & crossed
    fwd = active & inside & ~crossed & (not last)
    upd = fwd & (l >= 0)
    fill = fwd & (l < 0) & (other & nan).any(dim=1)
    stuck = (active & ~inside) | (fwd & ~upd & ~fill)
    lo_t, hi_t = _f32_scalar(lo, dt, dev), _f32_scalar(hi, dt, dev)
    # the backward step of a crossed iterate
    u = _fab_norm(x - x0, norm)
    better = cross & (u < norm_best)
    done = cross & (u == 0)
    back = cross & ~done & (not last)
    x_back = torch.minimum(torch.maximum(x0 + _f32_scalar(beta, dt, dev) * (x - x0), lo_t), hi_t)
    # the forward step along the two projections
    lc = l.clamp_min(0)
    wl, r1 = w[ar, lc], f[ar, lc]
    r2 = r1 + (wl * (x0 - x)).sum(dim=1)
    d1 = fab_projection_reference(wl, x, r1, lo, hi, norm)
    d2 = fab_projection_reference(wl, x0, r2, lo, hi, norm)
    n1, n2 = _fab_norm(d1, norm), _fab_norm(d2, norm)
    al = torch.where(n1 + n2 > 0, n1 / (n1 + n2), torch.zeros_like(n1))
    al = torch.minimum(al, _f32_scalar(alpha_max, dt, dev))[:, None]
    e = _f32_scalar(eta, dt, dev)
    x_fwd = ((1 - al) * (x + e * d1) + al * (x0 + e * d2)).clamp(float(lo_t), float(hi_t))
    qn = torch.full((), float("nan"), dtype=dt, device=dev)
    x_new = torch.where(back[:, None], x_back, torch.where(upd[:, None], x_fwd, torch.where(fill[:, None], qn, x)))
    proj = torch.stack([d1, d2], dim=1)
    proj = torch.where(upd[:, None, None], proj, torch.where(fill[:, None, None], qn, torch.zeros_like(proj)))
    st = status.reshape(M).clone()
    st[done] = FAB_DONE
    st[stuck] = FAB_STUCK
    return (x_new, torch.where(better[:, None], x, x_best), torch.where(better, u, norm_best), st,
            iters.reshape(M) + (back | upd | fill).to(iters.dtype), proj)


def fab_step(dx: torch.Tensor, loss_rows: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x: torch.Tensor,
             x_best: torch.Tensor, norm_best: torch.Tensor, rows: torch.Tensor, status: torch.Tensor,
             iters: torch.Tensor, alpha_max: float, eta: float, beta: float, lo: float, hi: float, norm: str,
             last: bool = False, proj: torch.Tensor | None = None, M: int | None = None) -> None:
    """One FAB iteration per image (``csrc/kernels/fab.hip``), one launch, in place: from the ten gradient rows
    ``dx[10 i + c]`` (float32 [>= 10 M, 784], what ``input_grad`` wrote), the losses ``loss_rows[10 i + c]`` = -log p_c
    (float32 [>= 10 M]), the class ``y[i]`` being left (int32 [>= M]) and the clean image ``x0[i]``, the update of
    ``fab_step_reference`` on ``x``, ``x_best`` (float32 [>= M, 784]), ``norm_best`` (float32 [>= M], +inf at the
    start), the image's ten ``rows`` (float32 [>= 10 M, 784]), ``status`` and ``iters`` (int32 [>= M]).  ``proj``
    (float32 [>= M, 2, 784], optional) receives the two projections of every image that made a forward step.  ``norm``:
    "linf" or "l2".  float32 throughout, every sum in a fixed order: the same operands give the same bits.  An image
    with ``status`` != 0 is frozen: nothing of it is stored.  ``last``: the round after the last update - the best
    point is brought up to date, no iterate moves.  ``M``: the images of the launch (default ``y.numel()``); nothing
    past M is touched."""
    if norm not in FAB_NORMS:
        raise ValueError(f"fab_step: norm must be 'linf' or 'l2', got {norm!r}")
    if dx.dim() != 2 or dx.device.type != "cuda":
        raise ValueError("fab_step: dx must be a float32 [10 M, 784] tensor on the GPU")
    dev = dx.device
    M = int(y.numel() if M is None else M)
    if M < 1 or M > DF_MAX_M:
        raise ValueError(f"fab_step: M = {M} images must be in [1, DF_MAX_M = {DF_MAX_M}] a launch")
    _f32_rows("fab_step", "dx", dx, DF_CLASSES * M, dev, at_least="10 M")
    _f32_rows("fab_step", "rows", rows, DF_CLASSES * M, dev, at_least="10 M")
    for what, t in (("x0", x0), ("x", x), ("x_best", x_best)):
        _f32_rows("fab_step", what, t, M, dev, at_least="M")
    _df_vec("fab_step", "loss_rows", loss_rows, torch.float32, DF_CLASSES * M, dev, "10 M")
    _df_vec("fab_step", "y", y, torch.int32, M, dev, "M")
    _df_vec("fab_step", "norm_best", norm_best, torch.float32, M, dev, "M")
    _df_vec("fab_step", "status", status, torch.int32, M, dev, "M")
    _df_vec("fab_step", "iters", iters, torch.int32, M, dev, "M")
    bufs = [dx, x0, x, x_best, rows]
    if proj is not None:
        _df_vec("fab_step", "proj", proj, torch.float32, 2 * 784 * M, dev, "2 * 784 M")
        bufs.append(proj)
    if len({t.data_ptr() for t in bufs}) != len(bufs):
        raise ValueError("fab_step: dx, x0, x, x_best, rows and proj must be buffers of their own")
    if not (eta >= 1 and 0 < beta <= 1 and 0 <= alpha_max <= 1 and lo <= hi):
        raise ValueError("fab_step: need eta >= 1, beta in (0, 1], alpha_max in [0, 1] and lo <= hi")
    p = native.ptr
    _C().fab_step(p(dx), p(loss_rows), p(y), p(x0), p(x), p(x_best), p(norm_best), p(rows), p(status), p(iters),
                  p(proj), float(alpha_max), float(eta), float(beta), float(lo), float(hi), FAB_NORMS[norm],
                  bool(last), M, _s())


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


APGD_L1_N = 784
APGD_L1_K_INIT = APGD_L1_N - (APGD_L1_N * 4) // 5          # 157: the first step moves the top 20 % of the coordinates
# columns of the per-image records (kernels.h ApgdL1StepArgs)
APGD_L1_ETA, APGD_L1_LOSS_BEST, APGD_L1_LAM, APGD_L1_THR = 0, 1, 2, 3          # fstate, float32 [M, 4]
APGD_L1_K_SEL, APGD_L1_SP_OLD, APGD_L1_ITERS, APGD_L1_RESTARTED = 0, 1, 2, 3   # istate, int32 [M, 4]


def apgd_l1_checkpoints(steps: int) -> tuple:
    """The checkpoint schedule of L1 Auto-PGD (Croce & Hein 2021) for ``steps`` iterations: a tuple of
    ``(iteration, k)`` - a checkpoint after every k = max(int(0.04 steps), 1) updates (1-based), the last one <=
    ``steps``.  steps = 100: iterations 4, 8, ..., 100."""
    n = int(steps)
    if n < 1:
        raise ValueError("apgd_l1_checkpoints: steps must be at least 1")
    k = max(int(0.04 * n), 1)
    return tuple((at, k) for at in range(k, n + 1, k))


def apgd_l1_k_sel(sp):
    """The coordinates the next L1 Auto-PGD steps move, from the count ``sp`` (an int or an integer tensor) of changed
    pixels of the best point: ceil(2 sp / 3) in exact integers, at least 1 and at most 784.  (The authors' float form
    floor((1 - sp / n / 1.5) n) counts the coordinates left out and differs by one at 34 values of sp.)"""
    k = (2 * sp + 2) // 3
    if isinstance(k, torch.Tensor):
        return k.clamp(1, APGD_L1_N)
    return min(max(int(k), 1), APGD_L1_N)


def l1_box_projection_reference(z: torch.Tensor, x0: torch.Tensor, eps: float, lo: float, hi: float):
    """``(delta, lam)``: per row the Euclidean projection of the perturbation ``z`` ([M, n], any float dtype and
    device) onto the intersection of the L1 ball of radius ``eps`` and the box lo <= x0 + delta <= hi, in the sorted
    form of ``csrc/kernels/apgd_l1.hip``.  s = sgn(z), a = |z|, cap = max(s > 0 ? hi - x0 : x0 - lo, 0), w = min(a, cap):

        eps == 0:        delta = s 0, lam = 0
        sum w <= eps:    delta = s w, lam = 0
        otherwise:       delta = s min(max(a - lam, 0), cap),  lam the root of  sum min(max(a - lam, 0), cap) = eps

    With b = max(a - cap, 0) the sum is sum_{a > lam} (a - lam) - sum_{b > lam} (b - lam); on the 2 n breakpoints
    sorted ascending (a stable sort, the a before the b), S_k / N_k the sums over the positions >= k of +a, -b /
    of +-1 (S in float64): k = the first position with N_k > 0 and S_k - tau_k N_k <= eps, lam = (S_k - eps) / N_k
    in float64, rounded to the dtype once (a row with no
    such position - a NaN in it - gets lam = NaN and a NaN delta)."""
    M, n = z.shape
    dt, dev = z.dtype, z.device
    x0 = x0.reshape(M, n).to(dt)
    s = torch.where(z != z, z, torch.sign(z))
    if eps == 0:
        return s * 0.0, torch.zeros(M, dtype=dt, device=dev)
    a = z.abs()
    cap = torch.where(s > 0, hi - x0, x0 - lo).clamp_min(0)
    w = torch.where(cap < a, cap, a)
    b = (a - cap).clamp_min(0)
    tau, order = torch.sort(torch.cat((a, b), dim=1), dim=1, stable=True)
    unit = torch.cat((torch.ones(M, n, dtype=dt, device=dev), -torch.ones(M, n, dtype=dt, device=dev)), dim=1)
    unit = unit.gather(1, order)
    # S, phi and the quotient in float64 in every dtype and on every device, as the kernel has them (a float32 cumsum
    # on the CPU accumulates in float64 anyway): S_k cancels +a against -b and then eps; lam is rounded once
    tau64, unit64 = tau.double(), unit.double()
    S = (tau64 * unit64).flip(1).cumsum(dim=1).flip(1)
    N = unit64.flip(1).cumsum(dim=1).flip(1)
    ok = (N > 0) & (S - tau64 * N <= eps)
    k = ok.to(torch.int8).argmax(dim=1, keepdim=True)
    lam = ((S.gather(1, k) - eps) / N.gather(1, k))[:, 0].to(dt)
    lam = torch.where(ok.any(dim=1), lam, torch.full_like(lam, float("nan")))
    t = a - lam[:, None]
    t = torch.where(t < 0, torch.zeros_like(t), t)
    t = torch.where(cap < t, cap, t)
    inside = w.sum(dim=1) <= eps
    return torch.where(inside[:, None], s * w, s * t), torch.where(inside, torch.zeros_like(lam), lam)


def apgd_l1_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, x: torch.Tensor,
                           x_best: torch.Tensor | None, g_best: torch.Tensor | None, fstate: torch.Tensor | None,
                           istate: torch.Tensor | None, sign: float, eps: float, lo: float, hi: float,
                           first: bool = False, last: bool = False, window: int = 0):
    """``apgd_l1_step`` in torch ops on any device, in the dtype of ``dx`` (float32: the CPU / fp32 path of
    ``Predictor.auto_pgd_l1``; float64: the oracle of the kernel's tests).  Same operands - ``dx``, ``x0``, ``x``,
    ``x_best``, ``g_best`` [M, 784], ``loss_rows`` [M], ``fstate`` [M, 4] (eta, loss_best, lam, thr), ``istate``
    integers [M, 4] (k_sel, sp_old, iters, restarted) - none of them modified; returns the new ``(x, x_best, g_best,
    fstate, istate)``.  With ``first`` the last four inputs are not read (None will do).  Per image, with L = sign *
    loss and g = sign * dx:

        first:   eta = eps; loss_best = L; x_best = x; g_best = dx; k_sel = 157; sp_old = 784; iters = 0;
                 restarted = 0; (src, gs) = (x, g)
        else:    L > loss_best: loss_best = L, x_best = x, g_best = dx
                 last: stop here
                 (src, gs) = (x, g); restarted = 0
                 window > 0: sp = #{x_best != x0}; red = 100 sp < 95 sp_old; k_sel = ``apgd_l1_k_sel(sp)``;
                             red: eta = eps, (src, gs) = (x_best, sign g_best), restarted = 1;
                             else eta = max(eta / 1.5, eps / 10);  sp_old = sp
        step:    thr = the k_sel-th largest |gs|; sel = {|gs| >= thr and gs != 0} (and every NaN); m = |sel|
                 t = src + (eta / max(m, 1)) sgn(gs) on sel, src elsewhere
        project: delta, lam = ``l1_box_projection_reference(t - x0, x0, eps, lo, hi)``; x = clamp(x0 + delta, lo, hi);
                 iters += 1

    ``eps``, ``lo`` and ``hi`` are rounded to float32 first, as the kernel receives them."""
    import numpy as np
    if sign not in (1, -1) or (first and last) or window < 0:
        raise ValueError("apgd_l1_step_reference: sign is +1 or -1, window >= 0, and a launch is not first and last")
    if not eps >= 0:
        raise ValueError("apgd_l1_step_reference: eps must be >= 0")
    dt, dev = dx.dtype, dx.device
    M = dx.shape[0]
    eps, lo, hi = (float(np.float32(v)) for v in (eps, lo, hi))
    sgn = float(sign)
    x0, x = x0.reshape(M, 784).to(dt), x.reshape(M, 784).to(dt)
    L = sgn * loss_rows.reshape(M).to(dt)
    i32 = dict(dtype=torch.int32, device=dev)
    eps_t = torch.full((M,), eps, dtype=dt, device=dev)
    if first:
        eta, loss_best = eps_t.clone(), L.clone()
        lam, thr = torch.zeros(M, dtype=dt, device=dev), torch.zeros(M, dtype=dt, device=dev)
        k_sel, sp_old = torch.full((M,), APGD_L1_K_INIT, **i32), torch.full((M,), APGD_L1_N, **i32)
        iters, restarted = torch.zeros(M, **i32), torch.zeros(M, **i32)
        xb, gb = x.clone(), dx.clone()
    else:
        eta, loss_best, lam, thr = fstate.reshape(M, 4).to(dt).unbind(dim=1)
        k_sel, sp_old, iters, restarted = istate.reshape(M, 4).to(torch.int32).unbind(dim=1)
        improved = L > loss_best
        loss_best = torch.where(improved, L, loss_best)
        xb = torch.where(improved[:, None], x, x_best.reshape(M, 784).to(dt))
        gb = torch.where(improved[:, None], dx, g_best.reshape(M, 784).to(dt))
    pack = lambda: (torch.stack((eta, loss_best, lam, thr), dim=1),                          # noqa: E731
                    torch.stack((k_sel, sp_old, iters, restarted), dim=1))
    if last:
        return (x.clone(), xb, gb, *pack())
    red = torch.zeros(M, dtype=torch.bool, device=dev)
    if not first:
        restarted = torch.zeros(M, **i32)
        if window > 0:
            sp = (xb != x0).sum(dim=1).to(torch.int32)
            red = 100 * sp < 95 * sp_old
            k_sel = apgd_l1_k_sel(sp)
            # the step size is float32 state in every dtype, as the kernel keeps it (tensor divisors: a true division
            # on every device, never a multiplication by a rounded reciprocal)
            e32, eps32 = eta.to(torch.float32), eps_t.to(torch.float32)
            shrunk = torch.maximum(e32 / torch.full_like(e32, 1.5), eps32 / torch.full_like(e32, 10.0))
            eta = torch.where(red, eps_t, shrunk.to(dt))
            restarted = red.to(torch.int32)
            sp_old = sp
    src = torch.where(red[:, None], xb, x)
    gs = sgn * torch.where(red[:, None], gb, dx)
    ag = gs.abs()
    at = (k_sel.long().clamp(1, APGD_L1_N) - 1)[:, None]
    thr = torch.sort(ag, dim=1, descending=True)[0].gather(1, at)[:, 0]
    sel = ((ag >= thr[:, None]) | (gs != gs)) & (gs != 0)
    m = sel.sum(dim=1).clamp_min(1).to(dt)
    sg = torch.where(gs != gs, gs, torch.sign(gs))
    t = torch.where(sel, src + (eta / m)[:, None] * sg, src)
    delta, lam = l1_box_projection_reference(t - x0, x0, eps, lo, hi)
    x_new = (x0 + delta).clamp(lo, hi)
    iters = iters + 1
    return (x_new, xb, gb, *pack())


def apgd_l1_step(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, x: torch.Tensor, x_best: torch.Tensor,
                 g_best: torch.Tensor, fstate: torch.Tensor, istate: torch.Tensor, sign: float, eps: float, lo: float,
                 hi: float, first: bool = False, last: bool = False, window: int = 0, M: int | None = None) -> None:
    """One L1 Auto-PGD iteration per image (``csrc/kernels/apgd_l1.hip``), one launch, in place: from the gradient
    rows ``dx`` (float32 [>= M, 784], what ``input_grad`` wrote) and losses ``loss_rows`` (float32 [>= M]) at the
    iterate ``x``, and the clean images ``x0``, the update of ``apgd_l1_step_reference`` on ``x``, ``x_best``,
    ``g_best`` (float32 [>= M, 784]), ``fstate`` (float32 [>= M, 4]) and ``istate`` (int32 [>= M, 4]).  float32
    throughout, every sum in a fixed order, the counts in integers: the same operands give the same bits.  ``eps``:
    the L1 radius in normalised units.  ``first``: no state is read, all of it is written; ``last``: only the best
    point is brought up to date; ``window`` > 0: this launch is a checkpoint.  ``M``: the images of the launch
    (default ``x.shape[0]``); nothing past M is touched."""
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("apgd_l1_step: x must be a float32 [M, 784] tensor on the GPU")
    dev = x.device
    M = int(x.shape[0] if M is None else M)
    if M < 1 or M > APGD_MAX_M:
        raise ValueError(f"apgd_l1_step: M = {M} images must be in [1, APGD_MAX_M = {APGD_MAX_M}] a launch")
    rows = (("dx", dx), ("x0", x0), ("x", x), ("x_best", x_best), ("g_best", g_best))
    for what, t in rows:
        _f32_rows("apgd_l1_step", what, t, M, dev, at_least="M")
    _df_vec("apgd_l1_step", "loss_rows", loss_rows, torch.float32, M, dev, "M")
    _df_vec("apgd_l1_step", "fstate", fstate, torch.float32, 4 * M, dev, "4 M")
    _df_vec("apgd_l1_step", "istate", istate, torch.int32, 4 * M, dev, "4 M")
    ptrs = [t.data_ptr() for _, t in rows]
    if len(set(ptrs)) != len(ptrs):
        raise ValueError("apgd_l1_step: dx, x0, x, x_best and g_best must be five buffers")
    if not (eps >= 0 and lo <= hi) or sign not in (1, -1) or int(window) < 0 or (first and last):
        raise ValueError("apgd_l1_step: need eps >= 0, lo <= hi, sign +1 or -1, window >= 0, and not first and last")
    p = native.ptr
    _C().apgd_l1_step(p(dx), p(loss_rows), p(x0), p(x), p(x_best), p(g_best), p(fstate), p(istate), float(sign),
                      float(eps), float(lo), float(hi), bool(first), bool(last), int(window), M, _s())


CW_SHRINK = 0.999999                # pulls the clean image's tanh-space point inside (-1, 1) (kernels.h CW_SHRINK)
CW_C_INF, CW_C_BIG = 1e10, 1e9      # c_hi before any success; "c_hi is still unset" is c_hi >= CW_C_BIG (kernels.h)
CW_BETA1, CW_BETA2, CW_ADAM_EPS = 0.9, 0.999, 1e-8       # Adam's constants, as in Carlini's code (tf.train.AdamOptimizer)
CW_MAX_M = 1 << 20                  # most images one cw_step launch takes (kernels.h INPUT_GRAD_MAX_B)
# columns of the per-image records (kernels.h CwStepArgs)
CW_C, CW_C_LO, CW_C_HI, CW_D_BEST = 0, 1, 2, 3            # fstate, float32 [M, 4]
CW_SUCC, CW_FOUND_SEARCH, CW_ITERS, CW_SPARE = 0, 1, 2, 3    # istate, int32 [M, 4]


def cw_dist_scale() -> float:
    """MNIST_STD^2: with it the distance term of the CW objective is the squared L2 distance in pixel units."""
    from ..data.datasets import MNIST_STD
    return MNIST_STD * MNIST_STD


def cw_bias_corrections(t: int, beta1: float = CW_BETA1, beta2: float = CW_BETA2) -> tuple:
    """``(1 - beta1^t, 1 - beta2^t)`` of Adam's step ``t`` >= 1: computed in float64, rounded to float32 once."""
    import numpy as np
    if int(t) < 1:
        raise ValueError("cw_bias_corrections: t must be at least 1")
    return float(np.float32(1.0 - float(beta1) ** int(t))), float(np.float32(1.0 - float(beta2) ** int(t)))


def cw_w0(x0: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """atanh((((x0 - lo) / (hi - lo)) * 2 - 1) * CW_SHRINK) in float32: the tanh-space point of the clean image."""
    import numpy as np
    lo32 = np.float32(lo)
    # (a tensor divisor: a true division on every device, never a multiplication by the reciprocal)
    span = torch.tensor(float(np.float32(hi) - lo32), dtype=torch.float32, device=x0.device)
    return torch.atanh((((x0.to(torch.float32) - float(lo32)) / span) * 2.0 - 1.0) * float(np.float32(CW_SHRINK)))


def cw_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, w: torch.Tensor | None,
                      m1: torch.Tensor | None, v: torch.Tensor | None, x: torch.Tensor, x_best: torch.Tensor | None,
                      fstate: torch.Tensor | None, istate: torch.Tensor | None, sign: float, kappa: float, lr: float,
                      c_init: float, t: int, search: int, lo: float, hi: float, beta1: float = CW_BETA1,
                      beta2: float = CW_BETA2, adam_eps: float = CW_ADAM_EPS, dist_scale: float | None = None,
                      first: bool = False, search_end: bool = False, last: bool = False):
    """``cw_step`` operation by operation in torch float32 on any device (the CPU / fp32 path of
    ``Predictor.carlini_wagner``, and what the kernel's tests hold it against).  Same operands - ``dx``, ``x0``, ``w``,
    ``m1``, ``v``, ``x``, ``x_best`` [M, 784], ``loss_rows`` [M], ``fstate`` [M, 4] (c, c_lo, c_hi, d_best), ``istate``
    integers [M, 4] (succ, found_search, iters, spare) - none of them modified; returns the new ``(w, m1, v, x, x_best,
    fstate, istate)``.  With ``first`` w, m1, v, x_best and the records are not read (None will do) and ``x`` is the
    clean image.  Per image, with L = sign * loss, D = sum (x - x0)^2 and w0 = ``cw_w0(x0)``:

        first:       c = c_init; c_lo = 0; c_hi = CW_C_INF; d_best = inf; succ = found_search = iters = 0
                     w = w0; m1 = v = 0; x_best = x0
        evaluate:    ok = L > 0 and L >= kappa;  ok: succ = 1, and if D < d_best: d_best = D, x_best = x,
                     found_search = search + 1
        last:        stop here
        search_end:  succ: c_hi = min(c_hi, c), c = (c_lo + c_hi) / 2 if c_hi < CW_C_BIG
                     else: c_lo = max(c_lo, c), c = (c_lo + c_hi) / 2 if c_hi < CW_C_BIG else 10 c
                     succ = 0; w = w0; m1 = v = 0; x = x0
        otherwise:   th = tanh(w); act = L < kappa
                     gx = (2 dist_scale) (x - x0) - (sign c act) dx;  gw = gx ((0.5 (hi - lo)) (1 - th th))
                     m1 = beta1 m1 + (1 - beta1) gw;  v = beta2 v + ((1 - beta2) gw) gw
                     w = w - (lr (m1 / bc1)) / (sqrt(v / bc2) + adam_eps),  (bc1, bc2) = ``cw_bias_corrections(t)``
                     x = clamp(lo + (hi - lo) (0.5 (tanh(w) + 1)), lo, hi); iters += 1

    Every scalar is rounded to float32 first, as the kernel receives it."""
    import numpy as np
    if sign not in (1, -1) or (first and last) or not kappa >= 0 or not lr > 0 or int(search) < 0:
        raise ValueError("cw_step_reference: sign is +1 or -1, kappa >= 0, lr > 0, search >= 0, and a launch is not "
                         "first and last")
    if first and not c_init > 0:
        raise ValueError("cw_step_reference: c_init must be > 0")
    f32 = np.float32
    dt, dev = torch.float32, dx.device
    M = dx.shape[0]
    kap, lo32, hi32 = float(f32(kappa)), f32(lo), f32(hi)
    span = hi32 - lo32
    big = float(f32(CW_C_BIG))
    x0, x = x0.reshape(M, 784).to(dt), x.reshape(M, 784).to(dt)
    L = float(sign) * loss_rows.reshape(M).to(dt)
    i32 = dict(dtype=torch.int32, device=dev)
    if first:
        c = torch.full((M,), float(f32(c_init)), dtype=dt, device=dev)
        c_lo, c_hi = torch.zeros_like(c), torch.full_like(c, float(f32(CW_C_INF)))
        d_best = torch.full_like(c, float("inf"))
        succ, found, iters, spare = (torch.zeros(M, **i32) for _ in range(4))
        xb = x0
    else:
        c, c_lo, c_hi, d_best = fstate.reshape(M, 4).to(dt).unbind(dim=1)
        succ, found, iters, spare = istate.reshape(M, 4).to(torch.int32).unbind(dim=1)
        xb = x_best.reshape(M, 784).to(dt)
    D = (x - x0).square().sum(dim=1)
    ok = (L > 0) & (L >= kap)
    improved = ok & (D < d_best)
    succ = torch.where(ok, torch.ones_like(succ), succ)
    d_best = torch.where(improved, D, d_best)
    found = torch.where(improved, torch.full_like(found, int(search) + 1), found)
    xb = torch.where(improved[:, None], x, xb)
    pack = lambda: (torch.stack((c, c_lo, c_hi, d_best), dim=1),                              # noqa: E731
                    torch.stack((succ, found, iters, spare), dim=1))
    w0 = cw_w0(x0, lo, hi)
    if last:
        return (w.reshape(M, 784).clone(), m1.reshape(M, 784).clone(), v.reshape(M, 784).clone(), x.clone(), xb,
                *pack())
    if search_end:
        s = succ > 0
        hi_s = torch.minimum(c_hi, c)
        c_s = torch.where(hi_s < big, (c_lo + hi_s) * 0.5, c)
        lo_f = torch.maximum(c_lo, c)
        c_f = torch.where(c_hi < big, (lo_f + c_hi) * 0.5, c * 10.0)
        c, c_lo, c_hi = torch.where(s, c_s, c_f), torch.where(s, c_lo, lo_f), torch.where(s, hi_s, c_hi)
        succ = torch.zeros_like(succ)
        return (w0, torch.zeros_like(x0), torch.zeros_like(x0), x0.clone(), xb, *pack())
    if first:
        w, m1, v = w0, torch.zeros_like(x0), torch.zeros_like(x0)
    else:
        w, m1, v = (q.reshape(M, 784).to(dt) for q in (w, m1, v))
    b1, b2 = f32(beta1), f32(beta2)
    bc1, bc2 = (torch.tensor(q, dtype=dt, device=dev) for q in cw_bias_corrections(t, beta1, beta2))   # (as cw_w0)
    k2 = float(f32(2.0) * f32(cw_dist_scale() if dist_scale is None else dist_scale))
    s = ((float(sign) * c) * (L < kap).to(dt))[:, None]
    th = torch.tanh(w)
    gx = k2 * (x - x0) - s * dx.reshape(M, 784).to(dt)
    gw = gx * (float(f32(0.5) * span) * (1.0 - th * th))
    m1 = float(b1) * m1 + float(f32(1.0) - b1) * gw
    v = float(b2) * v + (float(f32(1.0) - b2) * gw) * gw
    w = w - (float(f32(lr)) * (m1 / bc1)) / (torch.sqrt(v / bc2) + float(f32(adam_eps)))
    x_new = (float(lo32) + float(span) * (0.5 * (torch.tanh(w) + 1.0))).clamp(float(lo32), float(hi32))
    iters = iters + 1
    return (w, m1, v, x_new, xb, *pack())


def cw_step(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, w: torch.Tensor, m1: torch.Tensor,
            v: torch.Tensor, x: torch.Tensor, x_best: torch.Tensor, fstate: torch.Tensor, istate: torch.Tensor,
            sign: float, kappa: float, lr: float, c_init: float, t: int, search: int, lo: float, hi: float,
            beta1: float = CW_BETA1, beta2: float = CW_BETA2, adam_eps: float = CW_ADAM_EPS,
            dist_scale: float | None = None, first: bool = False, search_end: bool = False, last: bool = False,
            M: int | None = None) -> None:
    """One Carlini-Wagner L2 iteration per image (``csrc/kernels/cw.hip``), one launch, in place: from the gradient
    rows ``dx`` (float32 [>= M, 784], what ``input_grad`` wrote) and the CW margins ``loss_rows`` (float32 [>= M], what
    ``head_margin`` stored) at the iterate ``x``, and the clean images ``x0``, the update of ``cw_step_reference`` on
    ``w``, ``m1``, ``v``, ``x``, ``x_best`` (float32 [>= M, 784]), ``fstate`` (float32 [>= M, 4]) and ``istate``
    (int32 [>= M, 4]).  float32 throughout, the distance a fixed tree: the same operands give the same bits.
    ``first``: no state is read, all of it is written, and ``x`` must hold ``x0``; ``search_end``: the bisection of c
    and the restart from the clean image; ``last``: only the best point and the records are brought up to date.
    ``t``: Adam's step index inside the search step (>= 1); ``search``: the search step's index.  ``M``: the images
    of the launch (default ``x.shape[0]``); nothing past M is touched."""
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("cw_step: x must be a float32 [M, 784] tensor on the GPU")
    dev = x.device
    M = int(x.shape[0] if M is None else M)
    if M < 1 or M > CW_MAX_M:
        raise ValueError(f"cw_step: M = {M} images must be in [1, CW_MAX_M = {CW_MAX_M}] a launch")
    rows = (("dx", dx), ("x0", x0), ("w", w), ("m1", m1), ("v", v), ("x", x), ("x_best", x_best))
    for what, q in rows:
        _f32_rows("cw_step", what, q, M, dev, at_least="M")
    _df_vec("cw_step", "loss_rows", loss_rows, torch.float32, M, dev, "M")
    _df_vec("cw_step", "fstate", fstate, torch.float32, 4 * M, dev, "4 M")
    _df_vec("cw_step", "istate", istate, torch.int32, 4 * M, dev, "4 M")
    ptrs = [q.data_ptr() for _, q in rows]
    if len(set(ptrs)) != len(ptrs):
        raise ValueError("cw_step: dx, x0, w, m1, v, x and x_best must be seven buffers")
    if sign not in (1, -1) or not kappa >= 0 or not lr > 0 or not lo < hi or int(search) < 0 or (first and last):
        raise ValueError("cw_step: need sign +1 or -1, kappa >= 0, lr > 0, lo < hi, search >= 0, and not first and last")
    if first and not c_init > 0:
        raise ValueError("cw_step: c_init must be > 0")
    if not (0 <= beta1 < 1 and 0 <= beta2 < 1 and adam_eps > 0):
        raise ValueError("cw_step: need beta1, beta2 in [0, 1) and adam_eps > 0")
    bc1, bc2 = cw_bias_corrections(t, beta1, beta2)
    p = native.ptr
    _C().cw_step(p(dx), p(loss_rows), p(x0), p(w), p(m1), p(v), p(x), p(x_best), p(fstate), p(istate), float(sign),
                 float(kappa), float(lr), float(c_init), float(beta1), float(beta2), float(adam_eps), bc1, bc2,
                 float(cw_dist_scale() if dist_scale is None else dist_scale), float(lo), float(hi), int(search),
                 bool(first), bool(search_end), bool(last), M, _s())


EAD_RULES = {"en": 0, "l1": 1}      # the distance the best point is chosen by (kernels.h EadRule)
EAD_MAX_M = CW_MAX_M // 2           # most images one ead_step launch takes: the chain runs two rows an image


def ead_schedule(k: int, steps: int, lr: float) -> tuple:
    """``(lr_k, zeta_k)`` of update ``k`` in [0, steps) of an EAD search step: lr sqrt(1 - k / steps), the authors'
    square-root decay, and the FISTA momentum k / (k + 3); computed in float64, rounded to float32 once."""
    import numpy as np
    k, steps = int(k), int(steps)
    if steps < 1 or not 0 <= k < steps:
        raise ValueError("ead_schedule: need steps >= 1 and k in [0, steps)")
    return float(np.float32(float(lr) * (1.0 - k / steps) ** 0.5)), float(np.float32(k / (k + 3.0)))


def ead_beta_n(beta: float) -> float:
    """beta / MNIST_STD: the shrinkage threshold in normalised units; float64, rounded to float32 once."""
    import numpy as np
    from ..data.datasets import MNIST_STD
    return float(np.float32(float(beta) / MNIST_STD))


def _row_tree_sum(t: torch.Tensor) -> torch.Tensor:
    """The sum over a [M, 784] row in the row kernels' order (row_ops.h): each thread's (t0 + t1) + (t2 + t3) of its
    float4, the xor butterfly 32 .. 1 over the wave's 64 lanes (60 idle threads add zeros), then (w0 + w1) + (w2 + w3)."""
    M = t.shape[0]
    q = t.reshape(M, 196, 4)
    s = torch.zeros(M, 256, dtype=t.dtype, device=t.device)
    s[:, :196] = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    s = s.view(M, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s[..., :o] + s[..., o:]
    s = s[..., 0]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def ead_step_reference(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, x: torch.Tensor,
                       x_best: torch.Tensor | None, fstate: torch.Tensor | None, istate: torch.Tensor | None,
                       sign: float, kappa: float, lr: float, c_init: float, beta: float, k: int, steps: int,
                       search: int, lo: float, hi: float, rule: str = "en", first: bool = False,
                       search_end: bool = False, last: bool = False):
    """``ead_step`` operation by operation in torch float32 on any device, the two distance sums in the kernel's own
    tree (the CPU / fp32 path of ``Predictor.elastic_net``, and what the kernel's tests hold it against).  Same
    operands - ``dx``, ``x0``, ``y``, ``x``, ``x_best`` [M, 784], ``loss_rows`` [2 M] (the margins at the y rows, then
    at the x rows), ``fstate`` [M, 4] (c, c_lo, c_hi, d_best), ``istate`` integers [M, 4] (succ, found_search, iters,
    spare) - none of them modified; returns the new ``(y, x, x_best, fstate, istate)``.  With ``first`` x_best and the
    records are not read (None will do) and ``x`` = ``y`` = the clean image.  Per image, with L_y, L_x = sign * the
    two margins, s2 = MNIST_STD^2, D1 = sum |x - x0|, D2 = sum (x - x0)^2:

        first:       c = c_init; c_lo = 0; c_hi = CW_C_INF; d_best = inf; succ = found_search = iters = 0; x_best = x0
        evaluate:    dist = STD D1 ("l1") or s2 D2 + beta (STD D1) ("en");  ok = L_x > 0 and L_x >= kappa
                     ok: succ = 1, and if dist < d_best: d_best = dist, x_best = x, found_search = search + 1
        last:        stop here
        search_end:  ``cw_step_reference``'s bisection of c;  succ = 0;  x = y = x0
        otherwise:   act = L_y < kappa;  (lr_k, zeta_k) = ``ead_schedule(k, steps, lr)``
                     z = y - (lr_k / s2) ((2 s2) (y - x0) - (sign c act) dx);  d = z - x0
                     x+ = min(z - beta_n, hi) where d > beta_n, max(z + beta_n, lo) where d < -beta_n, else x0
                     y+ = x+ + zeta_k (x+ - x);  iters += 1

    Every scalar is rounded to float32 first, as the kernel receives it."""
    import numpy as np
    from ..data.datasets import MNIST_STD
    if sign not in (1, -1) or (first and last) or not kappa >= 0 or not lr > 0 or not beta >= 0 or int(search) < 0:
        raise ValueError("ead_step_reference: sign is +1 or -1, kappa >= 0, lr > 0, beta >= 0, search >= 0, and a "
                         "launch is not first and last")
    if rule not in EAD_RULES:
        raise ValueError(f"ead_step_reference: rule must be 'en' or 'l1', got {rule!r}")
    if first and not c_init > 0:
        raise ValueError("ead_step_reference: c_init must be > 0")
    f32 = np.float32
    dt, dev = torch.float32, dx.device
    M = x0.shape[0]
    kap, lo32, hi32 = float(f32(kappa)), float(f32(lo)), float(f32(hi))
    std, s2, b32, bn = f32(MNIST_STD), f32(cw_dist_scale()), f32(beta), f32(ead_beta_n(beta))
    big = float(f32(CW_C_BIG))
    x0, x, y = (q.reshape(M, 784).to(dt) for q in (x0, x, y))
    L = float(sign) * loss_rows.reshape(-1)[:2 * M].to(dt)
    Ly, Lx = L[:M], L[M:]
    i32 = dict(dtype=torch.int32, device=dev)
    if first:
        c = torch.full((M,), float(f32(c_init)), dtype=dt, device=dev)
        c_lo, c_hi = torch.zeros_like(c), torch.full_like(c, float(f32(CW_C_INF)))
        d_best = torch.full_like(c, float("inf"))
        succ, found, iters, spare = (torch.zeros(M, **i32) for _ in range(4))
        xb = x0
    else:
        c, c_lo, c_hi, d_best = fstate.reshape(M, 4).to(dt).unbind(dim=1)
        succ, found, iters, spare = istate.reshape(M, 4).to(torch.int32).unbind(dim=1)
        xb = x_best.reshape(M, 784).to(dt)
    d = x - x0
    dist = float(std) * _row_tree_sum(d.abs())
    if rule == "en":
        dist = float(s2) * _row_tree_sum(d * d) + float(b32) * dist
    ok = (Lx > 0) & (Lx >= kap)
    improved = ok & (dist < d_best)
    succ = torch.where(ok, torch.ones_like(succ), succ)
    d_best = torch.where(improved, dist, d_best)
    found = torch.where(improved, torch.full_like(found, int(search) + 1), found)
    xb = torch.where(improved[:, None], x, xb)
    pack = lambda: (torch.stack((c, c_lo, c_hi, d_best), dim=1),                              # noqa: E731
                    torch.stack((succ, found, iters, spare), dim=1))
    if last:
        return (y.clone(), x.clone(), xb, *pack())
    if search_end:
        s = succ > 0
        hi_s = torch.minimum(c_hi, c)
        c_s = torch.where(hi_s < big, (c_lo + hi_s) * 0.5, c)
        lo_f = torch.maximum(c_lo, c)
        c_f = torch.where(c_hi < big, (lo_f + c_hi) * 0.5, c * 10.0)
        c, c_lo, c_hi = torch.where(s, c_s, c_f), torch.where(s, c_lo, lo_f), torch.where(s, hi_s, c_hi)
        succ = torch.zeros_like(succ)
        return (x0.clone(), x0.clone(), xb, *pack())
    lr_k, zeta_k = ead_schedule(k, steps, lr)
    lrs, k2, bnf = float(f32(lr_k) / s2), float(f32(2.0) * s2), float(bn)
    sc = ((float(sign) * c) * (Ly < kap).to(dt))[:, None]
    z = y - lrs * (k2 * (y - x0) - sc * dx.reshape(-1, 784)[:M].to(dt))
    d = z - x0
    x_new = torch.where(d > bnf, (z - bnf).clamp(max=hi32), torch.where(d < -bnf, (z + bnf).clamp(min=lo32), x0))
    y_new = x_new + zeta_k * (x_new - x)
    iters = iters + 1
    return (y_new, x_new, xb, *pack())


def ead_step(dx: torch.Tensor, loss_rows: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, x: torch.Tensor,
             x_best: torch.Tensor, fstate: torch.Tensor, istate: torch.Tensor, sign: float, kappa: float, lr: float,
             c_init: float, beta: float, k: int, steps: int, search: int, lo: float, hi: float, rule: str = "en",
             first: bool = False, search_end: bool = False, last: bool = False, M: int | None = None) -> None:
    """One EAD (elastic-net) iteration per image (``csrc/kernels/ead.hip``), one launch, in place: from the gradient
    rows ``dx`` (float32 [>= M, 784], what ``input_grad`` wrote for the y rows) and the CW margins ``loss_rows``
    (float32 [>= 2 M]: entry i at the slack point ``y[i]``, entry M + i at the shrunk point ``x[i]``, what
    ``head_margin`` stored for a chain over the y rows followed by the x rows), and the clean images ``x0``, the update
    of ``ead_step_reference`` on ``y``, ``x``, ``x_best`` (float32 [>= M, 784]), ``fstate`` (float32 [>= M, 4]) and
    ``istate`` (int32 [>= M, 4]).  float32 throughout, the distances a fixed tree: the same operands give the same
    bits.  ``first``: no state is read, all of it is written, and ``x`` and ``y`` must hold ``x0``; ``search_end``:
    the bisection of c and the restart from the clean image; ``last``: only the best point and the records are brought
    up to date.  ``k``: the update's index inside the search step, in [0, ``steps``) (not read by a ``search_end`` or
    ``last`` launch); ``search``: the search step's index.  ``M``: the images of the launch (default ``x.shape[0]``);
    nothing past M is touched."""
    from ..data.datasets import MNIST_STD
    if x.dim() != 2 or x.device.type != "cuda":
        raise ValueError("ead_step: x must be a float32 [M, 784] tensor on the GPU")
    dev = x.device
    M = int(x.shape[0] if M is None else M)
    if M < 1 or M > EAD_MAX_M:
        raise ValueError(f"ead_step: M = {M} images must be in [1, EAD_MAX_M = {EAD_MAX_M}] a launch")
    rows = (("dx", dx), ("x0", x0), ("y", y), ("x", x), ("x_best", x_best))
    for what, q in rows:
        _f32_rows("ead_step", what, q, M, dev, at_least="M")
    _df_vec("ead_step", "loss_rows", loss_rows, torch.float32, 2 * M, dev, "2 M")
    _df_vec("ead_step", "fstate", fstate, torch.float32, 4 * M, dev, "4 M")
    _df_vec("ead_step", "istate", istate, torch.int32, 4 * M, dev, "4 M")
    ptrs = [q.data_ptr() for _, q in rows]
    if len(set(ptrs)) != len(ptrs):
        raise ValueError("ead_step: dx, x0, y, x and x_best must be five buffers")
    if sign not in (1, -1) or not kappa >= 0 or not lr > 0 or not lo < hi or int(search) < 0 or (first and last):
        raise ValueError("ead_step: need sign +1 or -1, kappa >= 0, lr > 0, lo < hi, search >= 0, and not first and last")
    if first and not c_init > 0:
        raise ValueError("ead_step: c_init must be > 0")
    if not beta >= 0 or rule not in EAD_RULES:
        raise ValueError("ead_step: need beta >= 0 and rule 'en' or 'l1'")
    lr_k, zeta_k = (float(lr), 0.0) if (search_end or last) else ead_schedule(k, steps, lr)
    p = native.ptr
    _C().ead_step(p(dx), p(loss_rows), p(x0), p(y), p(x), p(x_best), p(fstate), p(istate), float(sign), float(kappa),
                  float(c_init), lr_k, zeta_k, float(beta), ead_beta_n(beta), float(MNIST_STD), cw_dist_scale(),
                  float(lo), float(hi), int(search), EAD_RULES[rule], bool(first), bool(search_end), bool(last), M,
                  _s())


IBP_SPLITS = 36                     # fc1 split-K of ibp_fc1: fixed, whatever the batch (kernels.h IBP_SPLITS)
IBP_MAX_B = 65535                   # most images one ibp launch takes (kernels.h IBP_MAX_B)
IBP_EPS, IBP_LO, IBP_HI, IBP_MARGIN = 0, 1, 2, 3         # columns of the per-image record, float32 [M, 4]


def _ibp_setup(net_or_params, dtype, lo, hi):
    """(parameters as ``dtype`` tensors by torch name, MNIST_STD / lo / hi as the float32 values the kernels get)."""
    import numpy as np
    from ..data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
    named = dict(net_or_params.named_parameters()) if hasattr(net_or_params, "named_parameters") else net_or_params
    f32 = lambda v: float(np.float32(v))                                                       # noqa: E731
    return ({k: v.detach().to(dtype) for k, v in named.items()}, f32(MNIST_STD),
            f32(PIXEL_LO if lo is None else lo), f32(PIXEL_HI if hi is None else hi))


def ibp_trunk_reference(net_or_params, x: torch.Tensor, eps: torch.Tensor, lo: float | None = None,
                        hi: float | None = None, dtype=torch.float32):
    """``ibp_trunk`` in torch ops on any device: ``(pl, pu)`` [M, 9216], the bounds after the pool in torch flatten
    order, of the box ``[max(x - eps / STD, lo), min(x + eps / STD, hi)]`` (``x`` [M, 784] normalised, ``eps`` [M] in
    pixel units) through conv1, ReLU, conv2, ReLU and the pool, each affine layer in centre / radius form: mu = (l + u)
    / 2, r = (u - l) / 2, c = W mu + b, rad = |W| r, l' = c - rad, u' = c + rad.  A NaN passes every clamp."""
    import torch.nn.functional as F
    P, std, lo, hi = _ibp_setup(net_or_params, dtype, lo, hi)
    M = x.shape[0]
    x = x.reshape(M, 784).to(dtype)
    e = (eps.reshape(M).to(dtype) / torch.tensor(std, dtype=dtype, device=x.device))[:, None]
    l, u = torch.clamp(x - e, min=lo).view(M, 1, 28, 28), torch.clamp(x + e, max=hi).view(M, 1, 28, 28)
    for name in ("conv1", "conv2"):
        W, b = P[name + ".weight"], P[name + ".bias"]
        c, rad = F.conv2d((l + u) * 0.5, W, b), F.conv2d((u - l) * 0.5, W.abs())
        l, u = F.relu(c - rad), F.relu(c + rad)
    return F.max_pool2d(l, 2).flatten(1), F.max_pool2d(u, 2).flatten(1)


def ibp_fc1_reference(net_or_params, pl: torch.Tensor, pu: torch.Tensor, dtype=torch.float32):
    """``ibp_fc1`` summed over its splits: ``(z1c, z1r)`` [M, 128] = fc1.weight (pl + pu) / 2, |fc1.weight| (pu - pl) / 2
    (no bias: ``ibp_head`` adds it)."""
    W = _ibp_setup(net_or_params, dtype, None, None)[0]["fc1.weight"]
    pl, pu = pl.to(dtype), pu.to(dtype)
    return ((pl + pu) * 0.5) @ W.t(), ((pu - pl) * 0.5) @ W.abs().t()


def ibp_head_reference(net_or_params, part: torch.Tensor, labels: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``ibp_head`` operation by operation: ``lb`` [M, 10] from the fc1 partial sums ``part`` [S, M, 2, 128] (centre,
    radius; any S): the splits summed in order, + fc1.bias, l = relu(c - rad), u = relu(c + rad), then for j != y with
    C = fc2.weight[y] - fc2.weight[j]: lb_j = sum_k (max(C_k, 0) l_k + min(C_k, 0) u_k) + (b_y - b_j), the sum as
    (t_k + t_{k+64}) then the xor butterfly 32 .. 1 of the kernel's wave; lb_y = +inf."""
    P = _ibp_setup(net_or_params, dtype, None, None)[0]
    part = part.to(dtype)
    M, y = part.shape[1], labels.reshape(-1).long()
    c, rad = part[0, :, 0], part[0, :, 1]
    for z in range(1, part.shape[0]):
        c, rad = c + part[z, :, 0], rad + part[z, :, 1]
    c = c + P["fc1.bias"]
    l, u = torch.relu(c - rad)[:, None, :], torch.relu(c + rad)[:, None, :]
    W2, b2 = P["fc2.weight"], P["fc2.bias"]
    Cm = W2[y][:, None, :] - W2[None]
    t = Cm.clamp(min=0) * l + Cm.clamp(max=0) * u
    s = t[..., :64] + t[..., 64:]
    idx = torch.arange(64, device=s.device)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ o]
    lb = s[..., 0] + (b2[y][:, None] - b2[None, :])
    lb[torch.arange(M, device=lb.device), y] = float("inf")
    return lb


def ibp_reference(net_or_params, x: torch.Tensor, labels: torch.Tensor, eps, dtype=torch.float32,
                  lo: float | None = None, hi: float | None = None) -> dict:
    """Interval bound propagation of the Net (inference semantics) over the L-inf box of radius ``eps`` (pixel units,
    a number or [M]) around the normalised rows ``x`` [M, 784], clipped to the valid pixel range, in torch ops on any
    device - the kernels' formulas, stage by stage: ``pl``, ``pu`` [M, 9216] (after the pool), ``z1c``, ``z1r`` [M, 128]
    (fc1 centre and radius, before the bias), ``lb`` [M, 10] (lower bounds of z_y - z_j, +inf at y), ``margin`` [M]
    (min_j lb_j, NaN where any is) and ``certified`` (margin > 0).  ``net_or_params``: a Net, or its parameters by
    torch name."""
    M = x.shape[0]
    eps = torch.as_tensor(eps, dtype=dtype, device=x.device).expand(M)
    pl, pu = ibp_trunk_reference(net_or_params, x, eps, lo, hi, dtype)
    z1c, z1r = ibp_fc1_reference(net_or_params, pl, pu, dtype)
    lb = ibp_head_reference(net_or_params, torch.stack((z1c, z1r), dim=1)[None], labels, dtype)
    margin = lb.min(dim=1).values
    return {"pl": pl, "pu": pu, "z1c": z1c, "z1r": z1r, "lb": lb, "margin": margin, "certified": margin > 0}


def ibp_search_reference(rec: torch.Tensor, lb: torch.Tensor) -> torch.Tensor:
    """The record update of ``ibp_head`` with ``search``: from ``rec`` [M, 4] = (eps, lo, hi, margin) and ``lb``
    [M, 10]: margin = min_j lb_j; margin > 0 (a NaN is not): lo = eps, else hi = eps; eps = lo + 0.5 (hi - lo)."""
    rec = rec.to(torch.float32)
    margin = lb.to(torch.float32).min(dim=1).values
    cert = margin > 0
    lo, hi = torch.where(cert, rec[:, IBP_EPS], rec[:, IBP_LO]), torch.where(cert, rec[:, IBP_HI], rec[:, IBP_EPS])
    return torch.stack((lo + 0.5 * (hi - lo), lo, hi, margin), dim=1)


def _ibp_buf(name: str, what: str, t: torch.Tensor | None, count: int, dev, dtype=torch.float32) -> torch.Tensor:
    """The float32 array ``t`` of at least ``count`` entries of an ibp launch; a new one when None."""
    if t is None:
        return torch.empty(count, dtype=dtype, device=dev)
    _df_vec(name, what, t, dtype, count, dev, str(count))
    return t


def _ibp_param(name: str, param: torch.Tensor, M: int) -> None:
    if param.dtype != torch.float32 or param.device.type != "cuda" or not param.is_contiguous() or \
            param.numel() != _C().PARAM_TOTAL:
        raise ValueError(f"{name}: param must be the flat float32 parameter buffer on the GPU")
    if M < 1 or M > IBP_MAX_B:
        raise ValueError(f"{name}: M = {M} images must be in [1, IBP_MAX_B = {IBP_MAX_B}] a launch")


def ibp_trunk(param: torch.Tensor, x: torch.Tensor, rec: torch.Tensor, pl: torch.Tensor | None = None,
              pu: torch.Tensor | None = None, lo: float | None = None, hi: float | None = None, M: int | None = None):
    """One launch of ``ibp_trunk`` (csrc/kernels/ibp.hip): ``(pl, pu)`` float32 [>= M, 9216] in torch flatten order
    from the normalised rows ``x`` (float32 [>= M, 784]) and each image's eps ``rec[i, 0]`` (float32 [>= M, 4], pixel
    units), through the flat fp32 parameters ``param`` (``ModelState.param``).  Nothing past M is touched."""
    M = int(x.shape[0] if M is None else M)
    _ibp_param("ibp_trunk", param, M)
    dev = param.device
    _f32_rows("ibp_trunk", "x", x, M, dev, at_least="M")
    _df_vec("ibp_trunk", "rec", rec, torch.float32, 4 * M, dev, "4 M")
    pl, pu = (_ibp_buf("ibp_trunk", k, q, M * NFLAT, dev) for k, q in (("pl", pl), ("pu", pu)))
    _, std, lo, hi = _ibp_setup({}, torch.float32, lo, hi)
    if not lo < hi or pl.data_ptr() == pu.data_ptr():
        raise ValueError("ibp_trunk: need lo < hi and two output buffers")
    p = native.ptr
    _C().ibp_trunk(p(param), p(x), p(rec), p(pl), p(pu), std, lo, hi, M, _s())
    return pl.view(-1, NFLAT), pu.view(-1, NFLAT)


def ibp_fc1(param: torch.Tensor, pl: torch.Tensor, pu: torch.Tensor, part: torch.Tensor | None = None,
            M: int | None = None) -> torch.Tensor:
    """One launch of ``ibp_fc1``: the split-K partial sums ``part`` (float32, ``IBP_SPLITS * M * 256`` entries laid out
    [IBP_SPLITS, M, 2, 128]: centre, radius) of fc1 over the bounds ``pl``, ``pu`` (float32 [>= M, 9216], torch flatten
    order).  An image's values do not depend on M or on its row.  Nothing past that many entries is touched."""
    M = int(pl.shape[0] if M is None else M)
    _ibp_param("ibp_fc1", param, M)
    dev = param.device
    for what, q in (("pl", pl), ("pu", pu)):
        _df_vec("ibp_fc1", what, q, torch.float32, M * NFLAT, dev, "M * 9216")
    part = _ibp_buf("ibp_fc1", "part", part, IBP_SPLITS * M * 2 * NH, dev)
    p = native.ptr
    _C().ibp_fc1(p(param), p(pl), p(pu), p(part), M, _s())
    return part


def ibp_head(param: torch.Tensor, part: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor,
             lb: torch.Tensor | None = None, search: bool = False, M: int | None = None) -> torch.Tensor:
    """One launch of ``ibp_head``: ``lb`` float32 [>= M, 10] (``ibp_head_reference``) from ``part`` ([IBP_SPLITS, M,
    2, 128] as ``ibp_fc1`` wrote it) and the int32 ``labels`` [>= M] in [0, 10) (not checked).  ``search``: the records
    ``rec`` (float32 [>= M, 4]) are updated as ``ibp_search_reference`` does from this launch's ``lb``; else only read."""
    M = int(labels.numel() if M is None else M)
    _ibp_param("ibp_head", param, M)
    dev = param.device
    _df_vec("ibp_head", "part", part, torch.float32, IBP_SPLITS * M * 2 * NH, dev, "IBP_SPLITS * M * 256")
    _df_vec("ibp_head", "labels", labels, torch.int32, M, dev, "M")
    _df_vec("ibp_head", "rec", rec, torch.float32, 4 * M, dev, "4 M")
    lb = _ibp_buf("ibp_head", "lb", lb, M * NCLS, dev)
    p = native.ptr
    _C().ibp_head(p(param), p(part), p(labels), p(lb), p(rec), bool(search), M, _s())
    return lb.view(-1, NCLS)


CROWN_SPEC = 16                     # specification slots an image in crown_lambda / crown_fc (kernels.h CROWN_SPEC)
CROWN_SLICES = 576                  # 16-column slices of crown_fc's bias partials (kernels.h CROWN_SLICES)
CROWN_STRIPS = 7                    # strips of 4 input rows of crown_bwd (kernels.h CROWN_STRIPS)


def relu_relax_reference(l: torch.Tensor, u: torch.Tensor):
    """``(sL, sU, bU)`` of relu over [l, u]: sL z <= relu(z) <= sU z + bU.  l >= 0: (1, 1, 0); u <= 0: zeros; else
    sU = u / (u - l), bU = -l u / (u - l) and sL = 1 where u > -l, else 0."""
    pos = l >= 0
    un = ~pos & ~(u <= 0)
    one, zero, d = torch.ones_like(l), torch.zeros_like(l), u - l
    return (torch.where(pos | (un & (u > -l)), one, zero), torch.where(pos, one, torch.where(un, u / d, zero)),
            torch.where(un, (-l * u) / d, zero))


def _windows(t: torch.Tensor) -> torch.Tensor:
    """[M, 64, 24, 24] -> [M, 9216, 4]: each pool window's pixels in row-major order, windows in torch flatten order."""
    M = t.shape[0]
    return t.view(M, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(M, NFLAT, 4)


def _relaxed(A, sL, sU):
    return torch.where(A > 0, A * sL, A * sU)


def _relax_bias(A, bU):
    return torch.where(A < 0, A * bU, torch.zeros_like(A))


def crown_ibp_reference(net_or_params, x: torch.Tensor, labels: torch.Tensor, eps, dtype=torch.float32,
                        lo: float | None = None, hi: float | None = None, record: dict | None = None) -> dict:
    """CROWN-IBP (Zhang et al. 2020) of the Net over the box of ``ibp_reference``, in torch ops on any device - the
    formulas of csrc/kernels/crown.hip stage by stage.  IBP bounds every hidden pre-activation; the ten margin rows
    C_j = fc2.weight[y] - fc2.weight[j] then go backward through one linear relaxation a layer: outgoing coefficients
    A+ sL + A- sU, the bias gains sum A- bU, an affine layer adds A b and gives A W, and at the input
    lb_j = sum(A0+ xl + A0- xu) + bias.  The ReLU and the pool behind it are one relaxation a pooled unit, on the
    window's pixel i* (first argmax of the lower bounds): below sL z_i*; above sU z_i* + bU when pixel i* dominates the
    window (l2[i*] >= every other u2), else the constant U = max u2.

    Stages: ``pl``, ``pu``, ``z1c``, ``z1r``, ``lb_ibp`` as ``ibp_reference``; the record ``sL``, ``sU``, ``bU`` [M, 9216]
    and ``istar`` (int64 [M, 9216], 0 .. 3 row-major in the window); ``lam`` [M, 16, 128] (rows y and 10 .. 15 zero) and
    ``fcb`` [M, 16] (the bias down to fc1's input); ``v`` [M, 10, 9216] and ``vb`` [M, 576, 10] (the pool's and conv2's
    bias terms by 16-column slice); ``sp`` [M, 7, 10, 2] ((concretised sum, bias) of each strip of 4 input rows);
    ``lb_crown``; ``lb`` = max(lb_crown, lb_ibp) (+inf at y); ``margin`` and ``certified``.  ``record``: the backward
    pass runs from these ``sL``, ``sU``, ``bU``, ``istar`` instead of the ones computed here."""
    import torch.nn.functional as F
    M, dev = x.shape[0], x.device
    y = labels.reshape(-1).long().to(dev)
    P, xl, xu, pre1 = crown_box_reference(net_or_params, x, eps, dtype, lo, hi)
    l, u = F.relu(pre1[0]), F.relu(pre1[1])
    c, rad = F.conv2d((l + u) * 0.5, P["conv2.weight"], P["conv2.bias"]), F.conv2d((u - l) * 0.5, P["conv2.weight"].abs())
    pl, pu = F.max_pool2d(F.relu(c - rad), 2).flatten(1), F.max_pool2d(F.relu(c + rad), 2).flatten(1)
    l2w, u2w = _windows(c - rad), _windows(c + rad)
    istar = l2w.argmax(dim=2)
    ls, us, U = l2w.gather(2, istar[..., None])[..., 0], u2w.gather(2, istar[..., None])[..., 0], u2w.max(dim=2).values
    dom = ((ls[..., None] >= u2w) | F.one_hot(istar, 4).bool()).all(dim=2)
    sL, sU, bU = relu_relax_reference(ls, us)
    zero = torch.zeros_like(sL)
    sU, bU = torch.where(dom, sU, zero), torch.where(dom, bU, U)
    sL, sU, bU = (torch.where(U <= 0, zero, t) for t in (sL, sU, bU))
    out = {"pl": pl, "pu": pu, "sL": sL, "sU": sU, "bU": bU, "istar": istar}
    if record is not None:
        sL, sU, bU = (record[k].to(dev, dtype) for k in ("sL", "sU", "bU"))
        istar = record["istar"].to(dev).long()
    z1c, z1r = ibp_fc1_reference(net_or_params, pl, pu, dtype)
    lb_ibp = ibp_head_reference(net_or_params, torch.stack((z1c, z1r), dim=1)[None], y, dtype)
    lam, fcb = crown_lambda_reference(P, z1c, z1r, y)
    v, vb = crown_fc_reference(P, lam, sL, sU, bU)
    sp = crown_bwd_reference(P, xl, xu, pre1, v, istar)
    lbc, lb = crown_head_reference(fcb, vb, sp, lb_ibp, y)
    margin = lb.min(dim=1).values
    out.update(z1c=z1c, z1r=z1r, lb_ibp=lb_ibp, lam=lam, fcb=fcb, v=v, vb=vb, sp=sp, lb_crown=lbc, lb=lb, margin=margin,
               certified=margin > 0)
    return out


def _wave_sum128(t: torch.Tensor) -> torch.Tensor:
    """The sum over the last axis (128) in a wave's order: (t_k + t_{k+64}), then the xor butterfly 32 .. 1."""
    s = t[..., :64] + t[..., 64:]
    idx = torch.arange(64, device=s.device)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ o]
    return s[..., 0]


def crown_lambda_reference(P: dict, z1c, z1r, y):
    """``crown_lambda``: ``(lam [M, 16, 128], fcb [M, 10])`` from the fc1 sums (before the bias) and the labels."""
    M, dev = z1c.shape[0], z1c.device
    W2f, b2f, b1f = P["fc2.weight"], P["fc2.bias"], P["fc1.bias"]
    c3 = z1c + b1f
    s3L, s3U, b3U = (t[:, None, :] for t in relu_relax_reference(c3 - z1r, c3 + z1r))
    Cm = W2f[y][:, None, :] - W2f[None]
    keep = torch.ones(M, NCLS, dtype=torch.bool, device=dev)
    keep[torch.arange(M, device=dev), y] = False
    lam = _relaxed(Cm, s3L, s3U) * keep[..., None]
    fcb = (_wave_sum128(_relax_bias(Cm, b3U) + lam * b1f) + (b2f[y][:, None] - b2f[None, :])) * keep
    return torch.cat([lam, torch.zeros(M, CROWN_SPEC - NCLS, NH, dtype=lam.dtype, device=dev)], dim=1), fcb


def crown_fc_reference(P: dict, lam, sL, sU, bU):
    """``crown_fc``: ``(v [M, 10, 9216], vb [M, 576, 10])`` from ``lam`` and the pooled record."""
    M = lam.shape[0]
    Ap = lam[:, :NCLS] @ P["fc1.weight"]
    v = _relaxed(Ap, sL[:, None], sU[:, None])
    tb = _relax_bias(Ap, bU[:, None]) + v * P["conv2.bias"].repeat_interleave(144)
    return v, tb.view(M, NCLS, CROWN_SLICES, 16).sum(dim=3).transpose(1, 2)


def crown_bwd_reference(P: dict, xl, xu, pre1, v, istar):
    """``crown_bwd``: ``sp`` [M, 7, 10, 2] from the box ``xl``, ``xu`` [M, 1, 28, 28], the conv1 pre-activation bounds
    ``pre1`` = (l1, u1), the rows ``v`` and each window's ``istar``, in gather form as the kernel runs it."""
    import torch.nn.functional as F
    M = xl.shape[0]
    Vd = (v[..., None] * F.one_hot(istar, 4)[:, None]).view(M * NCLS, 64, 12, 12, 2, 2)
    Vd = Vd.permute(0, 1, 2, 4, 3, 5).reshape(M * NCLS, 64, 24, 24)
    A1 = F.conv2d(F.pad(Vd, (2, 2, 2, 2)), P["conv2.weight"].transpose(0, 1).flip(2, 3)).view(M, NCLS, 32, 26, 26)
    s1L, s1U, b1U = (t[:, None] for t in relu_relax_reference(*pre1))
    A1r = _relaxed(A1, s1L, s1U)
    t1 = _relax_bias(A1, b1U) + A1r * P["conv1.bias"].view(1, 1, 32, 1, 1)
    A0 = F.conv2d(F.pad(A1r.view(M * NCLS, 32, 26, 26), (2, 2, 2, 2)),
                  P["conv1.weight"].transpose(0, 1).flip(2, 3)).view(M, NCLS, 28, 28)
    t0 = torch.where(A0 > 0, A0 * xl, A0 * xu)
    rows1 = F.pad(t1.sum(dim=(2, 4)), (0, 2))                                    # [M, 10, 28]: conv1 rows, by owner
    return torch.stack((t0.sum(dim=3).view(M, NCLS, CROWN_STRIPS, 4).sum(dim=3),
                        rows1.view(M, NCLS, CROWN_STRIPS, 4).sum(dim=3)), dim=3).transpose(1, 2).contiguous()


def crown_head_reference(fcb, vb, sp, lb_ibp, y):
    """``crown_head``: ``(lb_crown, lb)`` [M, 10] from the partials; +inf at the label."""
    lbc = fcb + sp.sum(dim=(1, 3)) + vb.sum(dim=1)
    lbc[torch.arange(lbc.shape[0], device=lbc.device), y] = float("inf")
    return lbc, torch.maximum(lbc, lb_ibp)


def crown_box_reference(net_or_params, x, eps, dtype=torch.float32, lo=None, hi=None):
    """``(P, xl, xu, (l1, u1))``: the parameters, the clipped box [M, 1, 28, 28] and conv1's pre-activation bounds, as
    ``crown_bwd`` recomputes them."""
    import torch.nn.functional as F
    P, std, lo, hi = _ibp_setup(net_or_params, dtype, lo, hi)
    M = x.shape[0]
    x = x.reshape(M, 784).to(dtype)
    e = (torch.as_tensor(eps, dtype=dtype, device=x.device).expand(M) / torch.tensor(std, dtype=dtype, device=x.device))[:, None]
    xl, xu = torch.clamp(x - e, min=lo).view(M, 1, 28, 28), torch.clamp(x + e, max=hi).view(M, 1, 28, 28)
    c = F.conv2d((xl + xu) * 0.5, P["conv1.weight"], P["conv1.bias"])
    rad = F.conv2d((xu - xl) * 0.5, P["conv1.weight"].abs())
    return P, xl, xu, (c - rad, c + rad)


def _crown_rec(rec4: torch.Tensor) -> dict:
    """The kernels' record [M, 9216, 4] (sL, sU, bU, bits of i*) as the reference's fields."""
    return {"sL": rec4[..., 0], "sU": rec4[..., 1], "bU": rec4[..., 2],
            "istar": rec4[..., 3].contiguous().view(torch.int32).long()}


def crown_relax(param: torch.Tensor, x: torch.Tensor, rec: torch.Tensor, pl: torch.Tensor | None = None,
                pu: torch.Tensor | None = None, relax: torch.Tensor | None = None, lo: float | None = None,
                hi: float | None = None, M: int | None = None):
    """One launch of ``crown_relax`` (csrc/kernels/crown.hip): ``(pl, pu, relax)``: ``ibp_trunk``'s bounds and the
    relaxation record float32 [>= M, 9216, 4] = (sL, sU, bU, bits of i*) of every pooled unit.  Arguments as
    ``ibp_trunk``.  Nothing past M is touched."""
    M = int(x.shape[0] if M is None else M)
    _ibp_param("crown_relax", param, M)
    dev = param.device
    _f32_rows("crown_relax", "x", x, M, dev, at_least="M")
    _df_vec("crown_relax", "rec", rec, torch.float32, 4 * M, dev, "4 M")
    pl, pu = (_ibp_buf("crown_relax", k, q, M * NFLAT, dev) for k, q in (("pl", pl), ("pu", pu)))
    relax = _ibp_buf("crown_relax", "relax", relax, M * NFLAT * 4, dev)
    _, std, lo, hi = _ibp_setup({}, torch.float32, lo, hi)
    if not lo < hi or pl.data_ptr() == pu.data_ptr():
        raise ValueError("crown_relax: need lo < hi and two bound buffers")
    p = native.ptr
    _C().crown_relax(p(param), p(x), p(rec), p(pl), p(pu), p(relax), std, lo, hi, M, _s())
    return pl.view(-1, NFLAT), pu.view(-1, NFLAT), relax.view(-1, NFLAT, 4)


def crown_lambda(param: torch.Tensor, part: torch.Tensor, labels: torch.Tensor, lam: torch.Tensor | None = None,
                 fcb: torch.Tensor | None = None, M: int | None = None):
    """One launch of ``crown_lambda``: ``(lam, fcb)`` from the slab ``part`` of ``ibp_fc1`` and the int32 ``labels``:
    the relaxed margin rows float32 [>= M, 16, 128] and [>= M, 2, 16] = (the bias down to fc1's input, lb_ibp)."""
    M = int(labels.numel() if M is None else M)
    _ibp_param("crown_lambda", param, M)
    dev = param.device
    _df_vec("crown_lambda", "part", part, torch.float32, IBP_SPLITS * M * 2 * NH, dev, "IBP_SPLITS * M * 256")
    _df_vec("crown_lambda", "labels", labels, torch.int32, M, dev, "M")
    lam = _ibp_buf("crown_lambda", "lam", lam, M * CROWN_SPEC * NH, dev)
    fcb = _ibp_buf("crown_lambda", "fcb", fcb, M * 2 * CROWN_SPEC, dev)
    p = native.ptr
    _C().crown_lambda(p(param), p(part), p(labels), p(lam), p(fcb), M, _s())
    return lam.view(-1, CROWN_SPEC, NH), fcb.view(-1, 2, CROWN_SPEC)


def crown_fc(param: torch.Tensor, relax: torch.Tensor, lam: torch.Tensor, v: torch.Tensor | None = None,
             vb: torch.Tensor | None = None, M: int | None = None):
    """One launch of ``crown_fc``: ``(v, vb)`` = lam fc1.weight through the pool relaxation ``relax``: float32
    [>= M, 10, 9216] and the bias partials [>= M, 576, 16] (slots 10 .. 15 are not written)."""
    M = int(lam.shape[0] if M is None else M)
    _ibp_param("crown_fc", param, M)
    dev = param.device
    _df_vec("crown_fc", "relax", relax, torch.float32, M * NFLAT * 4, dev, "M * 9216 * 4")
    _df_vec("crown_fc", "lam", lam, torch.float32, M * CROWN_SPEC * NH, dev, "M * 2048")
    v = _ibp_buf("crown_fc", "v", v, M * NCLS * NFLAT, dev)
    vb = _ibp_buf("crown_fc", "vb", vb, M * CROWN_SLICES * CROWN_SPEC, dev)
    p = native.ptr
    _C().crown_fc(p(param), p(relax), p(lam), p(v), p(vb), M, _s())
    return v.view(-1, NCLS, NFLAT), vb.view(-1, CROWN_SLICES, CROWN_SPEC)


def crown_bwd(param: torch.Tensor, x: torch.Tensor, rec: torch.Tensor, relax: torch.Tensor, v: torch.Tensor,
              labels: torch.Tensor, sp: torch.Tensor | None = None, lo: float | None = None, hi: float | None = None,
              M: int | None = None) -> torch.Tensor:
    """One launch of ``crown_bwd``: ``sp`` float32 [>= M, 7, 10, 2], each strip's (concretised sum, bias) of the rows
    ``v`` taken back through conv2, the conv1 relaxation (from the box of ``x`` and ``rec[i, 0]``) and conv1."""
    M = int(x.shape[0] if M is None else M)
    _ibp_param("crown_bwd", param, M)
    dev = param.device
    _f32_rows("crown_bwd", "x", x, M, dev, at_least="M")
    _df_vec("crown_bwd", "rec", rec, torch.float32, 4 * M, dev, "4 M")
    _df_vec("crown_bwd", "relax", relax, torch.float32, M * NFLAT * 4, dev, "M * 9216 * 4")
    _df_vec("crown_bwd", "v", v, torch.float32, M * NCLS * NFLAT, dev, "M * 92160")
    _df_vec("crown_bwd", "labels", labels, torch.int32, M, dev, "M")
    sp = _ibp_buf("crown_bwd", "sp", sp, M * CROWN_STRIPS * NCLS * 2, dev)
    _, std, lo, hi = _ibp_setup({}, torch.float32, lo, hi)
    if not lo < hi:
        raise ValueError("crown_bwd: need lo < hi")
    p = native.ptr
    _C().crown_bwd(p(param), p(x), p(rec), p(relax), p(v), p(labels), p(sp), std, lo, hi, M, _s())
    return sp.view(-1, CROWN_STRIPS, NCLS, 2)


def crown_head(fcb: torch.Tensor, vb: torch.Tensor, sp: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor,
               lb: torch.Tensor | None = None, lbc: torch.Tensor | None = None, search: bool = False,
               M: int | None = None) -> torch.Tensor:
    """One launch of ``crown_head``: ``lb`` float32 [>= M, 10] = max(lb_crown, lb_ibp) from the partials of the other
    kernels, +inf at the label (``lbc``, when given: lb_crown).  ``search``: the records are bisected as
    ``ibp_search_reference`` does from this launch's ``lb``."""
    M = int(labels.numel() if M is None else M)
    dev = fcb.device
    if dev.type != "cuda" or M < 1 or M > IBP_MAX_B:
        raise ValueError(f"crown_head: needs GPU buffers and M in [1, {IBP_MAX_B}]")
    _df_vec("crown_head", "fcb", fcb, torch.float32, M * 2 * CROWN_SPEC, dev, "32 M")
    _df_vec("crown_head", "vb", vb, torch.float32, M * CROWN_SLICES * CROWN_SPEC, dev, "M * 9216")
    _df_vec("crown_head", "sp", sp, torch.float32, M * CROWN_STRIPS * NCLS * 2, dev, "140 M")
    _df_vec("crown_head", "labels", labels, torch.int32, M, dev, "M")
    _df_vec("crown_head", "rec", rec, torch.float32, 4 * M, dev, "4 M")
    lb = _ibp_buf("crown_head", "lb", lb, M * NCLS, dev)
    if lbc is not None:
        _df_vec("crown_head", "lbc", lbc, torch.float32, M * NCLS, dev, "10 M")
    p = native.ptr
    _C().crown_head(p(fcb), p(vb), p(sp), p(labels), 0 if lbc is None else p(lbc), p(lb), p(rec), bool(search), M, _s())
    return lb.view(-1, NCLS)


SQUARE_PHILOX_DOMAIN = 0x53515231  # Philox counter word 1 of square_init / square_step (csrc/include/kernels.h)
SQUARE_MAX_M = 1 << 20             # most images one square_init / square_step launch takes (kernels.h INPUT_GRAD_MAX_B)
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
    return tuple(min(max(int(math.floor(math.sqrt(p * 784.0) + 0.5)), 1), SQUARE_MAX_SIDE)
                 for p in _square_p_schedule("square_sides", p_init, queries))


def _square_p_schedule(name: str, p_init: float, queries: int) -> list:
    """The share p of the image the proposal of each query index q = 1 .. queries - 1 covers (float64): the schedule
    ``square_sides`` describes, shared with ``square_sides_l2``."""
    queries = int(queries)
    if queries < 1:
        raise ValueError(f"{name}: queries must be at least 1")
    if not 0.0 < p_init <= 1.0:
        raise ValueError(f"{name}: p_init must be in (0, 1], got {p_init}")
    out = []
    for q in range(1, queries):
        it = int(q / queries * 10000)
        div = next((d for top, d in _SQUARE_SCHEDULE if it <= top), 512)
        out.append(float(p_init) / div)
    return out


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


def _square_decide(logp, y, x_best, x_cand, state, first: bool, targeted: bool):
    """The record half of ``square_step_reference`` (and of its L2 form), before the proposal: ``(active, broken, xb,
    margin, used, done, spare)`` - the images that are not frozen, those whose best margin is now below zero, the new
    ``x_best``, and the new record's columns (``margin`` to be kept only where ``active``)."""
    M, dev = x_cand.shape[0], x_cand.device
    L = square_margin_reference(logp, y, targeted).to(dev)
    if first:
        active = accept = torch.ones(M, dtype=torch.bool, device=dev)
        margin = L
        used = torch.ones(M, dtype=torch.int32, device=dev)
        done_was = spare = torch.zeros(M, dtype=torch.int32, device=dev)
        xb = x_cand
    else:
        was = square_state_margin(state)
        done_was, spare = state[:, SQUARE_DONE], state[:, 3]
        active = done_was == 0
        accept = active & (L < was)
        margin = torch.where(accept, L, was)
        used = state[:, SQUARE_QUERIES] + active.to(torch.int32)
        xb = torch.where(accept[:, None], x_cand, x_best.detach().reshape(M, 784).to(torch.float32))
    broken = margin < 0
    done = torch.where(active, broken.to(torch.int32), done_was)
    return active, broken, xb, margin, used, done, spare


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
    if not first:
        state = state.reshape(M, 4).to(torch.int32)
    active, broken, xb, margin, used, done, spare = _square_decide(logp, y, x_best, x_cand, state, first, targeted)
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


SQUARE_L2_PHILOX_DOMAIN = 0x53514C32   # Philox counter word 1 of square_l2_init / square_l2_step (kernels.h)
SQUARE_L2_SIDES = tuple(range(3, SQUARE_MAX_SIDE + 1, 2))   # the odd window sides of the L2 attack
SQUARE_L2_INIT_SIDE = 5                 # the tiles of the start: 5 x 5 of them on rows and columns 1 .. 25
SQUARE_NORMS = ("linf", "l2")
_SQUARE_L2_TABLES: dict = {}


def square_norm(name: str, norm: str) -> bool:
    """True for "l2", False for "linf"; any other ``norm`` is a ValueError under ``name``."""
    if norm not in SQUARE_NORMS:
        raise ValueError(f"{name}: norm must be one of {SQUARE_NORMS}, got {norm!r}")
    return norm == "l2"


def square_l2_pattern(s: int) -> torch.Tensor:
    """float32 [s, s]: the pattern E_s an L2 Square Attack proposal adds to its window (the authors'
    ``meta_pseudo_gaussian_pert(s)``), s odd >= 3, built in float64 and rounded once.  rect(h, w): zeros [h, w] with
    1 / (k + 1)^2 added to the centred block of (2k + 1)^2 pixels clipped to the array, k = 0 .. max(h // 2, w // 2),
    divided by its L2 norm; E_s[: s // 2] = rect(s // 2, s), E_s[s // 2 :] = -rect(s - s // 2, s), divided by its L2
    norm: unit norm, the upper half positive, the lower half negative."""
    import numpy as np
    s = int(s)
    if s < 3 or s % 2 == 0:
        raise ValueError(f"square_l2_pattern: the side must be odd and at least 3, got {s}")

    def rect(h, w):
        out = np.zeros((h, w), dtype=np.float64)
        r0, c0 = h // 2, w // 2
        for k in range(max(h // 2, w // 2) + 1):
            out[max(r0, 0):min(r0 + 2 * k + 1, h), max(c0, 0):min(c0 + 2 * k + 1, w)] += 1.0 / (k + 1) ** 2
            r0, c0 = r0 - 1, c0 - 1
        return out / np.sqrt((out ** 2).sum())
    e = np.concatenate((rect(s // 2, s), -rect(s - s // 2, s)), axis=0)
    return torch.from_numpy((e / np.sqrt((e ** 2).sum())).astype(np.float32))


def square_sides_l2(p_init: float, queries: int) -> tuple:
    """``square_sides`` for the L2 attack: the same schedule of the share p, then in float64 s = max(floor(sqrt(p *
    784) + 0.5), 3), + 1 when even, min(s, 27): odd sides in [3, 27]."""
    import math
    out = []
    for p in _square_p_schedule("square_sides_l2", p_init, queries):
        s = max(int(math.floor(math.sqrt(p * 784.0) + 0.5)), 3)
        out.append(min(s + 1 if s % 2 == 0 else s, SQUARE_MAX_SIDE))
    return tuple(out)


def square_l2_table_offset(s: int) -> int:
    """The first element of E_s in ``square_l2_tables``: the tables of the odd sides 3 .. 27 lie one after another."""
    s = int(s)
    if s not in SQUARE_L2_SIDES:
        raise ValueError(f"square_l2: side must be odd and in [3, {SQUARE_MAX_SIDE}], got {s}")
    return sum(t * t for t in SQUARE_L2_SIDES if t < s)


def square_l2_tables(device) -> torch.Tensor:
    """float32 [3654]: ``square_l2_pattern(s)`` of every odd s = 3 .. 27, row-major, E_s at
    ``square_l2_table_offset(s)``, on ``device``; built once per device and kept."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    tab = _SQUARE_L2_TABLES.get(device)
    if tab is None:
        tab = torch.cat([square_l2_pattern(s).reshape(-1) for s in SQUARE_L2_SIDES]).to(device)
        _SQUARE_L2_TABLES[device] = tab
    return tab


def _square_l2_table_ptr(name: str, tables: torch.Tensor | None, s: int, device) -> int:
    """The address of E_s inside ``tables`` (default ``square_l2_tables(device)``)."""
    off = square_l2_table_offset(s)
    if tables is None:
        tables = square_l2_tables(device)
    elif tables.dtype != torch.float32 or not tables.is_contiguous() or tables.device != device or \
            tables.numel() < square_l2_table_offset(SQUARE_MAX_SIDE) + SQUARE_MAX_SIDE ** 2:
        raise ValueError(f"{name}: tables must be square_l2_tables() of the images' device")
    return native.ptr(tables) + 4 * off


def _square_l2_pattern_rows(rows: torch.Tensor, cols: torch.Tensor, s: int, plus: torch.Tensor, swap: torch.Tensor,
                            dev) -> torch.Tensor:
    """float32 [..., 28, 28]: +-E_s (``plus``), transposed where ``swap``, laid with its corner at (rows, cols) - all
    four of one leading shape; the values outside the window are those of the nearest window pixel (masked by the
    caller)."""
    E = square_l2_pattern(s).to(dev)
    at = torch.arange(28, device=dev)
    rr = (at - rows[..., None]).clamp(0, s - 1)[..., :, None]
    cc = (at - cols[..., None]).clamp(0, s - 1)[..., None, :]
    pat = torch.where(swap[..., None, None], E[cc, rr], E[rr, cc])
    return torch.where(plus[..., None, None], pat, -pat)


def _square_window(row0: torch.Tensor, col0: torch.Tensor, s: int, dev) -> torch.Tensor:
    """bool [M, 784]: the s x s window with its corner at (row0, col0) of each image."""
    at = torch.arange(28, device=dev)
    rows = (at[None, :] >= row0[:, None]) & (at[None, :] < row0[:, None] + s)
    cols = (at[None, :] >= col0[:, None]) & (at[None, :] < col0[:, None] + s)
    return (rows[:, :, None] & cols[:, None, :]).reshape(-1, 784)


def square_l2_init_reference(x0: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, ids=None,
                             id_base: int = 0) -> torch.Tensor:
    """``square_l2_init`` in torch float32 on any device: the candidate of query 0 of the L2 attack.  The 25 tiles of
    side 5 at rows 1 + 5 tr and columns 1 + 5 tc hold +E_5 where bit t = 5 tr + tc of word 0 of ``philox4x32(counter
    = (0, SQUARE_L2_PHILOX_DOMAIN, id_i, 0), key = seed)`` is set, else -E_5, transposed where bit t of word 1 is;
    the border holds 0; x_cand = clamp(x0 + e * (eps / 5)).  Every tile has unit norm, so the perturbation has norm
    eps before the clamp.  The same bits as the kernel: there is no sum."""
    import numpy as np
    from .philox import philox4x32
    M, dev = x0.shape[0], x0.device
    x0 = x0.detach().reshape(M, 784).to(torch.float32)
    ids = _square_ids("square_l2_init_reference", ids, id_base, M)
    w = philox4x32(0, SQUARE_L2_PHILOX_DOMAIN, ids, 0, seed)                                     # [M, 4]
    t = np.arange(25, dtype=np.uint32)
    plus = torch.from_numpy(((w[:, 0:1] >> t) & 1).astype(np.bool_)).to(dev).view(M, 5, 5)
    swap = torch.from_numpy(((w[:, 1:2] >> t) & 1).astype(np.bool_)).to(dev).view(M, 5, 5)
    E = square_l2_pattern(SQUARE_L2_INIT_SIDE).to(dev)
    tiles = torch.where(swap[..., None, None], E.t(), E)                                        # [M, 5, 5, 5, 5]
    tiles = torch.where(plus[..., None, None], tiles, -tiles)
    e = torch.zeros(M, 28, 28, dtype=torch.float32, device=dev)
    e[:, 1:26, 1:26] = tiles.permute(0, 1, 3, 2, 4).reshape(M, 25, 25)
    g = torch.tensor(float(np.float32(eps)), dtype=torch.float32, device=dev) / 5.0
    return (x0 + e.reshape(M, 784) * g).clamp(float(np.float32(lo)), float(np.float32(hi)))


def square_l2_step_reference(logp: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x_best: torch.Tensor | None,
                             x_cand: torch.Tensor, state: torch.Tensor | None, eps: float, lo: float, hi: float,
                             seed: int = 0, q: int = 1, side: int = 3, ids=None, id_base: int = 0,
                             first: bool = False, last: bool = False, targeted: bool = False):
    """``square_l2_step`` in torch float32 on any device (the CPU / fp32 path of ``Predictor.square_attack(norm=
    "l2")``): ``square_step_reference``'s operands, record rules and return, with the L2 proposal for a live image
    that is not done on a round that is not the last.  With d = x_best - x0 (x_best the point just accepted or kept),
    wa / wb = philox4x32(counter = (q, SQUARE_L2_PHILOX_DOMAIN, id_i, 0 / 1), key = seed), W1 the ``side`` x ``side``
    window at ((wa0 * (29 - side)) >> 32, (wa1 * (29 - side)) >> 32), W2 the one wb gives the same way, +E_side when
    wa2 & 1 else -E_side, transposed when wa2 & 2:

        S1, SU, SI = sum of d^2 over W1, over W1 u W2, over the image
        n  = +-E[.] + d / (1e-10 + sqrt(S1)) on W1;  SN = sum_W1 n^2
        d' = n * (sqrt(max(eps^2 - SI, 0) + SU) / sqrt(SN)) on W1, 0 on W2 \\ W1, d elsewhere;  SD = sum d'^2
        x_cand = clamp(x0 + d' / sqrt(SD) * eps);  SN == 0 or SD == 0: x_cand = x_best

    The kernel's formulas operation by operation; the sums are torch's, in torch's order: the same decisions and
    record, ``x_cand`` up to the rounding of five sums."""
    import numpy as np
    from .philox import philox4x32
    side, q = int(side), int(q)
    square_l2_table_offset(side)
    if not 0 <= q < 1 << 32:
        raise ValueError("square_l2_step_reference: q must fit 32 bits")
    M = x_cand.shape[0]
    dev = x_cand.device
    x0 = x0.detach().reshape(M, 784).to(torch.float32)
    x_cand = x_cand.detach().reshape(M, 784).to(torch.float32)
    ids = _square_ids("square_l2_step_reference", ids, id_base, M)
    if not first:
        state = state.reshape(M, 4).to(torch.int32)
    active, broken, xb, margin, used, done, spare = _square_decide(logp, y, x_best, x_cand, state, first, targeted)
    xc = x_cand
    if not last:
        wa = philox4x32(q, SQUARE_L2_PHILOX_DOMAIN, ids, 0, seed).astype(np.uint64)              # [M, 4]
        wb = philox4x32(q, SQUARE_L2_PHILOX_DOMAIN, ids, 1, seed).astype(np.uint64)
        span = np.uint64(29 - side)
        row1, col1, row2, col2 = (torch.from_numpy(((w * span) >> np.uint64(32)).astype(np.int64)).to(dev)
                                  for w in (wa[:, 0], wa[:, 1], wb[:, 0], wb[:, 1]))
        plus = torch.from_numpy((wa[:, 2] & np.uint64(1)).astype(np.bool_)).to(dev)
        swap = torch.from_numpy((wa[:, 2] & np.uint64(2)).astype(np.bool_)).to(dev)
        w1, w2 = _square_window(row1, col1, side, dev), _square_window(row2, col2, side, dev)
        e = torch.tensor(float(np.float32(eps)), dtype=torch.float32, device=dev)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        d = xb - x0
        qd = d * d
        S1, SU, SI = torch.where(w1, qd, zero).sum(1), torch.where(w1 | w2, qd, zero).sum(1), qd.sum(1)
        b = 1e-10 + S1.sqrt()
        n = _square_l2_pattern_rows(row1, col1, side, plus, swap, dev).reshape(M, 784) + d / b[:, None]
        SN = torch.where(w1, n * n, zero).sum(1)
        h = e * e - SI
        h = torch.where(h < 0, zero, h)                                                          # (a NaN passes)
        f = (h + SU).sqrt() / SN.sqrt()
        dn = torch.where(w1, n * f[:, None], torch.where(w2, zero, d))
        SD = (dn * dn).sum(1)
        prop = (x0 + (dn / SD.sqrt()[:, None]) * e).clamp(float(np.float32(lo)), float(np.float32(hi)))
        prop = torch.where(((SN == 0) | (SD == 0))[:, None], xb, prop)
        xc = torch.where((active & ~broken)[:, None], prop, torch.where(active[:, None], xb, x_cand))
    margin_bits = torch.where(active, margin, square_state_margin(state) if not first else margin)
    new = torch.stack((margin_bits.contiguous().view(torch.int32), used, done, spare), dim=1)
    return xb, xc, new


def square_l2_init(x0: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, id_base: int = 0,
                   out: torch.Tensor | None = None, M: int | None = None,
                   tables: torch.Tensor | None = None) -> torch.Tensor:
    """The start of an L2 Square Attack (``csrc/kernels/square.hip``), one launch: ``out[i]`` = the tiled point of
    ``square_l2_init_reference`` for the M images ``x0``, in ``square_init``'s conventions.  ``tables``:
    ``square_l2_tables`` of the device (looked up when None).  Bit for bit the reference."""
    if x0.dim() != 2 or x0.device.type != "cuda":
        raise ValueError("square_l2_init: x0 must be a float32 [M, 784] tensor on the GPU")
    M = int(x0.shape[0] if M is None else M)
    _square_common("square_l2_init", eps, lo, hi, int(id_base), M)
    _f32_rows("square_l2_init", "x0", x0, M, x0.device, at_least="M")
    out = _out_rows("square_l2_init", "out", out, M, x0.device, at_least="M")
    if out.data_ptr() == x0.data_ptr():
        raise ValueError("square_l2_init: x0 and out must be two buffers")
    tab = _square_l2_table_ptr("square_l2_init", tables, SQUARE_L2_INIT_SIDE, x0.device)
    _C().square_l2_init(native.ptr(x0), native.ptr(out), tab, float(eps), float(lo), float(hi),
                        int(seed) & (2 ** 64 - 1), int(id_base), M, _s())
    return out


def square_l2_step(logp: torch.Tensor, y: torch.Tensor, x0: torch.Tensor, x_best: torch.Tensor, x_cand: torch.Tensor,
                   state: torch.Tensor, eps: float, lo: float, hi: float, seed: int = 0, q: int = 1, side: int = 3,
                   id_base: int = 0, first: bool = False, last: bool = False, targeted: bool = False,
                   M: int | None = None, tables: torch.Tensor | None = None) -> None:
    """One L2 Square Attack query per image (``csrc/kernels/square.hip``), one launch, in place: ``square_step``'s
    operands and rules with the proposal of ``square_l2_step_reference``.  ``side``: odd, in [3, 27]; ``tables``:
    ``square_l2_tables`` of the device (looked up when None).  The record, ``x_best`` and the decisions are bit for
    bit the reference's; ``x_cand`` up to the order of its five sums."""
    if x_cand.dim() != 2 or x_cand.device.type != "cuda":
        raise ValueError("square_l2_step: x_cand must be a float32 [M, 784] tensor on the GPU")
    dev = x_cand.device
    M = int(x_cand.shape[0] if M is None else M)
    _square_common("square_l2_step", eps, lo, hi, int(id_base), M)
    rows = (("x0", x0), ("x_best", x_best), ("x_cand", x_cand))
    for what, t in rows:
        _f32_rows("square_l2_step", what, t, M, dev, at_least="M")
    _df_vec("square_l2_step", "logp", logp, torch.float32, NCLS * M, dev, "10 M")
    _df_vec("square_l2_step", "y", y, torch.int32, M, dev, "M")
    _df_vec("square_l2_step", "state", state, torch.int32, 4 * M, dev, "4 M")
    if len({t.data_ptr() for _, t in rows}) != len(rows):
        raise ValueError("square_l2_step: x0, x_best and x_cand must be three buffers")
    tab = _square_l2_table_ptr("square_l2_step", tables, side, dev)
    if not 0 <= int(q) < 1 << 32:
        raise ValueError("square_l2_step: q must fit 32 bits")
    p = native.ptr
    _C().square_l2_step(p(logp), p(y), p(x0), p(x_best), p(x_cand), p(state), tab, float(eps), float(lo), float(hi),
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
