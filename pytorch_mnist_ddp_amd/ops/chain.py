"""The launch chains the native loops behind ``Predictor`` share, every pointer bound before the first launch.

    EvalChain:  trunk_fwd (eval form) -> fc1_fwd -> head_eval                  (``Predictor._native``, ``ops.smooth``)
    GradChain:  trunk_fwd (xin, training form, STEP_FLAG_NO_DROPOUT) -> fc1_fwd
                -> head_train (labels given directly, loss scale 1.0: the summed NLL)
                   or, with a margin loss, head_margin (the summed CW / DLR / targeted DLR loss, scale 1.0)
                -> fc_bwd, role B only (the dy records; no fc weight gradient is formed)
                then input_grad, plain or step form, on those records          (``ops.attack``, ``ops.attribute``)

A chain is built once per call of its loop (``ModelState.bind`` can move the parameters between calls) and resolves
the extension, the stream and every pointer then; its ``run`` only enqueues launches on that stream: no allocation,
no host sync.  Arguments of the launching methods are raw device pointers (0 = absent).

Role B alone is enough at every batch size: it reads ``dz1`` (head_train), ``pmask`` (trunk_fwd), the ``w1t`` shadow
and the step flags, and its ceil(rows / 16) x 36 tiles write every byte of every image's 144 records (128 B of
gradients + 16 B of argmax planes each) - all that ``input_grad`` reads of ``dyc``.  Roles A and C write the fc
gradients only (above 1024 rows: their split partials), which nothing here reads.
"""
from __future__ import annotations

from collections import namedtuple

from . import native

ParamPtrs = namedtuple("ParamPtrs", "c1w c1b c2b f1b f2w f2b w2f w2d w1 w1t")
CHAIN_LOSSES = ("ce", "cw", "dlr", "dlr_t")       # GradChain(loss=...): head_train, or head_margin's three kinds


def chain_loss(name: str, loss: str, targeted: bool) -> str:
    """The ``GradChain`` loss of an attack loop's ``loss`` argument ("ce", "cw" or "dlr"; ``name``: the loop, for the
    message): the targeted form of "dlr" is the chain's "dlr_t", which takes the true labels beside the targets."""
    if loss not in ("ce", "cw", "dlr"):
        raise ValueError(f"{name}: loss must be 'ce', 'cw' or 'dlr', got {loss!r}")
    return "dlr_t" if loss == "dlr" and targeted else loss


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def param_ptrs(ms) -> ParamPtrs:
    """The device pointers, as they are now, of the float32 parameters the kernels take one by one (inside the flat
    ``ms.param``) and of the four bf16 shadows."""
    o = ms.offsets
    P = ms.param.data_ptr()
    return ParamPtrs(P + 4 * o["conv1.weight"], P + 4 * o["conv1.bias"], P + 4 * o["conv2.bias"],
                     P + 4 * o["fc1.bias"], P + 4 * o["fc2.weight"], P + 4 * o["fc2.bias"],
                     ms.w2f.data_ptr(), ms.w2d.data_ptr(), ms.w1.data_ptr(), ms.w1t.data_ptr())


def margin_operands(name: str, kind: str, lab, true_labels, B: int, dev):
    """``(labels, targets)`` as ``GradChain.run`` takes them (int32 [B] tensors on ``dev``; targets None unless
    ``kind`` is "dlr_t": then the loop's ``lab`` are the targets and ``true_labels``, required, the labels)."""
    import torch
    if kind != "dlr_t":
        return lab, None
    if true_labels is None:
        raise ValueError(f"{name}: the targeted DLR loss needs true_labels")
    if true_labels.numel() != B:
        raise ValueError(f"{name}: {true_labels.numel()} true_labels for {B} images")
    return true_labels.reshape(B).to(dev, torch.int32).contiguous(), lab


class EvalChain:
    """The eval forward of ``ms`` on the ``functional.EvalBuffers`` set ``buf``, for launches of up to ``buf.rows``."""
    __slots__ = ("_bound",)

    def __init__(self, ms, buf):
        p, w = native.ptr, param_ptrs(ms)
        self._bound = (native.load(), native.stream_handle(), w.c1w, w.c1b, w.c2b, w.f1b, w.f2w, w.f2b, w.w2f, w.w1,
                       p(buf.p), p(buf.z1part), p(buf.loss_rows), p(buf.correct), p(buf.logp))

    def run(self, rows: int, *, u8: int = 0, xin: int = 0, labels: int = 0) -> None:
        """Rows [0, ``rows``) of ``buf.logp`` (of ``loss_rows`` / ``correct`` too with int32 ``labels``) from the
        uint8 rows ``u8`` or the normalised float32 rows ``xin``."""
        C, s, c1w, c1b, c2b, f1b, f2w, f2b, w2f, w1, pp, z1part, loss_rows, correct, logp = self._bound
        C.trunk_fwd(u8, 0, 0, 0, c1w, c1b, w2f, c2b, 0, pp, 0, rows, False, s, xin=xin)
        C.fc1_fwd(pp, w1, z1part, rows, s)
        C.head_eval(z1part, f1b, f2w, f2b, labels, 0, loss_rows, correct, logp, rows, s)


class GradChain:
    """The gradient of the summed loss wrt normalised input rows, in inference semantics (no dropout), on one
    activation set of ``rows_max`` rows taken from the fused state ``st``'s pool.  ``loss``: "ce" (the NLL,
    ``head_train``) or a margin loss of ``head_margin`` - "cw", "dlr", "dlr_t" - which takes ``head_train``'s place
    in the chain, everything else the same.  The caller has run ``st.sync()``; ``st.rng_offset`` stays (nothing is
    drawn).  ``release`` gives the set back once the last launch is enqueued: the next taker is stream ordered after
    it."""
    __slots__ = ("_st", "_buf", "_state", "_bound", "_ig", "_kind")

    def __init__(self, st, rows_max: int, loss: str = "ce"):
        from .functional import FC_ROLE_B, MARGIN_KINDS
        from .fused_net import _step_state
        if loss not in CHAIN_LOSSES:
            raise ValueError(f"GradChain: loss must be one of {CHAIN_LOSSES}, got {loss!r}")
        self._kind = None if loss == "ce" else MARGIN_KINDS[loss]
        ms = st.ms
        self._st = st
        self._state = _step_state(st, False, ms.device, 1)    # zero seed and counter, STEP_FLAG_NO_DROPOUT
        self._buf = buf = st.take(rows_max, ms.device)
        p, w = native.ptr, param_ptrs(ms)
        C, s = native.load(), native.stream_handle()
        self._bound = (C, s, p(self._state), FC_ROLE_B, w.c1w, w.c1b, w.c2b, w.f1b, w.f2w, w.f2b, w.w2f, w.w1, w.w1t,
                       p(buf.a1), p(buf.p), p(buf.pmask), p(buf.z1part), p(buf.loss_rows),
                       p(buf.dz1), p(buf.h_bf), p(buf.dl_bf), p(buf.dyc), p(buf.fcpart))
        self._ig = (C, s, p(buf.dyc), p(buf.a1), w.w2d, w.c1w)      # what the two input_grad forms read

    def run(self, px: int, plab: int, rows: int, ptgt: int = 0) -> None:
        """The dy records of the float32 rows at ``px`` against the int32 labels at ``plab`` ("dlr_t": ``plab`` the true
        labels, ``ptgt`` the int32 targets)."""
        (C, s, pst, role_b, c1w, c1b, c2b, f1b, f2w, f2b, w2f, w1, w1t,
         a1, pp, pmask, z1part, loss_rows, dz1, h_bf, dl_bf, dyc, fcpart) = self._bound
        Bp = round_up(rows, 32)
        C.trunk_fwd(0, 0, 0, pst, c1w, c1b, w2f, c2b, a1, pp, pmask, rows, True, s, xin=px)
        C.fc1_fwd(pp, w1, z1part, rows, s)
        if self._kind is None:
            C.head_train(z1part, f1b, f2w, f2b, plab, 0, 0, pst, 1.0, loss_rows, dz1, h_bf, dl_bf, rows, Bp, s)
        else:
            C.head_margin(z1part, f1b, f2w, f2b, plab, ptgt, self._kind, 1.0, loss_rows, dz1, h_bf, dl_bf, rows, Bp, s)
        C.fc_bwd(dz1, pp, pmask, w1t, h_bf, dl_bf, loss_rows, pst, 0, dyc, 0, 1.0, 1.0, rows, Bp, s,
                 role=role_b, part=fcpart)

    def input_grad(self, pdx: int, rows: int) -> None:
        """After ``run``: the float32 [rows, 784] gradient to ``pdx`` (every element is written)."""
        C, s, dyc, a1, w2d, c1w = self._ig
        C.input_grad(dyc, a1, w2d, c1w, pdx, rows, s)

    def input_grad_step(self, px: int, px0: int, pout: int, alpha: float, eps: float, lo: float, hi: float,
                        rows: int) -> None:
        """After ``run``: ``functional.input_grad_step``'s projected step from ``px`` around ``px0`` to ``pout``."""
        C, s, dyc, a1, w2d, c1w = self._ig
        C.input_grad_step(dyc, a1, w2d, c1w, px, px0, pout, alpha, eps, lo, hi, rows, s)

    @property
    def loss_rows(self) -> int:
        """The device pointer of the set's ``loss_rows``: after ``run``, row r holds -log p of its label (a margin
        chain: its margin loss)."""
        return native.ptr(self._buf.loss_rows)

    def release(self) -> None:
        buf, self._buf = self._buf, None
        if buf is not None:
            self._st.give(buf)
