"""Square Attack (Andriushchenko, Croce, Flammarion, Hein, ECCV 2020: the score-based black-box attack of
AutoAttack), L-inf, on the fused MI355X kernels: the native loop behind ``Predictor.square_attack``.

The attack reads nothing but the log-probabilities of its candidates: no gradient, so a net whose gradients are
masked gets no credit for it.  One query is four launches on the current stream, with no autograd, no allocation and
no host sync:

    trunk_fwd (eval form, xin = the candidates) -> fc1_fwd -> head_eval         ``ops.chain.EvalChain``
    -> square_step (csrc/kernels/square.hip: the margin of the candidate, accept or reject, freeze a broken image,
       draw the next square from Philox, write the next candidate)

preceded once by ``square_init`` (the stripe start, query 0).  ``queries`` queries are ``queries`` rounds: round 0 has
``first``, round ``queries - 1`` has ``last``; round j writes the proposal of query index j + 1 with the side
``functional.square_sides`` gives it.
"""
from __future__ import annotations

import torch

from . import native
from .chain import EvalChain
from .functional import SQUARE_DONE, SQUARE_QUERIES, EvalBuffers, square_sides, square_state_margin
from .fused_net import fused_state


def _buffers(st, rows: int, dev) -> EvalBuffers:
    """The activation set of the loop with the candidate rows ``x`` on it, kept on the net's fused state and reused
    while it is large enough (as ``ops.smooth`` keeps ``smooth_buf``)."""
    buf = getattr(st, "square_buf", None)
    if buf is None or buf.rows < rows or buf.x.device != dev:
        buf = st.square_buf = EvalBuffers.allocate(rows, dev)
        buf.x = torch.zeros(rows, 784, dtype=torch.float32, device=dev)
    return buf


def square_runs(ids) -> list:
    """The launch plan of ``fused_square_attack``: tuples (i0, m) - images [i0, i0 + m) with consecutive ``ids``,
    one ``id_base`` per launch."""
    runs, i, B = [], 0, len(ids)
    while i < B:
        m = 1
        while i + m < B and ids[i + m] == ids[i] + m:
            m += 1
        runs.append((i, m))
        i += m
    return runs


def fused_square_attack(net, x0: torch.Tensor, labels: torch.Tensor, eps: float, queries: int, lo: float, hi: float,
                        p_init: float = 0.8, seed: int = 0, ids=None, targeted: bool = False, check_every: int = 64):
    """``(x_best, margin_best, queries_used)``: the L-inf Square Attack with at most ``queries`` queries per image on
    the margin of ``labels`` (untargeted lp[y] - max_{j != y} lp[j]; ``targeted``: ``labels`` are the classes to reach
    and the negative is used; < 0: broken), in inference semantics (no dropout), inside the ``eps`` box around ``x0``
    and the range [lo, hi] (``functional.square_step_reference`` has the exact form).

    ``x0``: float32 [B, 784] normalised images on the net's device; ``labels``: [B] integers in [0, 10) (not checked
    here: ``Predictor.square_attack`` does); ``eps``, ``lo``, ``hi`` in normalised units.  Image j draws under the id
    ``ids[j]`` (default j) from the Philox stream keyed by ``seed``: its squares depend on (seed, id, query index)
    alone, not on B.  Returns the float32 [B, 784] point of the lowest margin among the candidates queried, float32
    [B] that margin as ``head_eval``'s log-probabilities gave it, and int32 [B] the queries made until the image broke
    (``queries`` when it did not).  An image that is broken is frozen: none of its later candidates is looked at.

    Images with consecutive ids run together (``square_runs``).  ``check_every`` = k > 0 reads a run's ``done`` flags
    on the host after every k queries and ends the run once every image is broken; 0 never syncs; the result does
    not depend on it by a bit.  The candidate rows and the activation set stay on the net's fused state, the call
    allocates the results; the net's mode, parameters and ``.grad`` are untouched."""
    queries, check_every = int(queries), int(check_every)
    if queries < 1 or queries >= 1 << 32:
        raise ValueError("fused_square_attack: queries must be in [1, 2**32)")
    if check_every < 0:
        raise ValueError(f"fused_square_attack: check_every must be >= 0, got {check_every}")
    sides = square_sides(p_init, queries)
    st = fused_state(net)
    st.sync()                                   # once: the bf16 shadows follow the parameters
    dev = st.ms.device
    if x0.dim() != 2 or x0.shape[1] != 784 or x0.dtype != torch.float32 or x0.device != dev:
        raise ValueError("fused_square_attack: x0 must be float32 [B, 784] on the net's device")
    B = x0.shape[0]
    if B < 1:
        raise ValueError("fused_square_attack: B must be positive")
    if labels.numel() != B:
        raise ValueError(f"fused_square_attack: {labels.numel()} labels for {B} images")
    ids = list(range(B)) if ids is None else [int(v) for v in ids]
    if len(ids) != B:
        raise ValueError(f"fused_square_attack: {len(ids)} ids for {B} images")
    x0 = x0.contiguous()
    lab = labels.reshape(B).to(dev, torch.int32).contiguous()
    runs = square_runs(ids)
    mc = max(m for _, m in runs)
    # every element of these is written by round 0 before it is read
    x_best = torch.empty(B, 784, dtype=torch.float32, device=dev)
    state = torch.empty(B, 4, dtype=torch.int32, device=dev)
    seen = torch.empty(mc, dtype=torch.int32, pin_memory=True) if check_every else None
    buf = _buffers(st, mc, dev)
    chain = EvalChain(st.ms, buf)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px0, pbest, pcand, plab, pstate, plogp = p(x0), p(x_best), p(buf.x), p(lab), p(state), p(buf.logp)
    seed = int(seed) & (2 ** 64 - 1)
    run, step = chain.run, C.square_step
    for i0, m in runs:
        o784, o4, o16, idb = 3136 * i0, 4 * i0, 16 * i0, ids[i0]
        C.square_init(px0 + o784, pcand, eps, lo, hi, seed, idb, m, s)
        for j in range(queries):
            last = j == queries - 1
            run(m, xin=pcand)
            step(plogp, plab + o4, px0 + o784, pbest + o784, pcand, pstate + o16, eps, lo, hi, seed, j + 1, idb,
                 1 if last else sides[j], j == 0, last, targeted, m, s)
            if check_every and (j + 1) % check_every == 0 and not last:
                seen[:m].copy_(state[i0:i0 + m, SQUARE_DONE])             # the one host sync: every image frozen?
                if bool((seen[:m] != 0).all()):
                    break
    return x_best, square_state_margin(state), state[:, SQUARE_QUERIES].clone()
