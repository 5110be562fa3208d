"""Randomized smoothing (Cohen, Rosenfeld, Kolter 2019) on the fused MI355X kernels: the native vote loop behind
``Predictor.smoothed_counts`` / ``Predictor.certify``, and the certificate itself (pure host code).

The smoothed classifier g(x) = argmax_c P(f(x + N(0, sigma^2 I)) = c) is estimated by classifying many noised
copies of x.  One chunk of rows is five launches on the current stream, with no autograd, no allocation and no
host sync:

    smooth_noise (csrc/kernels/smooth.hip: the noised fp32 rows, from the uint8 or fp32 image)
    -> the three launches of the eval chain (``ops.chain.EvalChain``, xin = those rows)
    -> smooth_vote (accumulate: the per-image class counts)

The certificate: with cA the class most voted among ``n0`` selection samples and k its count among ``n``
disjoint estimation samples, p_L = the one-sided Clopper-Pearson lower bound of level 1 - alpha on its vote
share; if p_L > 1/2 the smoothed classifier returns cA within the L2 radius sigma * Phi^-1(p_L) of x with
probability >= 1 - alpha, otherwise the procedure abstains.
"""
from __future__ import annotations

import functools
import math
from statistics import NormalDist

import torch

from . import native
from .chain import EvalChain
from .functional import NCLS, SMOOTH_MAX_ROWS, EvalBuffers

ABSTAIN = -1


# ---------------------------------------------------------------------------- the certificate (host, float64)
def _log_binom_pmf(j: int, n: int, p: float) -> float:
    return (math.lgamma(n + 1) - math.lgamma(j + 1) - math.lgamma(n - j + 1)
            + j * math.log(p) + (n - j) * math.log1p(-p))


def _binom_sf(k: int, n: int, p: float) -> float:
    """P(X >= k) for X ~ Binomial(n, p), 1 <= k <= n, 0 < p < 1, in float64: the terms of the side that does
    not hold the mode are summed away from k (the first from ``math.lgamma``, the next ones by the ratio of
    neighbouring terms), stopping once they no longer count."""
    mode = min(max(int((n + 1) * p), 0), n)
    upper = k > mode                         # sum the tail that does not hold the mode: it is the small one
    lo, hi = (k, n) if upper else (0, k - 1)
    start = lo if upper else hi              # its largest term sits next to k
    ref = _log_binom_pmf(start, n, p)
    odds = p / (1.0 - p)
    total, t, j = 0.0, 1.0, start           # t = pmf(j) / pmf(start), by the ratio of neighbouring terms
    while True:
        total += t
        if upper:
            if j == hi:
                break
            t *= (n - j) / (j + 1.0) * odds
            j += 1
        else:
            if j == lo:
                break
            t *= j / (n - j + 1.0) / odds
            j -= 1
        if t < 1e-18 * total:
            break
    tail = math.exp(ref) * total
    return tail if upper else 1.0 - tail


@functools.lru_cache(maxsize=1 << 16)
def lower_confidence_bound(k: int, n: int, alpha: float) -> float:
    """The one-sided Clopper-Pearson lower bound of level 1 - alpha for a binomial proportion with ``k``
    successes in ``n`` trials: the ``alpha`` quantile of Beta(k, n - k + 1), i.e. the p at which
    P(Binomial(n, p) >= k) = alpha.  0 for k = 0; alpha^(1/n) exactly for k = n (< 1 for alpha > 0, so 1 cannot
    occur).  Bisection on the binomial tail (monotone in p), no dependency beyond ``math``."""
    if not 0 <= k <= n or n < 1:
        raise ValueError(f"lower_confidence_bound: need 0 <= k <= n and n >= 1, got k={k}, n={n}")
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"lower_confidence_bound: alpha must be in (0, 1), got {alpha}")
    if k == 0:
        return 0.0
    if k == n:
        return alpha ** (1.0 / n)
    lo, hi = 0.0, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _binom_sf(k, n, mid) < alpha:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def certify_from_counts(counts0, counts, sigma: float, alpha: float):
    """(class, radius) of one image from its selection counts ``counts0`` and its estimation counts ``counts``
    (ten integers each, from disjoint samples): cA = argmax ``counts0`` (first maximum), k = ``counts[cA]``,
    n = sum of ``counts``, p_L = ``lower_confidence_bound(k, n, alpha)``; (cA, sigma * Phi^-1(p_L)) when
    p_L > 1/2, else (``ABSTAIN`` = -1, 0.0).  The radius is in the units of ``sigma``.  Host code, float64."""
    c0 = [int(v) for v in counts0]
    c = [int(v) for v in counts]
    if len(c0) != NCLS or len(c) != NCLS:
        raise ValueError("certify_from_counts: ten counts each")
    cA = max(range(NCLS), key=lambda j: (c0[j], -j))
    n = sum(c)
    if n < 1:
        return ABSTAIN, 0.0
    p_l = lower_confidence_bound(c[cA], n, alpha)
    if not p_l > 0.5:
        return ABSTAIN, 0.0
    return cA, float(sigma) * NormalDist().inv_cdf(p_l)


# ---------------------------------------------------------------------------- the native loop
def smooth_chunks(B: int, n: int, ids, rows_per_launch: int):
    """The launch plan of ``fused_smooth_counts``: tuples (i0, m, s0, ns) - images [i0, i0 + m) with samples
    [s0, s0 + ns) each, m * ns <= ``rows_per_launch`` rows.  It chunks over images (whole images, each run with
    consecutive ``ids``: one ``id_base`` per launch) and, when n > ``rows_per_launch``, over samples."""
    if not 1 <= rows_per_launch <= SMOOTH_MAX_ROWS:
        raise ValueError(f"rows_per_launch must be in [1, SMOOTH_MAX_ROWS = {SMOOTH_MAX_ROWS}]")
    plan = []
    if n > rows_per_launch:
        for i in range(B):
            for s0 in range(0, n, rows_per_launch):
                plan.append((i, 1, s0, min(rows_per_launch, n - s0)))
        return plan
    per = max(1, rows_per_launch // n)
    i = 0
    while i < B:
        m = 1
        while m < per and i + m < B and ids[i + m] == ids[i] + m:
            m += 1
        plan.append((i, m, 0, n))
        i += m
    return plan


def _buffers(st, rows: int, dev) -> EvalBuffers:
    """The activation set of the loop with the row buffer ``x`` on it, kept on the net's fused state and reused
    while it is large enough."""
    buf = getattr(st, "smooth_buf", None)
    if buf is None or buf.rows < rows or buf.x.device != dev:
        buf = st.smooth_buf = EvalBuffers.allocate(rows, dev)
        buf.x = torch.zeros(rows, 784, dtype=torch.float32, device=dev)
    return buf


def fused_smooth_counts(net, x: torch.Tensor, sigma_n: float, n: int, seed: int = 0, ids=None,
                        sample_base: int = 0, rows_per_launch: int = 8192) -> torch.Tensor:
    """int32 [B, 10] class counts of ``n`` Gaussian-noised copies of each image, in inference semantics.

    ``x``: uint8 [B, 784] raw rows or float32 [B, 784] normalised rows on the net's device; ``sigma_n`` >= 0 in
    normalised units; image j draws samples [``sample_base``, ``sample_base`` + n) under id ``ids[j]`` (default
    j): its noised rows depend on (seed, id, sample range, sigma, image) alone, bit for bit, not on B or
    ``rows_per_launch``.  (Its counts follow, up to fc1_fwd's split-K, which is 32-way below 512 rows per launch
    and 4-way from there: a log-probability's last bits, hence a vote on an exact near-tie, can differ between
    launches of either kind.)
    Per chunk of ``smooth_chunks``: smooth_noise -> trunk_fwd(xin) -> fc1_fwd -> head_eval -> smooth_vote, on one
    buffer set kept on the net's fused state, with no host sync.  The net's mode, parameters and ``.grad`` are
    untouched."""
    from .fused_net import fused_state
    st = fused_state(net)
    st.sync()
    dev = st.ms.device
    if x.dim() != 2 or x.shape[1] != 784 or x.dtype not in (torch.uint8, torch.float32) or x.device != dev:
        raise ValueError("fused_smooth_counts: x must be uint8 or float32 [B, 784] on the net's device")
    B, n = x.shape[0], int(n)
    if B < 1 or n < 1:
        raise ValueError("fused_smooth_counts: B and n must be positive")
    ids = list(range(B)) if ids is None else [int(v) for v in ids]
    if len(ids) != B:
        raise ValueError(f"fused_smooth_counts: {len(ids)} ids for {B} images")
    x = x.contiguous()
    plan = smooth_chunks(B, n, ids, rows_per_launch)
    buf = _buffers(st, max(m * ns for _, m, _, ns in plan), dev)
    counts = torch.empty(B, NCLS, dtype=torch.int32, device=dev)
    chain = EvalChain(st.ms, buf)
    C, s, p = native.load(), native.stream_handle(), native.ptr
    px, plogp, pcounts = p(buf.x), p(buf.logp), p(counts)
    u8 = x.dtype == torch.uint8
    src, row_bytes = p(x), 784 * x.element_size()
    seed = int(seed) & (2 ** 64 - 1)
    run = chain.run
    for i0, m, s0, ns in plan:
        rows = m * ns
        at = src + i0 * row_bytes
        C.smooth_noise(at if u8 else 0, 0 if u8 else at, px, sigma_n, seed, sample_base + s0, ids[i0], m, ns, s)
        run(rows, xin=px)
        C.smooth_vote(plogp, pcounts + 4 * NCLS * i0, m, ns, s0 > 0, s)
    return counts
