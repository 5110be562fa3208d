"""Host-side references shared by the randomized-smoothing tests (CPU and GPU): the numpy emulation of the
``smooth_noise`` and ``smooth_vote`` kernels (csrc/kernels/smooth.hip) on ``refmodel.philox4x32``, in float32
(every operation rounded on its own, as the kernel) and in float64 (the oracle), with the single mutations the
comparators must catch."""
import numpy as np

import refmodel as R

SMOOTH_PHILOX_DOMAIN = 0x534D5431       # csrc/include/kernels.h
ADV_PHILOX_DOMAIN = 0x41445631
F32, F64 = np.float32, np.float64
TWO_PI32 = F32(6.28318530717958647692)
NO_MUTATION = frozenset()


def smooth_counters(M: int, n: int, sample_base: int = 0, id_base: int = 0, swap: bool = False):
    """The four Philox counter words, uint64 arrays [M * n * 196], of row r = i * n + s, float4 v:
    (sample_base + s, DOMAIN, id_base + i, v).  ``swap`` (mutation 1): sample index and image id exchanged."""
    i, s, v = np.meshgrid(np.arange(M, dtype=np.uint64), np.arange(n, dtype=np.uint64),
                          np.arange(196, dtype=np.uint64), indexing="ij")
    c0 = (np.uint64(sample_base) + s).ravel()
    c2 = (np.uint64(id_base) + i).ravel()
    if swap:
        c0, c2 = c2, c0
    return c0, np.full_like(c0, SMOOTH_PHILOX_DOMAIN), c2, v.ravel()


def smooth_words(M: int, n: int, seed: int, sample_base: int = 0, id_base: int = 0, swap: bool = False):
    """uint32 [M * n, 196, 4]: the Philox words of every float4 of every row."""
    ctr = smooth_counters(M, n, sample_base, id_base, swap)
    w = R.philox4x32(ctr, (seed & R.MASK, (seed >> 32) & R.MASK))
    w = np.stack([np.asarray(x, dtype=np.uint64) & np.uint64(R.MASK) for x in w], axis=1)
    return w.astype(np.uint32).reshape(M * n, 196, 4)


def box_muller(words: np.ndarray, dtype=F64, mut=NO_MUTATION) -> np.ndarray:
    """z [rows, 784] from the words [rows, 196, 4]: (w0, w1) -> elements 4v, 4v + 1 (cos, sin), (w2, w3) ->
    4v + 2, 4v + 3.  float32: every operation rounded on its own, numpy's float32 log / sqrt / cos / sin;
    float64: the same u1, u2 (exact in either format), everything after them in float64 with the exact 2 pi.
    Mutations: "u1" (2: no + 1), "sincos" (3: sin and cos swapped)."""
    wa = words[:, :, 0::2].astype(np.int64) >> 8                     # [rows, 196, 2]: w0, w2
    wb = words[:, :, 1::2].astype(np.int64) >> 8                     #                 w1, w3
    u1 = ((wa if "u1" in mut else wa + 1).astype(dtype)) * dtype(2.0 ** -24)
    u2 = wb.astype(dtype) * dtype(2.0 ** -24)
    with np.errstate(divide="ignore"):
        r = np.sqrt(dtype(-2.0) * np.log(u1))
    t = (TWO_PI32 if dtype is F32 else F64(2.0 * np.pi)) * u2
    c, s = np.cos(t), np.sin(t)
    if "sincos" in mut:
        c, s = s, c
    z = np.stack([r * c, r * s], axis=3)                             # [rows, 196, 2 pairs, (cos, sin)]
    assert z.dtype == dtype
    return z.reshape(words.shape[0], 784)


def noise_emulation(x0: np.ndarray, sigma: float, n: int, seed: int, sample_base: int = 0, id_base: int = 0,
                    dtype=F64, mut=NO_MUTATION) -> np.ndarray:
    """``smooth_noise``: out[i * n + s] = x0[i] + sigma * z, [M * n, 784] in ``dtype``; x0 float32 [M, 784] (the
    normalised rows), sigma the float32 value the kernel gets.  Mutations as ``box_muller``, "swap" (1) and
    "sigma2" (4: sigma applied twice)."""
    M = x0.shape[0]
    z = box_muller(smooth_words(M, n, seed, sample_base, id_base, "swap" in mut), dtype, mut)
    sg = dtype(F32(sigma))
    if "sigma2" in mut:
        z = sg * z
    out = np.repeat(x0.astype(dtype), n, axis=0) + sg * z
    assert out.dtype == dtype
    return out


def noise_eps(out32: np.ndarray, out64: np.ndarray) -> float:
    """The project's tolerance rule for an fp32 stage: 8 x max |numpy fp32 emulation - float64 oracle| on the same
    operands, not below 4 fp32 ulps of the largest output."""
    _, e = np.frexp(np.abs(out64).max())
    return max(8.0 * float(np.abs(out32.astype(F64) - out64).max()), 4.0 * 2.0 ** (int(e) - 24))


def vote_reference(logp: np.ndarray, M: int, n: int, counts=None, accumulate: bool = False,
                   mut=NO_MUTATION) -> np.ndarray:
    """``smooth_vote``: int32 [M, 10] - each of the n rows of image i votes for its first maximum, a row holding a
    NaN for nothing; ``accumulate`` adds to ``counts``.  Mutations: "last" (5: the last maximum wins), "nan0" (6:
    NaN rows vote for class 0), "overwrite" (7: accumulate overwrites)."""
    lp = np.asarray(logp, dtype=F32)[:M * n].reshape(M, n, 10)
    nan = np.isnan(lp).any(axis=2)
    safe = np.where(np.isnan(lp), -np.inf, lp)
    if "last" in mut:
        arg = 9 - np.argmax(safe[:, :, ::-1], axis=2)
    else:
        arg = np.argmax(safe, axis=2)
    out = np.zeros((M, 10), dtype=np.int32)
    for i in range(M):
        votes = arg[i] if "nan0" in mut else arg[i][~nan[i]]
        if "nan0" in mut:
            votes = np.where(nan[i], 0, votes)
        out[i] = np.bincount(votes, minlength=10).astype(np.int32)
    if accumulate and "overwrite" not in mut:
        out = out + np.asarray(counts, dtype=np.int32)[:M]
    return out


def hand_logp(M: int, n: int, seed: int = 0) -> np.ndarray:
    """float32 [M * n, 10] hand-made log-probabilities on a coarse grid (many exact ties), with rows of all-equal
    values, rows holding a NaN (alone, and next to the maximum), +inf and -inf entries, and an all -inf row."""
    g = np.random.default_rng(seed)
    lp = (g.integers(-6, 0, size=(M * n, 10)) * 0.5).astype(F32)
    rows = M * n
    for k, r in enumerate(range(0, rows, 7)):
        kind = k % 6
        if kind == 0:
            lp[r] = -1.0                                    # ten-way tie: class 0
        elif kind == 1:
            lp[r, g.integers(0, 10)] = np.nan
        elif kind == 2:
            lp[r, 3] = np.inf
            lp[r, 8] = np.inf                               # tie of +inf: class 3
        elif kind == 3:
            lp[r] = -np.inf                                 # all -inf: class 0
        elif kind == 4:
            lp[r, 0] = np.nan
            lp[r, 9] = np.inf
        else:
            lp[r, :9] = -np.inf                             # only class 9 finite
    return lp
