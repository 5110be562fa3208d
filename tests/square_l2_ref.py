"""A plain float64 numpy emulation of the L2 Square Attack kernels (csrc/kernels/square.hip, the L2 section), image
by image, on ``ops.philox``: ``pattern`` (E_s), ``init_oracle`` (square_l2_init) and ``step_oracle``
(square_l2_step).  The record, the accept decisions and ``x_best`` read nothing but fp32 margins and are exact (fp32
bits, ``square_ref.mismatches`` applies to them); ``x_cand`` is the formula in float64 on the same fp32 operands."""
import numpy as np

import square_ref as R
from pytorch_mnist_ddp_amd.ops.philox import philox4x32

F32, F64 = np.float32, np.float64
DOMAIN = 0x53514C32                                        # kernels.h SQUARE_L2_PHILOX_DOMAIN ("SQL2")
EPS = 2.0 / R.MNIST_STD


def ball_slack(eps_n: float) -> float:
    """Upper bound of ||x_adv - x0||_2 (evaluated in float64) of a point the L2 attack wrote, with u = 2^-24 and n =
    784, for ANY order of the 784-term sum SD - ``ball_slack`` of tests/test_attack_l2_cpu.py step by step:
      * t = fl(sqrt(SD_hat)), SD_hat an fp32 sum of n rounded squares: t >= ||d'|| (1 - (n / 2 + 2) u);
      * two roundings of the scale: fl(d'_i / t) and fl(. * eps), (1 + u) each; d' is the fp32 vector SD was taken of;
      * x_cand_i = fl(x0_i + .) is off by at most u max(|lo|, |hi|) per element, sqrt(n) = 28 times that in the norm;
      * the clamp moves x_cand_i towards x0_i (x0 is inside [lo, hi]): it only shrinks.
    The start has no sum: 25 unit tiles rounded to fp32, g = fl(eps / 5) and fl(e g): eps (1 + 3 u), far inside.
    Together eps_n (1 + (n / 2 + 4) u), doubled for the higher-order terms as there, + 28 u max(|lo|, |hi|)."""
    return eps_n * (1.0 + 4 * 2.0 ** -23 * (784 / 8 + 1)) + 28 * 2.0 ** -24 * max(abs(R.LO), abs(R.HI))


def _rect(h, w):
    out = np.zeros((h, w), dtype=F64)
    r0, c0 = h // 2, w // 2
    for k in range(max(h // 2, w // 2) + 1):
        out[max(r0, 0):min(r0 + 2 * k + 1, h), max(c0, 0):min(c0 + 2 * k + 1, w)] += 1.0 / (k + 1) ** 2
        r0, c0 = r0 - 1, c0 - 1
    return out / np.sqrt((out ** 2).sum())


def pattern(s: int):
    """E_s as the kernels read it: float64 arithmetic, rounded once to fp32 (returned as float64)."""
    e = np.concatenate((_rect(s // 2, s), -_rect(s - s // 2, s)), axis=0)
    return (e / np.sqrt((e ** 2).sum())).astype(F32).astype(F64)


def _clamp(t, lo, hi):
    t = np.where(t < F64(F32(lo)), F64(F32(lo)), t)
    return np.where(t > F64(F32(hi)), F64(F32(hi)), t)


def init_oracle(x0, eps, seed, ids, lo=R.LO, hi=R.HI):
    M = x0.shape[0]
    E, out = pattern(5), np.empty((M, 784), dtype=F64)
    for i in range(M):
        w = philox4x32(0, DOMAIN, int(ids[i]), 0, seed)
        e = np.zeros((28, 28), dtype=F64)
        for t in range(25):
            tr, tc = divmod(t, 5)
            tile = E.T if (int(w[1]) >> t) & 1 else E
            e[1 + 5 * tr:6 + 5 * tr, 1 + 5 * tc:6 + 5 * tc] = tile if (int(w[0]) >> t) & 1 else -tile
        out[i] = _clamp(x0[i].astype(F64) + e.reshape(784) * (F64(F32(eps)) / 5.0), lo, hi)
    return out


def _proposal(xb, x0, eps, seed, q, s, image_id, lo, hi):
    wa, wb = (philox4x32(q, DOMAIN, image_id, k, seed).astype(np.uint64) for k in (0, 1))
    span = np.uint64(29 - s)
    (r1, c1), (r2, c2) = ((int((w[0] * span) >> np.uint64(32)), int((w[1] * span) >> np.uint64(32))) for w in (wa, wb))
    E = pattern(s)
    E = E.T if int(wa[2]) & 2 else E
    E = E if int(wa[2]) & 1 else -E
    eps = F64(F32(eps))
    with np.errstate(all="ignore"):
        d = (xb.astype(F64) - x0.astype(F64)).reshape(28, 28)
        W1 = (slice(r1, r1 + s), slice(c1, c1 + s))
        W2 = (slice(r2, r2 + s), slice(c2, c2 + s))
        union = np.zeros((28, 28), dtype=bool)
        union[W1] = union[W2] = True
        S1, SU, SI = (d[W1] ** 2).sum(), (d[union] ** 2).sum(), (d ** 2).sum()
        n = E + d[W1] / (F64(F32(1e-10)) + np.sqrt(S1))
        SN = (n ** 2).sum()
        h = eps * eps - SI
        new = d.copy()
        new[W2] = 0.0
        new[W1] = n * (np.sqrt((0.0 if h < 0 else h) + SU) / np.sqrt(SN))
        SD = (new ** 2).sum()
        if SN == 0 or SD == 0:
            return xb.astype(F64)
        return _clamp(x0.astype(F64) + (new / np.sqrt(SD) * eps).reshape(784), lo, hi)


def step_oracle(case, side=3, q=1, first=False, last=False):
    """(x_best fp32, x_cand float64, state int32 [M, 4]) after one square_l2_step on ``case`` (the keys of
    ``square_ref.make_case``; nothing of it is modified)."""
    M = case["x0"].shape[0]
    xb, xc, st = case["x_best"].copy(), case["x_cand"].astype(F64), case["state"].copy()
    lo, hi = case.get("lo", R.LO), case.get("hi", R.HI)
    for i in range(M):
        L = R.margin(case["logp"][i], int(case["y"][i]), case["targeted"])
        if first:
            best, used, spare, accept = L, 1, 0, True
        else:
            was = st[i, :1].view(F32)[0]
            if st[i, 2] != 0:                                # frozen: nothing is stored
                continue
            used, spare = int(st[i, 1]) + 1, int(st[i, 3])
            accept = bool(L < was)
            best = L if accept else was
        if accept:
            xb[i] = case["x_cand"][i]
        done = bool(best < 0)
        if not last:
            xc[i] = xb[i] if done else _proposal(xb[i], case["x0"][i], case["eps"], case["seed"], q, side,
                                                  int(case["ids"][i]), lo, hi)
        st[i] = R.pack(best, used, int(done), spare)
    return xb, xc, st


def make_case(M, seed, targeted=False, eps=EPS):
    """``square_ref.make_case`` (its hand-made log-probabilities, labels, records, ids and the NaN pixel of image 1)
    with L2 perturbations: ``x_best`` / ``x_cand`` = clamp(x0 + d), d a normal direction.  Where i + seed is even d
    has norm ``eps`` before the clamp, which then takes a good part of it: SI is well below eps^2.  Where it is odd d
    is rescaled and clamped until the clamped perturbation itself has norm ``eps``: SI = eps^2 up to rounding, the
    cancellation in eps^2 - SI.  With ``eps`` = 0 both points are x0."""
    case = R.make_case(M, seed, targeted, eps)
    g = np.random.default_rng(1000 + seed)
    x0 = case["x0"]
    x0n = np.nan_to_num(x0).astype(F64)
    full = (np.arange(M) + seed) % 2 == 1
    for key in ("x_best", "x_cand"):
        d = g.standard_normal((M, 784))
        for n in range(40):
            scale = eps / np.maximum(np.sqrt((d ** 2).sum(1)), 1e-300)
            if n:
                scale = np.where(full, scale, 1.0)
            d = np.clip(x0n + d * scale[:, None], R.LO, R.HI) - x0n
        x = np.clip(x0n + d, F32(R.LO), F32(R.HI)).astype(F32)
        case[key] = np.where(np.isnan(x0), x0, x).astype(F32)
    return case
