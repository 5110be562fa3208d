"""A numpy emulation of the Square Attack kernels (csrc/kernels/square.hip), image by image, on
``refmodel.philox4x32``: ``init_oracle`` (square_init) and ``step_oracle`` (square_step).  Every operation of the
kernel is an integer operation, a select, one float32 add and one clamp, so the emulation is exact: the tests compare
bit for bit (``mismatches``).  The one exception is the payload of a NaN margin - inf - inf is the hardware's default
NaN, whose sign differs between x86 and the GPU - so two NaNs compare equal; every decision treats all NaNs alike.

``MUTATIONS`` names single deliberate mistakes (``mut=``); the comparators must catch each on ``make_case``."""
import numpy as np

import refmodel as Rm
import smooth_ref
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO

F32 = np.float32
LO, HI = PIXEL_LO, PIXEL_HI
DOMAIN = 0x53515231                                        # kernels.h SQUARE_PHILOX_DOMAIN ("SQR1")
EPS = 0.3 / MNIST_STD
INIT_MUTATIONS = ("stripes_per_row", "c3_fixed", "no_clamp", "sign_inverted")
STEP_MUTATIONS = ("swap_row_col", "sign_inverted", "side_plus_one", "offset_on_best", "no_clamp", "accept_le",
                  "frozen_proposes", "frozen_counts")
MUTATIONS = tuple(dict.fromkeys(INIT_MUTATIONS + STEP_MUTATIONS))


def words(q: int, image_id: int, k: int, seed: int):
    seed &= 2 ** 64 - 1
    return Rm.philox4x32((q, DOMAIN, image_id, k), (seed & Rm.MASK, seed >> 32))


def vertex(x0, plus, eps, lo=LO, hi=HI, clamp=True):
    """clamp(x0 + eps) where ``plus`` else clamp(x0 - eps), float32, each operation rounded on its own; a NaN passes."""
    x0, eps, lo, hi = np.asarray(x0, dtype=F32), F32(eps), F32(lo), F32(hi)
    t = np.where(plus, x0 + eps, x0 - eps).astype(F32)
    if clamp:
        t = np.where(t < lo, lo, t)
        t = np.where(t > hi, hi, t)
    return t.astype(F32)


def init_oracle(x0, eps, seed, ids, lo=LO, hi=HI, mut=None):
    M = x0.shape[0]
    out = np.empty((M, 784), dtype=F32)
    at = np.arange(28)
    for i in range(M):
        bit = [words(0, int(ids[i]), 0 if mut == "c3_fixed" else c >> 2, seed)[c & 3] & 1 for c in range(28)]
        plus = np.array(bit, dtype=bool)
        if mut == "sign_inverted":
            plus = ~plus
        grid = plus[at][:, None] if mut == "stripes_per_row" else plus[at][None, :]
        grid = np.broadcast_to(grid, (28, 28))
        out[i] = vertex(x0[i].reshape(28, 28), grid, eps, lo, hi, clamp=mut != "no_clamp").reshape(784)
    return out


def margin(lp, y: int, targeted: bool):
    """The margin square_step reads off one row: a NaN among the others goes through the maximum."""
    ly = F32(lp[y]) if 0 <= y < 10 else F32(np.nan)
    others = [F32(lp[k]) for k in range(10) if k != y]
    mo = others[0]
    for v in others[1:]:
        if v > mo or v != v:
            mo = v
    with np.errstate(invalid="ignore"):
        return F32(mo - ly) if targeted else F32(ly - mo)


def _proposal(base, x0, eps, seed, q, side, image_id, lo, hi, mut):
    w = words(q, image_id, 0, seed)
    span = 29 - side
    row0, col0 = (w[0] * span) >> 32, (w[1] * span) >> 32
    if mut == "swap_row_col":
        row0, col0 = col0, row0
    plus = bool(w[2] & 1) != (mut == "sign_inverted")
    s = side + 1 if mut == "side_plus_one" else side
    out = base.copy().reshape(28, 28)
    src = (base if mut == "offset_on_best" else x0).reshape(28, 28)
    v = vertex(src, plus, eps, lo, hi, clamp=mut != "no_clamp")
    out[row0:row0 + s, col0:col0 + s] = v[row0:row0 + s, col0:col0 + s]
    return out.reshape(784)


def pack(margin_best, used, done, spare=0):
    return np.array([np.array(margin_best, dtype=F32).view(np.int32), used, done, spare], dtype=np.int32)


def step_oracle(case, side=1, q=1, first=False, last=False, mut=None):
    """(x_best, x_cand, state int32 [M, 4]) after one square_step on ``case`` (``make_case``'s keys; nothing of it
    is modified)."""
    M = case["x0"].shape[0]
    xb, xc, st = case["x_best"].copy(), case["x_cand"].copy(), case["state"].copy()
    x0, eps, seed, ids = case["x0"], case["eps"], case["seed"], case["ids"]
    lo, hi = case.get("lo", LO), case.get("hi", HI)
    for i in range(M):
        L = margin(case["logp"][i], int(case["y"][i]), case["targeted"])
        prop = lambda base: _proposal(base, x0[i], eps, seed, q, side, int(ids[i]), lo, hi, mut)   # noqa: E731
        if first:
            best, used, spare, accept = L, 1, 0, True
        else:
            was = st[i, :1].view(F32)[0]
            if st[i, 2] != 0:                                # frozen: nothing is stored
                if mut == "frozen_counts":
                    st[i, 1] += 1
                if mut == "frozen_proposes" and not last:
                    xc[i] = prop(xb[i])
                continue
            used, spare = int(st[i, 1]) + 1, int(st[i, 3])
            accept = bool(L <= was) if mut == "accept_le" else bool(L < was)
            best = L if accept else was
        if accept:
            xb[i] = xc[i]
        done = bool(best < 0)
        if not last:
            xc[i] = xb[i] if done else prop(xb[i])
        st[i] = pack(best, used, int(done), spare)
    return xb, xc, st


def make_case(M, seed, targeted=False, eps=EPS):
    """Hand-made operands of one square_step on M images: images with many pixels at both ends of the range (the
    clamp acts) and one NaN pixel, x_best / x_cand random vertices of the box, ``smooth_ref.hand_logp`` rows (exact
    ties, NaN, +-inf, all -inf), labels that are the arg-max on every third image (a margin >= 0), and records that
    are done, not done, tied with this round's margin exactly, and NaN."""
    g = np.random.default_rng(seed)
    u8 = g.integers(0, 256, size=(M, 784))
    u8[g.random((M, 784)) < 0.4] = 0
    u8[g.random((M, 784)) < 0.2] = 255
    x0 = ((u8 / 255.0 - 0.1307) / 0.3081).astype(F32)
    x0 = np.clip(x0, F32(LO), F32(HI)).astype(F32)
    if M > 1:
        x0[1, 300] = np.nan
    ids = np.arange(M, dtype=np.int64) + 7 + 1000 * seed
    x_best = vertex(x0, g.random((M, 784)) < 0.5, eps)
    x_cand = vertex(x0, g.random((M, 784)) < 0.5, eps)
    logp = smooth_ref.hand_logp(M, 1, seed)
    y = g.integers(0, 10, size=M).astype(np.int32)
    for i in range(0, M, 3):
        row = np.where(np.isnan(logp[i]), -np.inf, logp[i])
        y[i] = int(np.argmax(row))
    state = np.zeros((M, 4), dtype=np.int32)
    for i in range(M):
        L = margin(logp[i], int(y[i]), targeted)
        kind = i % 6
        if kind == 0:
            mb, done = F32(50.0), 0                          # any finite margin is accepted
        elif kind == 1:
            mb, done = L if L == L else F32(1.0), 0          # an exact tie with this round's margin: not accepted
        elif kind == 2:
            mb, done = F32(-0.5), 1                          # frozen
        elif kind == 3:
            mb, done = F32(np.nan), 0                        # a NaN best: nothing is ever lower
        elif kind == 4:
            mb, done = F32(0.0), 0
        else:
            mb, done = F32(-2.0), 3                          # frozen by any non-zero flag
        if mb == mb and mb < 0 and done == 0:
            done = 1                                         # (a tie below zero belongs to a frozen image)
        state[i] = pack(mb, int(g.integers(1, 40)), done, int(g.integers(-5, 5)))
    return dict(x0=x0, x_best=x_best, x_cand=x_cand, logp=logp, y=y, state=state, ids=ids, eps=float(eps),
                seed=int(0x1234567 + seed) | (seed << 40), targeted=bool(targeted))


def _same_f32(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def mismatches(got, want):
    """Names of the outputs (x_best, x_cand, margin_best, queries_used, done, spare) of ``got`` that are not bit for
    bit those of ``want`` (two NaNs are equal: the module's note)."""
    bad = [n for n, a, b in zip(("x_best", "x_cand"), got[:2], want[:2]) if not _same_f32(a, b).all()]
    gs, ws = np.ascontiguousarray(got[2], dtype=np.int32), np.ascontiguousarray(want[2], dtype=np.int32)
    if not _same_f32(gs[:, 0].copy().view(F32), ws[:, 0].copy().view(F32)).all():
        bad.append("margin_best")
    bad += [n for k, n in ((1, "queries_used"), (2, "done"), (3, "spare")) if not np.array_equal(gs[:, k], ws[:, k])]
    return bad


def init_mismatch(got, want) -> bool:
    return not _same_f32(got, want).all()
