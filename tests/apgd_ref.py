"""Shared by the Auto-PGD tests (tests/test_apgd_cpu.py, tests/test_gpu_apgd.py): the step of ``apgd_step`` spelled out
per image with Python branches (``step_oracle``; ``variant=`` makes one deliberate mistake), the operand generator
that forces every discrete branch by construction (``make_case``), the derived bound of the L2 form and the
comparator (``mismatches``).

THE L2 BOUND (``step_oracle`` returns it per image; derived, not measured).  u = 2^-24 is the fp32 unit roundoff,
n = 784, rho = (n / 2 + 2) u bounds the relative error of sqrt(fp32 sum of n fp32 squares) in ANY summation order
(test_attack_l2_cpu.py ``ball_slack``: (1 + u)^n on the sum, (1 + u) a square, the root halves it and rounds once).
Every vector carries an element-wise error bound E and a 2-norm error bound N (N <= 28 E, but an error that is a
multiple of the vector itself is far smaller element-wise than in norm, which is why both are kept):

  step      t = src + (eta / |gs|) gs, gamma = max|gs_i| / |gs|: the scale is off by (rho + 2u) relative, the product
            and the sum round once each:   E = eta gamma (rho + 3u) + u (max|src| + eta gamma)
                                           N = eta (rho + 3u) + 28 u (max|src| + eta gamma)      (zero gradient: 0, 0)
  P(t)      d = t - x0 (one rounding, Dm = max|d_i|): E_d = E + u Dm, N_d = N + 28 u Dm.  m = |d| is off by at most
            N_d + m rho; s = min(1, eps / m) is 1-Lipschitz in eps / m, so d_i s moves by at most
            s E_d + kappa (s N_d + min(m, eps) (rho + 2u)), kappa = Dm / m; the product, the scale's own division and
            the sum x0 + d s round once each:
                                           E' = s E_d + kappa (s N_d + min(m, eps)(rho + 2u)) + u (3 Dm s + max|x0|)
                                           N' = 2 s N_d + min(m, eps)(rho + 2u) + 28 u (3 Dm s + max|x0|)
            the clamp to [lo, hi] moves nothing apart.
  mix       (src + a (z - src)) + (1 - a)(src - x_old): six roundings on values below V + 2 R, V = max|src|,
            R = max(|z - src|, |src - x_old|):  E = a E_z + 6u (V + 2R), N = a N_z + 168 u (V + 2R)

The bound of x is twice the E of the last projection (first order, doubled for the higher-order terms, as
``ball_slack`` does).  With eps ~ 5 and eta ~ 10 it comes to about 1e-4 on values of size 1: some hundred fp32 ulps -
the any-order rho is what makes it that wide - and far below what any of the mutations moves.
"""
import numpy as np
import torch

from pytorch_mnist_ddp_amd.data.datasets import PIXEL_HI, PIXEL_LO

LO, HI = PIXEL_LO, PIXEL_HI
TINY = np.float32(1e-12)
U = 2.0 ** -24
RHO = (784 / 2 + 2) * U
WINDOW = 8                      # the k of the generator's window launches: 4 n_up <= 3 k is n_up <= 6
VARIANTS = ("first_momentum", "halve_no_restart", "restart_dx", "osc_strict", "stall_ignores_reduced", "n_up_kept",
            "best_ge", "x_old_kept", "no_second_projection", "sign_loss_only", "last_moves_x")
NAMES = ("x", "x_old", "x_best", "g_best", "fstate", "istate")


def _clamp(t, lo, hi):
    """min(max(t, lo), hi) as comparisons: a NaN passes (numpy's clip would too; this is the kernel's form)."""
    t = np.where(t < lo, lo, t)
    return np.where(t > hi, hi, t)


def _sgn(g):
    return np.where(g > 0, 1.0, np.where(g < 0, -1.0, np.where(g == g, 0.0, g))).astype(g.dtype)


def step_oracle(case, norm, first=False, last=False, window=0, dtype=np.float64, variant=None):
    """The new ``(x, x_old, x_best, g_best, fstate, istate)`` as numpy arrays (floats in ``dtype``; float32 rounds
    every operation on its own, as the kernel's linf form does) and, for "l2", the per-image bound of x (module
    docstring; None for "linf").  ``case``: what ``make_case`` returns.  ``variant``: one of ``VARIANTS``."""
    assert variant is None or variant in VARIANTS
    f = lambda t: t.numpy().astype(dtype)                                                   # noqa: E731
    dx, x0, x, x_old, x_best, g_best = (f(case[k]) for k in ("dx", "x0", "x", "x_old", "x_best", "g_best"))
    loss, fs, ist = f(case["loss_rows"]), f(case["fstate"]), case["istate"].numpy().copy()
    sign, eps, lo, hi = dtype(case["sign"]), dtype(np.float32(case["eps"])), dtype(np.float32(LO)), dtype(np.float32(HI))
    M = dx.shape[0]
    out_x, out_old, out_best, out_g = x.copy(), x_old.copy(), x_best.copy(), g_best.copy()
    out_f, out_i = fs.copy(), ist.copy()
    bound = np.zeros(M) if norm == "l2" else None
    a75, half, one, two = dtype(0.75), dtype(0.5), dtype(1.0), dtype(2.0)
    for i in range(M):
        L = sign * loss[i]
        if first:
            eta, loss_best, loss_prev, loss_check = two * eps, L, L, L
            n_up, reduced, iters, restarted = 0, 1, 0, 0
            improved = True
        else:
            eta, loss_best, loss_prev, loss_check = fs[i]
            n_up, reduced, iters, restarted = (int(v) for v in ist[i])
            if L > loss_prev:
                n_up += 1
            loss_prev = L
            improved = (L >= loss_best) if variant == "best_ge" else (L > loss_best)
            if improved:
                loss_best = L
        if improved:
            out_best[i], out_g[i] = x[i], dx[i]
        if last:
            out_f[i] = (eta, loss_best, loss_prev, loss_check)
            out_i[i] = (n_up, reduced, iters, restarted)
            if variant != "last_moves_x":
                continue
        src, graw, a, mom = x[i], dx[i], (a75 if variant == "first_momentum" else one) if first else a75, not first
        if not first:
            restarted = 0
            if window > 0 and not last:
                osc = (4 * n_up < 3 * window) if variant == "osc_strict" else (4 * n_up <= 3 * window)
                stall = (loss_check >= loss_best) if variant == "stall_ignores_reduced" else \
                    (reduced == 0 and loss_check >= loss_best)
                r = bool(osc or stall)
                reduced, loss_check = int(r), loss_best
                if variant != "n_up_kept":
                    n_up = 0
                if r:
                    eta, restarted = half * eta, 1
                    if variant != "halve_no_restart":
                        src = out_best[i]
                        graw = dx[i] if variant == "restart_dx" else out_g[i]
        gs = graw if variant == "sign_loss_only" else sign * graw
        c = x0[i]
        xo = x_old[i]

        def mix(z):
            t = src + a * (z - src)
            return t + (one - a) * (src - xo) if mom else t

        if norm == "linf":
            el, eh = c - eps, c + eps
            box = lambda t: _clamp(_clamp(t, el, eh), lo, hi)                               # noqa: E731
            z = box(src + eta * _sgn(gs))
            x_new = mix(z) if variant == "no_second_projection" else box(mix(z))
        else:
            def proj(t, E, N):
                d = t - c
                m = np.sqrt(np.sum(d * d))
                s = eps / (TINY.astype(dtype) if m < TINY else m)
                s = one if s > 1 else s
                Dm = float(np.max(np.abs(d))) if np.isfinite(d).all() else 0.0
                kappa = Dm / float(m) if m > 0 else 0.0
                Ed, Nd, mm = E + U * Dm, N + 28 * U * Dm, min(float(m), float(eps))
                cm = float(np.max(np.abs(c)))
                E2 = float(s) * Ed + kappa * (float(s) * Nd + mm * (RHO + 2 * U)) + U * (3 * Dm * float(s) + cm)
                N2 = 2 * float(s) * Nd + mm * (RHO + 2 * U) + 28 * U * (3 * Dm * float(s) + cm)
                return _clamp(c + d * s, lo, hi), E2, N2
            n = np.sqrt(np.sum(gs * gs))
            rr = eta / (TINY.astype(dtype) if n < TINY else n)
            V = float(np.max(np.abs(src)))
            if n > 0 and np.isfinite(n):
                gamma = float(np.max(np.abs(gs)) / n)
                E = float(eta) * gamma * (RHO + 3 * U) + U * (V + float(eta) * gamma)
                N = float(eta) * (RHO + 3 * U) + 28 * U * (V + float(eta) * gamma)
            else:
                E = N = 0.0
            z, Ez, Nz = proj(src + rr * gs, E, N)
            t2 = mix(z)
            R = max(float(np.nanmax(np.abs(z - src), initial=0.0)), float(np.max(np.abs(src - xo))) if mom else 0.0)
            Em, Nm = float(a) * Ez + 6 * U * (V + 2 * R), float(a) * Nz + 168 * U * (V + 2 * R)
            if variant == "no_second_projection":
                x_new = t2
            else:
                x_new, E3, _ = proj(t2, Em, Nm)
                bound[i] = 2 * E3
        if variant != "x_old_kept":
            out_old[i] = src
        out_x[i] = x_new
        if not last:
            out_f[i] = (eta, loss_best, loss_prev, loss_check)
            out_i[i] = (n_up, reduced, iters + 1, restarted)
    return (out_x, out_old, out_best, out_g, out_f, out_i), bound


# The scenarios of a middle launch, image i takes scenario i % len(SCENARIOS):
#   up / same / down: L against loss_prev;  improve: L against loss_best (eq: L == loss_best exactly, no improvement)
#   n_up: the counter before the launch (WINDOW = 8: osc is n_up <= 6 after the increment; 6 is the equality)
#   reduced, check: loss_check against the loss_best after the launch's own improvement (ge -> stall when reduced == 0)
SCENARIOS = (
    dict(prev="up", improve=True, n_up=5, reduced=1, check="lt"),      # 0 osc at 4 n_up == 3 k: restart right after
                                                                       #   an improvement (the launch's own x and dx)
    dict(prev="up", improve=False, n_up=6, reduced=0, check="ge"),     # 1 no osc; stall: restart from the stored best
    dict(prev="up", improve=False, n_up=6, reduced=1, check="ge"),     # 2 no osc; reduced == 1 holds the stall: no restart
    dict(prev="up", improve=True, n_up=7, reduced=0, check="lt"),      # 3 no osc, no stall; the best point moves
    dict(prev="down", improve=False, n_up=6, reduced=1, check="lt"),   # 4 osc at the equality, no increment
    dict(prev="down", improve=False, n_up=7, reduced=0, check="eq"),   # 5 no osc; stall at loss_check == loss_best
    dict(prev="same", improve="eq", n_up=7, reduced=1, check="lt"),    # 6 L == loss_prev, L == loss_best: neither counts
    dict(prev="up", improve=False, n_up=6, reduced=1, check="ge", grad="zero"),       # 7 a zero gradient
    dict(prev="up", improve=False, n_up=6, reduced=1, check="ge", grad="nan"),        # 8 a NaN in the gradient
    dict(prev="nan", improve=False, n_up=7, reduced=0, check="lt"),                   # 9 a NaN loss
    dict(prev="up", improve=True, n_up=7, reduced=0, check="lt", pixels="edge"),      # 10 pixels on lo and hi
)


def make_case(norm, M, seed, sign=1, eps=None):
    """Seeded float32 operands of one launch for M images (a dict of CPU tensors, never modified by the helpers):
    image i is built for scenario i % 11 of ``SCENARIOS``.  Every point lies in the eps ball and the range."""
    gen = torch.Generator().manual_seed(seed)
    if eps is None:
        eps = 0.1 / 0.3081 if norm == "linf" else 1.5 / 0.3081
    eps = float(np.float32(eps))
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float32)                         # noqa: E731
    x0 = r(M, 784) * (HI - LO) + LO
    loss = r(M) * 2.0 + 0.5                                   # |L| of the launch, in [0.5, 2.5)
    dx = torch.randn(M, 784, generator=gen) * torch.logspace(-3, 1, M).view(M, 1)
    g_best = torch.randn(M, 784, generator=gen)
    fstate, istate = torch.empty(M, 4), torch.empty(M, 4, dtype=torch.int32)
    for i in range(M):
        sc = SCENARIOS[i % len(SCENARIOS)]
        if sc.get("pixels") == "edge":
            x0[i, ::3], x0[i, 1::3] = LO, HI
        if sc.get("grad") == "zero":
            dx[i] = 0.0
        if sc.get("grad") == "nan":
            dx[i, 100 + i % 50] = float("nan")
        Lr = float(sign) * float(loss[i])                     # L of the launch (the NaN loss: what the state is built on)
        if sc["prev"] == "nan":
            loss[i] = float("nan")
        prev = {"up": Lr - 0.25, "down": Lr + 0.25, "same": Lr, "nan": Lr}[sc["prev"]]
        best = {True: Lr - 0.125, False: Lr + 0.5, "eq": Lr}[sc["improve"]]
        best_after = Lr if sc["improve"] is True else best
        check = {"lt": best_after - 0.0625, "ge": best_after + 0.0625, "eq": best_after}[sc["check"]]
        fstate[i] = torch.tensor([2.0 * eps * 0.5 ** (i % 3), best, prev, check])
        istate[i] = torch.tensor([sc["n_up"], sc["reduced"], 3 + i % 5, i % 2], dtype=torch.int32)

    def inside(scale):
        if norm == "linf":
            p = x0 + (2.0 * r(M, 784) - 1.0) * (scale * eps)
        else:
            d = torch.randn(M, 784, generator=gen)
            p = x0 + d * (scale * eps * r(M, 1) / d.norm(dim=1, keepdim=True))
        return p.clamp(LO, HI)

    x, x_old, x_best = inside(0.9), inside(0.9), inside(0.9)
    return dict(dx=dx, loss_rows=loss, x0=x0, x=x, x_old=x_old, x_best=x_best, g_best=g_best, fstate=fstate,
                istate=istate, sign=sign, eps=eps, norm=norm)


def reference_step(case, dtype, first=False, last=False, window=0):
    """``functional.apgd_step_reference`` on the case's operands in ``dtype``, as numpy arrays."""
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    t = lambda k: case[k].to(dtype)                                                         # noqa: E731
    out = Fk.apgd_step_reference(t("dx"), t("loss_rows"), t("x0"), t("x"), t("x_old"), t("x_best"), t("g_best"),
                                 t("fstate"), case["istate"], case["sign"], case["eps"], LO, HI, norm=case["norm"],
                                 first=first, last=last, window=window)
    return tuple(o.numpy() for o in out)


def mismatches(got, want, x_bound=None):
    """The names of the outputs of ``got`` that differ from the oracle's ``want`` (both as ``NAMES``, numpy): the
    integers and, without ``x_bound``, every float must be equal bit for bit as float32 values (a NaN matches a
    NaN); with ``x_bound`` (float64 [M], the l2 form) x must lie within its image's bound of the oracle, NaNs in the
    same places, and every other float - copies, comparisons and halvings of inputs - is still exact."""
    bad = []
    for name, g, w in zip(NAMES, got, want):
        if name == "istate":
            ok = g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64))
        elif name == "x" and x_bound is not None:
            gn, wn = np.isnan(g), np.isnan(w)
            with np.errstate(invalid="ignore"):
                far = np.abs(g.astype(np.float64) - w.astype(np.float64)) > x_bound[:, None]
            ok = g.shape == w.shape and np.array_equal(gn, wn) and not (far & ~wn).any()
        else:
            ok = g.shape == w.shape and np.array_equal(g.astype(np.float32), w.astype(np.float32), equal_nan=True)
        if not ok:
            bad.append(name)
    return bad
