"""Shared by the L1 Auto-PGD tests (tests/test_apgd_l1_cpu.py, tests/test_gpu_apgd_l1.py): ``apgd_l1_step`` per image in
numpy (``step_oracle``: decisions on float32 values, x and lam in float64, lam by bisection; ``variant=`` makes one
deliberate mistake), seeded operands (``make_case``), hand-made images that force each branch (``hand_case``), the
branches an operand set takes (``census``) and the one comparator of kernel, reference and mutants (``check_launch``).

NaN, as the oracle spells it out.  A NaN |gs| ranks above every number (the order of the float32 bit patterns, which is
the kernel's) and is always selected.  For eps > 0 a row that holds a NaN after the step gets lam = NaN and a NaN x in
every element; for eps = 0 the ball is the point x0: lam = 0, x = x0, and the NaN shows in the element it entered by
and in no other.  A NaN loss is never greater than ``loss_best``: it never becomes the best after the first launch.

THE PER-ELEMENT BOUND OF x (derived, not measured; ulp(v) is the float32 spacing at |v| of the oracle's float64 value).
Between the operands and the store the kernel rounds, each once and to nearest (error at most half an ulp):
    step = eta / m            (selected elements only)           ulp(step) / 2
    t    = src + step sgn     (selected elements only)           ulp(t) / 2
    z    = t - x0                                                ulp(z) / 2
    cap  = hi - x0 or x0 - lo                                    ulp(cap) / 2
    a - lam                   (the sort branch only)             ulp(a - lam) / 2
    x    = x0 + d                                                ulp(x) / 2
s, |z|, max(., 0), min(., cap) and the clamp to [lo, hi] are exact and 1-Lipschitz: they move nothing apart.  x depends
on lam with slope at most 1, so the image's lam bound B_lam adds in full.  First order, doubled for the higher-order
terms (an ulp taken in the neighbouring binade, an error carried into the next operation), as ``apgd_ref`` does:

    |x_e - oracle| <= B_lam + ulp(step) + ulp(t) + ulp(z) + ulp(cap) + ulp(a - lam) + ulp(x)

with the step terms on selected elements and the ``a - lam`` term on the sort branch only; on a ``last`` launch and
under eps = 0 nothing is rounded and the bound is 0.  B_lam = max(4 x |lam of the float32 reference - oracle|, one ulp
of the oracle's lam) on that image - the same number that bounds lam itself - and 0 where lam is not unique (a flat
piece of phi: every element above the crossing sits on its cap and x does not depend on where in the piece lam lies).

THE BOUND OF THE FLOAT32 REFERENCE'S OWN lam (``lam_bound`` of the census; derived).  lam = (S_k - eps) / N_k with S_k
a sum of at most 1568 terms +a_e / -b_e.  u = 2^-24.  A term carries its operands' roundings, e_a = (ulp(step) +
ulp(t) + ulp(z)) / 2 and e_b = e_a + (ulp(cap) + ulp(b)) / 2; a sum of n terms in any order is off by at most
(n - 1) u sum |term|; the subtraction of eps and the division round once each on values below sum |term| + eps:

    |lam - oracle| <= 2 ((n_k + 1) u (T_k + eps) + sum e) / N_k + 2 u lam,    T_k = sum |term|, n_k = the terms summed

(doubled as above: a crossing picked one position early or late is the same lam by continuity, to first order).
"""
import numpy as np
import torch

from pytorch_mnist_ddp_amd.data.datasets import PIXEL_HI, PIXEL_LO

LO, HI, N = float(np.float32(PIXEL_LO)), float(np.float32(PIXEL_HI)), 784
KINDS = ("inside", "free", "caps", "flat", "zero_grad", "ties", "k1", "k784", "sp_old0", "eta_floor")   # image i % 10
ALL_KINDS = KINDS + ("partial",)
U = 2.0 ** -24
ULP_BOX = float(np.spacing(np.float32(max(abs(LO), abs(HI)))))
STORES = N * U * max(abs(LO), abs(HI))                     # the rounding of a row's stores, in L1 mass
NAMES = ("dx", "loss_rows", "x0", "x", "x_best", "g_best", "fstate", "istate")
# deliberate mistakes of the oracle; EQUIVALENT: the two that no operand can tell from the rule (see the CPU test)
VARIANTS = ("ball_then_clamp", "cap_wrong_side", "thr_next", "ties_cut", "zeros_selected", "m_is_k_sel", "sp_on_x",
            "restart_le", "k_sel_floor", "no_eta_floor", "restart_dx", "sp_old_kept", "crossing_n_ge0", "lam_neighbour",
            "pick_strict", "nan_loss_best", "restarted_kept", "lam_offset")
EQUIVALENT = ("crossing_n_ge0", "pick_strict")
_SORTED = ("crossing_n_ge0", "lam_neighbour", "pick_strict")


def _sgn(g):
    return np.where(g > 0, 1.0, np.where(g < 0, -1.0, np.where(g == g, 0.0, g)))


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _root_sorted(a, b, eps, variant):
    """lam by the kernel's sorted form in float64 (the a before the b among equals), with the pick's mistakes."""
    tau = np.concatenate((a, b))
    unit = np.concatenate((np.ones_like(a), -np.ones_like(b)))
    order = np.argsort(tau, kind="stable")
    tau, unit = tau[order], unit[order]
    S, Nk = np.cumsum((tau * unit)[::-1])[::-1], np.cumsum(unit[::-1])[::-1]
    phi = S - tau * Nk
    ok = (Nk >= 0 if variant == "crossing_n_ge0" else Nk > 0) & (phi < eps if variant == "pick_strict" else phi <= eps)
    k = int(np.argmax(ok))
    if variant == "lam_neighbour":                           # the segment one breakpoint value further up
        above = np.nonzero((tau > tau[k]) & (Nk > 0))[0]
        k = int(above[0]) if len(above) else k - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((S[k] - eps) / Nk[k])


def project(z, x0, eps, variant=None):
    """(delta, lam, unique) for one float64 row: z projected onto {|d|_1 <= eps, LO <= x0 + d <= HI}; lam by bisection;
    ``unique``: N at the root > 0 (False on a flat piece of phi, where delta is determined and lam is not)."""
    s, a = _sgn(z), np.abs(z)
    up = (s < 0) if variant == "cap_wrong_side" else (s > 0)
    cap = np.maximum(np.where(up, HI - x0, x0 - LO), 0.0)
    if variant == "ball_then_clamp":                         # the shortcut: the ball alone, the caller's clamp after it
        cap = np.full_like(a, np.inf)
    if eps == 0:
        return s * 0.0, 0.0, True
    if np.isnan(z).any():
        return np.full_like(z, np.nan), float("nan"), True
    phi = lambda lam: np.minimum(np.maximum(a - lam, 0.0), cap).sum()                       # noqa: E731
    if phi(0.0) <= eps:
        return s * np.minimum(a, cap), 0.0, True
    b = np.where(np.isinf(cap), 0.0, np.maximum(a - np.where(np.isinf(cap), 0.0, cap), 0.0))
    if variant in _SORTED:
        hi = _root_sorted(a, b, eps, variant)
    else:
        lo, hi = 0.0, float(a.max())
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if phi(mid) > eps else (lo, mid)
    right = hi * (1.0 + 1e-12)                               # (the bisection stops within rounding of the root)
    if variant == "lam_offset":                              # a sloppy root: 1e-7 off, under the launch-wide ulp floor
        hi += 1e-7
    unique = int((a > right).sum()) - int((b > right).sum()) > 0
    return s * np.minimum(np.maximum(a - hi, 0.0), cap), hi, unique


def step_oracle(case, first=False, last=False, window=0, variant=None, info=None):
    """The new (x, x_best, g_best, fstate, istate) of a launch: x and lam in float64, the rest what the kernel stores.
    ``variant``: one of ``VARIANTS``.  ``info``: a list that receives one dict an image (what ``census`` reports)."""
    assert variant is None or variant in VARIANTS
    dx, x0, x, loss = (case[k].numpy() for k in ("dx", "x0", "x", "loss_rows"))
    f32, sign, eps = np.float32, np.float32(case["sign"]), np.float32(case["eps"])
    out_x, out_best, out_g = x.astype(np.float64), case["x_best"].numpy().copy(), case["g_best"].numpy().copy()
    out_f, out_i = case["fstate"].numpy().astype(np.float64), case["istate"].numpy().copy()
    for i in range(dx.shape[0]):
        L = sign * loss[i]
        eta, loss_best, (k_sel, sp_old, iters, was) = f32(out_f[i, 0]), f32(out_f[i, 1]), (int(v) for v in out_i[i])
        if first:
            eta, loss_best, k_sel, sp_old, iters = eps, L, 157, N, 0
        improved = bool(first or L > loss_best or (variant == "nan_loss_best" and not L <= loss_best))
        if improved:
            loss_best, out_best[i], out_g[i] = L, x[i], dx[i]
        out_f[i, 1] = loss_best
        rec = dict(path="last", improved=improved, restart=False, checkpoint=False, floor=False, unique=True,
                   partial=0, m=0, k_sel=k_sel, crossing=None, lam_bound=0.0, x_bound=np.zeros(N))
        if info is not None:
            info.append(rec)
        if last:
            continue
        src, graw, restarted = x[i], dx[i], (was if variant == "restarted_kept" else 0)
        if window > 0 and not first:
            sp = int(((x[i] if variant == "sp_on_x" else out_best[i]) != x0[i]).sum())
            k_sel = min(max((2 * sp // 3) if variant == "k_sel_floor" else -(-2 * sp // 3), 1), N)
            red = 100 * sp <= 95 * sp_old if variant == "restart_le" else 100 * sp < 95 * sp_old
            if red:
                eta, src, graw, restarted = eps, out_best[i], (dx[i] if variant == "restart_dx" else out_g[i]), 1
            else:
                shrunk, floor_ = f32(eta / f32(1.5)), f32(eps / f32(10.0))
                rec["floor"] = bool(shrunk <= floor_)
                eta = shrunk if variant == "no_eta_floor" else max(shrunk, floor_)
            rec.update(checkpoint=True, restart=bool(red))
            if variant != "sp_old_kept":
                sp_old = sp
        gs = sign * graw
        ks = min(max(k_sel, 1), N)                           # a record from elsewhere: still a slot
        keys = np.abs(gs).view(np.int32)                     # non-negative floats order as their bits, NaN above +inf
        at = N - ks - (1 if variant == "thr_next" and ks < N else 0)
        thr_key = np.partition(keys, at)[at]
        sel = keys >= thr_key
        if variant != "zeros_selected":
            sel &= keys != 0
        if variant == "ties_cut":                            # the first k_sel of them by index, not all
            sel &= np.cumsum(sel) <= ks
        m = int(sel.sum())
        step = np.float64(eta) / max(ks if variant == "m_is_k_sel" else m, 1)
        t = src.astype(np.float64)
        t[sel] += step * _sgn(gs[sel].astype(np.float64))
        c = x0[i].astype(np.float64)
        delta, lam, unique = project(t - c, c, float(eps), variant)
        out_x[i] = c + delta
        out_x[i] = np.where(out_x[i] < LO, LO, np.where(out_x[i] > HI, HI, out_x[i]))       # a NaN passes
        thr = np.array([thr_key], dtype=np.int32).view(np.float32)[0]
        out_f[i], out_i[i] = (eta, loss_best, lam, 0.0), (k_sel, sp_old, iters + 1, restarted)
        out_f[i, 3] = thr                                    # (a float32 in a float64 slot: the NaN payload may go)
        rec.update(m=m, k_sel=k_sel, unique=unique, thr_bits=int(thr_key))
        if info is not None and variant is None:
            rec.update(_bounds(t - c, c, sel, step, float(eps), lam, unique))
    return out_x, out_best, out_g, out_f, out_i


def _bounds(z, c, sel, step, eps, lam, unique):
    """The projection path of one image, its partially binding caps, the crossing's kind and the derived bounds."""
    if eps == 0:
        return dict(path="eps0")
    if np.isnan(z).any():
        return dict(path="nan")
    s, a = _sgn(z), np.abs(z)
    cap = np.maximum(np.where(s > 0, HI - c, c - LO), 0.0)
    b = np.maximum(a - cap, 0.0)
    e_a = 0.5 * (sel * (_ulp(step) + _ulp(c + s * a)) + _ulp(z))
    rounds = 2.0 * e_a + _ulp(cap) + _ulp(c + s * np.minimum(np.maximum(a - lam, 0.0), cap))
    if lam == 0.0 and np.minimum(a, cap).sum() <= eps:
        return dict(path="inside", x_bound=rounds)
    near = lam * (1.0 - 1e-12)
    ta, tb = a[a >= near], b[(b >= near) & (b > 0)]
    crossing = "b" if len(tb) and (not len(ta) or tb.min() < ta.min()) else "a"
    e_b = e_a + 0.5 * (_ulp(cap) + _ulp(b))
    n_k, T, E = len(ta) + len(tb), ta.sum() + tb.sum(), e_a[a >= near].sum() + e_b[(b >= near) & (b > 0)].sum()
    N_k = max(int((a > lam).sum()) - int((b > lam).sum()), 1)
    return dict(path="sort", partial=int(((cap > 0) & (cap < a - lam)).sum()),
                partial_sel=int(((cap > 0) & (cap < a - lam) & sel).sum()), crossing=crossing,
                lam_bound=2.0 * ((n_k + 1) * U * (T + eps) + E) / N_k + 2.0 * U * lam,
                x_bound=rounds + _ulp(a - lam))


def census(case, **kw):
    """One dict an image: ``path`` ("eps0", "inside", "sort", "nan", "last"), with "sort" the number of partially
    binding caps ``partial`` (0 < cap < a - lam) and ``crossing`` ("a" or "b": the kind of the breakpoint the root's
    segment ends at); ``checkpoint``, ``restart``, ``improved``; ``floor`` (the eta floor binds); ``m`` against
    ``k_sel``; ``unique``; the derived ``lam_bound`` and ``x_bound`` (module docstring)."""
    info = []
    step_oracle(case, info=info, **kw)
    return info


def branches(rec):
    """The names of the branches an image of ``census`` takes (the CPU test counts them)."""
    out = ["path:" + rec["path"], "improved" if rec["improved"] else "stored"]
    if rec["path"] == "sort":
        out += ["crossing:" + rec["crossing"], "caps:partial" if rec["partial"] else "caps:none"]
    if rec["checkpoint"]:
        out += [("restart:" if rec["restart"] else "shrink:") + ("improved" if rec["improved"] else "stored")]
        if not rec["restart"]:
            out += ["floor:binds" if rec["floor"] else "floor:free"]
    if rec["path"] not in ("last",):
        ks = min(max(rec["k_sel"], 1), N)
        out += ["m<k" if rec["m"] < ks else "m=k" if rec["m"] == ks else "m>k"]
    return out


BRANCHES = ("path:eps0", "path:inside", "path:sort", "path:last", "improved", "stored", "crossing:a", "crossing:b",
            "caps:partial", "caps:none", "restart:improved", "restart:stored", "shrink:improved", "shrink:stored",
            "floor:binds", "floor:free", "m<k", "m=k", "m>k")


def make_case(M, seed, sign=1, eps=10.0 / 0.3081, restart=False, kinds=None):
    """Seeded float32 operands of one launch, image i of kind ``kinds[i]`` (default: i % 10 of ``KINDS``); ``restart``:
    sp_old = 784, else 1 ("sp_old0": 0).  "partial": built for a launch that is no checkpoint - the selected
    coordinates start at x0, which sits within a fraction of the per-coordinate step eta / k_sel of ``hi`` on half
    of those that move up and of ``lo`` on half of those that move down, the rest of x on the ball's surface."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float32)                         # noqa: E731
    eps = float(np.float32(eps))
    x0 = r(M, N) * (HI - LO - 2.0) + (LO + 1.0)              # "free": at least 1 of room both ways
    dx = torch.randn(M, N, generator=gen) * torch.logspace(-3, 1, M).view(M, 1)
    g_best, loss = torch.randn(M, N, generator=gen), r(M) * 2.0 + 0.5
    kinds = [KINDS[i % len(KINDS)] for i in range(M)] if kinds is None else list(kinds)
    assert len(kinds) == M and all(k in ALL_KINDS for k in kinds)
    for i, kind in enumerate(kinds):
        if kind != "free":                                   # MNIST-like: 70 % at lo exactly, some at hi
            u = r(N)
            x0[i] = torch.where(u < 0.7, torch.tensor(LO), torch.where(u > 0.9, torch.tensor(HI), x0[i]))
        if kind == "flat":                                   # one background: hundreds of equal breakpoints
            x0[i], x0[i, 300:340] = LO, HI
        dx[i] = dx[i] * (kind != "zero_grad")
        if kind == "ties":                                   # a few distinct magnitudes: ties at the threshold
            dx[i], g_best[i] = torch.round(dx[i] / dx[i].abs().max() * 4.0) / 4.0, torch.round(g_best[i])
    of = lambda *names: torch.tensor([k in names for k in kinds])                             # noqa: E731
    i, L, one = torch.arange(M), float(sign) * loss, torch.ones(M)
    mass = torch.where(of("inside"), 0.3, torch.where(of("partial"), 1.0, 0.9)).view(M, 1)   # "partial": on the surface
    fstate = torch.stack((torch.where(of("inside", "eta_floor"), 0.1, 0.7) * eps,            # eta, loss_best, lam, thr
                          torch.where(i % 2 == 1, L - 0.125, L + 0.5), 0.25 * one, 0.5 * one), dim=1)
    istate = torch.stack((torch.where(of("k1"), 1, torch.where(of("k784"), N, 20 + 37 * i % 400)),   # k_sel, sp_old, ..
                          torch.where(of("sp_old0"), 0, N if restart else 1), 3 + i % 5, i % 2), dim=1).to(torch.int32)
    moved = torch.zeros(M, N, dtype=torch.bool)
    for j, kind in enumerate(kinds):
        if kind == "partial":
            k = int(istate[j, 0])
            top = torch.topk(dx[j].abs(), k).indices
            step, u = float(fstate[j, 0]) / k, r(k) * 0.2 + 0.05
            up, near = float(sign) * dx[j, top] > 0, torch.arange(k) % 2 == 0
            x0[j, top] = torch.where(near, torch.where(up, HI - u * step, LO + u * step), x0[j, top]).clamp(LO, HI)
            moved[j, top] = True

    def sparse():                                            # a sparse point inside the ball and the box
        d = torch.randn(M, N, generator=gen)                 # ("partial": half of the pixels, so that lam stays small)
        d = d * (r(M, N) < torch.where(of("partial").view(M, 1), 0.5, 0.05 + r(M, 1) * 0.35)) * ~moved
        d = (x0 + d).clamp(LO, HI) - x0
        return (x0 + d * (mass * eps / d.abs().sum(dim=1, keepdim=True).clamp_min(1e-30)).clamp_max(1.0)).clamp(LO, HI)

    return dict(dx=dx, loss_rows=loss, x0=x0, x=sparse(), x_best=sparse(), g_best=g_best, fstate=fstate, istate=istate,
                sign=sign, eps=eps)


def _changed(x0, sp, mass, perm):
    """x0 with exactly ``sp`` pixels changed (the first sp of ``perm``), inside the box, ``mass`` in all."""
    x = x0.clone()
    at = perm[:sp]
    d = min(mass / max(sp, 1), 0.25)
    x[at] = torch.where(x0[at] <= HI - 1.0, x0[at] + d, x0[at] - d)
    assert int((x != x0).sum()) == sp and bool((x >= LO).all()) and bool((x <= HI).all())
    return x


RESTART_PAIRS = ((94, 100), (95, 100), (96, 100), (744, 784), (745, 784), (0, 0), (0, 1), (19, 20))


def hand_case():
    """Small, fully specified launches, the oracle deciding every expectation: name -> dict(case, kw, labels (one an
    image), flat (the images whose lam is not unique), clean (the same operands without the NaNs, or None), nan (the
    images that hold one)).  Every image is plain arithmetic on in-range operands."""
    out = {}
    f32 = lambda v: float(np.float32(v))                                                      # noqa: E731
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))

    # --- a checkpoint launch, eps = 30 (eps / 10 = 3 and 4.5 / 1.5 = 3 exactly): restart boundary, k_sel, step size
    rows = [(sp, old, form) for sp, old in RESTART_PAIRS for form in ("stored", "improved")]
    rows += [(sp, N, "stored") for sp in (1, 2, 3, N)] + [(40, 0, "eta")] * 3
    M = len(rows)
    c = make_case(M, seed=701, eps=30.0, kinds=["caps"] * M)
    labels = []
    for j, (sp, old, form) in enumerate(rows):
        other = (min(N, old) if old else 5) if 100 * sp < 95 * old else (0 if old else 5)     # flips the decision
        mine, theirs = _changed(c["x0"][j], sp, 0.9 * 30.0, perm), _changed(c["x0"][j], other, 0.9 * 30.0, perm)
        c["x"][j], c["x_best"][j] = (mine, theirs) if form == "improved" else (theirs, mine)
        c["fstate"][j, 1] = float(c["loss_rows"][j]) + (-0.125 if form == "improved" else 0.5)
        c["istate"][j, 1] = old
        labels.append(f"sp={sp} sp_old={old} {form}")
    for j, eta in zip(range(M - 3, M), (6.0, 4.5, 3.0)):     # eta / 1.5 above, equal to and below eps / 10
        c["fstate"][j, 0] = eta
    out["checkpoint"] = dict(case=c, kw=dict(window=2), labels=labels)

    # --- a plain launch, eps = 8: selection, projection, records from elsewhere
    sel_rows = ("ties", "all_equal", "few_nonzero", "zero_grad", "neg_zero_denormal", "ascending", "descending",
                "organ_pipe", "alt64", "alt256", "huge_among_denormals")
    prj_rows = ("exact", "flat", "b_crossing", "equal_breakpoints", "outside_box")
    foreign = (0, -5, 785, 1 << 30)
    labels = list(sel_rows) + list(prj_rows) + [f"k_sel={k}" for k in foreign]
    M = len(labels)
    c = make_case(M, seed=702, eps=8.0, kinds=["caps"] * M)
    c["fstate"][:, 0], e = 4.0, torch.arange(N, dtype=torch.float32)
    sg = torch.where(torch.arange(N) % 3 == 0, -1.0, 1.0)
    tiny = float(np.float32(1.4e-45))
    grads = {"ties": (torch.arange(N) * 7 % 3 + 1.0, 100), "all_equal": (torch.full((N,), 0.75), 10),
             "few_nonzero": (torch.where(torch.arange(N) % 16 == 3, e + 1.0, 0.0), 500),
             "zero_grad": (torch.zeros(N), 157),
             "neg_zero_denormal": (torch.where(e < 100, e + 1.0, torch.where(e < 300, (e - 99.0) * tiny,
                                                                             torch.where(e % 2 == 0, -0.0, 0.0))), 250),
             "ascending": ((e + 1.0) * 1e-3, 157), "descending": ((N - e) * 1e-3, 157),
             "organ_pipe": (torch.minimum(e, N - 1 - e) + 1.0, 157),
             "alt64": (1.0 + (torch.arange(N) // 64 % 2), 157), "alt256": (1.0 + (torch.arange(N) // 256 % 2), 157),
             "huge_among_denormals": (torch.where(e == 391, 1e30, (e + 1.0) * tiny), 3)}
    for j, name in enumerate(sel_rows):
        g, k = grads[name]
        c["dx"][j] = g * sg if name != "neg_zero_denormal" else torch.where(g == 0, g, g * sg)
        c["istate"][j, 0] = k
    c["x"][3] = c["x0"][3] + (c["x"][3] - c["x0"][3]) * 0.5  # the zero gradient stays inside the ball
    # projection: x0 = 1 (free both ways) but where stated; 16 coordinates step by eta / 16 = 0.5, the rest of z is x - x0
    j0, hi_half, big = len(sel_rows), f32(np.float32(HI) - np.float32(0.5)), 16.0 - torch.arange(16.0)
    assert f32(np.float32(HI) - np.float32(hi_half)) == 0.5  # the cap of those pixels is 0.5 exactly
    for j in range(j0, j0 + 4):
        c["x0"][j], c["dx"][j], c["fstate"][j, 0], c["istate"][j, 0] = 1.0, 0.0, 8.0, 16
        c["dx"][j, :16] = big
    z = torch.zeros(4, N)
    z[0, :16], z[0, 100:116] = 0.25, 0.25                    # exact: phi(0.25) = 16 * 0.5 = eps at an a breakpoint
    c["x0"][j0 + 1, :16], z[1, :16], z[1, 100:116] = hi_half, 0.25, 0.125       # flat: phi = 16 caps = eps on [1/8, 1/4]
    c["x0"][j0 + 2, :16], z[2, :8], z[2, 8:16], z[2, 100:104] = hi_half, 0.25, 0.375, 0.5   # the root 1/3 ends at b = 3/8
    z[3, 100:400] = 2.0 ** -6                                # 300 equal a breakpoints hold the crossing
    c["x"][j0:j0 + 4] = c["x0"][j0:j0 + 4] + z
    j = j0 + 4                                               # x0 outside the box on six pixels: cap clamped to 0
    c["x0"][j, :3], c["x0"][j, 3:6] = HI + torch.tensor([0.5, 0.25, 0.125]), LO - torch.tensor([0.5, 0.25, 0.125])
    c["x"][j, :16], c["dx"][j, :16], c["istate"][j, 0] = c["x0"][j, :16], 100.0 + big, 16
    c["dx"][j, 3:6] *= -1.0
    c["istate"][j + 1:, 0] = torch.tensor(foreign, dtype=torch.int32)
    c["x_best"] = torch.minimum(torch.maximum(c["x_best"], torch.tensor(LO)), torch.tensor(HI))
    for name, eps in (("plain", 8.0), ("plain_eps_down", float(np.nextafter(np.float32(8.0), np.float32(0)))),
                      ("plain_eps_up", float(np.nextafter(np.float32(8.0), np.float32(9))))):
        out[name] = dict(case=dict(c, eps=eps), kw={}, labels=labels, flat=[j0 + 1] if name == "plain" else [])

    # --- NaN: a NaN loss and a NaN in dx on a plain launch, a NaN in g_best on a restarting, not improved launch,
    # a NaN in dx under eps = 0; image 0 and the last image hold none
    for name, kw, eps, restart in (("nan_plain", {}, 10.0 / 0.3081, False),
                                   ("nan_restart", dict(window=2), 10.0 / 0.3081, True), ("nan_eps0", {}, 0.0, False)):
        clean = make_case(4, seed=703, eps=eps, restart=restart, kinds=["caps", "free", "caps", "flat"])
        clean["fstate"][:, 1] = clean["loss_rows"] + 0.5     # no image improves: a restart reads g_best
        c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in clean.items()}
        if name == "nan_restart":
            c["g_best"][1, 17], labels = float("nan"), ["clean", "nan g_best", "clean", "clean"]
        else:
            c["loss_rows"][1], c["fstate"][1, 1] = float("nan"), clean["loss_rows"][1] - 1.0
            c["dx"][2, 400], labels = float("nan"), ["clean", "nan loss", "nan dx", "clean"]
        out[name] = dict(case=c, kw=kw, labels=labels, clean=clean, nan=[1] if name == "nan_restart" else [1, 2])
    out["last"] = dict(out["checkpoint"], kw=dict(last=True, window=2))
    for g in out.values():
        g.setdefault("flat", []), g.setdefault("clean", None), g.setdefault("nan", [])
    return out


def reference_launch(case, dtype=torch.float32, **kw):
    """``apgd_l1_step_reference`` on the operands of ``case`` in ``dtype``: the five outputs as numpy arrays."""
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    ops = [case[k].to(dtype) if case[k].is_floating_point() else case[k] for k in NAMES]
    return [o.numpy() for o in Fk.apgd_l1_step_reference(*ops, case["sign"], case["eps"], LO, HI, **kw)]


def rounded(out):
    """An oracle's outputs as the kernel would store them: the floats rounded to float32 once."""
    return [o.astype(np.float32) if o.dtype == np.float64 else o for o in out]


def check_launch(got, case, kw, ref, figures=None, oracle=None):
    """The comparator of one launch.  ``got``: the five outputs (x, x_best, g_best, fstate, istate) of the kernel (or of
    a stand-in for it) as numpy arrays; ``ref``: the same of ``apgd_l1_step_reference`` in float32 on the same
    operands, whose own deviation from the oracle scales the bounds.  Returns a list of ``(rule, message)``, empty
    when all of them hold:

      discrete  x_best, g_best, istate, eta, loss_best and thr bit for bit the oracle's
      nan       x and lam are NaN where the oracle's are, and nowhere else
      launch    over the launch: x and lam within max(4 x the reference's largest error, one ulp of max(|lo|, |hi|)),
                the L1 excess within the stores' rounding + 4 x the reference's
      box       lo <= x <= hi; under eps = 0, x = x0 bit for bit (but a NaN element)
      image_lam per image with a unique root: lam within max(4 x the reference's error on that image, one ulp of lam)
      elem_x    per element: x within that image's lam bound + the roundings between lam and the store (module
                docstring)

    ``figures``: a dict that receives the largest lam and x deviations over eps, over their bounds and (lam) over the
    derived bound of the float32 reference, and the count of images over the lam bound.  ``oracle``:
    ``(step_oracle(case, info=info, **kw), info)`` where the caller has it already."""
    info, bad = [], []
    want, info = (step_oracle(case, info=info, **kw), info) if oracle is None else oracle
    bits = lambda t: np.ascontiguousarray(t).view(np.int32)                                   # noqa: E731
    for k, name in ((1, "x_best"), (2, "g_best"), (4, "istate")):
        if not np.array_equal(bits(got[k]), bits(want[k])):
            bad.append(("discrete", name))
    w3 = want[3][:, [0, 1]].astype(np.float32)
    if not np.array_equal(bits(got[3][:, [0, 1]]), bits(w3)):
        bad.append(("discrete", "eta, loss_best"))
    thr_bits = np.array([r.get("thr_bits", b) for r, b in zip(info, bits(case["fstate"].numpy()[:, 3]))], dtype=np.int32)
    if not np.array_equal(bits(got[3][:, 3]), thr_bits):
        bad.append(("discrete", "thr"))
    x0, eps = case["x0"].numpy().astype(np.float64), float(np.float32(case["eps"]))
    gx, rx, wx = got[0].astype(np.float64), ref[0].astype(np.float64), want[0]
    gl, rl, wl = got[3][:, 2].astype(np.float64), ref[3][:, 2].astype(np.float64), want[3][:, 2]
    if not (np.array_equal(np.isnan(gx), np.isnan(wx)) and np.array_equal(np.isnan(gl), np.isnan(wl))):
        bad.append(("nan", "the NaN elements of x or lam are not the oracle's"))
    if not (np.array_equal(np.isnan(rx), np.isnan(wx)) and np.array_equal(np.isnan(rl), np.isnan(wl))):
        bad.append(("nan", "the reference's NaN elements are not the oracle's"))
    ok, uniq = ~np.isnan(wx), np.array([r["unique"] for r in info]) & ~np.isnan(wl)
    z = lambda v, keep: np.where(keep, np.nan_to_num(v), 0.0)                                 # noqa: E731
    dev = lambda o, ol: (z(np.abs(o - wx), ok), z(np.abs(ol - wl), uniq),                     # noqa: E731
                         max((z(np.abs(o - x0), ok).sum(axis=1) - eps).max(), 0.0))
    (gdx, gdl, gm), (rdx, rdl, rm) = dev(gx, gl), dev(rx, rl)
    if not (gdx.max() <= max(4 * rdx.max(), ULP_BOX) and gdl.max() <= max(4 * rdl.max(), ULP_BOX)
            and gm <= STORES + 4 * rm):
        bad.append(("launch", f"x {gdx.max():.3g} / {rdx.max():.3g}, lam {gdl.max():.3g} / {rdl.max():.3g}, "
                              f"mass {gm:.3g} / {rm:.3g}"))
    if not ((z(gx, ok) >= np.where(ok, LO, 0.0)).all() and (z(gx, ok) <= np.where(ok, HI, 0.0)).all()):
        bad.append(("box", "x leaves [lo, hi]"))
    if eps == 0 and not np.array_equal(got[0][ok], case["x0"].numpy()[ok]):
        bad.append(("box", "eps = 0 and x is not x0"))
    lam_b = np.where(uniq, np.maximum(4 * rdl, _ulp(np.nan_to_num(wl))), 0.0)
    worst = np.argmax(gdl - lam_b)
    if (gdl > lam_b).any():
        bad.append(("image_lam", f"image {worst}: lam off by {gdl[worst]:.3g}, bound {lam_b[worst]:.3g}"))
    x_b = lam_b[:, None] * np.array([r["path"] == "sort" for r in info])[:, None] + np.stack([r["x_bound"] for r in info])
    if (gdx > x_b).any():
        i, e = np.unravel_index(np.argmax(gdx - x_b), gdx.shape)
        bad.append(("elem_x", f"image {i} element {e}: x off by {gdx[i, e]:.3g}, bound {x_b[i, e]:.3g}"))
    if figures is not None:
        for k, v in (("lam_dev_over_eps", gdl.max() / eps if eps else 0.0), ("x_dev_over_eps", gdx.max() / eps if eps else 0.0),
                     ("lam_dev_over_bound", float((gdl[uniq] / lam_b[uniq]).max()) if uniq.any() else 0.0),
                     ("x_dev_over_bound", float((gdx / np.maximum(x_b, 1e-300)).max())),
                     ("lam_dev_over_derived", max([d / r["lam_bound"] for d, r in zip(gdl, info) if r["lam_bound"]] + [0.0])),
                     ("lam_images_over", float((gdl > lam_b).sum())), ("lam_images", float(uniq.sum()))):
            figures[k] = figures.get(k, 0.0) + v if k.startswith("lam_images") else max(figures.get(k, 0.0), float(v))
    return bad


LAUNCHES = [dict(first=True), dict(), dict(window=2, restart=True), dict(window=2), dict(last=True, window=2),
            dict(window=2, eps=0.0)]
EPS = 10.0 / 0.3081


def seeded_case(M, sign, launch):
    """(case, kw) of the kernel test's seeded launch ``launch`` (one of ``LAUNCHES``) at M images."""
    kw = dict(launch)
    case = make_case(M, seed=100 * M + 10 * (sign > 0) + LAUNCHES.index(launch), sign=sign,
                     restart=kw.pop("restart", False), eps=kw.pop("eps", EPS))
    return case, kw


def kind_case(kind, M, launch):
    """(case, kw): M images, all of one kind, under the plain or the restarting checkpoint launch."""
    kw = dict(launch)
    seed = 5000 + 100 * ALL_KINDS.index(kind) + 10 * M + LAUNCHES.index(launch)
    return make_case(M, seed=seed, restart=kw.pop("restart", False), kinds=[kind] * M), kw


def launch_sets():
    """Every operand set the GPU test launches but the trajectory's: (id, case, kw, group or None)."""
    out = [(f"seeded-M{M}-s{sign}-{LAUNCHES.index(la)}", *seeded_case(M, sign, la), None)
           for M in (1, 3, 33) for sign in (1, -1) for la in LAUNCHES]
    out += [(f"kind-{kind}-{LAUNCHES.index(la)}", *kind_case(kind, 1, la), None)
            for kind in ALL_KINDS for la in (LAUNCHES[1], LAUNCHES[2]) if not (kind == "partial" and la is LAUNCHES[2])]
    out += [(f"partial-M{M}", *kind_case("partial", M, LAUNCHES[1]), None) for M in (3, 33)]
    out += [(f"hand-{name}", g["case"], g["kw"], g) for name, g in hand_case().items()]
    return out
