"""The float64 stage oracle of ``head_margin`` (csrc/kernels/fc_head.hip) and its checks, in the manner of
``refmodel.stage_head`` / ``check_head_train``; the seeded cases the CPU and the GPU tests share.

``stage_head_margin`` is written from the kernel's specification alone (its own selection loop, its own order of the
``dl`` terms); ``tie_expected`` is a third, scalar implementation in numpy float32 for the hand-made tie rows.
"""
import functools

import numpy as np
import torch

import refmodel as R
from refmodel import F32, F64

KINDS = ("cw", "dlr", "dlr_t")
SIZES = (1, 5, 33, 512)                     # one row, a part-filled pad, one row past a pad, the first KS = 4 launch
GUARD = 1e-12
SENT = 0x7FC1                               # bf16 NaN sentinel bits (test_gpu_forward_stages.SENT)
MUTATIONS = ("runner_incl_y", "no_pi3", "pi4_weight_1", "sign", "dz1_unmasked", "pad_unwritten", "dl_col12")
# the kinds a mutation applies to (default: all three; the targeted form has no runner-up)
MUT_KINDS = {"runner_incl_y": ("cw", "dlr"), "no_pi3": ("dlr", "dlr_t"), "pi4_weight_1": ("dlr_t",)}
TIE_BIAS = (1.0, 3.0, 3.0, 2.0, 2.0, 2.0, 0.0, 0.0, -1.0, -1.0)
TOP3_BIAS = (5.0, 5.0, 5.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0)            # d = 1e-12 exactly
# (label, target): the label is one of the equals (1, 2, 3, 4), the runner-up is the first of equals (0, 3, 6)
TIE_ROWS = ((1, 0), (2, 1), (3, 1), (4, 3), (0, 2), (6, 7), (9, 1))
TOP3_ROWS = ((0, 1), (1, 2), (3, 0), (9, 3))


def first_max(z, free, last=False):
    """(value, index) per row: the first maximum of z [R,10] over the classes with ``free`` [R,10] set, explicit >
    in ascending class order (``last``: >=, the last of equals - a mutation)."""
    R_ = z.shape[0]
    best = torch.zeros(R_, dtype=z.dtype)
    idx = torch.full((R_,), -1, dtype=torch.long)
    for c in range(z.shape[1]):
        beats = (z[:, c] >= best) if last else (z[:, c] > best)
        take = free[:, c] & ((idx < 0) | beats)
        best = torch.where(take, z[:, c], best)
        idx = torch.where(take, torch.full_like(idx, c), idx)
    return best, idx


def stage_head_margin(z1part, b_fc1, w_fc2, b_fc2, labels, kind, targets=None, scale=1.0, dtype=F64, mut=None):
    """``refmodel.stage_head`` (dropout off) up to the logits, then the margin loss of ``kind``: ``loss`` [R], ``dl``
    [R,10] (terms added in the kernel's order), ``dz1`` = (dl . w_fc2) (z1 > 0), the denominator ``d`` [R] (CW: 1)
    and ``gap`` [R], the smallest difference of logits any selection of the row rests on."""
    out = R.stage_head(z1part, b_fc1, w_fc2, b_fc2, dtype=dtype)
    z, z1 = out["logits"], out["z1"]
    n = z.shape[0]
    cls = torch.arange(10)[None, :]
    y = labels.long().view(-1, 1)
    last = mut == "last_of_equals"
    not_y = torch.ones(n, 10, dtype=torch.bool) if mut == "runner_incl_y" else cls != y
    zo, o = first_max(z, not_y, last)
    free = torch.ones(n, 10, dtype=torch.bool)
    pv, pi = [], []
    for _ in range(4):
        v, i = first_max(z, free, last)
        pv.append(v)
        pi.append(i)
        free = free & (cls != i[:, None])
    zy = z.gather(1, y).squeeze(1)
    dl = torch.zeros_like(z)
    add = lambda i, v: dl.scatter_add_(1, i.view(-1, 1), v.view(-1, 1))      # noqa: E731
    s = torch.full((n,), float(scale), dtype=dtype)
    sg = -1.0 if mut == "sign" else 1.0
    srt = z.sort(dim=1, descending=True)[0]
    others = z.masked_fill(cls == y, float("-inf")).sort(dim=1, descending=True)[0]
    gap_o = others[:, 0] - others[:, 1]
    if kind == "cw":
        d = torch.ones(n, dtype=dtype)
        loss = zo - zy
        add(o, s)
        add(y, -s * sg)
        gap = gap_o
    elif kind == "dlr":
        d = (pv[0] - pv[2]) + GUARD
        loss = (zo - zy) / d
        add(o, s / d)
        add(y, -(s / d) * sg)
        q = (s * loss) / d
        add(pi[0], -q)
        if mut != "no_pi3":
            add(pi[2], q)
        gap = torch.stack((gap_o, srt[:, 0] - srt[:, 1], srt[:, 1] - srt[:, 2], srt[:, 2] - srt[:, 3])).amin(0)
    else:
        t = targets.long().view(-1, 1)
        zt = z.gather(1, t).squeeze(1)
        d = (pv[0] - 0.5 * (pv[2] + pv[3])) + GUARD
        loss = (zy - zt) / d
        add(y, (s / d) * sg)
        add(t, -(s / d))
        q = (s * loss) / d
        w = 1.0 if mut == "pi4_weight_1" else 0.5
        add(pi[0], -q)
        if mut != "no_pi3":
            add(pi[2], w * q)
        add(pi[3], w * q)
        gap = torch.stack((srt[:, 0] - srt[:, 1], srt[:, 1] - srt[:, 2], srt[:, 2] - srt[:, 3],
                           srt[:, 3] - srt[:, 4])).amin(0)
    dz1 = dl @ w_fc2.to(dtype)
    if mut != "dz1_unmasked":
        dz1 = dz1 * (z1 > 0)
    out.update(loss=loss, dl=dl, dz1=dz1, d=d, gap=gap)
    return out


def _rows(assert_fn, out, ref, eps_rows, rows, what):
    """``assert_fn`` (refmodel.assert_within / assert_rounded_bf16) row by row with that row's eps; the largest
    deviation over the rows."""
    worst = -float("inf")
    for r in rows:
        worst = max(worst, assert_fn(out[r:r + 1], ref[r:r + 1], float(eps_rows[r]), f"{what} row {r}"))
    return worst


def check_head_margin(z1part, hp, labels, kind, targets, scale, loss_rows, h_bf, dz1, dl_bf, name="head_margin"):
    """head_margin rows: z1part [ksplit,R,128], hp the fp32 head parameters by name, labels / targets [R]; outputs
    loss_rows f32 [R], h_bf / dz1 bf16 [R,128], dl_bf bf16 [R,16].

    eps: ``refmodel.stage_eps(fp32 run, float64 run, head=True)`` with the project's EPS_MARGIN / HEAD_ULPS, per
    tensor.  The DLR losses divide by d = z_pi1 - z_pi3 (or - (z_pi3 + z_pi4) / 2): an error e in the logits moves L by
    about e (1 + |L|) / d and dl, dz1 by about e (1 + |L|) / d^2, so one row with a small d would set a tensor-wide
    eps that checks nothing in the others.  There the eps is measured on the tensors scaled back by the oracle's d
    (loss) and d^2 (dl, dz1), where it is uniform, and each row gets that eps over its own d (d^2).

    Selections are decisions: a row's loss, dl and dz1 are compared only where every gap its selections rest on is at
    least tau = the logits' eps in the oracle; the share of rows left out must be <= refmodel.CAP.  The dz1 zero
    pattern is checked on all rows (it rests on z1 alone)."""
    a = (z1part, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], labels, kind, targets, scale)
    r64, r32 = stage_head_margin(*a), stage_head_margin(*a, dtype=F32)
    n = r64["z1"].shape[0]
    e = {k: R.stage_eps(r32[k], r64[k], head=True) for k in ("z1", "h", "logits")}
    stats = {"h_bf": (R.assert_rounded_bf16(h_bf, r64["h"], e["h"], f"{name} h_bf"), e["h"])}
    assert (dl_bf[:, 10:].to(F32) == 0).all(), f"{name}: dl_bf columns 10..15 are not 0"
    tau = e["logits"]
    firm = r64["gap"] >= tau
    share = 1.0 - float(firm.double().mean())
    assert share <= R.CAP, f"{name}: {share:.3g} of the rows rest on a logit gap below tau = {tau:.3g} (cap {R.CAP:.3g})"
    stats["rows_excluded"] = (share, R.CAP)
    rows = firm.nonzero()[:, 0].tolist()
    d = r64["d"]
    for key, out, ref_key, power, fn in (("loss_rows", loss_rows, "loss", 1, R.assert_within),
                                         ("dl_bf", dl_bf[:, :10], "dl", 2, R.assert_rounded_bf16),
                                         ("dz1", dz1, "dz1", 2, R.assert_rounded_bf16)):
        sc = d.pow(power).view(n, *([1] * (r64[ref_key].dim() - 1)))
        eps = R.stage_eps(r32[ref_key] * sc, r64[ref_key] * sc, head=True) / d.pow(power)
        stats[key] = (_rows(fn, out, r64[ref_key], eps, rows, f"{name} {key}"), float(eps.max()))
        if key == "dl_bf":
            eps_dl = eps
    # zero pattern of dz1: 0 <=> z1 <= 0, decided wherever |z1| >= tau - in the rows whose dl is not itself 0 within
    # its eps (a DLR row whose label ranks third has L = 1 identically: its gradient vanishes, and cancels exactly
    # in fp32); in those rows only z1 <= 0 => dz1 == 0 is asked
    live = r64["dl"].abs().amax(1) > eps_dl
    zero, off, m = dz1.to(F32) == 0, r64["z1"] <= 0, r64["z1"].abs()
    if live.any():
        stats["dz1_zero_excluded"] = (R.assert_decisions(zero[live], off[live], m[live], e["z1"], R.CAP,
                                                         f"{name} dz1 zero pattern"), R.CAP)
    dead = (~live)[:, None] & off & (m >= e["z1"])
    assert zero[dead].all(), f"{name}: dz1 is not 0 where z1 <= 0"
    return stats


# ---- the seeded inputs
@functools.lru_cache(maxsize=None)
def head_params():
    """The fp32 head parameters of the seeded Net (torch.manual_seed(1), as the stage tests' Box), by name."""
    from pytorch_mnist_ddp_amd.models.net import Net
    torch.manual_seed(1)
    net = Net()
    return {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith("fc")}


@functools.lru_cache(maxsize=None)
def margin_case(B: int):
    """(z1part [ksplit,B,128], labels [B], targets [B] != labels) of the seeded case of B rows: random partials whose
    sum has the scale of the net's fc1 pre-activations; every fourth row's label is its top class (the runner-up is
    then not the maximum), the others' are random."""
    g = torch.Generator().manual_seed(7000 + B)
    ks = R.fc1_ksplit(B)
    z1part = torch.randn(ks, B, 128, generator=g) * (4.0 / ks ** 0.5)
    labels = torch.randint(0, 10, (B,), generator=g)
    hp = head_params()
    labels[::4] = R.stage_head(z1part, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"])["logits"].argmax(1)[::4]
    targets = (labels + torch.randint(1, 10, (B,), generator=g)) % 10
    return z1part, labels, targets


def standin(z1part, hp, labels, kind, targets, scale, B, rows=None, mut=None):
    """What a correct fp32 kernel stores for the batch rows ``rows`` (default all B; ``z1part`` / ``labels`` /
    ``targets`` hold those rows) in whole buffers [round_up(B, 64), .] under the padding contract: a torch-fp32 run
    rounded to bf16 - or a mutation of it.  Batch rows not in ``rows`` are left 0."""
    r = stage_head_margin(z1part, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], labels, kind, targets, scale,
                          dtype=F32, mut=mut)
    n = torch.arange(B) if rows is None else torch.tensor(rows)
    size, Bp = (B + 63) // 64 * 64, (B + 31) // 32 * 32
    full = {k: torch.zeros(size, w, dtype=torch.bfloat16) for k, w in (("dz1", 128), ("h_bf", 128), ("dl_bf", 16))}
    for t in full.values():
        t.view(torch.int16)[Bp:] = SENT
    full["dz1"][n], full["h_bf"][n] = R.bf16_round(r["dz1"]), R.bf16_round(r["h"])
    dl = torch.zeros(len(n), 16, dtype=torch.bfloat16)
    dl[:, :10] = R.bf16_round(r["dl"])
    if mut == "dl_col12":
        dl[:, 12] = 1.0
    full["dl_bf"][n] = dl
    if mut == "pad_unwritten" and Bp > B:
        full["dz1"].view(torch.int16)[Bp - 1] = SENT
    return dict(loss_rows=torch.zeros(B).index_copy_(0, n, r["loss"]), **full)


def check_all(B, z1part, hp, labels, kind, targets, scale, got, rows=None, name="head_margin"):
    """``check_head_margin`` on the rows ``rows`` (default all B; ``z1part`` / ``labels`` / ``targets`` hold those
    rows) of whole output buffers, and ``check_head_padding`` on the buffers."""
    rows = list(range(B)) if rows is None else rows
    n = torch.tensor(rows)
    st = check_head_margin(z1part, hp, labels, kind, targets, scale, got["loss_rows"][n], got["h_bf"][n], got["dz1"][n],
                           got["dl_bf"][n], name=name)
    R.check_head_padding(B, got["dz1"], got["h_bf"], got["dl_bf"], SENT, name=name)
    return st


# ---- hand-made tie rows: h = 0, so the logits are the fc2 bias exactly
def tie_expected(bias, y, t, kind, s=1.0):
    """(L, dl[10]) in numpy float32, one operation at a time, straight from the kernel's specification."""
    f = np.float32
    z = [f(v) for v in bias]

    def pick(free):
        best = None
        for c in range(10):
            if free[c] and (best is None or z[c] > z[best]):
                best = c
        return best

    o = pick([c != y for c in range(10)])
    free, pi = [True] * 10, []
    for _ in range(4):
        pi.append(pick(free))
        free[pi[-1]] = False
    dl = [f(0.0)] * 10
    s = f(s)

    def add(i, v):
        dl[i] = f(dl[i] + v)

    if kind == "cw":
        L = f(z[o] - z[y])
        add(o, s)
        add(y, f(-s))
        return L, np.array(dl, dtype=f)
    if kind == "dlr":
        d = f(f(z[pi[0]] - z[pi[2]]) + f(GUARD))
        L = f(f(z[o] - z[y]) / d)
        add(o, f(s / d))
        add(y, f(-f(s / d)))
        q = f(f(s * L) / d)
        add(pi[0], f(-q))
        add(pi[2], q)
        return L, np.array(dl, dtype=f)
    d = f(f(z[pi[0]] - f(f(0.5) * f(z[pi[2]] + z[pi[3]]))) + f(GUARD))
    L = f(f(z[y] - z[t]) / d)
    add(y, f(s / d))
    add(t, f(-f(s / d)))
    q = f(f(s * L) / d)
    add(pi[0], f(-q))
    add(pi[2], f(f(0.5) * q))
    add(pi[3], f(f(0.5) * q))
    return L, np.array(dl, dtype=f)


def check_tie_rows(bias, pairs, kind, loss_rows, dl_bf, name="head_margin ties"):
    """Rows whose logits are ``bias`` exactly, row r with (label, target) = pairs[r].  CW: loss_rows and dl_bf are
    bitwise the numpy-float32 values.  DLR / DLR_T: which dl entries are non-zero, their signs, and their values within
    HEAD_ULPS fp32 ulps (then rounded to bf16); the loss within the same; everything finite."""
    for r, (y, t) in enumerate(pairs):
        L, dl = tie_expected(bias, y, t, kind)
        want = torch.from_numpy(dl)
        got = dl_bf[r, :10]
        assert torch.isfinite(loss_rows[r]) and torch.isfinite(got.to(F32)).all(), f"{name}: row {r} is not finite"
        if kind == "cw":
            assert R.same_bits(loss_rows[r:r + 1], torch.tensor([L])), (name, r, float(loss_rows[r]), float(L))
            assert torch.equal(got.view(torch.int16), R.bf16_round(want).view(torch.int16)), (name, r, got, want)
        else:
            assert torch.equal(got.to(F32) != 0, want != 0), f"{name}: row {r} non-zero pattern {got} against {want}"
            assert torch.equal(torch.sign(got.to(F32)), torch.sign(want)), f"{name}: row {r} signs {got} against {want}"
            _, e = torch.frexp(want.abs().max().to(F64))
            R.assert_rounded_bf16(got.reshape(1, 10), want.to(F64).reshape(1, 10), R.HEAD_ULPS * 2.0 ** (int(e) - 24),
                                  f"{name} row {r} dl")
            _, e = torch.frexp(torch.tensor(abs(float(L)) + 1e-30, dtype=F64))
            R.assert_within(loss_rows[r:r + 1], torch.tensor([float(L)], dtype=F64), R.HEAD_ULPS * 2.0 ** (int(e) - 24),
                            f"{name} row {r} loss")
        assert (dl_bf[r, 10:].to(F32) == 0).all(), f"{name}: row {r} dl_bf columns 10..15 are not 0"


def tie_inputs(bias, pairs):
    """(z1part [32,R,128], hp, labels, targets): partials that put every z1 below 0 (h = 0) and ``bias`` as fc2.bias."""
    n = len(pairs)
    z1part = torch.zeros(32, n, 128)
    z1part[0] = -100.0
    hp = dict(head_params())
    hp["fc2.bias"] = torch.tensor(bias)
    return (z1part, hp, torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs]))
