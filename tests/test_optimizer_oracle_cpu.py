"""The optimizer-stage oracle and its checks (tests/refmodel.py), proved on the CPU.

* over six chained steps the float64 oracle stays within the per-step eps of torch.optim.Adadelta, foreach and
  single-tensor, with and without weight decay;
* the op-by-op fp32 emulation of Ada::step, standing in for the kernels on a numpy model of the flat layout and the
  four shadow layouts, passes every comparator that tests/test_gpu_optimizer_stages.py applies (update, ownership,
  isolation, the fused reduce's own gradient);
* each single subtle mutation of the stand-in fails at least one of them - without the bit-for-bit comparison with
  the emulation, which would catch them trivially;
* the GPU test's inputs satisfy what the comparators assume.
"""
import numpy as np
import pytest
import torch

import refmodel as R
from refmodel import ADA_ALL, ADA_CONV, ADA_FC, F32, OFF_CONV, PARAM_TOTAL, bf16_round

f = np.float32
SENT = 0x7FC1
LR, WD = 0.7, 0.01


def _math(p, g, sq, acc, lr, wd, mut):
    """Ada::step in numpy float32, one operation at a time, with the arithmetic mutations."""
    lr, rho, eps, wd = f(lr), f(R.ADA_RHO), f(R.ADA_EPS), f(wd)
    c = f(1) - rho
    p, g, sq, acc = (t.numpy().astype(np.float32, copy=True) for t in (p, g, sq, acc))
    with np.errstate(all="ignore"):
        g0 = g
        if wd != 0 and mut != "wd_after":
            g = g - wd * p if mut == "wd_subtracted" else g + wd * p
        sq = sq * rho + ((g if mut == "no_one_minus_rho" else c * g) * g)
        if mut == "wd_after":
            g = g0 + wd * p
        if mut == "eps_outside_sqrt":
            sd, d = np.sqrt(sq) + eps, np.sqrt(acc) + eps
        else:
            sd, d = np.sqrt(sq + eps), np.sqrt(acc + eps)
        d = (d / sd) * g
        acc_new = acc * rho + (c * d) * d
        if mut == "acc_before_d":
            d = (np.sqrt(acc_new + eps) / sd) * g
        p = p + (-lr) * d
        if mut == "nan_leaks_in_float4":
            bad = np.isnan(g).reshape(-1, 4).any(1).repeat(4)
            p, sq, acc_new = (np.where(bad, f("nan"), t) for t in (p, sq, acc_new))
    return [torch.from_numpy(t.astype(np.float32)) for t in (p, sq, acc_new)]


def _shadows(param, mut):
    sh = R.stage_shadows(param)
    if mut == "shadow_truncated":
        trunc = lambda t: (t.contiguous().view(torch.int32) & -65536).view(F32).to(torch.bfloat16)
        fc1, o = param[:128 * 9216].view(128, 9216), R.ADA_OFFS["conv2.weight"]
        sh = {k: trunc(v) for k, v in R._shadow_layouts(fc1, param[o:o + 18432].view(64, 32, 3, 3)).items()}
    if mut == "w1t_tile_untransposed":       # each 64 (o) x 32 (i) tile stored as it lies, not transposed
        tiles = sh["w1"].view(2, 64, 288, 32).permute(0, 2, 1, 3).contiguous()        # [ot][it][ol][il]
        sh["w1t"] = tiles.view(2, 288, 32, 64).permute(1, 2, 0, 3).reshape(9216, 128).contiguous()
    if mut == "w2f_w2d_swapped":
        sh["w2f"], sh["w2d"] = sh["w2d"].reshape(64, 9, 32), sh["w2f"].reshape(9, 32, 64)
    return sh


def standin(before, own, shadows_owned, lr, wd, mut=None, lr_prev=None, reduced=None):
    """The stand-in launch: updates the flat elements in ``own`` from ``before`` (gradient: ``reduced`` when given,
    written to ``grad`` first, as the fused reduce does), writes the owned shadows; everything else is left alone."""
    after = {k: v.clone() for k, v in before.items()}
    upd = own.clone()
    if mut == "padding_skipped":
        upd[R.ada_padding()] = False
    if mut == "fc_touches_conv1":
        o = R.ADA_OFFS["conv1.weight"]
        upd[o:o + 288] = True
    g = before["grad"]
    if reduced is not None:
        after["grad"][own] = reduced[own]
        g = before["grad"] if mut == "stale_grad" else after["grad"]
    use_lr = lr_prev if mut == "previous_lr" else lr
    new = _math(before["param"][upd], g[upd], before["square_avg"][upd], before["acc_delta"][upd], use_lr, wd, mut)
    for k, v in zip(R.ADA_STATE, new):
        after[k][upd] = v
    sh = _shadows(before["param"] if mut == "shadow_from_old_param" else after["param"], mut)
    for k in shadows_owned:
        after[k] = sh[k].clone()
    return after


def _state(step=0, own=None, grad=None):
    """ada_case as the GPU test loads it: sentinels in every shadow and, outside ``own``, in the three tensors."""
    c = R.ada_case()
    st = {k: c[k].clone() for k in R.ADA_STATE}
    st["grad"] = (c["grads"][step] if grad is None else grad).clone()
    if own is not None:
        for k in R.ADA_STATE:
            st[k][~own] = R.ADA_SENTINEL
    shapes = {"w1": (128, 9216), "w1t": (9216, 128), "w2f": (64, 9, 32), "w2d": (9, 32, 64)}
    for k, s in shapes.items():
        st[k] = torch.full(s, SENT, dtype=torch.int16).view(torch.bfloat16)
    return st


REGIONS = {ADA_ALL: (R.own_mask(0, PARAM_TOTAL), R.ADA_SHADOWS), ADA_FC: (R.own_mask(0, OFF_CONV), ("w1", "w1t")),
           ADA_CONV: (R.own_mask(OFF_CONV, PARAM_TOTAL), ("w2f", "w2d"))}


def run_checks(mut=None):
    """Everything the GPU test asserts about one launch of each kind, on the stand-in (bit equality with the
    emulation aside).  Raises AssertionError at the first check that fails."""
    lr3 = LR * R.ADA_LR_GAMMA
    # 1. a region launch: third step, the lr rewritten before it
    region = ADA_FC if mut == "fc_touches_conv1" else ADA_ALL
    own, shadows = REGIONS[region]
    before = _state(2, own)
    after = standin(before, own, shadows, lr3, WD, mut, lr_prev=LR)
    R.check_adadelta_update(before, after, own, lr3, WD)
    R.check_ownership(before, after, own, shadows)
    # 2. isolation
    if mut in (None, "nan_leaks_in_float4"):
        idx = torch.tensor(R.ADA_POISON)
        dirty_in = {k: v.clone() for k, v in before.items()}
        dirty_in["grad"][idx] = float("nan")
        dirty = standin(dirty_in, own, shadows, lr3, WD, mut, lr_prev=LR)
        c = R.ada_case()
        emu = R.stage_adadelta(c["param"][idx], dirty_in["grad"][idx], c["square_avg"][idx], c["acc_delta"][idx],
                               lr3, R.ADA_RHO, R.ADA_EPS, WD, dtype=F32)
        R.check_isolation(after, dirty, idx, emu)
    # 3. a parts launch of the fused reduce: grad holds the last step's values, the launch writes its own sum
    if mut in (None, "stale_grad"):
        c = R.ada_case()
        sink = R.own_mask(idx=R.conv_sink_elements(0, R.RED_W2_PARTS))
        before = _state(0, sink, grad=c["grads"][1])
        after = standin(before, sink, ("w2f", "w2d"), LR, WD, mut, reduced=c["grads"][0])
        R.check_ownership(before, after, sink, ("w2f", "w2d"), grad_own=sink)
        R.check_adadelta_update(before, after, sink, LR, WD, grad=after["grad"])


MUTATIONS = ("eps_outside_sqrt", "acc_before_d", "no_one_minus_rho", "wd_subtracted", "wd_after", "previous_lr",
             "shadow_from_old_param", "shadow_truncated", "w1t_tile_untransposed", "w2f_w2d_swapped",
             "nan_leaks_in_float4", "padding_skipped", "fc_touches_conv1", "stale_grad")


def test_standin_passes_every_check():
    run_checks(None)
    for region, (own, shadows) in REGIONS.items():       # every region, first step, no weight decay
        before = _state(0, own)
        after = standin(before, own, shadows, 1.0, 0.0)
        stats = R.check_adadelta_update(before, after, own, 1.0, 0.0)
        R.check_ownership(before, after, own, shadows)
        assert all(stats[f"mismatch {k}"][0] == 0 for k in R.ADA_STATE)       # the stand-in is the emulation


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_mutation_fails_a_check(mut):
    assert len(MUTATIONS) == 14
    with pytest.raises(AssertionError):
        run_checks(mut)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("foreach", [False, True])
def test_oracle_within_eps_of_torch_over_six_steps(foreach, wd):
    c = R.ada_case()
    sl = slice(1100000, PARAM_TOTAL)                     # 100 000 elements with every regime and block
    par = torch.nn.Parameter(c["param"][sl].clone())
    opt = torch.optim.Adadelta([par], lr=LR, rho=R.ADA_RHO, eps=R.ADA_EPS, weight_decay=wd, foreach=foreach)
    opt.state[par] = {"step": torch.tensor(0.0), "square_avg": c["square_avg"][sl].clone(),
                      "acc_delta": c["acc_delta"][sl].clone()}
    for it in range(6):
        g = c["grads"][it % 3][sl] * (1.0 if it < 3 else 0.37)
        st = opt.state[par]
        ops = (par.detach().clone(), g, st["square_avg"].clone(), st["acc_delta"].clone())
        par.grad = g.clone()
        opt.step()
        r64 = R.stage_adadelta(*ops, LR, R.ADA_RHO, R.ADA_EPS, wd)
        emu = R.stage_adadelta(*ops, LR, R.ADA_RHO, R.ADA_EPS, wd, dtype=F32)
        e = R.ada_eps(r64, emu, R.torch_adadelta(*ops, LR, R.ADA_RHO, R.ADA_EPS, wd))
        for i, got in enumerate((par.detach(), st["square_avg"], st["acc_delta"])):
            assert 0 < e[i] < float("inf")
            R.assert_within(got, r64[i], e[i], f"torch step {it} {R.ADA_STATE[i]}")
            R.assert_within(emu[i], r64[i], e[i], f"emulation step {it} {R.ADA_STATE[i]}")


def test_inputs_satisfy_the_comparators():
    c = R.ada_case()
    pad = R.ada_padding()
    assert len(pad) == 118 and sum(R.ADA_NUMEL.values()) + len(pad) == PARAM_TOTAL
    assert all(torch.isfinite(c[k]).all() for k in R.ADA_STATE) and (c["square_avg"] >= 0).all() and (c["acc_delta"] >= 0).all()
    assert (c["param"][pad] == 0).all() and (c["square_avg"][pad] == 0).all() and (c["acc_delta"][pad] == 0).all()
    for a, b in R.ADA_ZERO_STATE:
        assert (c["square_avg"][a:b] == 0).all() and (c["acc_delta"][a:b] == 0).all()
    live = c["square_avg"][c["square_avg"] > 0]
    assert live.min() < 1e-11 and live.max() > 10
    for g in c["grads"]:
        assert torch.isfinite(g).all() and (g > 0).any() and (g < 0).any()
        for a, b in R.ADA_ZERO_GRAD:
            z = torch.ones(b - a, dtype=torch.bool)
            z[pad[(pad >= a) & (pad < b)] - a] = False
            assert (g[a:b][z] == 0).all()
        assert ((g[pad].abs() >= 0.1) & (g[pad].abs() <= 10)).all()
        gg = (g * f(0.1)) * g                            # (c g) g in fp32: normal, denormal and flushed to 0
        tiny = np.finfo(np.float32).tiny
        assert ((gg > 0) & (gg < tiny)).sum() > 100 and ((gg == 0) & (g != 0)).sum() > 100 and (g.abs() > 100).any()
        # every region sees a zero gradient, a first step and ordinary elements
        for lo, hi in ((0, R.ADA_OFFS["fc1.bias"]), (R.ADA_OFFS["fc1.bias"], OFF_CONV), (OFF_CONV, PARAM_TOTAL)):
            assert (g[lo:hi] == 0).any() and (c["square_avg"][lo:hi] == 0).any() and (c["square_avg"][lo:hi] > 0).any()
    # every float4 with a poisoned element keeps clean neighbours (the last of fc2.bias and the first padding element
    # share one): a leak within the vector is seen
    p = torch.tensor(R.ADA_POISON)
    assert len(set(R.ADA_POISON)) == 19 and int(torch.bincount(p // 4).max()) <= 2
    # the padding elements start from zero state with a gradient that moves them by far more than any eps
    own = R.own_mask(0, PARAM_TOTAL)
    before = _state(0, own)
    after = standin(before, own, R.ADA_SHADOWS, LR, WD)
    stats = R.check_adadelta_update(before, after, own, LR, WD)
    assert all(0 < stats[k][1] < float("inf") for k in R.ADA_STATE)
    assert float((after["param"][pad] - before["param"][pad]).abs().min()) > 10 * stats["param"][1]
    # the hand-placed shadow values: torch's bf16 rounding gives the bits written down by hand
    got = bf16_round(R.shadow_specials()).view(torch.int16).long() & 0xFFFF
    for g, want in zip(got.tolist(), R.SHADOW_SPECIAL_BITS):
        assert (g & 0x7F80) == 0x7F80 and g & 0x7F if want is None else g == want
    assert all(len(v) == len(R.SHADOW_SPECIAL_BITS) == len(set(v)) for v in R.SHADOW_SPECIAL_AT.values())
    src = R.shadow_sources()
    assert all(torch.equal(src[k].sort().values, src["w1" if k == "w1t" else "w2f" if k == "w2d" else k].sort().values)
               for k in src)
