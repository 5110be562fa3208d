"""The stage-wise forward oracle and its comparators (tests/refmodel.py), proved on the CPU.

* the float64 stages, chained, are the torch references;
* for the exact inputs of tests/test_gpu_forward_stages.py the share of decisions excluded as near-ties
  stays below the cap, with tau from the run-time rule;
* a stand-in for the kernels built from torch fp32 CPU ops (same layouts, same rounding points) passes
  every per-kernel check, and each single subtle mutation of it fails the check that the GPU test applies
  to the real kernels - the proof that those checks would catch such a kernel.
"""
import copy
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.models.net import Net

import refmodel as R
from refmodel import F32, F64, FWD_RNG_BASE, FWD_SEED, FWD_STEP, bf16_round

OFF1 = FWD_RNG_BASE + 2 * FWD_STEP          # dropout-1 offset of the step; dropout-2 is OFF1 + 1
SENT = 0x7FC1                               # bf16 NaN sentinel bits


@functools.lru_cache(maxsize=None)
def _params(trained=False):
    if trained:
        net = copy.deepcopy(R.trained_net())
    else:
        torch.manual_seed(1)
        net = Net()
    d = {n: p.detach().clone() for n, p in net.named_parameters()}
    d["w2q"], d["w1q"] = bf16_round(d["conv2.weight"]), bf16_round(d["fc1.weight"])
    return net, d


def _rows_input(B, rows, data_seed=5):
    imgs, labels, idx = R.forward_case(B, data_seed)
    src = idx[FWD_STEP * B + torch.as_tensor(rows)]
    return normalize_u8(imgs[src]).reshape(len(rows), 784), labels[src]


# ------------------------------------------------------------------ oracle == torch references
@pytest.mark.parametrize("dropout", [False, True])
def test_stages_chained_are_the_torch_references(dropout):
    B = 33
    net, d = _params()
    rows = list(range(B))
    x, y = _rows_input(B, rows)
    imgs, labels, idx = R.forward_case(B)
    u8 = imgs[idx[FWD_STEP * B:FWD_STEP * B + B]]
    k1 = R.keep_rows(OFF1, rows, 9216, 192) if dropout else None
    k2 = R.keep_rows(OFF1 + 1, rows, 128, 128) if dropout else None
    # with a mask the oracle scales by the kernel's float32(1/0.75), the references by float64 1/0.75
    # (2e-8 relative): exact without dropout; with it, rare p elements round to the other bf16 neighbour
    tol_exact, tol_bf16 = (1e-6, 2e-4) if dropout else (1e-10, 1e-10)
    # no rounding: reference_forward in float64
    c1 = R.stage_conv1(x, d["conv1.weight"], d["conv1.bias"])
    st = R.stage_conv2_pool(c1, d["conv2.weight"], d["conv2.bias"], k1)
    zp = R.stage_fc1_partials(st["p"], d["fc1.weight"], 32)
    hd = R.stage_head(zp, d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], y, k2, 1.0 / B)
    with torch.no_grad():
        lp = R.reference_forward(copy.deepcopy(net).double(), normalize_u8(u8).double(),
                                 None if k1 is None else k1.double(), None if k2 is None else k2.double())
    assert (hd["logp"] - lp).abs().max().item() < tol_exact
    # bf16 rounding at the kernel's points: emulated_bf16_step
    st = R.stage_conv2_pool(bf16_round(c1), d["w2q"], d["conv2.bias"], k1)
    for ks in (32, 4):
        zp = R.stage_fc1_partials(bf16_round(st["p"]), d["w1q"], ks)
        hd = R.stage_head(zp, d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], y, k2, 1.0 / B)
        loss, lp, _ = R.emulated_bf16_step(net, u8, y, k1, k2)
        assert (hd["logp"] - lp).abs().max().item() < tol_bf16
        assert abs(hd["nll"].mean().item() - loss.item()) < tol_bf16
    # the pool's own argmax rule is torch's on distinct values
    _, arg = torch.nn.functional.max_pool2d(torch.relu(R.pool_windows.__globals__["F"].conv2d(
        bf16_round(c1).double(), d["w2q"].double(), d["conv2.bias"].double())), 2, return_indices=True)
    code = (arg // 24 % 2) * 2 + arg % 24 % 2
    distinct = (st["gap"] > 0) & (st["pooled"] > 0)
    assert torch.equal(st["code"][distinct], code.reshape(B, 9216)[distinct])


def test_vector_keep_mask_is_the_scalar_rule():
    n = 9216 + 40
    assert torch.equal(R.keep_mask_at(FWD_SEED, OFF1, torch.arange(n), 192), R.keep_mask(FWD_SEED, OFF1, n, 192))
    e = torch.tensor([0, 15, 16, 2 ** 32 - 1, 2 ** 32, 2 ** 36 + 17, 1024 * 9216 + 9215])   # counter word 1 too
    want = torch.tensor([float(R.dropout_keep(FWD_SEED, OFF1 + 1, int(i), 128)) for i in e])
    assert torch.equal(R.keep_mask_at(FWD_SEED, OFF1 + 1, e, 128), want)


def test_halfulp_and_comparators_on_hand_values():
    x = torch.tensor([0.0, 1.0, 1.5, 0.999, -3.0, 2.0 ** -20], dtype=F64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7, 2.0 ** -28], dtype=F64)
    assert torch.equal(R.halfulp_bf16(x), want)
    ref = torch.tensor([1.0 + 2.0 ** -8 - 1e-9], dtype=F64)                  # just below the midpoint of 1, 1 + 2^-7
    lo, hi = torch.tensor([1.0]).bfloat16(), torch.tensor([1.0 + 2.0 ** -7]).bfloat16()
    R.assert_rounded_bf16(lo, ref, 0.0)
    R.assert_rounded_bf16(hi, ref, 1e-8)                                     # either neighbour within eps of it
    with pytest.raises(AssertionError):
        R.assert_rounded_bf16(hi, ref, 1e-10)
    with pytest.raises(AssertionError):
        R.assert_rounded_bf16(torch.tensor([float("nan")]).bfloat16(), ref, 1.0)
    got, want, m = torch.tensor([1, 2, 3, 0]), torch.tensor([1, 2, 0, 0]), torch.tensor([1.0, 1.0, 1e-9, 1.0], dtype=F64)
    assert R.assert_decisions(got, want, m, 1e-6, cap=0.25) == 0.25
    with pytest.raises(AssertionError, match="cap"):
        R.assert_decisions(got, want, m, 1e-6, cap=0.2)
    with pytest.raises(AssertionError, match="differ"):
        R.assert_decisions(got, want, m, 1e-10, cap=0.25)


# ------------------------------------------------------------------ the stand-in for the kernels
def _trunc_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(F32).to(torch.bfloat16)


def standin(B, mut=None, dropout=True, rows=None, data_seed=5, trained=False, ksplit=None):
    """What the forward kernels would leave for batch rows ``rows`` of a B-row step, from torch fp32 CPU
    ops; ``mut`` names one deliberate error."""
    _, d = _params(trained)
    rows = list(range(B)) if rows is None else rows
    R_ = len(rows)
    x, y = _rows_input(B, rows, data_seed)
    o = dict(B=B, rows=rows, x=x, y=y, dropout=dropout, ksplit=ksplit or R.fc1_ksplit(B), inv=float(torch.tensor(1.0 / B)))
    a1 = bf16_round(R.stage_conv1(x, d["conv1.weight"], d["conv1.bias"], F32))
    o["a1"] = a1.permute(0, 2, 3, 1).contiguous()                           # NHWC
    keep1 = torch.ones(R_, 9216)
    if dropout:
        rr = torch.tensor(rows).view(-1, 1)
        elems = rr * 9216 + torch.arange(9216)
        blocks = (torch.arange(9216) >> 4).expand(R_, 9216) if mut == "rowlocal_counter" else None
        keep1 = R.keep_mask_at(FWD_SEED, OFF1 + (mut == "philox_offset"), elems, 192, blocks)
    win = R.stage_conv2_pool(a1, d["w2q"], d["conv2.bias"], None, F32)["windows"]
    r = torch.relu(win)
    pooled, code = r[..., 0].clone(), torch.zeros(R_, 9216, dtype=torch.long)
    for k in range(1, 4):
        m = r[..., k] >= pooled if mut == "last_max" else r[..., k] > pooled
        pooled, code = torch.where(m, r[..., k], pooled), torch.where(m, torch.full_like(code, k), code)
    pos = pooled >= 0 if mut == "pos_geq" else pooled > 0
    scale = torch.tensor(R.INV_KEEP1_F32, dtype=F32) if dropout else torch.tensor(1.0)
    if mut == "scale_after_round":
        p = bf16_round(bf16_round(pooled).float() * keep1 * scale)
    elif mut == "p_truncated":
        p = _trunc_bf16(pooled * keep1 * scale)
    else:
        p = bf16_round(pooled * keep1 * scale)
    o["p"], o["pm"] = p, (code | (keep1.long() << 2) | (pos.long() << 3)).to(torch.uint8)
    z = R.stage_fc1_partials(p, d["w1q"], o["ksplit"], F32)
    if mut == "chunk_swap":
        z = z[[0, 2, 1] + list(range(3, o["ksplit"]))]
    if mut == "bias_every_chunk":
        z = z + d["fc1.bias"]
    o["z1part"] = z.contiguous()
    keep2 = R.keep_rows(OFF1 + 1, rows, 128, 128) if dropout else None
    h = R.stage_head(z, d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], y, keep2, o["inv"], F32)
    dl, dz1 = h["dl"].clone(), h["dz1"]
    if mut == "dz1_mask_h":                 # the whole factor keep2 * 2 * (z1 > 0) replaced by the 0/1 mask h > 0
        dz1 = (h["dl"] @ d["fc2.weight"]) * (h["h"] > 0)
    if mut == "dl_no_label":
        dl[R_ // 2] = h["logp"][R_ // 2].exp() * o["inv"]
    Bp = (R_ + 63) // 64 * 64
    pad = lambda t, w: torch.cat([bf16_round(t).reshape(R_, -1), torch.zeros((R_ + 31) // 32 * 32 - R_, w).bfloat16(),
                                  torch.full((Bp - (R_ + 31) // 32 * 32, w), SENT, dtype=torch.int16).view(torch.bfloat16)])
    o["h_bf"], o["dz1"] = pad(h["h"], 128), pad(dz1, 128)
    o["dl_bf"] = pad(torch.cat([dl, torch.zeros(R_, 6)], 1), 16)
    if mut == "stale_padding" :
        o["dz1"][R_] = 0.5
    o["loss_rows"], o["logp"] = h["nll"], h["logp"]
    o["correct"] = (R.first_strict_max(h["logp"])[1] == y).int()
    o["keep1"], o["keep2"] = (R.keep_rows(OFF1, rows, 9216, 192) if dropout else None), keep2
    return o


def run_checks(o, trained=False):
    """Every per-kernel check of the GPU test, on the stand-in's tensors."""
    _, d = _params(trained)
    n = len(o["rows"])
    stats = {}
    stats["trunk"] = R.check_trunk(o["x"], d["conv1.weight"], d["conv1.bias"], d["w2q"], d["conv2.bias"], o["p"],
                                   a1=o["a1"], pm=o["pm"], keep1=o["keep1"])
    stats["fc1"] = R.check_fc1(o["p"], d["w1q"], o["z1part"], o["ksplit"])
    stats["head"] = R.check_head_train(o["z1part"], d, o["y"], o["keep2"], o["inv"], o["loss_rows"], o["h_bf"][:n],
                                       o["dz1"][:n], o["dl_bf"][:n])
    if n == o["B"]:
        R.check_head_padding(n, o["dz1"], o["h_bf"], o["dl_bf"], SENT)
    return stats


@pytest.mark.parametrize("B,dropout", [(7, True), (33, True), (33, False)])
def test_standin_passes_every_comparator(B, dropout):
    stats = run_checks(standin(B, dropout=dropout))
    for stage, st in stats.items():
        for name, (dev, eps) in st.items():
            assert dev <= eps, (stage, name, dev, eps)


MUTATIONS = {
    "p_truncated": "trunk p:",
    "last_max": "argmax code",
    "pos_geq": "pooled > 0 bit",
    "scale_after_round": "trunk p:",
    "chunk_swap": "fc1 z1part",
    "philox_offset": "keep bits|not 0 where dropout-1",
    "rowlocal_counter": "keep bits|not 0 where dropout-1",
    "bias_every_chunk": "fc1 z1part",
    # `h > 0` after dropout is the same set as `keep && z1 > 0`; the error this stands for is using that 0/1
    # mask in place of the factor keep * 2 * (z1 > 0), which loses dropout-2's scale in dz1
    "dz1_mask_h": "head_train dz1:",
    "dl_no_label": "head_train dl_bf",
    "stale_padding": "padding rows",
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_each_single_mutation_fails(mut):
    with pytest.raises(AssertionError, match=MUTATIONS[mut]):
        run_checks(standin(33, mut=mut))


# ------------------------------------------------------------------ caps for the GPU test's inputs
@pytest.mark.parametrize("B", sorted(set(R.TRUNK_B + R.FC1_B)))
def test_caps_hold_for_the_gpu_tests_training_inputs(B):
    """check_trunk / check_head_train assert every cap (argmax near-ties, |pooled| < tau, |z1| < tau) with tau
    from the run-time rule; here on the stand-in for the rows, step, seed and data the GPU test uses."""
    rows = R.check_rows(B)
    stats = run_checks(standin(B, rows=rows))
    for key in (("trunk", "argmax_excluded"), ("trunk", "pos_excluded"), ("head", "dz1_zero_excluded")):
        share, cap = stats[key[0]][key[1]]
        assert share <= cap == 1e-3, (key, share)


@pytest.mark.parametrize("B", R.EVAL_B)
def test_caps_hold_for_the_gpu_tests_eval_inputs(B):
    """Top-two log-prob gap below tau on the trained net: the share head_eval's argmax / correct may exclude."""
    _, d = _params(True)
    o = standin(B, dropout=False, rows=R.check_rows(B), trained=True)
    st = R.check_head_logp(o["z1part"], d, o["logp"], labels=o["y"], loss_rows=o["loss_rows"], correct=o["correct"])
    assert st["argmax_excluded"][0] <= 1e-3
    # after the 32 steps the argmax is not one class for all rows: the decision check has something to decide
    assert len(set(R.first_strict_max(o["logp"])[1].tolist())) > 1
