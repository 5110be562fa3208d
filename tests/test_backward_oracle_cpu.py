"""The stage-wise backward oracle and its checks (tests/refmodel.py), proved on the CPU.

* the float64 stages, chained, give the parameter gradients of emulated_bf16_step (and so, within the existing
  bf16 tolerances, reference_step's);
* a stand-in for the backward kernels built from torch fp32 CPU ops (same layouts, same rounding points) passes
  every per-kernel check that tests/test_gpu_backward_stages.py applies, at that test's hand-made inputs;
* each single subtle mutation of the stand-in fails its check - the proof that the checks would catch such a kernel.
"""
import copy
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.ops.functional import route_codes

import refmodel as R
from refmodel import F32, F64, bf16_round


@functools.lru_cache(maxsize=None)
def _params():
    net = copy.deepcopy(R.trained_net())
    d = {n: p.detach().clone() for n, p in net.named_parameters()}
    d["w2q"], d["w1q"] = bf16_round(d["conv2.weight"]), bf16_round(d["fc1.weight"])
    return net, d


def _trunc_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(F32).to(torch.bfloat16)


# ------------------------------------------------------------------ layouts
def test_record_and_slab_layouts_round_trip():
    g = bf16_round(torch.randn(3, 9216))
    code = torch.randint(0, 4, (3, 9216))
    rec = R.dyc_pack(g, code)
    g2, c2 = R.dyc_unpack(rec)
    assert torch.equal(g2.view(torch.int16), g.view(torch.int16)) and torch.equal(c2, code)
    # one record by hand: image 1, pooled position 77, channel 42 = chunk 5, bit 2
    r = rec.view(3, 144, 144)[1, 77]
    assert r[:128].view(torch.bfloat16)[42] == g[1, 42 * 144 + 77]
    c = int(code[1, 42 * 144 + 77])
    assert (int(r[128 + 10]) >> 2) & 1 == c & 1 and (int(r[128 + 11]) >> 2) & 1 == c >> 1
    assert torch.equal(route_codes(R.route_planes(code.view(3, 144, 64))), code.view(3, 144, 64))
    dy = R.dense_dy(g, code).view(3, 64, 12, 2, 12, 2)
    assert dy[1, 42, 6, c >> 1, 5, c & 1] == g[1, 42 * 144 + 77] and int((dy[1, 42, 6, :, 5, :] != 0).sum()) <= 1
    w, b = torch.randn(4, 64, 32, 3, 3), torch.randn(4, 64)
    w2, b2 = R.w2part_unpack(R.w2part_pack(w, b))
    assert torch.equal(w2, w) and torch.equal(b2, b)
    pm = torch.randint(0, 16, (2, 9216), dtype=torch.uint8)
    from pytorch_mnist_ddp_amd.ops.functional import pmask_flat
    assert torch.equal(pmask_flat(R.pmask_device(pm)), pm)


# ------------------------------------------------------------------ the chained oracle == the step references
def test_chained_backward_oracle_is_the_emulated_step():
    B = 9
    net, d = _params()
    imgs, labels, _ = R.forward_case(B)
    u8, y = imgs[:B], labels[:B]
    k1 = R.keep_rows(R.FWD_RNG_BASE + 6, list(range(B)), 9216, 192)
    k2 = R.keep_rows(R.FWD_RNG_BASE + 7, list(range(B)), 128, 128)
    _, _, want = R.emulated_bf16_step(net, u8, y, k1, k2)
    x = normalize_u8(u8).reshape(B, 784)
    a1 = bf16_round(R.stage_conv1(x, d["conv1.weight"], d["conv1.bias"]))
    st = R.stage_conv2_pool(a1, d["w2q"], d["conv2.bias"], k1)
    p = bf16_round(st["p"])
    hd = R.stage_head(R.stage_fc1_partials(p, d["w1q"], 32), d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], y, k2, 1.0 / B)
    dz1, h, dl = bf16_round(hd["dz1"]), bf16_round(hd["h"]), bf16_round(torch.cat([hd["dl"], torch.zeros(B, 6)], 1))
    got = R.stage_fc_wgrads(dz1, p, h, dl, 1.0, hd["nll"])
    pm = st["code"] | (k1.long().view(B, 9216) << 2) | ((st["pooled"] > 0).long() << 3)
    dg = R.stage_fc_dgrad(dz1, d["w1q"], pm)
    dy = R.dense_dy(bf16_round(dg["g"]), dg["code"])
    cw = R.stage_conv2_wgrad(a1, dy)
    c1 = R.stage_conv2_dgrad_conv1(dy, d["w2q"], x, a1)
    got.update(R.stage_conv_reduce(cw["w"], cw["b"], c1["c1part"]))
    for k, w in want.items():
        # the same roundings at the same points; the oracle scales by float32(1/0.75), the step by float64's (2e-8
        # relative), so rare g elements round to the other bf16 neighbour: the bf16 tolerance of the forward twin
        assert R.rel_err(got[k], w) < 2e-4, (k, R.rel_err(got[k], w))
    assert abs(float(got["loss"]) - float(hd["nll"].mean())) < 1e-12
    # a1 > 0 (what the kernel masks with) is conv1's ReLU decision wherever a1 does not round to 0
    z0 = R.stage_conv1(x, d["conv1.weight"], d["conv1.bias"])
    assert torch.equal(c1["mask"], z0 > 0)


# ------------------------------------------------------------------ the stand-in for the fc_bwd kernel
def fc_standin(B, mut=None, grad_scale=1.0, no_dropout=False):
    """What fc_bwd (+ fc_grad_reduce) would leave at R.fc_hand_case(B), from torch fp32 CPU ops."""
    _, d = _params()
    h = R.fc_hand_case(B)
    Bp = (B + 31) // 32 * 32
    rows = R.dyc_check_rows(B)
    n = Bp if mut == "p_padding_read" else B
    S = R.fc_splits(B)
    parts = []
    for s in range(S):
        r = slice(1024 * s, min(n, 1024 * (s + 1)))
        z, dl = h["dz1"][r].float(), h["dl_bf"][r, :10].float()
        parts.append({"fc1.weight": z.t() @ h["p"][r].float(), "fc1.bias": z.sum(0),
                      "fc2.weight": dl.t() @ h["h_bf"][r].float(), "fc2.bias": dl.sum(0),
                      "loss": h["loss_rows"][1024 * s:min(B, 1024 * (s + 1))].sum()})
    use = parts[:1] if mut == "split_dropped" else parts + parts[1:] if mut == "split_twice" else parts
    sc = grad_scale * grad_scale if mut == "scale_twice" else grad_scale
    grads = {k: sum(q[k] for q in use) * torch.tensor(sc) for k in R.FC_NAMES}
    loss = sum(q["loss"] for q in parts) / (Bp if mut == "loss_over_bp" else B)
    rr = torch.tensor(rows)
    pm = h["pm"][rr].long()
    live = (pm & 8) != 0 if mut == "mask_bit3_only" else (pm & 12) == 12
    g = h["dz1"][rr].float() @ d["w1q"].float()
    if not no_dropout and mut != "no_drop_scale":
        g = g * torch.tensor(R.INV_KEEP1_F32)
    g = torch.where(live, g, torch.zeros_like(g))
    code = pm & 3
    if mut == "planes_swapped":
        code = ((code & 1) << 1) | (code >> 1)
    rec = R.dyc_pack(_trunc_bf16(g) if mut == "g_truncated" else bf16_round(g), code)
    return dict(h=h, rows=rr, grads=grads, loss=loss, parts=parts if S > 1 else None, rec=rec)


def fc_checks(o, grad_scale=1.0, no_dropout=False):
    _, d = _params()
    h = o["h"]
    st = R.check_fc_wgrads(h["dz1"], h["p"], h["h_bf"], h["dl_bf"], grad_scale, o["grads"], h["loss_rows"], o["loss"],
                           o["parts"])
    st.update(R.check_fc_dgrad(h["dz1"][o["rows"]], d["w1q"], h["pm"][o["rows"]], no_dropout, o["rec"]))
    return st


@pytest.mark.parametrize("B,scale,nodrop", [(33, 1.0, False), (33, 0.25, False), (33, 1.0, True), (1025, 1.0, False),
                                            (1025, 0.25, False)])
def test_fc_standin_passes(B, scale, nodrop):
    for name, (dev, eps) in fc_checks(fc_standin(B, grad_scale=scale, no_dropout=nodrop), scale, nodrop).items():
        assert dev <= eps, (name, dev, eps)


FC_MUTATIONS = {
    "g_truncated": (33, "dyc g:"),
    "no_drop_scale": (33, "dyc g:"),
    "mask_bit3_only": (33, "dyc g:|not 0 where the flags"),
    "planes_swapped": (33, "code planes"),
    "p_padding_read": (33, "fc1.weight"),
    "split_dropped": (1025, "fc_bwd fc"),
    "split_twice": (1025, "fc_bwd fc"),
    "scale_twice": (33, "fc_bwd fc"),
    "loss_over_bp": (33, "loss_log"),
}


@pytest.mark.parametrize("mut", sorted(FC_MUTATIONS))
def test_each_fc_mutation_fails(mut):
    B, what = FC_MUTATIONS[mut]
    scale = 0.25 if mut == "scale_twice" else 1.0
    with pytest.raises(AssertionError, match=what):
        fc_checks(fc_standin(B, mut=mut, grad_scale=scale), scale)


# ------------------------------------------------------------------ the stand-in for the conv backward kernels
def conv_standin(B, mut=None, grad_scale=1.0):
    """What conv2_wgrad, conv2_dgrad, c1_prereduce and conv_grad_reduce would leave at R.conv_hand_case(B)."""
    _, d = _params()
    h = R.conv_hand_case(B)
    dy = R.dense_dy(h["g"], h["code"])
    a1 = h["a1"].permute(0, 3, 1, 2).contiguous()
    G = R.conv_wgrad_groups(B)
    wg = R.stage_conv2_wgrad(a1, dy, G, taps_transposed=mut == "taps_transposed",
                             drop_last_row_of=G // 2 if mut == "wgrad_row_dropped" else None, dtype=F32)
    slabs = R.w2part_pack(wg["w"], wg["b"])
    c1part = R.stage_conv2_dgrad_conv1(dy, d["w2q"], h["x"], a1, relu_geq=mut == "relu_geq", dtype=F32)["c1part"]
    if mut == "last_strip_missing":
        c1part[-1] = 0
    stale = torch.randn(1, 18496) * float(slabs.abs().max())        # what an earlier, larger launch left behind
    c1stale = torch.randn(3, 320) * float(c1part.abs().max())
    c1red = R.stage_c1_prereduce(c1part, F32)
    if mut == "c1red_past_end":                                     # the last non-empty slab runs its R rows
        R_ = R.c1red_rows(4 * B)
        j = (4 * B - 1) // R_
        c1red[j] = torch.cat([c1part, c1stale])[j * R_:(j + 1) * R_].sum(0)
    w, b = R.w2part_unpack(torch.cat([slabs, stale]) if mut == "stale_slab" else slabs)
    grads = R.stage_conv_reduce(w, b, c1part, grad_scale, F32)
    grads_pre = R.stage_conv_reduce(w, b, c1red, grad_scale, F32)
    return dict(dy=dy, a1=a1, x=h["x"], slabs=slabs, c1part=c1part, c1red=c1red, grads=grads, grads_pre=grads_pre)


def conv_checks(o, grad_scale=1.0):
    _, d = _params()
    st = R.check_conv2_wgrad(o["a1"], o["dy"], o["slabs"])
    st.update(R.check_conv2_dgrad(o["dy"], d["w2q"], o["x"], o["a1"], o["c1part"]))
    st.update(R.check_c1red(o["c1part"], o["c1red"]))
    st.update(R.check_conv_reduce(o["slabs"], o["c1part"], grad_scale, o["grads"]))
    st.update({"pre " + k: v for k, v in R.check_conv_reduce(o["slabs"], o["c1red"], grad_scale, o["grads_pre"],
                                                             name="conv_grad_reduce pre").items()})
    return st


@pytest.mark.parametrize("B,scale", [(2, 0.25), (86, 1.0)])
def test_conv_standin_passes(B, scale):
    for name, (dev, eps) in conv_checks(conv_standin(B, grad_scale=scale), scale).items():
        assert dev <= eps, (name, dev, eps)


CONV_MUTATIONS = {
    "wgrad_row_dropped": "w2part",
    "taps_transposed": "w2part weight",
    "last_strip_missing": "c1part",
    "relu_geq": "c1part",
    "stale_slab": "conv_grad_reduce conv2",
    "c1red_past_end": "c1red",
}
MUT_B = {"c1red_past_end": 130}              # 520 partial rows in slabs of 3: the last slab holds one


@pytest.mark.parametrize("mut", sorted(CONV_MUTATIONS))
def test_each_conv_mutation_fails(mut):
    with pytest.raises(AssertionError, match=CONV_MUTATIONS[mut]):
        conv_checks(conv_standin(MUT_B.get(mut, 65), mut=mut))
