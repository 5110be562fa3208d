"""The input-gradient oracle and its check (tests/refmodel.py stage_input_grad / check_input_grad), proved on the CPU.

* the oracle, behind the chained backward stages on the real chain, is float64 autograd's ``x.grad`` through
  conv1 -> ReLU -> conv2 on the same bf16 operands;
* a stand-in for the kernel built from torch fp32 CPU ops passes every rule (whole launch, each image alone, the
  border ring, the guard row) at the shapes tests/test_gpu_input_grad_stages.py runs;
* each single subtle mutation of the stand-in fails the check - the proof that it would catch such a kernel;
* three of them pass the norm-wise 1e-4 bound of test_gpu_input_grad.py::test_input_grad_kernel_stagewise, which is
  why the element-wise rules exist;
* the support sets of the two single-record images are the ones the GPU test asserts.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8

import refmodel as R
from refmodel import F32, F64, bf16_round

HAND_B = (1, 2, 5, 33, 129)                  # the GPU test's hand-made batch sizes


@functools.lru_cache(maxsize=None)
def _params():
    net = copy.deepcopy(R.trained_net())
    d = {n: p.detach().clone() for n, p in net.named_parameters()}
    d["w2q"], d["w1q"] = bf16_round(d["conv2.weight"]), bf16_round(d["fc1.weight"])
    return d


# ------------------------------------------------------------------ the oracle == autograd
@pytest.mark.parametrize("B", [3, 33])
def test_oracle_behind_the_chained_stages_is_autograd(B):
    d = _params()
    imgs, labels, _ = R.forward_case(B)
    x, y = normalize_u8(imgs[:B]).reshape(B, 784), labels[:B]
    k1 = R.keep_rows(R.FWD_RNG_BASE + 6, list(range(B)), 9216, 192)
    k2 = R.keep_rows(R.FWD_RNG_BASE + 7, list(range(B)), 128, 128)
    a1 = bf16_round(R.stage_conv1(x, d["conv1.weight"], d["conv1.bias"]))
    st = R.stage_conv2_pool(a1, d["w2q"], d["conv2.bias"], k1)
    hd = R.stage_head(R.stage_fc1_partials(bf16_round(st["p"]), d["w1q"], 32), d["fc1.bias"], d["fc2.weight"],
                      d["fc2.bias"], y, k2, 1.0 / B)
    pm = st["code"] | (k1.long().view(B, 9216) << 2) | ((st["pooled"] > 0).long() << 3)
    dg = R.stage_fc_dgrad(bf16_round(hd["dz1"]), d["w1q"], pm)
    dy = R.dense_dy(bf16_round(dg["g"]), dg["code"])
    args = (dy, d["w2q"], a1, d["conv1.weight"])
    got, got32 = R.stage_input_grad(*args), R.stage_input_grad(*args, dtype=F32)
    # float64 autograd through conv1 -> ReLU -> conv2 (bf16 weight) against the same dy: d <conv2(.), dy> / d x
    xg = x.double().view(B, 1, 28, 28).requires_grad_()
    z0 = F.conv2d(xg, d["conv1.weight"].double(), d["conv1.bias"].double())
    y2 = F.conv2d(F.relu(z0), d["w2q"].double(), d["conv2.bias"].double())
    want, = torch.autograd.grad((y2 * dy.double()).sum(), xg)
    assert torch.equal(a1.float() > 0, z0 > 0)               # the stored a1 decides as conv1's ReLU does here
    fp32_dev = float((got32.double() - got).abs().max())
    assert want.abs().max() > 0 and fp32_dev > 0
    assert float((got - want).abs().max()) <= fp32_dev, (float((got - want).abs().max()), fp32_dev)


# ------------------------------------------------------------------ the stand-in for the kernel
def standin(B, mut=None):
    """What input_grad would leave at R.input_grad_hand_case(B), from torch fp32 CPU ops: dx [B,784] and the guard
    row after it."""
    d, h = _params(), R.input_grad_hand_case(B)
    code = h["code"]
    if mut == "planes_swapped":
        code = ((code & 1) << 1) | (code >> 1)
    if mut == "odd_by_even":                 # channel 2k + 1 routed by the code of channel 2k
        code = code.view(B, 32, 2, 144)[:, :, :1].expand(B, 32, 2, 144).reshape(B, 9216)
    dy = R.dense_dy(h["g"], code)
    a1 = h["a1"].permute(0, 3, 1, 2).contiguous()
    dx = R.stage_input_grad(dy, d["w2q"], a1, d["conv1.weight"], dtype=F32, mut=mut).reshape(B, 784)
    guard = torch.full((784,), float("nan"))
    if mut == "guard_row_written":
        guard[0] = 0.0
    return dict(dy=R.dense_dy(h["g"], h["code"]), a1=a1, dx=dx, guard=guard)


def checks(o):
    d = _params()
    return R.check_input_grad(o["dy"], d["w2q"], o["a1"], d["conv1.weight"], o["dx"], o["guard"])


@pytest.mark.parametrize("B", HAND_B)
def test_standin_passes_every_rule(B):
    st = checks(standin(B))
    assert set(st) == {"dx", "dx image", "dx ring"}
    for name, (dev, eps) in st.items():
        assert 0 < dev <= eps, (name, dev, eps)


MUT_B = {"pixel_27_27_zeroed": 33, "corner_scaled": 33, "guard_row_written": 33}
MUT_WHAT = {"guard_row_written": "guard row"}


@pytest.mark.parametrize("mut", R.IG_MUTATIONS)
def test_each_mutation_fails(mut):
    with pytest.raises(AssertionError, match=MUT_WHAT.get(mut, "input_grad dx")):
        checks(standin(MUT_B.get(mut, 5), mut=mut))


@pytest.mark.parametrize("mut", ["da1_bf16", "pixel_27_27_zeroed", "halo_zero_2", "denormal_off"])
def test_mutations_fail_at_one_image_too(mut):
    with pytest.raises(AssertionError, match="input_grad dx"):
        checks(standin(1, mut=mut))


# ------------------------------------------------------------------ what the norm-wise bound could not see
@pytest.mark.parametrize("mut", ["pixel_27_27_zeroed", "corner_scaled", "guard_row_written"])
def test_old_norm_wise_bound_passes_these_mutations(mut):
    """rel_err < 1e-4 over the launch and over the ring as one vector (test_input_grad_kernel_stagewise) at B = 33:
    passed, while test_each_mutation_fails shows the element-wise rules failing on the same outputs."""
    d, o = _params(), standin(33, mut=mut)
    want = R.stage_input_grad(o["dy"], d["w2q"], o["a1"], d["conv1.weight"])
    got, ring = o["dx"].view(33, 1, 28, 28), R.ig_ring()
    assert want.norm() > 0 and want[..., ring].norm() > 0
    assert R.rel_err(got, want) < 1e-4 and R.rel_err(got[..., ring], want[..., ring]) < 1e-4


# ------------------------------------------------------------------ the hand case holds what it says
def test_hand_case_edges_scales_and_special_images():
    h = R.input_grad_hand_case(33)
    a1, g, code = h["a1"], h["g"].view(33, 64, 144), h["code"].view(33, 64, 144)
    for k, (y, x) in enumerate(R.IG_EDGE_AT):
        bits = a1[:, y, x].view(torch.int16).long() & 0xFFFF
        assert set(bits.flatten().tolist()) == set(R.IG_EDGE_BITS), (y, x)
        on = a1[0, y, x].float() > 0                         # as the oracle decides ...
        assert torch.equal(on, a1[0, y, x].view(torch.int16) > 0)   # ... and as the kernel does (int16 > 0)
        assert int(on.sum()) in (20, 21, 22)                 # 4 of the 6 edge values are positive, over 32 channels
    rows = {y for y, _ in R.IG_EDGE_AT}
    assert {0, 5, 6, 7, 12, 13, 14, 19, 20, 21, 25} <= rows
    amp = g.float().abs().amax((1, 2))
    ordinary = [b for b in range(33) if b not in (R.IG_ZERO_IMAGE, R.IG_CORNER_IMAGE, R.IG_ORIGIN_IMAGE)]
    assert amp[0] > 0.2 and amp[32] < 2e-8 and bool((amp[ordinary][1:] < amp[ordinary][:-1]).all())
    assert not g[R.IG_ZERO_IMAGE].any() and not code[R.IG_ZERO_IMAGE].any()
    for b, pos in ((R.IG_CORNER_IMAGE, 143), (R.IG_ORIGIN_IMAGE, 0)):
        others = torch.arange(144) != pos
        assert not g[b][:, others].any() and not code[b][:, others].any() and bool((g[b][:, pos] != 0).all())
        assert set(code[b][:, pos].tolist()) == {0, 1, 2, 3}
    for b in ordinary:                       # dense: every gradient non-zero, every code in every 8-channel chunk
        assert bool((g[b] != 0).all())
        assert all(set(code[b, c:c + 8, 7].tolist()) == {0, 1, 2, 3} for c in range(0, 64, 8))
    assert not R.input_grad_hand_case(2)["g"].eq(0).any()    # below 5 images: ordinary images only


def test_support_sets_of_the_single_record_images():
    d, o = _params(), standin(33)
    want = R.stage_input_grad(o["dy"], d["w2q"], o["a1"], d["conv1.weight"]).view(33, 28, 28)
    assert torch.equal(want[R.IG_CORNER_IMAGE] != 0, R.ig_support(11, 11))
    assert torch.equal(want[R.IG_ORIGIN_IMAGE] != 0, R.ig_support(0, 0))
    assert int(R.ig_support(11, 11).sum()) == 36 and bool(R.ig_support(11, 11)[22:, 22:].all())
    assert not want[R.IG_ZERO_IMAGE].any()
    dx = o["dx"].view(33, 28, 28)            # and the fp32 stand-in is exactly zero outside them
    assert not dx[R.IG_ZERO_IMAGE].any() and not dx[R.IG_CORNER_IMAGE][~R.ig_support(11, 11)].any()
    assert not dx[R.IG_ORIGIN_IMAGE][~R.ig_support(0, 0)].any()
    assert int(R.ig_ring().sum()) == 208


# ------------------------------------------------------------------ the grid keyword on the host
def test_negative_grid_is_a_value_error_before_any_launch():
    from pytorch_mnist_ddp_amd import _build
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops import native
    _build.build()
    C = native.load(build_if_missing=False)
    with pytest.raises(ValueError, match="grid"):
        C.input_grad(8, 8, 8, 8, 8, 1, 0, grid=-1)
    with pytest.raises(ValueError, match="grid"):
        C.input_grad_step(8, 8, 8, 8, 8, 8, 8, 0.1, 0.1, 0.0, 1.0, 1, 0, grid=-3)
    assert Fk._grid_kw("input_grad", 0) == {} and Fk._grid_kw("input_grad", 5) == {"grid": 5}
    with pytest.raises(ValueError, match="input_grad_step: grid"):
        Fk._grid_kw("input_grad_step", -1)
