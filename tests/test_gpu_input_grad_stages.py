"""T1: the input-gradient kernel (csrc/kernels/input_grad.hip) on its own against the float64 stage oracle (MI355X only).

Every element of dx is held to refmodel.stage_input_grad on the operands the launch read, copied back (the dy
records unpacked, the stored a1, ``ms.w2d``, the fp32 conv1 weight), under refmodel.check_input_grad's three rules:
eps = 8 x the deviation of torch's fp32 CPU op from float64, measured here, over the whole launch, over each image
alone and over the border ring alone.  Inputs are the real chain (trained net, dropout on, step 3, rows by index),
the ``GradChain`` form the Predictor loops launch, and refmodel.input_grad_hand_case (dense records, gradient scales
1e2 .. 1e-6, a1 edge values, an all-zero image and two single-record images).  Every case also checks what the launch
must not touch: the guard row after dx, the operands' own bits, poisoned padding images, a second launch and a
fresh output.  The ``grid`` keyword shrinks the planned grid: any grid gives the planned launch's bits.
tests/test_input_grad_oracle_cpu.py proves on the CPU that these checks fail on subtly wrong outputs.  Each test
prints `stage B set deviation eps` (docs/COVERAGE.md 2.4 records the table).
"""
import copy

import pytest
import torch

from pytorch_mnist_ddp_amd import inference
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

import refmodel as R
from refmodel import bf16_round
from test_gpu_backward_stages import BwdBox
from test_gpu_forward_stages import SENT, _report

pytestmark = pytest.mark.gpu

EPS, ALPHA, LO, HI = 0.1 / MNIST_STD, 0.04 / MNIST_STD, PIXEL_LO, PIXEL_HI     # test_gpu_attack.py's step


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32
                               else t.dtype)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class IgBox(BwdBox):
    """BwdBox (one spare record row behind ``dyc``) with a spare image behind ``a1`` as well: the padding images that
    _check poisons."""

    def __init__(self, dev, B, trained=True):
        super().__init__(dev, B, trained=trained)
        self.buf.a1 = torch.zeros(B + 1, 26, 26, 32, dtype=torch.bfloat16, device=dev)

    def chain(self):
        """The forward kernels and fc_bwd once: the records of the real chain (dropout on, step 3, rows by index)."""
        self.forward()
        Fk.fc_bwd(self.ms, self.buf, 1.0, None)
        torch.cuda.synchronize()
        return self

    def load_hand(self):
        h, buf, B = R.input_grad_hand_case(self.B), self.buf, self.B
        buf.dyc[:B].copy_(R.dyc_pack(h["g"], h["code"]))
        buf.a1[:B].copy_(h["a1"])
        return self

    def launch(self, grid=0):
        return lambda out: Fk.input_grad(self.ms, self.buf, out, grid=grid)


def _guarded(B, dev):
    """dx [B,784] as the contiguous head of a larger NaN-filled allocation: row B is the guard."""
    big = torch.full((B + 1, 784), float("nan"), device=dev)
    return big, big[:B]


def _run(launch, B, dev):
    big, out = _guarded(B, dev)
    launch(out)
    torch.cuda.synchronize()
    big = big.cpu()
    assert (_bits(big[B]) == R.IG_SENT_BITS).all(), "the guard row after dx was written"
    assert torch.isfinite(big[:B]).all(), "an element of dx was not written (or is not finite)"
    return big


def _check(stage, B, launch, ms, dyc, a1, hand=False):
    """One case, whole: ownership around the launch, then every element against the oracle.  ``dyc`` / ``a1``: the
    device buffers the launch reads, with at least one row past B."""
    dev = dyc.device
    assert dyc.shape[0] > B and a1.shape[0] > B
    dyc[B:].zero_()
    a1[B:].zero_()
    clean = _run(launch, B, dev)
    dyc[B:].fill_(0xFF)                                     # padding images: 0xFF records, NaN activations
    a1[B:].view(torch.int16).fill_(SENT)
    before = [t.cpu().clone() for t in (dyc, a1, ms.w2d, ms.param)]
    big = _run(launch, B, dev)
    again = _run(launch, B, dev)
    fresh = torch.empty(B, 784, device=dev)
    launch(fresh)
    torch.cuda.synchronize()
    for name, t, was in zip(("dyc", "a1", "w2d", "param"), (dyc, a1, ms.w2d, ms.param), before):
        assert _same(t.cpu(), was), f"{stage}: the launch wrote its operand {name}"
    assert _same(big, clean), f"{stage}: poisoned padding images changed dx"
    assert _same(again, big), f"{stage}: a second launch differs"
    assert _same(fresh.cpu(), big[:B]), f"{stage}: a launch into a fresh output differs"
    # the oracle, from what the kernel read
    d = {n: v.detach().cpu() for n, v in ms.views(ms.param).items()}
    w2q = bf16_round(d["conv2.weight"])
    assert torch.equal(ms.w2d.cpu().view(9, 32, 64), w2q.permute(2, 3, 1, 0).reshape(9, 32, 64))
    g, code = R.dyc_unpack(dyc[:B].cpu())
    dy, a1n = R.dense_dy(g, code), a1[:B].cpu().permute(0, 3, 1, 2).contiguous()
    _report(stage, B, R.check_input_grad(dy, w2q, a1n, d["conv1.weight"], big[:B], big[B], name=stage))
    if hand and B >= 5:
        dx = big[:B].view(B, 28, 28)
        assert (_bits(dx[R.IG_ZERO_IMAGE]) & 0x7FFFFFFF == 0).all(), f"{stage}: the all-zero image's dx is not +-0"
        assert torch.equal(dx[R.IG_CORNER_IMAGE] != 0, R.ig_support(11, 11)), f"{stage}: support of record (11, 11)"
        assert torch.equal(dx[R.IG_ORIGIN_IMAGE] != 0, R.ig_support(0, 0)), f"{stage}: support of record (0, 0)"
    return big


# ------------------------------------------------------------------ the real chain
@pytest.mark.parametrize("B", [1, 7, 33])
def test_input_grad_real_chain(cuda_device, B):
    bx = IgBox(cuda_device, B).chain()
    big = _check("input_grad chain", B, bx.launch(), bx.ms, bx.buf.dyc, bx.buf.a1)
    assert big[:B].abs().max() > 0


@pytest.mark.parametrize("rows", ["u8", "f32"])
def test_input_grad_grad_chain_form(cuda_device, rows):
    """What the Predictor loops launch: ``GradChain`` (trunk_fwd training form without dropout, fc_bwd role B alone) on
    an activation set of more rows than the launch, then its ``input_grad``."""
    B, dev = 33, cuda_device
    net = copy.deepcopy(R.trained_net()).to(dev).train()
    st = fused_state(net)
    st.sync()
    imgs, labels, _ = R.forward_case(B)
    if rows == "u8":                                        # the package's input path for uint8 images
        x = inference._rows_f32(imgs[:B].to(dev), B, dev)
        assert torch.equal(x.cpu(), normalize_u8(imgs[:B]).reshape(B, 784))
    else:                                                   # rows off the 256-value lattice
        gen = torch.Generator().manual_seed(B)
        x = (normalize_u8(imgs[:B]).reshape(B, 784) + 0.3 * torch.randn(B, 784, generator=gen)).to(dev).contiguous()
    lab = labels[:B].to(dev, torch.int32).contiguous()
    chain = GradChain(st, B + 7)
    try:
        chain.run(x.data_ptr(), lab.data_ptr(), B)
        torch.cuda.synchronize()
        buf = chain._buf
        big = _check(f"input_grad GradChain {rows}", B, lambda out: chain.input_grad(out.data_ptr(), B), st.ms,
                     buf.dyc, buf.a1)
        assert big[:B].abs().max() > 0
    finally:
        chain.release()


# ------------------------------------------------------------------ hand-made operands
@pytest.mark.parametrize("B", [1, 2, 5, 33])
def test_input_grad_hand_made(cuda_device, B):
    bx = IgBox(cuda_device, B).load_hand()
    _check("input_grad hand", B, bx.launch(), bx.ms, bx.buf.dyc, bx.buf.a1, hand=True)


def test_input_grad_round_boundary(cuda_device):
    """The first batch size whose items exceed the cap of two workgroups per CU (129 on 256 CUs: 516 items, 258
    workgroups, two rounds): on the planned grid every workgroup runs the persistent loop twice."""
    C = native.load()
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    B = 2 * cus // 4 + 1
    plan, below = C.input_grad_plan(B, cus), C.input_grad_plan(B - 1, cus)
    assert below["rounds"] == 1 and below["grid"] == below["items"] == 4 * (B - 1)
    assert plan["rounds"] == 2 and plan["items"] == 4 * B and plan["grid"] == 2 * B
    bx = IgBox(cuda_device, B).load_hand()
    _check("input_grad two rounds", B, bx.launch(), bx.ms, bx.buf.dyc, bx.buf.a1, hand=True)


def test_input_grad_any_grid(cuda_device):
    """B = 33, 132 items: grids 1 and 3 make one workgroup walk every strip of consecutive images and every
    strip-to-strip transition through the aliased LDS tile; 3 and 5 are coprime to the 4 strips; 37 and 131 leave
    ragged last rounds.  Each equals the planned launch (held to the oracle) bit for bit."""
    B, dev = 33, cuda_device
    bx = IgBox(dev, B).load_hand()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert native.load().input_grad_plan(B, cus)["grid"] == 132 or cus < 66
    planned = _check("input_grad grid plan", B, bx.launch(), bx.ms, bx.buf.dyc, bx.buf.a1, hand=True)
    for grid in (1, 3, 5, 37, 131, 132, 100000):            # (at or above the plan: the plan)
        got = _run(bx.launch(grid), B, dev)
        assert _same(got, planned), f"grid {grid} differs from the planned grid"


# ------------------------------------------------------------------ the step form
def _formula(x, x0, dx, alpha, eps, lo=LO, hi=HI):
    """test_gpu_attack.py's torch formula of the projected step."""
    t = x + alpha * torch.sign(dx)
    t = torch.min(torch.max(t, x0 - eps), x0 + eps)
    return torch.clamp(t, lo, hi)


@pytest.mark.parametrize("grid", [0, 1])
def test_input_grad_step_form(cuda_device, grid):
    B, dev = 5, cuda_device
    bx = IgBox(dev, B).load_hand()
    ms, buf = bx.ms, bx.buf
    plain = _run(bx.launch(), B, dev)[:B].to(dev)
    gen = torch.Generator().manual_seed(B)
    x0 = normalize_u8(R.forward_case(B)[0][:B]).reshape(B, 784).to(dev)
    x = (x0 + ((2 * torch.rand(B, 784, generator=gen) - 1) * 0.9 * EPS).to(dev)).clamp(LO, HI)
    x_before = x.clone()
    want = _formula(x, x0, plain, ALPHA, EPS)
    assert torch.equal(want[R.IG_ZERO_IMAGE], x[R.IG_ZERO_IMAGE]) and not torch.equal(want, x)
    big, dx = _guarded(B, dev)
    out = Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI, dx=dx, grid=grid)
    torch.cuda.synchronize()
    assert _same(big[:B], plain) and (_bits(big[B]) == R.IG_SENT_BITS).all()      # the stored dx, its guard row
    assert _same(out, want) and _same(x, x_before) and out.data_ptr() != x.data_ptr()
    xi = x.clone()                                          # in place
    assert Fk.input_grad_step(ms, buf, xi, x0, EPS, ALPHA, LO, HI, out=xi, grid=grid).data_ptr() == xi.data_ptr()
    assert _same(xi, want)
    big.fill_(float("nan"))                                 # no dx asked for: the buffer of the launch before stays
    out = Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI, grid=grid)
    torch.cuda.synchronize()
    assert _same(out, want) and (_bits(big) == R.IG_SENT_BITS).all()
    assert _same(_run(bx.launch(grid), B, dev)[:B].to(dev), plain)                 # the plain form after the step form


# ------------------------------------------------------------------ refusals
def test_input_grad_grid_refusals(cuda_device):
    B, dev = 2, cuda_device
    bx = IgBox(dev, B).load_hand()
    ms, buf = bx.ms, bx.buf
    x = torch.zeros(B, 784, device=dev)
    sent = torch.full((B, 784), float("nan"), device=dev)
    with pytest.raises(ValueError, match="grid"):
        Fk.input_grad(ms, buf, sent, grid=-1)
    with pytest.raises(ValueError, match="grid"):
        Fk.input_grad_step(ms, buf, x, x.clone(), EPS, ALPHA, LO, HI, out=sent, grid=-1)
    with pytest.raises(ValueError, match="grid"):           # the binding's own check, under the wrapper's
        native.load().input_grad(sent.data_ptr(), sent.data_ptr(), sent.data_ptr(), sent.data_ptr(), sent.data_ptr(),
                                 B, native.stream_handle(), grid=-1)
    for bad in (torch.empty(B, 783, device=dev), torch.empty(B + 1, 784, device=dev),
                torch.empty(B, 784, device=dev, dtype=torch.float64), torch.empty(784, B, device=dev).t()):
        with pytest.raises(ValueError, match="out must be"):
            Fk.input_grad(ms, buf, bad, grid=3)
        with pytest.raises(ValueError, match="out must be"):
            Fk.input_grad_step(ms, buf, x, x.clone(), EPS, ALPHA, LO, HI, out=bad, grid=3)
    torch.cuda.synchronize()
    assert (_bits(sent) == R.IG_SENT_BITS).all()            # nothing was launched
