"""The input-gradient kernel (csrc/kernels/input_grad.hip), ``x.grad`` through the fused GPU ``Net`` and
``Predictor.input_gradient`` on the GPU.

The kernel keeps da1 in fp32 from the MFMA accumulators to the last fma (no bf16 rounding), so the
stage-wise oracle is the plain float64 one and the bound is the project's figure for fp32
accumulation over bf16 operands (1e-4, the conv2 weight gradient line of
``test_backward_kernels_stagewise_exact``).  The end-to-end bound against the fp32 CPU gradient is the
module path's existing bf16-vs-fp32 one (0.1, ``test_module_forward_backward_matches_cpu_reference``).

Predictor cases: the net of ``test_gpu_infer`` (seeded ``Net()`` after 32 seeded Adadelta steps on the
CPU, rebuilt here) on ``generate(B, seed=5)``.  Checked on the CPU reference: at B = 33 one row of 33
(3 %) is under the 0.1 top-2 margin; the single row of ``generate(1, seed=5)`` has a margin of 0.85, so
the B = 1 case uses it as it is.  Both facts are asserted again below on the reference itself.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
import torch.nn.grad as G

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

from refmodel import rel_err

pytestmark = pytest.mark.gpu

MARGIN = 0.1


def _ring(t):
    """Rows and columns 0, 1, 26, 27 of [B,1,28,28]: the pixels few taps reach."""
    m = torch.zeros(28, 28, dtype=torch.bool)
    m[[0, 1, 26, 27], :] = True
    m[:, [0, 1, 26, 27]] = True
    return t[..., m]


# B = 1: every strip and border of one image; 7: odd, several images; 65: past a group of 64; 200: 800
# items on a 2-round persistent grid (input_grad_plan: more than one item per workgroup)
@pytest.mark.parametrize("B", [1, 7, 65, 200])
def test_input_grad_kernel_stagewise(cuda_device, B):
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(B, seed=5)
    ms = ModelState(net, cuda_device)
    u8 = imgs.reshape(B, -1).contiguous().to(cuda_device)
    lab = labels.to(torch.int32).to(cuda_device)
    idx = torch.arange(B, dtype=torch.int32, device=cuda_device)
    buf = Fk.StepBuffers.allocate(B, cuda_device)
    ms.set_state(0, seed=9, rng_base=0)                     # dropout on
    Fk.train_step(ms, u8, lab, idx, buf, update=False)
    out = torch.full((B, 784), float("nan"), device=cuda_device)
    got = Fk.input_grad(ms, buf, out)
    again = Fk.input_grad(ms, buf)                          # its own (uninitialised) output buffer
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (B, 784) and got.dtype == torch.float32
    assert torch.isfinite(got).all()                        # every element was written
    assert torch.equal(got, again)                          # run to run
    # float64 oracle from what the kernel read
    d = {n: v.detach().cpu().double() for n, v in ms.views(ms.param).items()}
    q = lambda t: t.float().to(torch.bfloat16).double()
    dy = Fk.dense_dy(buf).cpu().double().permute(0, 3, 1, 2)
    a1 = buf.a1.cpu().double().permute(0, 3, 1, 2)
    assert torch.equal(ms.w2d.cpu().view(9, 32, 64).double(),
                       q(d["conv2.weight"]).permute(2, 3, 1, 0).reshape(9, 32, 64))
    da1 = G.conv2d_input(a1.shape, q(d["conv2.weight"]), dy) * (a1 > 0)
    want = G.conv2d_input((B, 1, 28, 28), d["conv1.weight"], da1)
    got = got.cpu().view(B, 1, 28, 28)
    e_all, e_ring = rel_err(got, want), rel_err(_ring(got), _ring(want))
    print(f"B={B} rel_err={e_all:.3e} ring={e_ring:.3e} |dx|={want.norm():.3e} |ring|={_ring(want).norm():.3e}")
    assert want.norm() > 0 and _ring(want).norm() > 0
    assert e_all < 1e-4, e_all
    assert e_ring < 1e-4, e_ring


def _seeded_pair(dev, dropout):
    torch.manual_seed(1)
    net = Net()
    ref = copy.deepcopy(net)
    net = net.to(dev)
    for m in (net, ref):
        m.dropout1.p, m.dropout2.p = dropout
    imgs, lab = generate(64, seed=5)
    return net.train(), ref.train(), normalize_u8(imgs), lab.long()


@pytest.mark.parametrize("shape", [(64, 1, 28, 28), (64, 784)])
def test_autograd_input_gradient_matches_cpu(cuda_device, shape):
    net, ref, x_cpu, y = _seeded_pair(cuda_device, (0.0, 0.0))
    # the same pass with an input that needs no gradient: the parameter gradients to compare with
    F.nll_loss(net(x_cpu.reshape(shape).to(cuda_device)), y.to(cuda_device)).backward()
    plain = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    x = x_cpu.reshape(shape).to(cuda_device).requires_grad_()
    F.nll_loss(net(x), y.to(cuda_device)).backward()
    assert x.grad is not None
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.device == x.device
    assert torch.isfinite(x.grad).all()
    xr = x_cpu.reshape(shape).clone().requires_grad_()
    F.nll_loss(ref(xr.reshape(64, 1, 28, 28)), y).backward()
    err = rel_err(x.grad, xr.grad)
    print(f"shape={shape} rel_err(x.grad)={err:.4f}")
    assert err < 0.1, err
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, plain[n]), n


def test_autograd_input_gradient_with_default_dropout(cuda_device):
    net, _, x_cpu, y = _seeded_pair(cuda_device, (0.25, 0.5))
    st = None
    for _ in range(2):                                      # the second pass refills the first one's buffers
        x = x_cpu.to(cuda_device).requires_grad_()
        F.nll_loss(net(x), y.to(cuda_device)).backward()
        assert torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0
        st = fused_state(net)
        assert [len(v) for v in st.pool.values()] == [1]    # handed back once, reused by the next pass


@functools.lru_cache(maxsize=None)
def _trained_net():
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(1024, seed=11)
    x, y = normalize_u8(imgs), labels.long()
    opt = torch.optim.Adadelta(net.parameters(), lr=1.0)
    net.train()
    with torch.enable_grad():
        for step in range(32):
            i = (step * 64) % 1024
            opt.zero_grad()
            F.nll_loss(net.forward_reference(x[i:i + 64]), y[i:i + 64]).backward()
            opt.step()
    net.zero_grad(set_to_none=True)
    return net.eval()


@functools.lru_cache(maxsize=None)
def _predictor_case(B, with_labels):
    """Images, labels and the CPU Predictor's (grad, log-probs): computed once, never modified."""
    imgs, labels = generate(B, seed=5)
    g, lp = Predictor(_trained_net()).input_gradient(imgs, labels if with_labels else None)
    return imgs, labels, g, lp


@pytest.fixture(scope="module")
def gpu_predictor(cuda_device):
    return Predictor(copy.deepcopy(_trained_net()).to(cuda_device).train())   # train mode: must not matter


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("form", ["u8", "float"])
@pytest.mark.parametrize("B", [1, 33])
def test_predictor_input_gradient_matches_cpu_predictor(cuda_device, gpu_predictor, B, form, with_labels):
    imgs, labels, g_ref, lp_ref = _predictor_case(B, with_labels)
    pr = gpu_predictor
    assert pr.native
    x = imgs.to(cuda_device) if form == "u8" else normalize_u8(imgs).to(cuda_device)
    g, lp = pr.input_gradient(x, labels.to(cuda_device) if with_labels else None)
    assert g.shape == (B, 1, 28, 28) and g.dtype == torch.float32 and g.is_cuda and lp.shape == (B, 10)
    assert torch.isfinite(g).all() and not g.requires_grad and not lp.requires_grad
    assert (lp - pr.log_probs(x)).abs().max().item() < 5e-2
    assert (lp.cpu() - lp_ref).abs().max().item() < 5e-2
    assert pr.net.training and (pr.net.dropout1.p, pr.net.dropout2.p) == (0.25, 0.5)
    # nothing accumulates into the parameters' gradients (on the GPU they are views of the flat, zeroed buffer)
    assert all(p.grad is None or not p.grad.any().item() for p in pr.net.parameters())
    rows = torch.ones(B, dtype=torch.bool)
    if not with_labels:                                     # the predicted class: clear rows only
        top2 = lp_ref.topk(2, dim=1).values
        rows = (top2[:, 0] - top2[:, 1]) > MARGIN
        assert (~rows).float().mean().item() <= 0.10
        assert torch.equal(lp.cpu().argmax(1)[rows], lp_ref.argmax(1)[rows])
    err = rel_err(g.cpu()[rows], g_ref[rows])
    print(f"B={B} {form} labels={with_labels} rows={int(rows.sum())} rel_err(grad)={err:.4f}")
    assert g_ref[rows].norm() > 0
    assert err < 0.1, err
