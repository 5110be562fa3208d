"""L-inf FGSM / PGD on the GPU: the step form of the input-gradient kernel (csrc/kernels/input_grad.hip),
the native loop ``ops.attack.fused_adversarial``, ``Predictor.adversarial`` / ``robust_evaluate`` and the
``mnist_predict.py --attack-eps`` line.

The step epilogue is elementwise fp32 arithmetic on the sum ``input_grad`` stores, so its oracle is that
formula in torch fp32 ops on the GPU from ``input_grad``'s own output, and the bound is equality of bits.
"""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor, adversarial_line
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.attack import fused_adversarial
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = PIXEL_LO, PIXEL_HI
EPS, ALPHA = 0.1 / MNIST_STD, 0.04 / MNIST_STD


def formula(x, x0, dx, alpha, eps, lo=LO, hi=HI):
    t = x + alpha * torch.sign(dx)
    t = torch.min(torch.max(t, x0 - eps), x0 + eps)
    return torch.clamp(t, lo, hi)


# B = 1: 4 items, fewer than the grid; 3: odd, several images; 65: no multiple of anything; 200: 800 items
# on 400 workgroups, the second round of the persistent loop
@pytest.mark.parametrize("B", [1, 3, 65, 200])
def test_input_grad_step_kernel_bitwise(cuda_device, B):
    dev = cuda_device
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(B, seed=5)
    ms = ModelState(net, dev)
    u8 = imgs.reshape(B, -1).contiguous().to(dev)
    lab = labels.to(torch.int32).to(dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    buf = Fk.StepBuffers.allocate(B, dev)
    ms.set_state(0, seed=9, rng_base=0)
    Fk.train_step(ms, u8, lab, idx, buf, update=False)
    dx = Fk.input_grad(ms, buf).clone()
    assert torch.isfinite(dx).all() and (dx != 0).any()
    gen = torch.Generator().manual_seed(B)
    x0 = normalize_u8(imgs).reshape(B, 784).to(dev)
    x = (x0 + ((2 * torch.rand(B, 784, generator=gen) - 1) * 0.9 * EPS).to(dev)).clamp(LO, HI)
    x_before = x.clone()

    # own output buffer, optional gradient output
    dx2 = torch.full((B, 784), float("nan"), device=dev)
    out = Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI, dx=dx2)
    want = formula(x, x0, dx, ALPHA, EPS)
    assert out.shape == (B, 784) and out.dtype == torch.float32 and out.data_ptr() != x.data_ptr()
    assert torch.equal(out, want) and torch.equal(dx2, dx)
    assert torch.equal(x, x_before) and not torch.equal(out, x)
    # a given buffer, no gradient output; then in place
    out2 = torch.full((B, 784), float("nan"), device=dev)
    assert Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI, out=out2).data_ptr() == out2.data_ptr()
    assert torch.equal(out2, want)
    xi = x.clone()
    Fk.input_grad_step(ms, buf, xi, x0, EPS, ALPHA, LO, HI, out=xi)
    assert torch.equal(xi, want)
    # the eps clamp binds wherever the gradient is not zero
    tiny = 1e-3 * EPS
    out = Fk.input_grad_step(ms, buf, x0, x0, tiny, ALPHA, -1e9, 1e9)
    assert torch.equal(out, formula(x0, x0, dx, ALPHA, tiny, -1e9, 1e9))
    nz = dx != 0
    assert torch.equal(out[nz], torch.where(dx > 0, x0 + tiny, x0 - tiny)[nz])
    # the range clamp binds: the ball's centre on the lower / upper end of the range
    for edge, toward in ((LO, dx < 0), (HI, dx > 0)):
        xe = torch.full((B, 784), edge, device=dev)
        out = Fk.input_grad_step(ms, buf, xe, xe, EPS, ALPHA, LO, HI)
        assert torch.equal(out, formula(xe, xe, dx, ALPHA, EPS))
        assert (out >= LO).all() and (out <= HI).all() and toward.any()
        assert (out[toward] == edge).all() and (out[~toward & nz] != edge).all()
    # the plain form gives the same bits after the step form ran on the same buffers
    assert torch.equal(Fk.input_grad(ms, buf), dx)
    # gradient exactly zero (the records of image 0 zeroed): x stays where it is there
    buf.dyc[0].zero_()
    dz = Fk.input_grad(ms, buf).clone()
    assert not dz[0].any() and torch.equal(dz[1:], dx[1:])
    out = Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI)
    assert torch.equal(out[0], x[0]) and torch.equal(out, formula(x, x0, dz, ALPHA, EPS))
    # validation of the functional wrapper
    for bad in (dict(out=x0), dict(dx=x), dict(out=x.double())):
        with pytest.raises(ValueError):
            Fk.input_grad_step(ms, buf, x, x0, EPS, ALPHA, LO, HI, **bad)
    with pytest.raises(ValueError):
        Fk.input_grad_step(ms, buf, x[:, :783], x0, EPS, ALPHA, LO, HI)
    with pytest.raises(ValueError):
        Fk.input_grad_step(ms, buf, x, x0, -1.0, ALPHA, LO, HI)


def _seeded(dev, B):
    torch.manual_seed(3)
    net = Net()
    imgs, labels = generate(B, seed=5)
    return net, copy.deepcopy(net).to(dev).train(), imgs, labels


def test_fused_adversarial_equals_hand_launched_steps(cuda_device):
    dev, B = cuda_device, 33
    _, net, imgs, labels = _seeded(dev, B)
    x_img = normalize_u8(imgs).to(dev)
    y = labels.long().to(dev)

    def train_pass():
        net.zero_grad(set_to_none=True)
        F.nll_loss(net(x_img), y).backward()
        return [p.grad.clone() for p in net.parameters()]

    st = fused_state(net)
    offset = st.rng_offset
    g_before = train_pass()                                  # default dropout: draws from the counter stream
    st.rng_offset = offset
    net.zero_grad(set_to_none=True)
    params = [p.detach().clone() for p in net.parameters()]

    # three iterations by hand, on a set from the pool: the same launches in the same order
    ms = st.ms
    st.sync()
    x0 = x_img.reshape(B, 784).clone()
    lab = y.to(torch.int32)
    state = torch.tensor([1 << 32, 0, 0], dtype=torch.int64).to(dev)   # step 0 | NO_DROPOUT, zero seed / counter
    buf = st.take(B, dev)
    x = x0.clone()
    for _ in range(3):
        Fk.trunk_fwd(ms, None, None, buf, True, state=state, xin=x)
        Fk.fc1_fwd(ms, buf)
        Fk.head_train(ms, lab, None, buf, state=state, inv_batch=1.0)
        Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=state)
        x = formula(x, x0, Fk.input_grad(ms, buf), ALPHA, EPS)
    st.give(buf)
    pooled = sum(len(v) for v in st.pool.values())

    got = fused_adversarial(net, x0, y, EPS, 3, ALPHA, LO, HI)
    assert got.shape == (B, 784) and got.data_ptr() != x0.data_ptr()
    assert torch.equal(got, x) and not torch.equal(got, x0)
    assert sum(len(v) for v in st.pool.values()) == pooled   # the set was taken from the pool and given back
    assert torch.equal(x0, x_img.reshape(B, 784))            # the clean images are read, not written
    # a start of its own
    x_init = (x0 + 0.5 * EPS).clamp(LO, HI)
    got1 = fused_adversarial(net, x0, y, EPS, 1, ALPHA, LO, HI, x_init=x_init)
    assert not torch.equal(got1, fused_adversarial(net, x0, y, EPS, 1, ALPHA, LO, HI))
    assert (got1 >= x0 - EPS).all() and (got1 <= x0 + EPS).all()
    # nothing of the net moved
    assert st.rng_offset == offset and net.training
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), params))
    assert all(p.grad is None or not p.grad.any().item() for p in net.parameters())
    g_after = train_pass()                                   # the same counter offset: the same masks
    assert all(torch.equal(a, b) for a, b in zip(g_before, g_after))


def test_predictor_input_gradient_unchanged_by_attack(cuda_device):
    dev, B = cuda_device, 33
    _, net, imgs, labels = _seeded(dev, B)
    pr = Predictor(net)
    assert pr.native
    g0, lp0 = pr.input_gradient(imgs.to(dev), labels.to(dev))
    xa, lpa = pr.adversarial(imgs.to(dev), labels.to(dev), eps=0.1, steps=2)
    assert xa.shape == (B, 1, 28, 28) and xa.dtype == torch.float32 and xa.is_cuda and lpa.shape == (B, 10)
    assert not xa.requires_grad and not lpa.requires_grad
    assert torch.equal(lpa, pr.log_probs(xa))                # the predictor's own forward of x_adv
    g1, lp1 = pr.input_gradient(imgs.to(dev), labels.to(dev))
    assert torch.equal(g0, g1) and torch.equal(lp0, lp1)
    assert pr.net.training and (pr.net.dropout1.p, pr.net.dropout2.p) == (0.25, 0.5)
    assert all(p.grad is None or not p.grad.any().item() for p in pr.net.parameters())
    # labels None: the class predicted on the clean input
    xb, _ = pr.adversarial(imgs.to(dev), None, eps=0.1, steps=2)
    xc, _ = pr.adversarial(imgs.to(dev), pr.predict(imgs.to(dev)), eps=0.1, steps=2)
    assert torch.equal(xb, xc)
    # the same start from the same generator state, on any generator device
    gen = lambda: torch.Generator().manual_seed(7)
    r1, _ = pr.adversarial(imgs, labels, eps=0.1, steps=2, random_start=True, generator=gen())
    r2, _ = pr.adversarial(imgs, labels, eps=0.1, steps=2, random_start=True, generator=gen())
    assert torch.equal(r1, r2) and not torch.equal(r1, xa)
    with pytest.raises(ValueError):
        pr.adversarial(imgs, torch.full((B,), 10))


def test_gpu_attack_against_cpu_reference(cuda_device):
    """B = 64, the seeds of tests/test_attack_cpu.py.  Asserted: the bf16 GPU attack's images, judged by
    the fp32 CPU ``forward_reference``, lose more than the clean ones (mean NLL strictly above), and both
    box conditions hold exactly.  Measured and printed, not asserted (one seed; also in
    docs/PERF_NOTES.md): the ratio of the GPU attack's gain in mean NLL to the fp32 CPU attack's, and the
    share of pixels whose displacement ``x_adv - x0`` has the same sign under both.  On an MI355X:
    1 step  +0.1091 against +0.1092, ratio 0.9989, 98.45 % of the pixels agree;
    4 steps +0.1597 against +0.1589, ratio 1.0050, 78.80 % (whole displacement after diverging iterates)."""
    dev = cuda_device
    ref, net, imgs, labels = _seeded(dev, 64)
    cpu, gpu = Predictor(ref), Predictor(net)
    assert gpu.native and not cpu.native
    y = labels.long()
    x0 = normalize_u8(imgs)
    eps_n = 0.1 / MNIST_STD
    nll = lambda x: F.nll_loss(cpu.log_probs(x), y).item()
    clean = nll(x0)
    for steps in (1, 4):
        xg, _ = gpu.adversarial(imgs, labels, eps=0.1, steps=steps)
        xc, _ = cpu.adversarial(imgs, labels, eps=0.1, steps=steps)
        xg = xg.cpu()
        up_g, up_c = nll(xg) - clean, nll(xc) - clean
        agree = (torch.sign(xg - x0) == torch.sign(xc - x0)).float().mean().item()
        print(f"steps={steps} clean {clean:.4f} gpu +{up_g:.4f} cpu +{up_c:.4f} ratio {up_g / up_c:.4f} "
              f"sign agreement {agree:.4f}")
        assert up_g > 0 and up_c > 0
        assert (xg >= x0 - eps_n).all() and (xg <= x0 + eps_n).all()
        lo, hi = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten()
        assert (xg >= lo).all() and (xg <= hi).all()
    xg, _ = gpu.adversarial(imgs, labels, eps=0.0)
    assert torch.equal(xg.cpu(), x0)                         # eps = 0: the clean images, exactly


def test_robust_evaluate_gpu(cuda_device):
    dev = cuda_device
    _, net, imgs, labels = _seeded(dev, 64)
    pr = Predictor(net)
    one = pr.robust_evaluate(imgs, labels, 0.1, steps=2, batch_size=64)
    parts = pr.robust_evaluate(imgs, labels, 0.1, steps=2, batch_size=24)
    assert one[1:] == parts[1:] and one[2] == 64
    assert parts[0] == pytest.approx(one[0], rel=1e-5)
    # eps = 0: the clean images bit for bit through the same kernels (only the sum's order differs)
    clean, zero = pr.evaluate(imgs, labels), pr.robust_evaluate(imgs, labels, 0.0)
    assert zero[1:] == clean[1:]
    assert zero[0] == pytest.approx(clean[0], rel=1e-5)
    assert one[0] > clean[0]


def test_predict_cli_attack_line_on_gpu(cuda_device, tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic",
                        "--synthetic-test-size", "40", "--checkpoint", ckpt, "--batch-size", "24",
                        "--attack-eps", "0.1", "--attack-steps", "2", "--json-log", log],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    pr = Predictor.from_checkpoint(ckpt, device=cuda_device)
    images = data.device_images(cuda_device)
    loss, correct, n = pr.robust_evaluate(images, data.targets, 0.1, steps=2, batch_size=24)
    assert len(lines) == 2 and lines[0].startswith("Test set:")
    assert lines[1] == adversarial_line(0.1, 2, loss / n, correct, n)
    with open(log) as f:
        rec = json.loads(f.read())
    assert rec["device"].startswith("cuda")
    assert (rec["adv_eps"], rec["adv_steps"], rec["adv_correct"]) == (0.1, 2, correct)
    assert rec["adv_loss"] == pytest.approx(loss / n, rel=1e-6)
