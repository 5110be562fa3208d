"""L2 and targeted PGD on the GPU: the L2 step kernel (csrc/kernels/attack_step.hip), the native loop
``ops.attack.fused_adversarial(norm=, targeted=)``, ``Predictor.adversarial`` / ``robust_evaluate`` and the
``mnist_predict.py --attack-norm l2`` line.

The step kernel sums 784 squares twice in its own fixed order, so its oracle is the formula evaluated in
float64 on the same fp32 operands, and each element is held to EPS_MARGIN x the largest deviation of the
same formula in torch fp32 on the CPU from that oracle (the convention of test_gpu_forward_stages.py), not
below FLOOR_ULPS fp32 ulps of the largest output magnitude: an output element is the end of a chain of five
individually rounded fp32 operations (r g, + x, - x0, * scale, + x0) on values of that size.
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
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor, adversarial_line
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import attack as attack_mod
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.attack import fused_adversarial
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = PIXEL_LO, PIXEL_HI
EPS_MARGIN, FLOOR_ULPS = 8.0, 4.0
EPS, ALPHA = 2.0 / MNIST_STD, 0.8 / MNIST_STD               # normalised units (pixel units 2.0 and 0.8)
SENTINEL = -12345.0
FWD_LAUNCHES = ["trunk_fwd", "fc1_fwd", "head_train", "fc_bwd"]


def ball_slack(eps_n: float) -> float:
    """Upper bound of ||x_adv - x0||_2 (in float64) after the fp32 projection to radius eps_n; derived in
    tests/test_attack_l2_cpu.py ``ball_slack`` for ANY order of the 784-term sum, the kernel's tree included."""
    return eps_n * (1.0 + 4 * 2.0 ** -23 * (784 / 8 + 1)) + 28 * 2.0 ** -24 * max(abs(LO), abs(HI))


def oracle_and_eps(dx, x, x0, eps, alpha, lo, hi):
    """(float64 oracle [B,784], per-launch tolerance) from the CPU copies of the fp32 operands; rows with a
    NaN are left out of the tolerance (they are checked for NaN instead)."""
    dx, x, x0 = dx.cpu(), x.cpu(), x0.cpu()
    ref64 = Fk.pgd_l2_step_reference(dx.double(), x.double(), x0.double(), eps, alpha, lo, hi)
    ref32 = Fk.pgd_l2_step_reference(dx, x, x0, eps, alpha, lo, hi)
    ok = torch.isfinite(ref64).all(dim=1)
    dev32 = float((ref32[ok].double() - ref64[ok]).abs().max())
    _, e = torch.frexp(ref64[ok].abs().max())
    return ref64, max(EPS_MARGIN * dev32, FLOOR_ULPS * 2.0 ** (int(e) - 24)), ok


def check(out, ref64, eps, ok, what):
    dev = float((out.cpu().double() - ref64)[ok].abs().max())
    print(f"\n{what:<44} dev {dev:10.3e}  eps {eps:10.3e}", end="")
    assert dev <= eps, (what, dev, eps)                      # (a NaN deviation compares false)
    return dev


# B = 1: one workgroup; 33: odd, several; 257: more workgroups than CUs
@pytest.mark.parametrize("B", [1, 33, 257])
def test_pgd_l2_step_kernel_against_float64(cuda_device, B):
    dev = cuda_device
    gen = torch.Generator().manual_seed(100 + B)
    x0 = (torch.rand(B, 784, generator=gen) * (HI - LO) + LO).clamp(LO, HI)
    # displacement norms from 0.1 EPS to 1.5 EPS over the rows: the projection binds for some rows only
    d = torch.randn(B, 784, generator=gen)
    d *= (EPS * torch.linspace(0.1, 1.5, B).view(B, 1).flip(0)) / d.norm(dim=1, keepdim=True)
    x = (x0 + d).clamp(LO, HI)
    dx = torch.randn(B, 784, generator=gen) * torch.logspace(-6, 2, B).view(B, 1)     # gradient scales 1e-6 .. 1e2
    g_dx, g_x, g_x0 = dx.to(dev), x.to(dev), x0.to(dev)
    for alpha in (ALPHA, -ALPHA):
        ref64, eps, ok = oracle_and_eps(dx, x, x0, EPS, alpha, LO, HI)
        assert ok.all()
        out = torch.full((B + 1, 784), SENTINEL, device=dev)
        got = Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, alpha, LO, HI, out=out[:B])
        assert got.shape == (B, 784) and got.data_ptr() == out.data_ptr()
        check(got, ref64, eps, ok, f"pgd_l2_step B={B} alpha={alpha:+.3f}")
        assert (out[B] == SENTINEL).all()                    # nothing past row B - 1 is written
        assert (got >= LO).all() and (got <= HI).all()
        dist = (got.cpu().double() - x0.double()).norm(dim=1)
        assert (dist <= ball_slack(EPS)).all()
        if B > 1:                                            # both sides of the projection are in the batch
            t64 = x.double() + alpha * dx.double() / dx.double().norm(dim=1, keepdim=True)
            binds = (t64 - x0.double()).norm(dim=1) > EPS
            assert binds.any() and not binds.all()
        assert torch.equal(g_x, x.to(dev)) and torch.equal(g_x0, x0.to(dev)) and torch.equal(g_dx, dx.to(dev))
    fresh = Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, -ALPHA, LO, HI)        # allocates; the same bits again
    assert fresh.data_ptr() != out.data_ptr() and torch.equal(fresh, out[:B])


def test_pgd_l2_step_hand_made_rows(cuda_device):
    dev = cuda_device
    gen = torch.Generator().manual_seed(4)
    B = 8
    mid = 0.5 * (LO + HI)
    x0 = torch.full((B, 784), mid)
    x = x0.clone()
    dx = torch.randn(B, 784, generator=gen)
    unit = lambda v: v / v.norm()
    # 0: one step of length ALPHA from the centre, ALPHA < EPS: the projection does not bind
    # 1: x already 1.5 EPS away from x0 (inside the box): the projection binds
    x[1] = x0[1] + 1.5 * EPS * unit(torch.randn(784, generator=gen))
    # 2 / 3: the ball's centre on the lower / upper end of the range: the range clamp binds
    x0[2], x[2], x0[3], x[3] = LO, LO, HI, HI
    # 4: gradient exactly zero, x off the centre
    x[4] = x0[4] + 0.3 * EPS * unit(torch.randn(784, generator=gen))
    dx[4] = 0.0
    # 5: one NaN in the gradient
    dx[5, 700] = float("nan")
    # 6: a gradient too small to square in fp32 (sum of squares underflows to 0): the floor TINY holds, no Inf
    dx[6] = 1e-30 * torch.randn(784, generator=gen)
    # 7: as row 0 with a huge gradient
    dx[7] = 1e15 * dx[0]
    assert (x >= LO).all() and (x <= HI).all()
    g_dx, g_x, g_x0 = dx.to(dev), x.to(dev), x0.to(dev)
    ref64, eps, ok = oracle_and_eps(dx, x, x0, EPS, ALPHA, LO, HI)
    assert ok.tolist() == [True] * 5 + [False, True, True]

    out = torch.full((B + 1, 784), SENTINEL, device=dev)
    got = Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, ALPHA, LO, HI, out=out[:B])
    check(got, ref64, eps, ok, "hand-made rows, ascent")
    assert (out[B] == SENTINEL).all()
    c = got.cpu()
    dist = (c.double() - x0.double()).norm(dim=1)
    assert abs(float(dist[0]) - ALPHA) <= 1e-5 * ALPHA and dist[0] < 0.5 * EPS          # row 0: a free step
    assert abs(float(dist[1]) - EPS) <= 1e-5 * EPS and dist[1] <= ball_slack(EPS)       # row 1: on the sphere
    assert (c[2][dx[2] < 0] == LO).all() and (c[2][dx[2] > 0] > LO).all()               # row 2: held at lo
    assert (c[3][dx[3] > 0] == HI).all() and (c[3][dx[3] < 0] < HI).all()               # row 3: held at hi
    assert (c >= LO)[ok].all() and (c <= HI)[ok].all()
    # row 4: t = x exactly, the scale is 1: the projected x, bit for bit
    assert torch.isfinite(c[4]).all() and torch.equal(c[4], (x0[4] + (x[4] - x0[4])).clamp(LO, HI))
    # row 5: the NaN fills its own row and no other
    assert torch.isnan(c[5]).all() and torch.isfinite(c[ok]).all()
    assert torch.equal(c[6], x[6])                           # row 6: 1e-30 / TINY * ALPHA is below half an ulp of x
    # negative alpha: the descent step, row 0 mirrored through the centre
    ref64n, epsn, okn = oracle_and_eps(dx, x, x0, EPS, -ALPHA, LO, HI)
    down = Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, -ALPHA, LO, HI)
    check(down, ref64n, epsn, okn, "hand-made rows, descent")
    dn = down.cpu()
    assert ((c[0] - x[0]) * dx[0]).sum() > 0 and ((dn[0] - x[0]) * dx[0]).sum() < 0
    assert torch.isnan(dn[5]).all() and torch.equal(dn[4], c[4])
    # in place (x_next = x) gives the out-of-place bits; so does a second launch
    xi = g_x.clone()
    assert Fk.pgd_l2_step(g_dx, xi, g_x0, EPS, ALPHA, LO, HI, out=xi).data_ptr() == xi.data_ptr()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))           # bits: NaN rows included
    assert same(xi, got)
    assert same(Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, ALPHA, LO, HI), got)
    # eps = 0: the centre, exactly (NaN row aside)
    zero = Fk.pgd_l2_step(g_dx, g_x, g_x0, 0.0, ALPHA, LO, HI)
    assert torch.equal(zero[ok.to(dev)], g_x0[ok.to(dev)])
    # validation of the functional wrapper
    for bad in (dict(out=g_x0), dict(out=g_dx), dict(out=g_x.double())):
        with pytest.raises(ValueError):
            Fk.pgd_l2_step(g_dx, g_x, g_x0, EPS, ALPHA, LO, HI, **bad)
    with pytest.raises(ValueError):
        Fk.pgd_l2_step(g_dx, g_x[:, :783], g_x0, EPS, ALPHA, LO, HI)
    with pytest.raises(ValueError):
        Fk.pgd_l2_step(g_dx, g_x, g_x0, -1.0, ALPHA, LO, HI)
    with pytest.raises(ValueError):
        Fk.pgd_l2_step(g_dx[:4], g_x, g_x0, EPS, ALPHA, LO, HI)


def _seeded(dev, B):
    torch.manual_seed(3)
    net = Net()
    imgs, labels = generate(B, seed=5)
    return net, copy.deepcopy(net).to(dev).train(), imgs, labels


class _Recorder:
    """The native module with every call's name noted."""

    def __init__(self, C):
        self._C, self.calls = C, []

    def __getattr__(self, name):
        v = getattr(self._C, name)
        if not callable(v):
            return v

        def call(*a, **k):
            self.calls.append(name)
            return v(*a, **k)
        return call


def test_fused_adversarial_l2_and_targeted_equal_hand_launched_steps(cuda_device, monkeypatch):
    dev, B = cuda_device, 33
    _, net, imgs, labels = _seeded(dev, B)
    x0 = normalize_u8(imgs).reshape(B, 784).to(dev)
    y = labels.long().to(dev)
    tgt = (y + 3) % 10
    st = fused_state(net)
    offset = st.rng_offset
    params = [p.detach().clone() for p in net.parameters()]
    grads = [None if p.grad is None else p.grad.clone() for p in net.parameters()]
    ms = st.ms
    st.sync()
    state = torch.tensor([1 << 32, 0, 0], dtype=torch.int64).to(dev)   # step 0 | NO_DROPOUT, zero seed / counter
    eps_inf, alpha_inf = 0.1 / MNIST_STD, 0.04 / MNIST_STD

    def by_hand(lab, step):
        buf = st.take(B, dev)
        x = x0.clone()
        dx = torch.empty(B, 784, device=dev)
        for _ in range(3):
            Fk.trunk_fwd(ms, None, None, buf, True, state=state, xin=x)
            Fk.fc1_fwd(ms, buf)
            Fk.head_train(ms, lab.to(torch.int32), None, buf, state=state, inv_batch=1.0)
            Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=state)
            step(buf, x, dx)
        st.give(buf)
        return x

    def l2(alpha):
        def step(buf, x, dx):
            Fk.input_grad(ms, buf, out=dx)
            Fk.pgd_l2_step(dx, x, x0, EPS, alpha, LO, HI, out=x)
        return step

    def linf(buf, x, dx):
        Fk.input_grad_step(ms, buf, x, x0, eps_inf, alpha_inf, LO, HI, out=x)

    def linf_down(buf, x, dx):                               # the descent step in torch ops from the plain form
        t = x - alpha_inf * torch.sign(Fk.input_grad(ms, buf, out=dx))
        x.copy_(torch.min(torch.max(t, x0 - eps_inf), x0 + eps_inf).clamp(LO, HI))

    want = {"l2": by_hand(y, l2(ALPHA)), "l2t": by_hand(tgt, l2(-ALPHA)), "linf": by_hand(y, linf),
            "linft": by_hand(tgt, linf_down)}
    pooled = sum(len(v) for v in st.pool.values())

    rec = _Recorder(attack_mod.native.load())
    monkeypatch.setattr(attack_mod.native, "load", lambda *a, **k: rec)

    def native_loop(lab, eps, alpha, launches, **kw):
        rec.calls.clear()
        got = fused_adversarial(net, x0, lab, eps, 3, alpha, LO, HI, **kw)
        assert rec.calls == launches * 3, rec.calls          # exactly these launches, nothing else of the extension
        assert got.shape == (B, 784) and got.data_ptr() != x0.data_ptr() and not torch.equal(got, x0)
        assert sum(len(v) for v in st.pool.values()) == pooled   # the set was taken from the pool and given back
        return got

    l2_launches = FWD_LAUNCHES + ["input_grad", "pgd_l2_step"]
    linf_launches = FWD_LAUNCHES + ["input_grad_step"]
    assert torch.equal(native_loop(y, EPS, ALPHA, l2_launches, norm="l2"), want["l2"])
    assert torch.equal(native_loop(tgt, EPS, ALPHA, l2_launches, norm="l2", targeted=True), want["l2t"])
    assert not torch.equal(want["l2"], want["l2t"])
    # the L-inf untargeted call: today's result and today's five launches, with and without the new keywords
    assert torch.equal(native_loop(y, eps_inf, alpha_inf, linf_launches), want["linf"])
    assert torch.equal(native_loop(y, eps_inf, alpha_inf, linf_launches, norm="linf", targeted=False), want["linf"])
    assert torch.equal(native_loop(tgt, eps_inf, alpha_inf, linf_launches, targeted=True), want["linft"])
    # a start of its own, inside the ball
    x_init = (x0 + 0.01).clamp(LO, HI)
    got1 = fused_adversarial(net, x0, y, EPS, 1, ALPHA, LO, HI, x_init=x_init, norm="l2")
    assert not torch.equal(got1, fused_adversarial(net, x0, y, EPS, 1, ALPHA, LO, HI, norm="l2"))
    assert ((got1 - x0).double().norm(dim=1) <= ball_slack(EPS)).all()
    with pytest.raises(ValueError):
        fused_adversarial(net, x0, y, EPS, 1, ALPHA, LO, HI, norm="l1")
    # nothing of the net moved
    assert torch.equal(x0, normalize_u8(imgs).reshape(B, 784).to(dev))
    assert st.rng_offset == offset and net.training and (net.dropout1.p, net.dropout2.p) == (0.25, 0.5)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), params))
    assert all((p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
               for p, g in zip(net.parameters(), grads))
    assert all(p.grad is None or not p.grad.any().item() for p in net.parameters())


def test_gpu_l2_attack_against_cpu_reference(cuda_device):
    """B = 64, the seeds of tests/test_attack_l2_cpu.py, eps = 2.0 in pixel units.  Asserted, as
    ``test_gpu_attack.py::test_gpu_attack_against_cpu_reference`` asserts for L-inf: the bf16 GPU attack's
    images, judged by the fp32 CPU ``forward_reference``, lose more than the clean ones (gain in mean NLL
    strictly above zero, for the GPU and the CPU attack), the ball (``ball_slack``) and the box hold; the
    targeted attack lowers the target's mean NLL.  Measured and printed, not asserted (one seed; also in
    docs/COVERAGE.md): the ratio of the GPU attack's gain to the fp32 CPU attack's."""
    dev = cuda_device
    ref, net, imgs, labels = _seeded(dev, 64)
    cpu, gpu = Predictor(ref), Predictor(net)
    assert gpu.native and not cpu.native
    y = labels.long()
    tgt = (y + 3) % 10
    x0 = normalize_u8(imgs)
    eps_n = 2.0 / MNIST_STD
    nll = lambda x, t: F.nll_loss(cpu.log_probs(x), t).item()
    clean, tclean = nll(x0, y), nll(x0, tgt)
    lo, hi = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten()
    for steps in (1, 3):
        for targeted, lab, base in ((False, labels, clean), (True, tgt, tclean)):
            xg, lpg = gpu.adversarial(imgs, lab, eps=2.0, steps=steps, norm="l2", targeted=targeted)
            xc, _ = cpu.adversarial(imgs, lab, eps=2.0, steps=steps, norm="l2", targeted=targeted)
            assert xg.is_cuda and xg.shape == (64, 1, 28, 28) and torch.equal(lpg, gpu.log_probs(xg))
            xg = xg.cpu()
            up_g, up_c = nll(xg, lab.long()) - base, nll(xc, lab.long()) - base
            print(f"\nsteps={steps} targeted={targeted} clean {base:.4f} gpu {up_g:+.4f} cpu {up_c:+.4f} "
                  f"ratio {up_g / up_c:.4f}", end="")
            if targeted:
                assert up_g < 0 and up_c < 0
            else:
                assert up_g > 0 and up_c > 0
            dist = (xg.double() - x0.double()).reshape(64, 784).norm(dim=1)
            assert (dist <= ball_slack(eps_n)).all() and (dist > 0).all()
            assert (xg >= lo).all() and (xg <= hi).all()
    xg, _ = gpu.adversarial(imgs, labels, eps=0.0, norm="l2")
    assert torch.equal(xg.cpu(), x0)                         # eps = 0: the clean images, exactly
    # the same start from the same generator state, on any generator device; inside the ball and the box
    gen = lambda: torch.Generator().manual_seed(7)
    r1, _ = gpu.adversarial(imgs, labels, eps=2.0, steps=2, random_start=True, generator=gen(), norm="l2")
    r2, _ = gpu.adversarial(imgs, labels, eps=2.0, steps=2, random_start=True, generator=gen(), norm="l2")
    plain, _ = gpu.adversarial(imgs, labels, eps=2.0, steps=2, norm="l2")
    assert torch.equal(r1, r2) and not torch.equal(r1, plain)
    assert ((r1.cpu().double() - x0.double()).reshape(64, 784).norm(dim=1) <= ball_slack(eps_n)).all()
    for kw in (dict(norm="l1"), dict(norm="l2", targeted=True)):
        with pytest.raises(ValueError):
            gpu.adversarial(imgs, None, **kw)


def test_robust_evaluate_l2_gpu(cuda_device):
    dev = cuda_device
    _, net, imgs, labels = _seeded(dev, 64)
    pr = Predictor(net)
    one = pr.robust_evaluate(imgs, labels, 2.0, steps=2, batch_size=64, norm="l2")
    parts = pr.robust_evaluate(imgs, labels, 2.0, steps=2, batch_size=24, norm="l2")
    assert one[1:] == parts[1:] and one[2] == 64
    assert parts[0] == pytest.approx(one[0], rel=1e-5)
    clean, zero = pr.evaluate(imgs, labels), pr.robust_evaluate(imgs, labels, 0.0, norm="l2")
    assert zero[1:] == clean[1:]
    assert zero[0] == pytest.approx(clean[0], rel=1e-5)
    assert one[0] > clean[0]
    assert one != pr.robust_evaluate(imgs, labels, 2.0, steps=2, batch_size=64)          # the default is L-inf


def test_predict_cli_l2_line_on_gpu(cuda_device, tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic",
                        "--synthetic-test-size", "40", "--checkpoint", ckpt, "--batch-size", "24",
                        "--attack-eps", "1.5", "--attack-steps", "2", "--attack-norm", "l2", "--json-log", log],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    pr = Predictor.from_checkpoint(ckpt, device=cuda_device)
    images = data.device_images(cuda_device)
    loss, correct, n = pr.robust_evaluate(images, data.targets, 1.5, steps=2, batch_size=24, norm="l2")
    assert len(lines) == 2 and lines[0].startswith("Test set:")
    assert lines[1] == adversarial_line(1.5, 2, loss / n, correct, n, "l2")
    assert lines[1].startswith("Adversarial set (L2 eps=1.5, steps=2): ")
    with open(log) as f:
        rec = json.loads(f.read())
    assert rec["device"].startswith("cuda")
    assert (rec["adv_eps"], rec["adv_steps"], rec["adv_correct"], rec["adv_norm"]) == (1.5, 2, correct, "l2")
    assert rec["adv_loss"] == pytest.approx(loss / n, rel=1e-6)
