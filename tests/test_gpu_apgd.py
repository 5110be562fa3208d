"""Auto-PGD on the GPU: the step kernel (csrc/kernels/apgd.hip) against the per-image oracle of tests/apgd_ref.py,
the native loop ``ops.apgd.fused_auto_pgd`` against its launches made by hand and under chunkings,
``Predictor.auto_pgd`` against the CPU reference and the ``mnist_predict.py --apgd-eps`` line.

First measured on the MI355X against ``reference_auto_pgd`` (docs/COVERAGE.md), 64 images, 20 steps: linf eps 0.1 -
mean loss_best ratio GPU / CPU 1.0001 (2.0504 / 2.0502), found 40 / 40, no image differs; l2 eps 1.5 - ratio 1.0005
(2.3159 / 2.3146), found 44 / 44, no image differs.  Each is held at twice its first deviation, not below the floors
(ratio 0.05, count 2): bf16 forwards flip near-ties, the margin absorbs that and nothing more."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import apgd_ref as R
from attr_ref import trained_net
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, reference_auto_pgd
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.apgd import fused_auto_pgd
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = R.LO, R.HI
SENTINEL, ISENTINEL = -12345.0, -77
# first deviations (docs/COVERAGE.md): ratio 0.0001 (linf) and 0.0005 (l2), images whose found differs 0 and 0
RATIO_MARGIN = max(2 * 0.0005, 0.05)
FOUND_MARGIN = max(2 * 0, 2)
LAUNCHES = [dict(first=True), dict(), dict(window=R.WINDOW), dict(last=True, window=R.WINDOW)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(case, dev, M, **kw):
    """One ``apgd_step`` on sentinel-filled buffers of M + 1 images: (outputs of the M images as numpy, guards ok)."""
    def rows(key):
        t = torch.full((M + 1, 784), SENTINEL, device=dev)
        t[:M] = case[key].to(dev)
        return t
    dx, x0, x, x_old, x_best, g_best = (rows(k) for k in ("dx", "x0", "x", "x_old", "x_best", "g_best"))
    if kw.get("first"):                                      # the first launch reads no state: give it sentinels
        for t in (x_old, x_best, g_best):
            t.fill_(SENTINEL)
    loss = torch.full((M + 1,), SENTINEL, device=dev)
    loss[:M] = case["loss_rows"].to(dev)
    fs = torch.full((M + 1, 4), SENTINEL, device=dev)
    ist = torch.full((M + 1, 4), ISENTINEL, dtype=torch.int32, device=dev)
    if not kw.get("first"):
        fs[:M], ist[:M] = case["fstate"].to(dev), case["istate"].to(dev)
    before = (dx.clone(), x0.clone(), loss.clone())
    Fk.apgd_step(dx, loss, x0, x, x_old, x_best, g_best, fs, ist, case["sign"], case["eps"], LO, HI, norm=case["norm"],
                 M=M, **kw)
    guards = all((t[M] == SENTINEL).all() for t in (x, x_old, x_best, g_best, fs)) and (ist[M] == ISENTINEL).all()
    inputs = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (dx, x0, loss)))
    return tuple(t[:M].cpu().numpy() for t in (x, x_old, x_best, g_best, fs, ist)), bool(guards) and inputs


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("M", [1, 3, 33])
def test_apgd_step_kernel_against_the_oracle(cuda_device, norm, M):
    n = 0
    for sign in (1, -1):
        for kw in LAUNCHES:
            n += 1
            case = R.make_case(norm, M, seed=100 * M + n, sign=sign)
            got, intact = _launch(case, cuda_device, M, **kw)
            assert intact, (sign, kw)                        # the guard image and the read-only operands
            if norm == "linf":                               # bitwise the per-operation float32 evaluation
                want, bound = R.step_oracle(case, norm, dtype=np.float32, **kw)
                assert R.mismatches(got, R.reference_step(case, torch.float32, **kw)) == []
            else:
                want, bound = R.step_oracle(case, norm, **kw)
            assert R.mismatches(got, want, bound) == [], (sign, kw)
            again, _ = _launch(case, cuda_device, M, **kw)   # the same inputs, the same bits
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))
            if kw.get("last"):                               # x and x_old do not move
                assert np.array_equal(got[0].view(np.int32), case["x"].numpy().view(np.int32))
                assert np.array_equal(got[1].view(np.int32), case["x_old"].numpy().view(np.int32))
    case = R.make_case(norm, M, seed=7, eps=0.0)             # eps = 0: the clean image
    got, intact = _launch(case, cuda_device, M, window=R.WINDOW)
    ok = ~np.isnan(got[0]).any(axis=1)
    assert intact and np.array_equal(got[0][ok], case["x0"].numpy()[ok])


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    case = R.make_case("linf", 4, seed=3)
    t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    keep = {k: v.clone() for k, v in t.items() if isinstance(v, torch.Tensor)}
    C, p, s = native.load(), native.ptr, native.stream_handle()
    ok = dict(dx=p(t["dx"]), loss_rows=p(t["loss_rows"]), x0=p(t["x0"]), x=p(t["x"]), x_old=p(t["x_old"]),
              x_best=p(t["x_best"]), g_best=p(t["g_best"]), fstate=p(t["fstate"]), istate=p(t["istate"]), sign=1.0,
              eps=0.1, lo=LO, hi=HI, l2=False, first=False, last=False, window=0, M=4, stream=s)
    for kw in (dict(M=0), dict(M=(1 << 20) + 1), dict(eps=-0.1), dict(sign=0.0), dict(x=ok["x"] + 4),
               dict(fstate=ok["fstate"] + 4), dict(x_best=0)):
        for l2 in (False, True):
            with pytest.raises(RuntimeError):
                C.apgd_step(**dict(ok, l2=l2, **kw))
    args = (t["dx"], t["loss_rows"], t["x0"], t["x"], t["x_old"], t["x_best"], t["g_best"], t["fstate"], t["istate"])
    for bad in (dict(eps=-1.0), dict(sign=0), dict(norm="l1"), dict(first=True, last=True), dict(M=5), dict(window=-1)):
        kw = dict(sign=1, eps=0.1, lo=LO, hi=HI)
        kw.update(bad)
        with pytest.raises(ValueError):
            Fk.apgd_step(*args, **kw)
    with pytest.raises(ValueError):                          # six buffers
        Fk.apgd_step(t["dx"], t["loss_rows"], t["x0"], t["x"], t["x"], t["x_best"], t["g_best"], t["fstate"],
                     t["istate"], 1, 0.1, LO, HI)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t[k]), _bits(v)) for k, v in keep.items())     # nothing ran


def _trained(dev):
    import copy
    return copy.deepcopy(trained_net()).to(dev)


def _images(dev, n=64):
    imgs, labels = generate(64, seed=5)
    return normalize_u8(imgs).reshape(64, 784)[:n].to(dev).contiguous(), labels[:n].long().to(dev)


@pytest.mark.parametrize("norm,eps", [("linf", 0.1 / MNIST_STD), ("l2", 1.5 / MNIST_STD)])
def test_fused_loop_equals_its_launches_by_hand(cuda_device, norm, eps):
    dev = cuda_device
    net = _trained(dev)
    x0, y = _images(dev, 8)
    steps = 6
    st = fused_state(net)
    st.sync()
    params = [(q.detach().clone(), q.grad) for q in net.parameters()]
    got = fused_auto_pgd(net, x0, y, eps, steps, LO, HI, norm=norm)
    chain = GradChain(st, 8)
    lab = y.to(torch.int32)
    x = x0.clone()
    dx, x_old, x_best, g_best = (torch.full((8, 784), SENTINEL, device=dev) for _ in range(4))
    fs, ist = torch.full((8, 4), SENTINEL, device=dev), torch.full((8, 4), ISENTINEL, dtype=torch.int32, device=dev)
    loss_rows = chain._buf.loss_rows
    window = dict(Fk.apgd_checkpoints(steps))
    for j in range(steps + 1):
        chain.run(native.ptr(x), native.ptr(lab), 8)
        chain.input_grad(native.ptr(dx), 8)
        Fk.apgd_step(dx, loss_rows, x0, x, x_old, x_best, g_best, fs, ist, 1, eps, LO, HI, norm=norm, first=j == 0,
                     last=j == steps, window=window.get(j, 0), M=8)
    chain.release()
    assert torch.equal(_bits(got[0]), _bits(x_best)) and torch.equal(_bits(got[1]), _bits(fs[:, Fk.APGD_LOSS_BEST]))
    assert ist[:, Fk.APGD_ITERS].tolist() == [steps] * 8
    assert net.training is False                             # the mode, the parameters and their .grad are untouched
    assert all(torch.equal(q, was) and q.grad is g for q, (was, g) in zip(net.parameters(), params))


@pytest.mark.parametrize("norm,eps", [("linf", 0.1 / MNIST_STD), ("l2", 1.5 / MNIST_STD)])
def test_fused_loop_under_chunkings(cuda_device, norm, eps):
    """64 images in one call and in chunks (every launch below fc1_fwd's 512-row change of split): the same bits."""
    dev = cuda_device
    net = _trained(dev)
    x0, y = _images(dev)
    whole = fused_auto_pgd(net, x0, y, eps, 8, LO, HI, norm=norm)
    for cuts in ((16, 48), (1, 31, 32)):
        parts, at = [], 0
        for c in cuts:
            parts.append(fused_auto_pgd(net, x0[at:at + c], y[at:at + c], eps, 8, LO, HI, norm=norm))
            at += c
        assert torch.equal(_bits(torch.cat([q[0] for q in parts])), _bits(whole[0])), cuts
        assert torch.equal(_bits(torch.cat([q[1] for q in parts])), _bits(whole[1])), cuts
    tg = fused_auto_pgd(net, x0, (y + 3) % 10, eps, 8, LO, HI, norm=norm, targeted=True)
    assert not torch.equal(tg[0], whole[0])


@pytest.mark.parametrize("norm,eps", [("linf", 0.1), ("l2", 1.5)])
def test_predictor_auto_pgd_against_the_cpu(cuda_device, norm, eps):
    dev = cuda_device
    net = _trained(dev)
    pr = Predictor(net)
    assert pr.native
    x0, y = _images(dev)
    eps_n = eps / MNIST_STD
    x_adv, lp, loss_best = pr.auto_pgd(x0.view(64, 1, 28, 28), y, eps=eps, steps=20, norm=norm)
    xa = x_adv.reshape(64, 784)
    assert (xa >= LO).all() and (xa <= HI).all()
    d = (xa - x0).double()
    if norm == "linf":
        assert (d.abs() <= eps_n + 2.0 ** -23 * max(abs(LO), abs(HI))).all()
    else:
        assert (d.norm(dim=1) <= eps_n * (1.0 + 4 * 2.0 ** -23 * (784 / 8 + 1)) + 28 * 2.0 ** -24 * max(abs(LO), abs(HI))).all()
    # the losses, by a GradChain run of the same size: the start point's and the best point's
    st = fused_state(net)
    st.sync()
    chain = GradChain(st, 64)
    lab = y.to(torch.int32)
    chain.run(native.ptr(x0), native.ptr(lab), 64)
    start = chain._buf.loss_rows[:64].clone()
    chain.run(native.ptr(xa.contiguous()), native.ptr(lab), 64)
    again = chain._buf.loss_rows[:64].clone()
    chain.release()
    assert (loss_best >= start).all()
    assert torch.equal(_bits(again), _bits(loss_best))
    # against the CPU reference (never against the kernel itself)
    cpu_net = trained_net()
    x_ref, loss_ref = reference_auto_pgd(cpu_net, x0.cpu(), y.cpu(), eps_n, 20, LO, HI, norm=norm)
    with torch.no_grad():
        found_ref = cpu_net.forward_reference(x_ref.view(64, 1, 28, 28)).argmax(1) != y.cpu()
    found = (lp.argmax(1) != y).cpu()
    ratio = float(loss_best.double().mean().cpu()) / float(loss_ref.double().mean())
    diff = int(found.sum()) - int(found_ref.sum())
    flips = int((found != found_ref).sum())
    print(f"\nauto_pgd {norm} eps {eps}: mean loss_best GPU {float(loss_best.mean()):.4f} CPU {float(loss_ref.mean()):.4f} "
          f"ratio {ratio:.4f}; found GPU {int(found.sum())} CPU {int(found_ref.sum())}, images that differ {flips}")
    assert abs(ratio - 1.0) <= RATIO_MARGIN, ratio
    assert flips <= FOUND_MARGIN, (diff, flips)


def test_predict_cli_apgd_on_gpu(cuda_device, tmp_path):
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(trained_net(), ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "200", "--checkpoint", ckpt, "--json-log", log, "--apgd-eps", "0.1", "--apgd-steps", "10"],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    with open(log) as f:
        rec = json.loads(f.read())
    assert len(lines) == 2 and lines[1].startswith("Auto-PGD set (Linf eps=0.1, steps=10, restarts=1): Average loss: ")
    assert rec["device"].startswith("cuda") and rec["apgd_correct"] <= rec["correct"]
    assert lines[1].endswith(f"Accuracy: {rec['apgd_correct']}/200 ({100.0 * rec['apgd_correct'] / 200:.0f}%)")
    assert rec["apgd_loss"] >= rec["test_loss"]
