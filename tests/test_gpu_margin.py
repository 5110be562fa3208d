"""The margin / DLR losses on the GPU (MI355X only): ``head_margin`` (csrc/kernels/fc_head.hip) against the float64
oracle of tests/margin_ref.py, on hand-made tie rows, with a planted NaN and against its launcher's refusals; then
``GradChain(loss=...)`` and the fused Auto-PGD loop against its launches by hand and under chunkings, ``Predictor`` against
the CPU, the worst-case ensemble against the AND of its attacks, and the ``mnist_predict.py`` lines.

tests/test_margin_cpu.py proves on the CPU that the oracle check fails on subtly wrong outputs.  The oracle tests
print `stage B tensor deviation eps`; the CPU comparison prints its ratios (docs/PERF_NOTES.md records both)."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import margin_ref as M
import refmodel as R
from attr_ref import trained_net
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import FLAG_NO_DROPOUT, ModelState
from pytorch_mnist_ddp_amd.inference import Predictor, auto_pgd_line, ensemble_line
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.apgd import fused_auto_pgd
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict
from test_margin_cpu import ENS, ensemble_by_hand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (float(v) for v in normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten())
OUTS = ("loss_rows", "dz1", "h_bf", "dl_bf")


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _sentinel(buf):
    buf.loss_rows.fill_(float("nan"))
    for t in (buf.dz1, buf.h_bf, buf.dl_bf):
        t.view(torch.int16).fill_(M.SENT)


class Head:
    """The seeded Net's head on the device, one activation set of B rows, and a launch of ``head_margin`` on given
    partials with sentinel-filled outputs, copied back."""

    def __init__(self, dev, B, fc2_bias=None):
        torch.manual_seed(1)
        net = Net()
        if fc2_bias is not None:
            with torch.no_grad():
                net.fc2.bias.copy_(torch.tensor(fc2_bias))
        self.dev, self.B = dev, B
        self.ms = ModelState(net, dev)
        self.buf = Fk.StepBuffers.allocate(B, dev)
        self.hp = {k: v.detach().cpu().clone() for k, v in self.ms.views(self.ms.param).items() if k.startswith("fc")}

    def load(self, z1part):
        ks = R.fc1_ksplit(self.B)
        self.buf.z1part.view(-1)[: ks * self.B * 128].copy_(z1part.reshape(-1))

    def run(self, labels, kind, targets=None, scale=1.0):
        _sentinel(self.buf)
        lab = labels.to(torch.int32).to(self.dev)
        tgt = None if targets is None else targets.to(torch.int32).to(self.dev)
        Fk.head_margin(self.ms, lab, self.buf, kind, tgt if kind == "dlr_t" else None, scale)
        torch.cuda.synchronize()
        return {k: getattr(self.buf, k).cpu() for k in OUTS}


def _report(stage, B, stats):
    for name, (dev, eps) in stats.items():
        print(f"\n{stage:22s} B={B:<5d} {name:18s} dev {dev:10.3e}  eps {eps:10.3e}", end="")


# ------------------------------------------------------------------ the kernel against the oracle
@pytest.mark.parametrize("B", M.SIZES)
def test_head_margin_against_the_oracle(cuda_device, B):
    hd = Head(cuda_device, B)
    z, y, t = M.margin_case(B)
    for k in ("fc1.bias", "fc2.weight", "fc2.bias"):
        assert torch.equal(hd.hp[k], M.head_params()[k])
    hd.load(z)
    rows = R.check_rows(B)
    n = torch.tensor(rows)
    for kind in M.KINDS:
        got = hd.run(y, kind, t)
        _report(f"head_margin {kind}", B, M.check_all(B, z[:, n], hd.hp, y[n], kind, t[n], 1.0, got, rows,
                                                      name=f"head_margin {kind}"))
    got = hd.run(y, "dlr", t, scale=-0.5)
    M.check_all(B, z[:, n], hd.hp, y[n], "dlr", t[n], -0.5, got, rows, name="head_margin dlr scale -0.5")


@pytest.mark.parametrize("B", [33, 512])
def test_head_margin_forward_is_head_trains_bits(cuda_device, B):
    """z1, h: head_train's with dropout off - the same h_bf bits, and the same dz1 zero pattern."""
    hd = Head(cuda_device, B)
    z, y, t = M.margin_case(B)
    hd.load(z)
    hd.ms.set_state(0, seed=0, rng_base=0, flags=FLAG_NO_DROPOUT)
    _sentinel(hd.buf)
    Fk.head_train(hd.ms, y.to(torch.int32).to(cuda_device), None, hd.buf, inv_batch=1.0)
    torch.cuda.synchronize()
    ht = {k: getattr(hd.buf, k).cpu() for k in OUTS}
    got = hd.run(y, "cw")
    assert torch.equal(_bits(got["h_bf"]), _bits(ht["h_bf"]))
    assert torch.equal(got["dz1"][:B].float() == 0, ht["dz1"][:B].float() == 0)


@pytest.mark.parametrize("bias,pairs", [(M.TIE_BIAS, M.TIE_ROWS), (M.TOP3_BIAS, M.TOP3_ROWS)])
def test_head_margin_tie_rows(cuda_device, bias, pairs):
    z, hp, y, t = M.tie_inputs(bias, pairs)
    hd = Head(cuda_device, len(pairs), fc2_bias=bias)
    hd.load(z)
    for kind in M.KINDS:
        got = hd.run(y, kind, t)
        n = len(pairs)
        assert (got["h_bf"][:n].float() == 0).all() and (got["dz1"][:n].float() == 0).all()
        M.check_tie_rows(bias, pairs, kind, got["loss_rows"], got["dl_bf"], name=f"head_margin {kind} ties")
        R.check_head_padding(n, got["dz1"], got["h_bf"], got["dl_bf"], M.SENT, name=f"head_margin {kind} ties")


def test_head_margin_nan_stays_in_its_row(cuda_device):
    B = 33
    hd = Head(cuda_device, B)
    z, y, t = M.margin_case(B)
    for kind in M.KINDS:
        hd.load(z)
        clean = hd.run(y, kind, t)
        zn = z.clone()
        zn[3, 7, :] = float("nan")                            # every hidden unit of row 7, one chunk
        hd.load(zn)
        got = hd.run(y, kind, t)
        others = torch.tensor([r for r in range(B) if r != 7])
        for k in OUTS:
            assert torch.equal(_bits(got[k])[others], _bits(clean[k])[others]), (kind, k)
            assert torch.equal(_bits(got[k])[B:], _bits(clean[k])[B:]), (kind, k)
        assert not torch.equal(_bits(got["h_bf"])[7], _bits(clean["h_bf"])[7])         # (the NaN did reach row 7)


def test_head_margin_launcher_refusals(cuda_device):
    B = 5
    hd = Head(cuda_device, B)
    z, y, t = M.margin_case(B)
    hd.load(z)
    _sentinel(hd.buf)
    keep = {k: getattr(hd.buf, k).clone() for k in OUTS}
    C, p, s, w, buf = native.load(), native.ptr, native.stream_handle(), Fk.param_ptrs(hd.ms), hd.buf
    lab, tgt = y.to(torch.int32).to(cuda_device), t.to(torch.int32).to(cuda_device)
    ok = dict(z1part=p(buf.z1part), b_fc1=w.f1b, w_fc2=w.f2w, b_fc2=w.f2b, labels=p(lab), targets=p(tgt), kind=0,
              scale=1.0, loss_rows=p(buf.loss_rows), dz1=p(buf.dz1), h_bf=p(buf.h_bf), dl_bf=p(buf.dl_bf), B=B, Bp=32,
              stream=s)
    for bad in (dict(kind=3), dict(kind=-1), dict(labels=0), dict(kind=2, targets=0), dict(B=0), dict(B=-4),
                dict(Bp=33), dict(Bp=0), dict(B=40, Bp=32), dict(z1part=0), dict(dl_bf=0)):
        with pytest.raises(RuntimeError, match="head_margin"):
            C.head_margin(**dict(ok, **bad))
    with pytest.raises(ValueError):
        Fk.head_margin(hd.ms, lab, buf, "ce")
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(getattr(buf, k)), _bits(v)) for k, v in keep.items())     # nothing ran
    C.head_margin(**dict(ok, kind=1, targets=0))              # targets are read by the targeted form only
    torch.cuda.synchronize()
    assert not torch.isnan(buf.loss_rows[:B]).any()


# ------------------------------------------------------------------ the chain and the loops
def _trained(dev):
    return copy.deepcopy(trained_net()).to(dev)


def _images(dev, n=64):
    imgs, labels = generate(64, seed=5)
    return normalize_u8(imgs).reshape(64, 784)[:n].to(dev).contiguous(), labels[:n].long().to(dev)


def _by_hand(st, x, lab, tgt, kind, B):
    """trunk_fwd, fc1_fwd, the head, fc_bwd role B and input_grad through ``ops.functional`` on a set of their own."""
    ms = st.ms
    buf = Fk.StepBuffers.allocate(B, ms.device)
    state = torch.tensor([1 << 32, 0, 0], dtype=torch.int64, device=ms.device)       # step 0 | STEP_FLAG_NO_DROPOUT
    Fk.trunk_fwd(ms, None, None, buf, True, state=state, xin=x)
    Fk.fc1_fwd(ms, buf)
    if kind == "ce":
        Fk.head_train(ms, lab, None, buf, state=state, inv_batch=1.0)
    else:
        Fk.head_margin(ms, lab, buf, kind, tgt)
    Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=state)
    dx = Fk.input_grad(ms, buf)
    return dx, buf.loss_rows[:B].clone()


@pytest.mark.parametrize("kind", ["ce", "cw", "dlr", "dlr_t"])
def test_grad_chain_equals_its_launches_by_hand(cuda_device, kind):
    dev, B = cuda_device, 8
    net = _trained(dev)
    x0, y = _images(dev, B)
    st = fused_state(net)
    st.sync()
    lab = y.to(torch.int32)
    tgt = ((y + 3) % 10).to(torch.int32) if kind == "dlr_t" else None
    chain = GradChain(st, B) if kind == "ce" else GradChain(st, B, kind)
    dx = torch.full((B, 784), float("nan"), device=dev)
    if kind == "ce":
        chain.run(native.ptr(x0), native.ptr(lab), B)         # the parent's call: three arguments
    else:
        chain.run(native.ptr(x0), native.ptr(lab), B, native.ptr(tgt))
    chain.input_grad(native.ptr(dx), B)
    loss = chain._buf.loss_rows[:B].clone()
    chain.release()
    want_dx, want_loss = _by_hand(st, x0, lab, tgt, kind, B)
    assert torch.equal(_bits(dx), _bits(want_dx)) and torch.equal(_bits(loss), _bits(want_loss))
    assert torch.isfinite(dx).all() and (dx != 0).any()       # (a DLR row whose label ranks third has no gradient)
    if kind != "ce":                                          # ... and the loss is the reference's on the GPU's log-probs
        lp = Predictor(net).log_probs(x0.view(B, 1, 28, 28))
        ref = Fk.margin_loss_reference(lp, y, kind, None if tgt is None else tgt.long())
        assert torch.allclose(loss, ref, rtol=1e-3, atol=1e-3)


def _apgd_by_hand(st, x0, lab, tgt, kind, sign, eps, steps):
    B, dev = x0.shape[0], x0.device
    chain = GradChain(st, B, kind)
    x = x0.clone()
    dx, x_old, x_best, g_best = (torch.full((B, 784), float("nan"), device=dev) for _ in range(4))
    fs, ist = torch.full((B, 4), float("nan"), device=dev), torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    window = dict(Fk.apgd_checkpoints(steps))
    for j in range(steps + 1):
        chain.run(native.ptr(x), native.ptr(lab), B, native.ptr(tgt))
        chain.input_grad(native.ptr(dx), B)
        Fk.apgd_step(dx, chain._buf.loss_rows, x0, x, x_old, x_best, g_best, fs, ist, sign, eps, LO, HI, first=j == 0,
                     last=j == steps, window=window.get(j, 0), M=B)
    chain.release()
    return x_best, sign * fs[:, Fk.APGD_LOSS_BEST]


@pytest.mark.parametrize("targeted", [False, True])
def test_fused_auto_pgd_dlr_equals_its_launches_and_chunks(cuda_device, targeted):
    dev, B, steps, eps = cuda_device, 8, 5, 0.1 / MNIST_STD
    net = _trained(dev)
    x0, y = _images(dev, B)
    st = fused_state(net)
    st.sync()
    labels = (y + 3) % 10 if targeted else y
    true = y if targeted else None
    got = fused_auto_pgd(net, x0, labels, eps, steps, LO, HI, targeted=targeted, loss="dlr", true_labels=true)
    if targeted:
        want = _apgd_by_hand(st, x0, y.to(torch.int32), labels.to(torch.int32), "dlr_t", -1, eps, steps)
    else:
        want = _apgd_by_hand(st, x0, y.to(torch.int32), None, "dlr", 1, eps, steps)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    parts = [fused_auto_pgd(net, x0[a:b], labels[a:b], eps, steps, LO, HI, targeted=targeted, loss="dlr",
                            true_labels=None if true is None else true[a:b]) for a, b in ((0, 3), (3, 8))]
    assert torch.equal(_bits(torch.cat([q[0] for q in parts])), _bits(got[0]))
    assert torch.equal(_bits(torch.cat([q[1] for q in parts])), _bits(got[1]))
    ce = fused_auto_pgd(net, x0, labels, eps, steps, LO, HI, targeted=targeted)
    assert not torch.equal(ce[0], got[0])
    if targeted:
        with pytest.raises(ValueError):
            fused_auto_pgd(net, x0, labels, eps, steps, LO, HI, targeted=True, loss="dlr")


# ------------------------------------------------------------------ against the CPU
@pytest.mark.parametrize("loss", ["cw", "dlr"])
@pytest.mark.parametrize("targeted", [False, True])
def test_margin_attacks_against_the_cpu_reference(cuda_device, loss, targeted):
    """B = 64, the seeds of tests/test_attack_cpu.py.  Asserted: both box conditions hold exactly; the loss of the
    GPU's points, judged by the fp32 CPU forward, moves the right way against the clean point (mean; Auto-PGD with 4
    and with 10 updates); eps = 0 returns the clean images.  Printed, not asserted (docs/PERF_NOTES.md): the ratio of the GPU
    attack's gain to the CPU attack's and the share of pixels displaced with the same sign."""
    dev = cuda_device
    torch.manual_seed(3)
    ref = Net()
    net = copy.deepcopy(ref).to(dev).train()
    imgs, labels = generate(64, seed=5)
    cpu, gpu = Predictor(ref), Predictor(net)
    assert gpu.native and not cpu.native
    y = labels.long()
    lab = (y + 3) % 10 if targeted else y
    true = y if targeted and loss == "dlr" else None
    kind = "dlr_t" if targeted and loss == "dlr" else loss
    x0 = normalize_u8(imgs)
    eps_n = 0.1 / MNIST_STD
    judge = lambda x: (Fk.margin_loss_reference(cpu.log_probs(x), y, kind, lab) if kind == "dlr_t"       # noqa: E731
                       else Fk.margin_loss_reference(cpu.log_probs(x), lab, kind)).mean().item()
    clean = judge(x0)
    kw = dict(targeted=targeted, loss=loss, true_labels=true)
    for name, run in (("apgd-4", lambda p: p.auto_pgd(imgs, lab, eps=0.1, steps=4, **kw)[0]),
                      ("apgd-10", lambda p: p.auto_pgd(imgs, lab, eps=0.1, steps=10, **kw)[0])):
        xg, xc = run(gpu).cpu(), run(cpu)
        up_g, up_c = judge(xg) - clean, judge(xc) - clean
        agree = (torch.sign(xg - x0) == torch.sign(xc - x0)).float().mean().item()
        print(f"\n{loss} targeted={targeted} {name}: clean {clean:.4f} gpu {up_g:+.4f} cpu {up_c:+.4f} "
              f"ratio {up_g / up_c:.4f} sign agreement {agree:.4f}", end="")
        assert (up_g < 0 and up_c < 0) if targeted else (up_g > 0 and up_c > 0)
        assert (xg >= x0 - eps_n).all() and (xg <= x0 + eps_n).all()
        assert (xg >= LO).all() and (xg <= HI).all()
    assert torch.equal(gpu.auto_pgd(imgs, lab, eps=0.0, steps=2, **kw)[0].cpu(), x0)


def test_auto_pgd_loss_best_is_the_chosen_loss(cuda_device):
    dev = cuda_device
    net = _trained(dev)
    pr = Predictor(net)
    x0, y = _images(dev)
    for loss in ("cw", "dlr"):
        xa, lp, lb = pr.auto_pgd(x0.view(64, 1, 28, 28), y, eps=0.1, steps=5, loss=loss)
        start = Fk.margin_loss_reference(pr.log_probs(x0.view(64, 1, 28, 28)), y, loss)
        assert torch.allclose(lb, Fk.margin_loss_reference(lp, y, loss), rtol=2e-2, atol=2e-2)
        assert (lb >= start - 2e-2).all() and lb.mean() > start.mean()
    with pytest.raises(ValueError):
        pr.auto_pgd(x0.view(64, 1, 28, 28), y, loss="dlr_t")


# ------------------------------------------------------------------ the ensemble and the command line
def test_ensemble_is_the_and_of_its_attacks_on_the_gpu(cuda_device):
    dev = cuda_device
    net = _trained(dev)
    pr = Predictor(net)
    imgs, labels = generate(16, seed=21)
    imgs_d = imgs.to(dev)
    eps = 0.15
    correct, n, after = pr.robust_evaluate_ensemble(imgs_d, labels, eps, **ENS)
    want = ensemble_by_hand(pr, imgs_d, labels, eps, **ENS)
    assert n == 16 and correct == int(want.sum()) == after["square"]
    counts = list(after.values())
    assert list(after) == ["clean", "apgd_ce", "apgd_t", "square"] and counts == sorted(counts, reverse=True)
    assert counts[0] == pr.evaluate(imgs_d, labels)[1]
    assert pr.robust_evaluate_ensemble(imgs_d, labels, eps, batch_size=7, **ENS) == (correct, n, after)


def test_predict_cli_margin_lines_on_gpu(cuda_device, tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt, log = str(tmp_path / "mnist_cnn.pt"), str(tmp_path / "log.jsonl")
    save_state_dict(net, ckpt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "24", "--checkpoint", ckpt, "--batch-size", "24", "--json-log", log, "--apgd-eps", "0.1",
                        "--apgd-steps", "3", "--apgd-loss", "dlr", "--ensemble-eps", "0.1", "--ensemble-steps", "3",
                        "--ensemble-targets", "2", "--ensemble-queries", "10"],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    with open(log) as f:
        rec = json.loads(f.read())
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=24, verbose=False)
    pr = Predictor(copy.deepcopy(net).to(cuda_device))
    images = data.device_images(cuda_device)
    ap = pr.robust_evaluate_apgd(images, data.targets, 0.1, steps=3, batch_size=24, loss="dlr")
    ens = pr.robust_evaluate_ensemble(images, data.targets, 0.1, steps=3, n_targets=2, queries=10, batch_size=24)
    assert rec["device"].startswith("cuda") and len(lines) == 3 and lines[0].startswith("Test set:")
    assert lines[1] == auto_pgd_line(0.1, 3, 1, ap[0] / 24, ap[1], 24, loss_name="dlr") and ", loss=dlr): " in lines[1]
    assert lines[2] == ensemble_line(0.1, 2, ens[0], 24)
    assert rec["apgd_loss_name"] == "dlr" and rec["apgd_correct"] == ap[1]
    assert (rec["ensemble_eps"], rec["ensemble_steps"], rec["ensemble_targets"], rec["ensemble_queries"],
            rec["ensemble_seed"], rec["ensemble_correct"], rec["ensemble_after"]) == (0.1, 3, 2, 10, 0, ens[0], ens[2])
