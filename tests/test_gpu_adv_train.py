"""Adversarial training on the GPU (MI355X only): the ``adv_init`` kernel against the LUT and the numpy emulation
of its random start, the engine's adversarial step against its hand-launched parts and against the plain step
(eps = 0), off-means-off, the scope refusals, the CPU module path as the fp32 reference, the defence's direction,
and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import driver
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import FLAG_NO_DROPOUT, ModelState
from pytorch_mnist_ddp_amd.engine.trainer import FusedTrainer, adversarial_config
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO, Predictor, adversarial_units
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.optim import Adadelta

from advtrain_ref import adv_init_emulation
from refmodel import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("param", "square_avg", "acc_delta")


def _state(dev, step, seed, rng_base=0, flags=0):
    """A 24-byte StepState tensor (step | flags << 32, seed, rng_base)."""
    vals = [(step & 0xFFFFFFFF) | (flags << 32), seed, rng_base]
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64).to(dev)


def _trainer(dev, graph_steps, n_train, B, seed=1, n_test=200, **kw):
    torch.manual_seed(seed)
    net = Net()
    tr = load_mnist(synthetic_data=True, train=True, synthetic_size=n_train, verbose=False)
    te = load_mnist(synthetic_data=True, train=False, synthetic_size=n_test, verbose=False)
    ms = ModelState(net, dev, lr=1.0)
    t = FusedTrainer(ms, tr, te, B, 1000, num_samples=n_train, seed=seed, graph_steps=graph_steps, **kw)
    return net, ms, t


def _snapshot(ms, t, steps):
    torch.cuda.synchronize()
    return {**{k: getattr(ms, k).clone() for k in STATE_KEYS}, "loss_log": t.loss_log[:steps].clone()}


def _run_stream(t, ms, idx, steps):
    t.start_stream(idx)
    t.run_steps(steps)
    t.synchronize()
    assert ms.get_step() == steps
    return _snapshot(ms, t, steps)


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.isfinite(a["param"]).all() and torch.isfinite(a["loss_log"]).all(), what


# ---------------------------------------------------------------------------- a. adv_init on its own
@pytest.mark.parametrize("B", [1, 33, 200])
def test_adv_init_kernel_bitwise(cuda_device, B):
    dev = cuda_device
    N, seed, SENT = 3 * B + 7, 0x1234ABCD5678, -7.25
    imgs, labels = generate(N, seed=21)
    u8 = imgs.reshape(N, 784).contiguous()
    order = torch.randperm(N, generator=torch.Generator().manual_seed(4))[:3 * B]      # rows of steps 0 .. 2
    u8_d, lab_d = u8.to(dev), labels.to(torch.int32).to(dev)
    idx_d = order.to(torch.int32).to(dev)
    pre_u8, pre_lab = u8[order].contiguous().to(dev), labels[order].to(torch.int32).to(dev)   # pre-gathered rows
    lut = _PIXEL_LUT.numpy()
    eps, lo, hi = adversarial_units(0.3, 1, None)[0], PIXEL_LO, PIXEL_HI
    for step in (0, 2):
        rows = order[step * B:(step + 1) * B]
        st = _state(dev, step, seed, rng_base=40)
        want_x0, want_x, _ = adv_init_emulation(u8[rows].numpy(), seed, step, eps, lo, hi, True)
        if B > 1:                                           # both clamps bind on some pixels
            assert (want_x == np.float32(lo)).any() and (want_x == np.float32(hi)).any()
            assert ((want_x != want_x0) & (want_x > np.float32(lo)) & (want_x < np.float32(hi))).any()
        assert np.array_equal(want_x0, lut[u8[rows].numpy().astype(np.int64)])
        for form in ("idx", "pre"):
            src = (u8_d, lab_d, idx_d) if form == "idx" else (pre_u8, pre_lab, None)
            for rs in (False, True):
                outs = []
                for _ in range(2):                           # a second launch gives the same bits
                    x0 = torch.full((B + 1, 784), SENT, dtype=torch.float32, device=dev)
                    x = torch.full((B + 1, 784), SENT, dtype=torch.float32, device=dev)
                    lab = torch.full((B + 1,), -99, dtype=torch.int32, device=dev)
                    Fk.adv_init(*src, st, B, idx_stride=B, eps=eps, lo=lo, hi=hi, random_start=rs, x0=x0, x=x,
                                labels_out=lab)
                    torch.cuda.synchronize()
                    outs.append((x0.cpu(), x.cpu(), lab.cpu()))
                (x0, x, lab), again = outs
                what = (B, step, form, rs)
                assert all(torch.equal(p, q) for p, q in zip(outs[0], again)), what
                assert np.array_equal(x0[:B].numpy(), want_x0), what                 # bit for bit the LUT
                assert torch.equal(lab[:B], labels[rows].to(torch.int32)), what
                assert np.array_equal(x[:B].numpy(), want_x if rs else want_x0), what
                assert (x0[B] == SENT).all() and (x[B] == SENT).all() and lab[B] == -99, what    # the guard row


# ---------------------------------------------------------------------------- b. engine step = its parts
def _hand_launched(dev, t, idx, steps, B, cfg, seed):
    """The adversarial steps launched kernel by kernel through ``ops.functional`` on a model state of its own:
    adv_init (by index vector), K x the five attack launches under the attack's state, then the SERIAL training
    step's launches with ``xin`` and direct labels."""
    torch.manual_seed(seed)
    ms = ModelState(Net(), dev, lr=1.0)
    buf = Fk.StepBuffers.allocate(B, dev)
    eps_n, alpha_n, lo, hi = adversarial_units(cfg["eps"], cfg["steps"], cfg["step_size"])
    idx_d = idx.to(torch.int32).to(dev)
    ms.set_state(0, seed, 0, 0)                                             # dropout on, keyed by (seed, step)
    att = _state(dev, 0, seed, 0, FLAG_NO_DROPOUT)
    x0 = torch.empty(B, 784, dtype=torch.float32, device=dev)
    x = torch.empty(B, 784, dtype=torch.float32, device=dev)
    lab = torch.empty(B, dtype=torch.int32, device=dev)
    loss_log = torch.zeros(steps, dtype=torch.float32, device=dev)
    for _ in range(steps):
        Fk.adv_init(t.train_u8, t.train_labels, idx_d, ms.state, B, idx_stride=B, eps=eps_n, lo=lo, hi=hi,
                    random_start=cfg["random_start"], x0=x0, x=x, labels_out=lab)
        for _ in range(cfg["steps"]):
            Fk.trunk_fwd(ms, None, None, buf, True, state=att, xin=x)
            Fk.fc1_fwd(ms, buf)
            Fk.head_train(ms, lab, None, buf, state=att, inv_batch=1.0)
            Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=att)
            Fk.input_grad_step(ms, buf, x, x0, eps_n, alpha_n, lo, hi, out=x)
        Fk.trunk_fwd(ms, None, None, buf, True, xin=x)
        Fk.fc1_fwd(ms, buf)
        Fk.head_train(ms, lab, None, buf)
        Fk.fc_bwd(ms, buf, 1.0, loss_log)
        Fk.conv_bwd(ms, None, None, buf, stages=Fk.CONV_WGRAD, xin=x)
        Fk.conv_bwd(ms, None, None, buf, stages=Fk.CONV_DGRAD, xin=x)
        Fk.conv_bwd(ms, None, None, buf, stages=Fk.CONV_REDUCE, xin=x, update=Fk.UPD_WHOLE, wt=True, advance_step=True)
    torch.cuda.synchronize()
    assert ms.get_step() == steps
    return {**{k: getattr(ms, k).clone() for k in STATE_KEYS}, "loss_log": loss_log}


@pytest.mark.parametrize("random_start", [False, True])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [33, 200])
def test_engine_adversarial_step_equals_hand_launched_parts(cuda_device, B, K, random_start):
    dev, steps, seed = cuda_device, 3, 1
    n = steps * B
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    adv = {"eps": 0.1, "steps": K, "random_start": random_start}
    got = {}
    for gs in (0, 3):                                    # eager, and one captured 3-step chunk replayed
        _, ms, t = _trainer(dev, gs, n, B, seed=seed, adversarial=adv)
        assert t.engine.schedule == t.C.SCHED_SERIAL and not t.overlap and t.engine.adversarial_steps == K
        assert t.engine.adversarial_bytes > 0
        got[gs] = _run_stream(t, ms, idx, steps)
    _assert_same(got[0], got[3], "graph replay against eager")
    want = _hand_launched(dev, t, idx, steps, B, adversarial_config(adv), seed)
    _assert_same(got[0], want, "engine against its hand-launched parts")
    _, ms_p, tp = _trainer(dev, 0, n, B, seed=seed, overlap=False)          # and it is not the plain step
    assert not torch.equal(_run_stream(tp, ms_p, idx, steps)["param"], got[0]["param"])


# ---------------------------------------------------------------------------- c. eps = 0 is the plain step
@pytest.mark.parametrize("B", [33, 200])
def test_zero_radius_equals_plain_serial_bitwise(cuda_device, B):
    """eps = 0, K = 1, no random start: the attack returns the clean batch (x = x0 bit for bit), so the step on
    ``xin`` computes what the plain step computes from the uint8 rows: trunk_fwd and conv2_dgrad read the same
    fp32 values from either input form."""
    dev, steps = cuda_device, 3
    n = steps * B
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    _, ms_a, ta = _trainer(dev, 3, n, B, adversarial={"eps": 0.0, "steps": 1})
    _, ms_p, tp = _trainer(dev, 3, n, B, overlap=False)
    assert ta.engine.schedule == tp.engine.schedule == ta.C.SCHED_SERIAL
    _assert_same(_run_stream(ta, ms_a, idx, steps), _run_stream(tp, ms_p, idx, steps), "eps = 0 against plain SERIAL")


# ---------------------------------------------------------------------------- d. off means off
def test_off_means_off(cuda_device):
    dev, B, steps = cuda_device, 33, 3
    n = steps * B
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    _, ms_a, ta = _trainer(dev, 3, n, B, adversarial={"eps": 0.1, "steps": 2, "random_start": True})
    _, ms_p, tp = _trainer(dev, 3, n, B, overlap=False)
    assert tp.adversarial is None and tp.engine.adversarial_steps == 0 and tp.engine.adversarial_bytes == 0
    ws = tp.engine.workspace_bytes
    assert ta.engine.workspace_bytes == ws                   # the workspace carve is untouched; the attack's
    assert ta.engine.adversarial_bytes >= 2 * B * 784 * 4    # buffers are an allocation of their own
    _run_stream(ta, ms_a, idx, steps)                        # adversarial steps (a captured chunk of that form)
    ta.set_adversarial(None)
    assert ta.adversarial is None and ta.engine.adversarial_steps == 0
    with torch.no_grad():                                    # a fresh plain trainer from the same state
        for k in STATE_KEYS:
            getattr(ms_p, k).copy_(getattr(ms_a, k))
    tp.engine.refresh_shadows()
    tp.rng_base = ta.rng_base
    torch.cuda.synchronize()
    _assert_same(_run_stream(ta, ms_a, idx, steps), _run_stream(tp, ms_p, idx, steps), "switched off against plain")
    ta.set_adversarial({"eps": 0.1, "steps": 2, "random_start": True})      # and on again: not the plain step
    with torch.no_grad():
        for k in STATE_KEYS:
            getattr(ms_p, k).copy_(getattr(ms_a, k))
    tp.engine.refresh_shadows()
    tp.rng_base = ta.rng_base
    torch.cuda.synchronize()
    assert not torch.equal(_run_stream(ta, ms_a, idx, steps)["param"], _run_stream(tp, ms_p, idx, steps)["param"])


# ---------------------------------------------------------------------------- e. refusals
def test_scope_refusals_launch_nothing(cuda_device):
    dev, B = cuda_device, 33
    args = (0.3, 0.1, 2, False, PIXEL_LO, PIXEL_HI)
    # OVERLAP: a SERIAL engine with the attack on refuses the schedule; an OVERLAP engine refuses the attack
    _, ms, t = _trainer(dev, 0, 3 * B, B, overlap=False)
    before = ms.param.clone()
    t.engine.set_adversarial(*args)
    with pytest.raises(RuntimeError, match="limited to the SERIAL schedule"):
        t.engine.set_schedule(t.C.SCHED_OVERLAP)
    assert t.engine.schedule == t.C.SCHED_SERIAL
    t.engine.set_adversarial(0.0, 0.0, 0, False, 0.0, 0.0)
    t.engine.set_schedule(t.C.SCHED_OVERLAP)                 # off: any schedule again
    with pytest.raises(RuntimeError, match="limited to the SERIAL schedule"):
        t.engine.set_adversarial(*args)
    with pytest.raises(ValueError, match="SERIAL"):
        t.set_adversarial({"eps": 0.1})
    assert t.engine.adversarial_steps == 0
    # fp32
    _, ms32, t32 = _trainer(dev, 0, 3 * B, B, overlap=False, fp32=True)
    with pytest.raises(RuntimeError, match="limited to the bf16 step"):
        t32.engine.set_adversarial(*args)
    assert t32.engine.adversarial_steps == 0 and t32.engine.adversarial_bytes == 0
    with pytest.raises(ValueError, match="bf16"):
        _trainer(dev, 0, 3 * B, B, fp32=True, adversarial={"eps": 0.1})
    # world 2 (an engine without a transport: nothing of it ever runs)
    s = t.compute.cuda_stream
    eng2 = t.C.Engine(ms.buffers(), B, 1, int(s), int(t.comm_stream.cuda_stream), 2, ms.rho, ms.eps, ms.weight_decay)
    with pytest.raises(RuntimeError, match="limited to world size 1"):
        eng2.set_adversarial(*args)
    assert eng2.adversarial_steps == 0 and eng2.adversarial_bytes == 0
    with pytest.raises(ValueError, match="world size 1"):
        FusedTrainer(ms, None, None, B, B, 3 * B, world_size=2, adversarial={"eps": 0.1})
    torch.cuda.synchronize()
    assert torch.equal(ms.param, before) and ms.get_step() == 0             # nothing was launched


# ---------------------------------------------------------------------------- f. against the fp32 reference
def test_adversarial_steps_against_cpu_module_path(cuda_device):
    """One epoch on 600 synthetic images, B = 200, eps = 0.1, K = 2, no random start, dropout off, against the CPU
    module path (``driver.craft_adversarial`` + the ordinary torch step, fp32) on the same batches.  The rule is
    that of tests/test_gpu_numerics.py for a clean train step against the fp32 reference: per tensor relative
    error below 0.1, the loss within 2e-2 * max(1, |loss|).  It is applied to the parameters after the first
    step; a sign flip of a near-zero input gradient moves a pixel by 2 alpha and every step starts from
    parameters that already deviate, so after step k the cap is k * 0.1 (each step adds at most its own)."""
    dev, B, n = cuda_device, 200, 600
    adv = {"eps": 0.1, "steps": 2}
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(9))
    net, ms, t = _trainer(dev, 0, n, B, adversarial=adv, dropout=False)
    ref = Net()
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    init = {k: v.detach().clone() for k, v in ref.named_parameters()}
    opt = Adadelta(ref.parameters(), lr=1.0)
    tr = load_mnist(synthetic_data=True, train=True, synthetic_size=n, verbose=False)
    cfg = adversarial_config(adv)
    t.start_stream(idx)
    ref.eval()                                               # dropout off in the training forward too
    worst = {}
    for s in range(3):
        t.run_steps(1)
        t.synchronize()
        rows = idx[s * B:(s + 1) * B]
        data, target = normalize_u8(tr.images[rows]), tr.targets[rows]
        x_adv = driver.craft_adversarial(ref, data, target, cfg)
        opt.zero_grad()
        loss = F.nll_loss(ref.forward_reference(x_adv), target)
        loss.backward()
        opt.step()
        got = {k: v.detach().cpu() for k, v in ms.views(ms.param).items()}
        errs = {k: rel_err(got[k], p.detach()) for k, p in ref.named_parameters()}
        moves = {k: rel_err(got[k] - init[k], p.detach() - init[k]) for k, p in ref.named_parameters()}
        gl = float(t.loss_log[s].item())
        print(f"step {s}: loss gpu {gl:.5f} ref {loss.item():.5f}; parameter rel err max {max(errs.values()):.3e} "
              f"({max(errs, key=errs.get)}); rel err of the parameters' movement max {max(moves.values()):.3e} "
              f"({max(moves, key=moves.get)})")
        worst[s] = max(errs.values())
        assert abs(gl - loss.item()) < 2e-2 * max(1.0, abs(loss.item())) * (s + 1), (s, gl, loss.item())
        assert all(e < 0.1 * (s + 1) for e in errs.values()), (s, errs)
        assert all(torch.isfinite(v).all() for v in got.values())


# ---------------------------------------------------------------------------- g. it defends
DEFEND_N, DEFEND_B = 2400, 100


def test_adversarial_training_defends(cuda_device):
    """Two epochs on DEFEND_N synthetic images with and without ``adversarial=dict(eps=0.1, steps=3)``, seeded;
    ``Predictor.robust_evaluate(eps=0.1, steps=10)`` on 400 test images counts strictly more correct ones for the
    adversarially trained net.  Only the direction is asserted; the four accuracies are printed.

    The set size comes from the CPU module path (same loop, batches of 100, fp32), attacked test images correct
    of 400, plain / adversarially trained: 600 images 129 / 110 (reversed: two epochs of 6 steps train neither),
    1200: 137 / 153, 1800: 157 / 183, 2400: 143 / 224.  2400 is the smallest of these at which the direction is
    clear (a margin of 81 images, against 16 and 26 below it)."""
    dev = cuda_device
    te = load_mnist(synthetic_data=True, train=False, synthetic_size=400, verbose=False)
    images = te.device_images(dev)
    res = {}
    for name, adv in (("plain", None), ("adversarial", {"eps": 0.1, "steps": 3})):
        net, ms, t = _trainer(dev, 6, DEFEND_N, DEFEND_B, adversarial=adv, overlap=False)
        lr = 1.0
        for ep in (1, 2):
            t.set_lr(lr)
            t.train_epoch(ep, torch.randperm(DEFEND_N, generator=torch.Generator().manual_seed(100 + ep)))
            lr *= 0.7
        t.synchronize()
        pr = Predictor(net)
        res[name] = (pr.evaluate(images, te.targets)[1], pr.robust_evaluate(images, te.targets, 0.1, steps=10,
                                                                           batch_size=400)[1])
        print(f"{name}: clean {res[name][0]}/400, attacked (eps 0.1, 10 steps) {res[name][1]}/400")
    assert res["adversarial"][1] > res["plain"][1], res


# ---------------------------------------------------------------------------- h. command line
def test_mnist_cli_adversarial_training_and_predict(gpu_box, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    log = str(tmp_path / "train.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist.py"), "--synthetic", "--synthetic-size", "400",
                        "--synthetic-test-size", "200", "--batch-size", "200", "--epochs", "1", "--adv-train-eps",
                        "0.1", "--save-model", "--json-log", log],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 2, lines                            # the reference's lines: batch 0's, the test set's
    assert lines[0].startswith("Train Epoch: 1 [0/400 (0%)]\tLoss: ") and lines[1].startswith("Test set: Average loss: ")
    with open(log) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    ep = [x for x in recs if "epoch" in x]
    assert len(ep) == 1 and (ep[0]["adv_train_eps"], ep[0]["adv_train_steps"], ep[0]["adv_train_step_size"],
                             ep[0]["adv_train_random_start"]) == (0.1, 1, 0.1, False)
    assert [x["schedule"] for x in recs if "schedule" in x] == ["serial"]
    assert (tmp_path / "mnist_cnn.pt").exists()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "200", "--attack-eps", "0.1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 2 and lines[0].startswith("Test set:")
    assert lines[1].startswith("Adversarial set (Linf eps=0.1, steps=1): Average loss: ")
