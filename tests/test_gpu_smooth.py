"""Randomized smoothing on the GPU (MI355X only): ``smooth_noise`` against the float64 Box-Muller emulation on the
same Philox words, its determinism, chunking and step form bit for bit, ``smooth_vote`` exactly against numpy,
``Predictor.smoothed_counts`` / ``certify`` against the launches made by hand, the engine's Gaussian-noise step
against its hand-launched parts and the plain step (sigma = 0), the scope refusals, the command line, and the
direction of the certificate on a noise-trained net."""
import json
import os
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.engine.trainer import FusedTrainer
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import smooth as S
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

import smooth_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("param", "square_avg", "acc_delta")
SENT = -7.25
SEED = 0x1234ABCD5678


def _state(dev, step, seed, rng_base=0, flags=0):
    vals = [(step & 0xFFFFFFFF) | (flags << 32), seed, rng_base]
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64).to(dev)


def _images(M, seed=21):
    imgs, labels = generate(M, seed=seed)
    return imgs.reshape(M, 784).contiguous(), labels


def _noise(dev, src, sigma, n, seed=SEED, sample_base=0, id_base=0):
    """One launch into a sentinel-filled buffer with a guard row; returns the [M * n, 784] rows on the CPU."""
    rows = src.shape[0] * n
    out = torch.full((rows + 1, 784), SENT, dtype=torch.float32, device=dev)
    Fk.smooth_noise(src.to(dev), sigma, n, seed, sample_base, id_base, out=out)
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[rows] == SENT).all(), "the guard row past M * n was written"
    return out[:rows]


# ---------------------------------------------------------------------------- a. smooth_noise
@pytest.mark.parametrize("sigma_px", [0.25, 1.0])
@pytest.mark.parametrize("M,n", [(1, 1), (3, 5), (2, 257)])
def test_smooth_noise_against_float64_emulation(cuda_device, M, n, sigma_px):
    """Both source forms against the float64 emulation on the same words, eps = 8 x max |numpy fp32 emulation -
    float64|, not below 4 fp32 ulps of the largest output (``smooth_ref.noise_eps``)."""
    dev, sigma = cuda_device, sigma_px / MNIST_STD
    u8, _ = _images(M)
    x0 = _PIXEL_LUT[u8.long()].contiguous()
    want64 = SR.noise_emulation(x0.numpy(), sigma, n, SEED, 3, 11, SR.F64)
    want32 = SR.noise_emulation(x0.numpy(), sigma, n, SEED, 3, 11, SR.F32)
    eps = SR.noise_eps(want32, want64)
    outs = {}
    for form, src in (("u8", u8), ("f32", x0)):
        got = _noise(dev, src, sigma, n, sample_base=3, id_base=11)
        again = _noise(dev, src, sigma, n, sample_base=3, id_base=11)
        assert torch.equal(got, again), (form, "a second launch gives other bits")
        assert not (got == SENT).any() and torch.isfinite(got).all(), form
        dev_max = float(np.abs(got.numpy().astype(np.float64) - want64).max())
        print(f"smooth_noise M={M} n={n} sigma={sigma_px} {form}: max |gpu - f64| {dev_max:.3e}, eps {eps:.3e}, "
              f"max |numpy f32 - f64| {float(np.abs(want32.astype(np.float64) - want64).max()):.3e}")
        assert dev_max <= eps, (form, dev_max, eps)
        outs[form] = got
    assert torch.equal(outs["u8"], outs["f32"])                  # the in-register normalisation is the LUT's


def test_smooth_noise_zero_sigma_chunking_and_ids(cuda_device):
    dev, sigma = cuda_device, 0.5 / MNIST_STD
    u8, _ = _images(2)
    x0 = _PIXEL_LUT[u8.long()].contiguous()
    for src in (u8, x0):
        zero = _noise(dev, src, 0.0, 3)
        assert torch.equal(zero, x0.repeat_interleave(3, dim=0))             # sigma = 0: x0 bit for bit
        whole = _noise(dev, src, sigma, 8).view(2, 8, 784)
        lo, hi = _noise(dev, src, sigma, 3).view(2, 3, 784), _noise(dev, src, sigma, 5, sample_base=3).view(2, 5, 784)
        assert torch.equal(whole, torch.cat([lo, hi], dim=1))                # samples [0,3) + [3,8) = [0,8)
        one = torch.cat([_noise(dev, src[:1], sigma, 8), _noise(dev, src[1:], sigma, 8, id_base=1)])
        assert torch.equal(whole.view(16, 784), one)                         # images [0,2) = [0,1) + [1,2)
        other = _noise(dev, src, sigma, 8, seed=SEED + 1)
        assert not torch.equal(whole.view(16, 784), other)


def test_smooth_noise_launcher_refusals(cuda_device):
    dev = cuda_device
    C = Fk.native.load()
    x = torch.zeros(2, 784, dtype=torch.float32, device=dev)
    out = torch.zeros(4, 784, dtype=torch.float32, device=dev)
    p, s = Fk.native.ptr, Fk.native.stream_handle()
    for args in ((0, 0, p(out), 1.0, 0, 0, 0, 2, 2, s),                      # no source
                 (0, p(x), 0, 1.0, 0, 0, 0, 2, 2, s),                        # no output
                 (0, p(x) + 4, p(out), 1.0, 0, 0, 0, 1, 1, s),               # misaligned source
                 (0, p(x), p(out) + 4, 1.0, 0, 0, 0, 1, 1, s),               # misaligned output
                 (0, p(x), p(out), 1.0, 0, 0, 0, 0, 2, s),                   # M * n = 0
                 (0, p(x), p(out), -1.0, 0, 0, 0, 2, 2, s),                  # sigma < 0
                 (0, p(x), p(out), 1.0, 0, (1 << 32) - 1, 0, 2, 2, s)):      # sample_base + n > 2^32
        with pytest.raises(RuntimeError, match="smooth_noise"):
            C.smooth_noise(*args)
    torch.cuda.synchronize()
    assert (out == 0).all()


@pytest.mark.parametrize("B", [1, 33, 200])
def test_smooth_noise_step_form_equals_plain_form(cuda_device, B):
    dev, sigma = cuda_device, 0.5 / MNIST_STD
    u8, _ = _images(B)
    x0 = _PIXEL_LUT[u8.long()].contiguous().to(dev)
    for step, rng_base in ((0, 0), (5, 40), (2, (1 << 32) - 3), (7, (1 << 40) + 9)):
        st = _state(dev, step, SEED, rng_base)
        c0 = (rng_base + 2 * step) & 0xFFFFFFFF
        want = torch.empty(B, 784, dtype=torch.float32, device=dev)
        Fk.smooth_noise(x0, sigma, 1, SEED, sample_base=c0, id_base=0, out=want)
        x = torch.full((B + 1, 784), SENT, dtype=torch.float32, device=dev)
        Fk.smooth_noise_step(st, x0, sigma, B, x=x)
        inplace = torch.full((B + 1, 784), SENT, dtype=torch.float32, device=dev)
        inplace[:B] = x0
        Fk.smooth_noise_step(st, inplace, sigma, B, x=inplace)
        torch.cuda.synchronize()
        assert torch.equal(x[:B], want) and torch.equal(inplace[:B], want), (B, step, rng_base)
        assert (x[B] == SENT).all() and (inplace[B] == SENT).all(), "rows past B were written"
        assert not torch.equal(want, x0)


# ---------------------------------------------------------------------------- b. smooth_vote
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_smooth_vote_exact(cuda_device, M, n):
    dev = cuda_device
    lp = SR.hand_logp(M, n, seed=n + M)
    want = SR.vote_reference(lp, M, n)
    if n > 1:
        assert want.sum() < M * n                                # some rows hold a NaN and vote for nothing
    lp_d = torch.from_numpy(lp).to(dev)
    counts = torch.full((M + 1, 10), -99, dtype=torch.int32, device=dev)
    Fk.smooth_vote(lp_d, M, n, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(counts[:M].cpu().numpy(), want), (M, n)
    assert (counts[M] == -99).all(), "the guard row of counts was written"
    if n > 1:                                                    # two launches, accumulated = one launch
        k = n // 3 + 1
        parts = torch.from_numpy(lp).view(M, n, 10)
        first, second = parts[:, :k].contiguous().to(dev), parts[:, k:].contiguous().to(dev)
        acc = torch.full((M + 1, 10), -99, dtype=torch.int32, device=dev)
        Fk.smooth_vote(first, M, k, counts=acc)
        Fk.smooth_vote(second, M, n - k, counts=acc, accumulate=True)
        torch.cuda.synchronize()
        assert np.array_equal(acc[:M].cpu().numpy(), want) and (acc[M] == -99).all(), (M, n, k)


# ---------------------------------------------------------------------------- c. Predictor
def _seeded_net(dev, seed=3):
    torch.manual_seed(seed)
    return Net().to(dev)


def _by_hand(net, src, sigma_n, n, seed, sample_base=0, id_base=0):
    """The five launches of one chunk through ``ops.functional``, on buffers of their own."""
    ms = fused_state(net).ms
    M = src.shape[0]
    buf = Fk.StepBuffers.allocate(M * n, src.device)
    x = Fk.smooth_noise(src, sigma_n, n, seed, sample_base, id_base)
    Fk.trunk_fwd(ms, None, None, buf, False, xin=x)
    Fk.fc1_fwd(ms, buf)
    Fk.head_eval(ms, None, None, buf)
    return Fk.smooth_vote(buf.logp, M, n)


def test_predictor_smoothed_counts_and_certify(cuda_device):
    dev = cuda_device
    net = _seeded_net(dev)
    net.train()
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    pr = Predictor(net)                      # (binds the parameters and their .grad to the flat buffers)
    grads = {k: None if v.grad is None else v.grad.clone() for k, v in net.named_parameters()}
    u8, _ = _images(3, seed=8)
    sigma, n, seed = 0.5, 40, 77
    got = pr.smoothed_counts(u8.view(3, 28, 28), sigma, n, seed=seed)
    assert got.dtype == torch.int32 and got.shape == (3, 10) and (got.sum(dim=1) == n).all()
    want = _by_hand(net, u8.to(dev), sigma / MNIST_STD, n, seed)
    assert torch.equal(got, want)
    buf = fused_state(net).smooth_buf
    ptr = buf.x.data_ptr()
    assert torch.equal(pr.smoothed_counts(u8, sigma, n, seed=seed), got)                    # twice: equal
    assert fused_state(net).smooth_buf is buf and buf.x.data_ptr() == ptr                   # the buffer set is reused
    xf = _PIXEL_LUT[u8.long()].view(3, 1, 28, 28)
    assert torch.equal(pr.smoothed_counts(xf, sigma, n, seed=seed), got)                    # fp32 source form
    # chunked over images, and over samples (n > rows_per_launch), all launches below fc1's 512-row split change
    for rpl in (n, 2 * n + 1, 7):
        assert torch.equal(S.fused_smooth_counts(net, u8.to(dev), sigma / MNIST_STD, n, seed, rows_per_launch=rpl),
                           got), rpl
    # ids and sample_base name the draw: image 2 alone under id 2 = row 2; samples [10, 30) by hand
    assert torch.equal(pr.smoothed_counts(u8[2:], sigma, n, seed=seed, ids=[2]), got[2:])
    part = pr.smoothed_counts(u8, sigma, 20, seed=seed, sample_base=10)
    assert torch.equal(part, _by_hand(net, u8.to(dev), sigma / MNIST_STD, 20, seed, sample_base=10))
    assert not torch.equal(pr.smoothed_counts(u8, sigma, n, seed=seed + 1), got)
    # certify = certify_from_counts of the selection and the (disjoint) estimation counts
    classes, radii, counts = pr.certify(u8, sigma, n0=10, n=40, alpha=0.01, seed=seed)
    c0 = pr.smoothed_counts(u8, sigma, 10, seed=seed).cpu()
    c1 = pr.smoothed_counts(u8, sigma, 40, seed=seed, sample_base=10).cpu()
    assert torch.equal(counts, c1) and classes.dtype == torch.int64 and radii.dtype == torch.float64
    for j in range(3):
        cls, rad = S.certify_from_counts(c0[j].tolist(), c1[j].tolist(), sigma, 0.01)
        assert (int(classes[j]), float(radii[j])) == (cls, rad)
    assert net.training and all(torch.equal(v, before[k]) for k, v in net.named_parameters())
    for k, v in net.named_parameters():
        assert (v.grad is None) == (grads[k] is None) and (v.grad is None or torch.equal(v.grad, grads[k])), k
    with pytest.raises(ValueError):
        pr.smoothed_counts(u8, 0.0, n)
    with pytest.raises(ValueError):
        pr.smoothed_counts(u8, sigma, n, ids=[0, 1])


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


CHUNK_LAUNCHES = ["smooth_noise", "trunk_fwd", "fc1_fwd", "head_eval", "smooth_vote"]


def test_smoothed_counts_launch_sequence(cuda_device, monkeypatch):
    """The native loop is exactly the five launches of a chunk, once per chunk of ``smooth_chunks``, and nothing
    else of the extension: whole images in one launch, chunked over images, chunked over samples (the accumulate
    path), and through ``Predictor.smoothed_counts`` / ``certify``."""
    dev = cuda_device
    net = _seeded_net(dev)
    pr = Predictor(net)
    u8, _ = _images(3, seed=8)
    src = u8.to(dev)
    sigma, n, seed = 0.5, 40, 77
    sigma_n = sigma / MNIST_STD
    want = _by_hand(net, src, sigma_n, n, seed)              # (also brings the shadows up to date)
    torch.cuda.synchronize()
    rec = _Recorder(S.native.load())
    monkeypatch.setattr(S.native, "load", lambda *a, **k: rec)
    for rpl, chunks in ((8192, 1), (3 * n, 1), (2 * n + 1, 2), (n, 3), (7, 3 * 6)):
        plan = S.smooth_chunks(3, n, [0, 1, 2], rpl)
        assert len(plan) == chunks and sum(m * ns for _, m, _, ns in plan) == 3 * n, (rpl, plan)
        rec.calls.clear()
        got = S.fused_smooth_counts(net, src, sigma_n, n, seed, rows_per_launch=rpl)
        assert rec.calls == CHUNK_LAUNCHES * chunks, (rpl, rec.calls)
        assert torch.equal(got, want), rpl
    assert any(s0 > 0 for _, _, s0, _ in S.smooth_chunks(3, n, [0, 1, 2], 7))      # rpl = 7 accumulates
    # ids that are not consecutive split a launch: one id_base per launch
    rec.calls.clear()
    S.fused_smooth_counts(net, src, sigma_n, n, seed, ids=[0, 1, 5])
    assert rec.calls == CHUNK_LAUNCHES * 2, rec.calls
    # the Predictor's calls go through the same loop: one chunk each, two for certify (selection, estimation)
    rec.calls.clear()
    assert torch.equal(pr.smoothed_counts(u8, sigma, n, seed=seed), want)
    assert rec.calls == CHUNK_LAUNCHES, rec.calls
    rec.calls.clear()
    pr.certify(u8, sigma, n0=10, n=n, alpha=0.01, seed=seed)
    assert rec.calls == CHUNK_LAUNCHES * 2, rec.calls


# ---------------------------------------------------------------------------- d. the engine's noise step
def _trainer(dev, graph_steps, n_train, B, seed=1, n_test=200, **kw):
    torch.manual_seed(seed)
    net = Net()
    tr = load_mnist(synthetic_data=True, train=True, synthetic_size=n_train, verbose=False)
    te = load_mnist(synthetic_data=True, train=False, synthetic_size=n_test, verbose=False)
    ms = ModelState(net, dev, lr=1.0)
    t = FusedTrainer(ms, tr, te, B, 1000, num_samples=n_train, seed=seed, graph_steps=graph_steps, **kw)
    return net, ms, t


def _run_stream(t, ms, idx, steps):
    t.start_stream(idx)
    t.run_steps(steps)
    t.synchronize()
    assert ms.get_step() == steps
    torch.cuda.synchronize()
    return {**{k: getattr(ms, k).clone() for k in STATE_KEYS}, "loss_log": t.loss_log[:steps].clone()}


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.isfinite(a["param"]).all() and torch.isfinite(a["loss_log"]).all(), what


def _hand_launched(dev, t, idx, steps, B, sigma_px, seed):
    """The noise steps launched kernel by kernel: adv_init (no random start), smooth_noise in its step form in
    place, then the SERIAL training step's launches with ``xin`` and direct labels."""
    torch.manual_seed(seed)
    ms = ModelState(Net(), dev, lr=1.0)
    buf = Fk.StepBuffers.allocate(B, dev)
    idx_d = idx.to(torch.int32).to(dev)
    ms.set_state(0, seed, 0, 0)
    x0 = torch.empty(B, 784, dtype=torch.float32, device=dev)
    x = torch.empty(B, 784, dtype=torch.float32, device=dev)
    lab = torch.empty(B, dtype=torch.int32, device=dev)
    loss_log = torch.zeros(steps, dtype=torch.float32, device=dev)
    for _ in range(steps):
        Fk.adv_init(t.train_u8, t.train_labels, idx_d, ms.state, B, idx_stride=B, x0=x0, x=x, labels_out=lab)
        Fk.smooth_noise_step(ms.state, x0, sigma_px / MNIST_STD, B, x=x)
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


@pytest.mark.parametrize("B", [33, 200])
def test_engine_noise_step_equals_hand_launched_parts(cuda_device, B):
    dev, steps, seed, sigma = cuda_device, 3, 1, 0.5
    n = steps * B
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    got = {}
    for gs in (0, 3):                                    # eager, and one captured 3-step chunk replayed
        _, ms, t = _trainer(dev, gs, n, B, seed=seed, noise_sigma=sigma)
        assert t.engine.schedule == t.C.SCHED_SERIAL and not t.overlap and t.engine.noise_on
        assert abs(t.engine.noise_sigma - sigma / MNIST_STD) < 1e-6 and t.engine.adversarial_bytes > 0
        got[gs] = _run_stream(t, ms, idx, steps)
    _assert_same(got[0], got[3], "graph replay against eager")
    _assert_same(got[0], _hand_launched(dev, t, idx, steps, B, sigma, seed), "engine against its hand-launched parts")
    _, ms_p, tp = _trainer(dev, 0, n, B, seed=seed, overlap=False)          # and it is not the plain step
    assert not torch.equal(_run_stream(tp, ms_p, idx, steps)["param"], got[0]["param"])


def test_zero_sigma_equals_plain_serial_and_off_means_off(cuda_device):
    dev, B, steps = cuda_device, 33, 3
    n = steps * B
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    _, ms_z, tz = _trainer(dev, 3, n, B, noise_sigma=0.0)
    _, ms_p, tp = _trainer(dev, 3, n, B, overlap=False)
    assert tz.engine.noise_on and not tp.engine.noise_on and tp.noise_sigma is None
    assert tp.engine.adversarial_bytes == 0                       # off: nothing of it is allocated
    assert tz.engine.workspace_bytes == tp.engine.workspace_bytes
    plain = _run_stream(tp, ms_p, idx, steps)
    _assert_same(_run_stream(tz, ms_z, idx, steps), plain, "sigma = 0 against plain SERIAL")
    # switched off on a built trainer: the plain step's launch count and bits
    _, ms_a, ta = _trainer(dev, 3, n, B, noise_sigma=0.5)
    ta.set_noise(None)
    assert ta.noise_sigma is None and not ta.engine.noise_on
    _assert_same(_run_stream(ta, ms_a, idx, steps), plain, "switched off against plain SERIAL")
    nodes = lambda t: t.engine.graph_nodes(t._graphs[(steps, B)])            # launches of the captured chunk
    assert nodes(ta) == nodes(tp) == nodes(tz) - 2 * steps                   # on: adv_init + smooth_noise per step


def test_noise_scope_refusals(cuda_device):
    dev, B = cuda_device, 33
    sigma_n = 0.5 / MNIST_STD
    _, ms, t = _trainer(dev, 0, 3 * B, B, overlap=False)
    before = ms.param.clone()
    t.engine.set_noise(sigma_n, True)
    with pytest.raises(RuntimeError, match="limited to the SERIAL schedule"):
        t.engine.set_schedule(t.C.SCHED_OVERLAP)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        t.engine.set_adversarial(0.3, 0.1, 2, False, -1.0, 1.0)
    t.engine.set_noise(0.0, False)
    t.engine.set_adversarial(0.3, 0.1, 2, False, -1.0, 1.0)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        t.engine.set_noise(sigma_n, True)
    t.engine.set_adversarial(0.0, 0.0, 0, False, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="sigma >= 0"):
        t.engine.set_noise(-1.0, True)
    t.engine.set_schedule(t.C.SCHED_OVERLAP)
    with pytest.raises(RuntimeError, match="limited to the SERIAL schedule"):
        t.engine.set_noise(sigma_n, True)
    with pytest.raises(ValueError, match="SERIAL"):
        t.set_noise(0.5)
    assert not t.engine.noise_on
    _, ms32, t32 = _trainer(dev, 0, 3 * B, B, overlap=False, fp32=True)
    with pytest.raises(RuntimeError, match="limited to the bf16 step"):
        t32.engine.set_noise(sigma_n, True)
    with pytest.raises(ValueError, match="bf16"):
        _trainer(dev, 0, 3 * B, B, fp32=True, noise_sigma=0.5)
    s = t.compute.cuda_stream
    eng2 = t.C.Engine(ms.buffers(), B, 1, int(s), int(t.comm_stream.cuda_stream), 2, ms.rho, ms.eps, ms.weight_decay)
    with pytest.raises(RuntimeError, match="limited to world size 1"):
        eng2.set_noise(sigma_n, True)
    with pytest.raises(ValueError, match="world size 1"):
        FusedTrainer(ms, None, None, B, B, 3 * B, world_size=2, noise_sigma=0.5)
    with pytest.raises(ValueError, match="mutually exclusive"):
        _trainer(dev, 0, 3 * B, B, noise_sigma=0.5, adversarial={"eps": 0.1})
    torch.cuda.synchronize()
    assert torch.equal(ms.param, before) and ms.get_step() == 0


def test_mnist_cli_noise_training_dry_run(gpu_box, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    log = str(tmp_path / "train.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist.py"), "--synthetic", "--synthetic-size", "400",
                        "--synthetic-test-size", "200", "--batch-size", "200", "--epochs", "1", "--noise-train-sigma",
                        "0.25", "--dry-run", "--json-log", log],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(log) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    ep = [x for x in recs if "epoch" in x]
    assert len(ep) == 1 and ep[0]["noise_train_sigma"] == 0.25 and "adv_train_eps" not in ep[0]
    assert [x["schedule"] for x in recs if "schedule" in x] == ["serial"]


# ---------------------------------------------------------------------------- e. it certifies
CERT_N, CERT_B, CERT_SIGMA, CERT_ALPHA = 2400, 100, 0.5, 0.001


def test_noise_training_certifies(cuda_device):
    """Two epochs on 2400 synthetic images (the setup of test_gpu_adv_train's "it defends"), one net plain and one
    with ``noise_sigma = 0.5``; ``certify(sigma = 0.5, n0 = 100, n = 1000)`` on 200 test images each.  Asserted: the
    noise-trained net's certified accuracy at radius 0.5 is strictly higher, and no radius exceeds
    0.5 * Phi^-1(alpha^(1/n)), the radius of a unanimous vote.  The figures at radii 0, 0.25 and 0.5 are printed
    (docs/COVERAGE.md records them); they are measurements, not thresholds."""
    dev = cuda_device
    te = load_mnist(synthetic_data=True, train=False, synthetic_size=200, verbose=False)
    images = te.device_images(dev)
    cap = CERT_SIGMA * NormalDist().inv_cdf(CERT_ALPHA ** (1.0 / 1000))
    res = {}
    for name, sigma in (("plain", None), ("noise", CERT_SIGMA)):
        net, ms, t = _trainer(dev, 6, CERT_N, CERT_B, noise_sigma=sigma, overlap=False)
        lr = 1.0
        for ep in (1, 2):
            t.set_lr(lr)
            t.train_epoch(ep, torch.randperm(CERT_N, generator=torch.Generator().manual_seed(100 + ep)))
            lr *= 0.7
        t.synchronize()
        classes, radii, counts = Predictor(net).certify(images, CERT_SIGMA, n0=100, n=1000, alpha=CERT_ALPHA, seed=5)
        assert (counts.sum(dim=1) == 1000).all() and float(radii.max()) <= cap
        right = classes == te.targets.long()
        res[name] = [int((right & (radii >= r)).sum()) for r in (0.0, 0.25, 0.5)]
        print(f"{name}: certified correct of 200 at radius 0 / 0.25 / 0.5: {res[name]}, abstained "
              f"{int((classes < 0).sum())}, largest radius {float(radii.max()):.4f} (cap {cap:.4f})")
    assert res["noise"][2] > res["plain"][2], res
