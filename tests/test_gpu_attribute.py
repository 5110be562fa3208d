"""Integrated gradients and SmoothGrad on the GPU (MI355X only): ``attr_path`` and ``attr_reduce`` bit for bit
against their numpy float32 emulations, the launcher refusals, ``fused_attribution`` against its seven launches made
by hand and under every chunking, and ``Predictor.attribute`` against the CPU reference on the trained test net."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import PIXEL_LO, _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import attribute as AT
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.ops.smooth import smooth_chunks
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import attr_ref as A
from refmodel import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25
MARGIN = 0.1                                                 # the clear-margin rule of test_gpu_input_grad.py
IG, SG = "integrated_gradients", "smoothgrad"


def _images(M, seed=21):
    imgs, labels = generate(M, seed=seed)
    return imgs.reshape(M, 784).contiguous(), labels


# ---------------------------------------------------------------------------- a. attr_path
def _path(dev, src, n_total, base, sample_base=0, ns=None):
    """One launch into a sentinel-filled buffer with a guard row; returns the rows on the CPU."""
    count = src.shape[0] * (n_total - sample_base if ns is None else ns)
    out = torch.full((count + 1, 784), SENT, dtype=torch.float32, device=dev)
    b = base.to(dev) if isinstance(base, torch.Tensor) else base
    got = Fk.attr_path(src.to(dev), n_total, sample_base, ns, b, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[count] == SENT).all(), "the guard row past M * ns was written"
    return out[:count].numpy()


@pytest.mark.parametrize("M,n", [(1, 1), (3, 5), (2, 257)])
def test_attr_path_bitwise(cuda_device, M, n):
    dev = cuda_device
    u8, _ = _images(M)
    x0 = _PIXEL_LUT[u8.long()].contiguous()
    other = _PIXEL_LUT[_images(M, seed=4)[0].long()].contiguous()
    for base in (0.0, PIXEL_LO, 0.37, other):                # the default scalar, scalars, a tensor of rows
        want = Fk.attr_path_reference(x0, n, base=base)
        for form, src in (("u8", u8), ("f32", x0)):
            got = _path(dev, src, n, base)
            assert np.array_equal(got, want), (form, base if not isinstance(base, torch.Tensor) else "tensor")
            assert np.array_equal(_path(dev, src, n, base), got), "a second launch gives other bits"
    assert np.array_equal(Fk.attr_path(u8.to(dev), n).cpu().numpy(), Fk.attr_path_reference(x0, n))   # out allocated
    if n == 257:                                             # samples [0, 100) + [100, 257) = the whole
        want = Fk.attr_path_reference(x0, n, base=other).reshape(M, n, 784)
        lo = _path(dev, u8, n, other, 0, 100).reshape(M, 100, 784)
        hi = _path(dev, u8, n, other, 100, 157).reshape(M, 157, 784)
        assert np.array_equal(np.concatenate([lo, hi], axis=1), want)
        assert np.array_equal(lo, Fk.attr_path_reference(x0, n, 0, 100, other).reshape(M, 100, 784))


# ---------------------------------------------------------------------------- b. attr_reduce
def _dx(M, n, seed):
    """Gradient rows with magnitudes from 1e-6 to 1e2, both signs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M * n, 784)) * 10.0 ** rng.uniform(-6, 2, (M * n, 784))).astype(np.float32)


def _guarded(dev, M, rows=None):
    t = torch.full((M + 1, 784), SENT, dtype=torch.float32, device=dev)
    if rows is not None:
        t[:M] = torch.from_numpy(rows).to(dev)
    return t


def _take(t, M):
    torch.cuda.synchronize()
    t = t.cpu()
    assert (t[M] == SENT).all(), "the guard row past M was written"
    return t[:M].numpy()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 1000])
def test_attr_reduce_bitwise(cuda_device, M, n):
    dev = cuda_device
    dx = _dx(M, n, seed=n + M)
    assert (dx > 0).any() and (dx < 0).any() and (n == 1 or (np.abs(dx).max() > 1.0 and np.abs(dx).min() < 1e-4))
    dxd = torch.from_numpy(dx).to(dev)
    u8, _ = _images(M, seed=9)
    x0 = _PIXEL_LUT[u8.long()].contiguous()
    base_t = _PIXEL_LUT[_images(M, seed=4)[0].long()].contiguous()
    scale = float(np.float32(-1.0) / np.float32(n))
    # the running sums
    want = Fk.attr_reduce_reference(dx, M, n)
    acc = _guarded(dev, M)
    assert Fk.attr_reduce(dxd, M, n, acc=acc).data_ptr() == acc.data_ptr()
    assert np.array_equal(_take(acc, M), want)
    Fk.attr_reduce(dxd, M, n, acc=acc)                                    # relaunch: the same bits
    assert np.array_equal(_take(acc, M), want)
    assert np.array_equal(Fk.attr_reduce(dxd, M, n).cpu().numpy(), want)  # acc allocated
    # finish: * scale; acc is left alone
    out = _guarded(dev, M)
    Fk.attr_reduce(dxd, M, n, acc=acc, scale=scale, out=out)
    assert np.array_equal(_take(out, M), Fk.attr_reduce_reference(dx, M, n, scale=scale))
    assert np.array_equal(_take(acc, M), want)
    # finish: * scale * (x - b), every source / baseline form; then out aliasing acc
    for src, base in ((u8, base_t), (x0, base_t), (u8, 0.37), (x0, PIXEL_LO)):
        wantp = Fk.attr_reduce_reference(dx, M, n, scale=scale, x=x0, base=base)
        b = base.to(dev) if isinstance(base, torch.Tensor) else base
        out = _guarded(dev, M)
        Fk.attr_reduce(dxd, M, n, scale=scale, x=src.to(dev), base=b, out=out)
        assert np.array_equal(_take(out, M), wantp), (str(src.dtype), type(base).__name__)
    one = _guarded(dev, M)
    got = Fk.attr_reduce(dxd, M, n, acc=one, scale=scale, x=x0.to(dev), base=PIXEL_LO, out=one)
    assert got.data_ptr() == one.data_ptr() and np.array_equal(_take(one, M), wantp)
    # accumulation over two launches = one launch (the second one finishes, in place)
    if n > 1:
        k = 100 if n == 257 else n // 3 + 1
        parts = torch.from_numpy(dx).view(M, n, 784)
        first, second = parts[:, :k].contiguous().to(dev), parts[:, k:].contiguous().to(dev)
        acc2 = _guarded(dev, M)
        Fk.attr_reduce(first, M, k, acc=acc2)
        Fk.attr_reduce(second, M, n - k, acc=acc2, accumulate=True)
        assert np.array_equal(_take(acc2, M), want), (M, n, k)
        Fk.attr_reduce(first, M, k, acc=acc2)
        Fk.attr_reduce(second, M, n - k, acc=acc2, accumulate=True, scale=scale, x=x0.to(dev), base=PIXEL_LO, out=acc2)
        assert np.array_equal(_take(acc2, M), wantp), (M, n, k)
        assert not np.array_equal(Fk.attr_reduce(second, M, n - k).cpu().numpy(), want)      # accumulate matters


def test_attr_reduce_nan_reaches_one_element(cuda_device):
    dev, M, n = cuda_device, 3, 257
    dx = _dx(M, n, seed=2)
    clean = Fk.attr_reduce_reference(dx, M, n, scale=-0.5)
    dx[1 * n + 130, 401] = np.nan
    got = Fk.attr_reduce(torch.from_numpy(dx).to(dev), M, n, scale=-0.5).cpu().numpy()
    assert np.isnan(got[1, 401]) and int(np.isnan(got).sum()) == 1
    got[1, 401] = clean[1, 401]
    assert np.array_equal(got, clean)


def test_attr_launcher_refusals(cuda_device):
    dev = cuda_device
    x = torch.zeros(2, 784, dtype=torch.float32, device=dev)
    dx = torch.zeros(8, 784, dtype=torch.float32, device=dev)
    acc = torch.zeros(2, 784, dtype=torch.float32, device=dev)
    for kw in (dict(x=x.double()), dict(x=x.cpu()), dict(x=x[:, :780]), dict(base=x.double()), dict(base=x.cpu()),
               dict(base=x[:1]), dict(out=dx.double()), dict(out=dx[:3]), dict(out=dx.cpu()), dict(sample_base=2, ns=3),
               dict(sample_base=-1, ns=2), dict(ns=0), dict(base="black")):
        args = dict(x=x, n_total=4)
        args.update(kw)
        with pytest.raises(ValueError, match="attr_path"):
            Fk.attr_path(**args, out=dx) if "out" not in args else Fk.attr_path(**args)
    with pytest.raises(ValueError, match="SMOOTH_MAX_ROWS"):
        Fk.attr_path(x, Fk.SMOOTH_MAX_ROWS, ns=Fk.SMOOTH_MAX_ROWS // 2 + 1)               # too many rows
    with pytest.raises(ValueError, match="ATTR_MAX_STEPS"):
        Fk.attr_path(x, Fk.ATTR_MAX_STEPS + 1, ns=1)
    for kw in (dict(dx=dx.double()), dict(dx=dx.cpu()), dict(dx=dx[:7]), dict(acc=acc.double()), dict(acc=acc[:1]),
               dict(acc=acc.cpu()), dict(accumulate=True, acc=None), dict(out=acc), dict(x=x),
               dict(scale=-0.25, out=acc.double()), dict(scale=-0.25, x=x.double()), dict(scale=-0.25, x=x.cpu()),
               dict(scale=-0.25, x=x, base=x.cpu()), dict(M=0)):
        args = dict(dx=dx, M=2, ns=4, acc=acc)
        args.update(kw)
        with pytest.raises(ValueError, match="attr_reduce"):
            Fk.attr_reduce(**args)
    with pytest.raises(ValueError, match="SMOOTH_MAX_ROWS"):
        Fk.attr_reduce(dx, 2, Fk.SMOOTH_MAX_ROWS // 2 + 1, acc=acc)                        # too many rows
    # the launchers themselves: null, misaligned and out-of-range arguments launch nothing
    C, p, s = Fk.native.load(), Fk.native.ptr, Fk.native.stream_handle()
    for args in ((0, 0, 0, 0.0, p(dx), 0, 4, 2, 4, s),                                     # no source
                 (0, p(x), 0, 0.0, 0, 0, 4, 2, 4, s),                                      # no output
                 (0, p(x) + 4, 0, 0.0, p(dx), 0, 4, 1, 4, s),                              # misaligned source
                 (0, p(x), p(x) + 4, 0.0, p(dx), 0, 4, 1, 4, s),                           # misaligned baseline
                 (0, p(x), 0, 0.0, p(dx), 2, 4, 2, 3, s),                                  # sample_base + ns > n_total
                 (0, p(x), 0, 0.0, p(dx), 0, 1 << 23, 2, (1 << 22) + 1, s)):               # M * ns out of range
        with pytest.raises(RuntimeError, match="attr_path"):
            C.attr_path(*args)
    for args in ((0, p(acc), 0, 0, 0, 0, 0.0, 0.0, 2, 4, False, 0, s),                     # no rows
                 (p(dx), p(acc), 0, 0, 0, 0, 0.0, -0.25, 2, 4, False, 1, s),               # finish without out
                 (p(dx), p(acc), p(acc), 0, 0, 0, 0.0, -0.25, 2, 4, False, 2, s),          # path finish without x
                 (p(dx), p(acc), p(acc), 0, 0, 0, 0.0, -0.25, 2, 4, False, 3, s),          # unknown finish
                 (p(dx) + 4, p(acc), 0, 0, 0, 0, 0.0, 0.0, 1, 4, False, 0, s),             # misaligned rows
                 (p(dx), p(acc), 0, 0, 0, 0, 0.0, 0.0, 2, (1 << 22) + 1, False, 0, s)):    # M * ns out of range
        with pytest.raises(RuntimeError, match="attr_reduce"):
            C.attr_reduce(*args)
    torch.cuda.synchronize()
    assert not dx.any() and not acc.any()


# ---------------------------------------------------------------------------- c. the native loop
def _seeded_net(dev, seed=3):
    torch.manual_seed(seed)
    return Net().to(dev)


def _by_hand(net, src, labels, method, n, base=PIXEL_LO, sigma_n=0.0, seed=0, id_base=0):
    """The seven launches of one chunk holding every image, through ``ops.functional``, on buffers of their own."""
    st = fused_state(net)
    st.sync()
    ms, dev = st.ms, src.device
    M = src.shape[0]
    buf = Fk.StepBuffers.allocate(M * n, dev)
    state = torch.tensor([1 << 32, 0, 0], dtype=torch.int64).to(dev)     # step 0 | NO_DROPOUT, zero seed / counter
    lab = labels.to(dev, torch.int32).repeat_interleave(n)
    if method == IG:
        x = Fk.attr_path(src, n, base=base)
    else:
        x = Fk.smooth_noise(src, sigma_n, n, seed, 0, id_base)
    Fk.trunk_fwd(ms, None, None, buf, True, state=state, xin=x)
    Fk.fc1_fwd(ms, buf)
    Fk.head_train(ms, lab, None, buf, state=state, inv_batch=1.0)
    Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=state)
    dx = Fk.input_grad(ms, buf)
    scale = float(np.float32(-1.0) / np.float32(n))
    if method == IG:
        return Fk.attr_reduce(dx, M, n, scale=scale, x=src, base=base)
    return Fk.attr_reduce(dx, M, n, scale=scale)


QUERIES = ("conv_wgrad_groups", "fc_bwd_splits")             # StepBuffers.allocate's sizing questions: pure host code


class _Recorder:
    """The native module with every call's name noted, but for the pure host queries (they launch nothing)."""

    def __init__(self, C):
        self._C, self.calls = C, []

    def __getattr__(self, name):
        v = getattr(self._C, name)
        if not callable(v):
            return v

        def call(*a, **k):
            if name not in QUERIES:
                self.calls.append(name)
            return v(*a, **k)
        return call


def _chunk_launches(method):
    return ["attr_path" if method == IG else "smooth_noise", "trunk_fwd", "fc1_fwd", "head_train", "fc_bwd",
            "input_grad", "attr_reduce"]


@pytest.mark.parametrize("method", [IG, SG])
def test_fused_attribution_equals_hand_launches_under_any_chunking(cuda_device, monkeypatch, method):
    """B = 3, n = 32: the loop equals its seven launches made by hand, bit for bit, at ``rows_per_launch`` 8192 (one
    chunk), 96, 64 (two chunks of whole images), 32 and 16 (sample chunks: the accumulate path) - every launch below
    fc1_fwd's 512-row split change - and runs exactly those seven launches once per chunk of the plan.  The net's
    mode, parameters, ``.grad`` and counter stream are untouched; the buffers are reused across calls."""
    dev, B, n = cuda_device, 3, 32
    net = _seeded_net(dev).train()
    pr = Predictor(net)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    grads = {k: None if v.grad is None else v.grad.clone() for k, v in net.named_parameters()}
    st = fused_state(net)
    offset = st.rng_offset
    u8, labels = _images(B, seed=8)
    src, sigma_n, seed = u8.to(dev), 0.15 / MNIST_STD, 77
    want = _by_hand(net, src, labels, method, n, PIXEL_LO, sigma_n, seed)
    assert torch.isfinite(want).all() and want.any()
    xf = _PIXEL_LUT[u8.long()].contiguous().to(dev)
    assert torch.equal(_by_hand(net, xf, labels, method, n, PIXEL_LO, sigma_n, seed), want)     # fp32 source form
    torch.cuda.synchronize()
    rec = _Recorder(AT.native.load())
    monkeypatch.setattr(AT.native, "load", lambda *a, **k: rec)
    for rpl, chunks in ((8192, 1), (96, 1), (64, 2), (32, 3), (16, 6)):
        plan = smooth_chunks(B, n, [0, 1, 2], rpl)
        assert len(plan) == chunks and max(m * ns for _, m, _, ns in plan) < 512, (rpl, plan)
        rec.calls.clear()
        got = AT.fused_attribution(net, src, labels.to(dev), method, n, PIXEL_LO, sigma_n, seed, rows_per_launch=rpl)
        assert rec.calls == _chunk_launches(method) * chunks, (rpl, rec.calls)
        assert got.shape == (B, 784) and got.dtype == torch.float32 and torch.equal(got, want), rpl
    assert any(s0 > 0 for _, _, s0, _ in smooth_chunks(B, n, [0, 1, 2], 16))               # rpl = 16 accumulates
    # the Predictor's call goes through the same loop (its own forward of the clean input comes first)
    rec.calls.clear()
    a, lp = pr.attribute(u8.view(B, 28, 28), labels, method, steps=n, sigma=0.15, seed=seed)
    assert rec.calls[-7:] == _chunk_launches(method) and "attr_reduce" not in rec.calls[:-7]
    assert torch.equal(a.reshape(B, 784), want) and a.shape == (B, 1, 28, 28) and torch.equal(lp, pr.log_probs(u8))
    # buffer reuse across calls: the row / gradient buffers stay, the activation set returns to the pool
    abuf = st.attr_buf
    ptrs, pooled = (abuf.x.data_ptr(), abuf.dx.data_ptr()), sum(len(v) for v in st.pool.values())
    again, _ = pr.attribute(xf.view(B, 1, 28, 28), labels, method, steps=n, sigma=0.15, seed=seed)
    assert torch.equal(again.reshape(B, 784), want)
    assert st.attr_buf is abuf and (abuf.x.data_ptr(), abuf.dx.data_ptr()) == ptrs
    assert sum(len(v) for v in st.pool.values()) == pooled
    if method == SG:                                         # ids name the draw: image j alone under id j = row j
        for j in range(B):
            alone, _ = pr.attribute(u8[j:j + 1], labels[j:j + 1], SG, steps=n, sigma=0.15, seed=seed, ids=[j])
            assert torch.equal(alone.reshape(784), want[j]), j
        rec.calls.clear()
        split, _ = pr.attribute(u8, labels, SG, steps=n, sigma=0.15, seed=seed, ids=[0, 1, 5])
        assert rec.calls.count("smooth_noise") == 2          # ids that are not consecutive split a launch
        assert torch.equal(split.reshape(B, 784)[:2], want[:2]) and not torch.equal(split.reshape(B, 784)[2], want[2])
        other, _ = pr.attribute(u8, labels, SG, steps=n, sigma=0.15, seed=seed + 1)
        assert not torch.equal(other.reshape(B, 784), want)
    else:                                                    # a tensor baseline, chunked over images: row offsets
        base = _PIXEL_LUT[_images(B, seed=4)[0].long()].contiguous().to(dev)
        wb = _by_hand(net, src, labels, IG, n, base)
        for rpl in (96, 32, 16):
            got = AT.fused_attribution(net, src, labels.to(dev), IG, n, base, rows_per_launch=rpl)
            assert torch.equal(got, wb) and not torch.equal(got, want), rpl
    # nothing of the net moved
    assert st.rng_offset == offset and net.training
    assert all(torch.equal(v, before[k]) for k, v in net.named_parameters())
    for k, v in net.named_parameters():
        assert (v.grad is None) == (grads[k] is None) and (v.grad is None or torch.equal(v.grad, grads[k])), k


@pytest.mark.parametrize("method", [IG, SG])
def test_across_the_512_row_split_change(cuda_device, method):
    """B = 2, n = 300: one launch of 600 rows (fc1_fwd splits K 4 ways) against two of 300 (32 ways).  The gradient
    rows can differ in their last bits there, so only the cap a single bf16 gradient is held to is asserted; the
    value is printed (docs/COVERAGE.md)."""
    dev = cuda_device
    net = copy.deepcopy(A.trained_net()).to(dev)
    u8, labels = _images(2, seed=8)
    args = (net, u8.to(dev), labels.to(dev), method, 300, PIXEL_LO, 0.15 / MNIST_STD, 5)
    one = AT.fused_attribution(*args, rows_per_launch=600)
    two = AT.fused_attribution(*args, rows_per_launch=300)
    err = rel_err(one, two)
    print(f"{method}: rel_err(600 rows a launch, 300 rows a launch) = {err:.3e}")
    assert torch.isfinite(one).all() and two.any() and err < 0.1, err


# ---------------------------------------------------------------------------- d. against the CPU reference
@functools.lru_cache(maxsize=None)
def _cpu_case(B, with_labels):
    """Images, labels and the CPU Predictor's integrated gradients (n = 32): computed once, never modified."""
    imgs, labels = generate(B, seed=5)
    a, lp = Predictor(A.trained_net()).attribute(imgs, labels if with_labels else None, IG, steps=32)
    return imgs, labels, a, lp


@pytest.fixture(scope="module")
def gpu_predictor(cuda_device):
    return Predictor(copy.deepcopy(A.trained_net()).to(cuda_device).train())   # train mode: must not matter


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("form", ["u8", "float"])
@pytest.mark.parametrize("B", [1, 33])
def test_integrated_gradients_match_cpu_reference(cuda_device, gpu_predictor, B, form, with_labels):
    imgs, labels, a_ref, lp_ref = _cpu_case(B, with_labels)
    pr = gpu_predictor
    assert pr.native
    x = imgs.to(cuda_device) if form == "u8" else normalize_u8(imgs).to(cuda_device)
    a, lp = pr.attribute(x, labels.to(cuda_device) if with_labels else None, IG, steps=32)
    assert a.shape == (B, 1, 28, 28) and a.dtype == torch.float32 and a.is_cuda and lp.shape == (B, 10)
    assert torch.isfinite(a).all() and not a.requires_grad and (lp.cpu() - lp_ref).abs().max().item() < 5e-2
    assert pr.net.training and all(p.grad is None or not p.grad.any().item() for p in pr.net.parameters())
    rows = torch.ones(B, dtype=torch.bool)
    if not with_labels:                                     # the predicted class: clear rows only
        top2 = lp_ref.topk(2, dim=1).values
        rows = (top2[:, 0] - top2[:, 1]) > MARGIN
        assert (~rows).float().mean().item() <= 0.10
        assert torch.equal(lp.cpu().argmax(1)[rows], lp_ref.argmax(1)[rows])
    err = rel_err(a.cpu()[rows], a_ref[rows])
    print(f"integrated gradients B={B} {form} labels={with_labels} rows={int(rows.sum())} rel_err(attr)={err:.4f}")
    assert a_ref[rows].norm() > 0
    assert err < 0.1, err


def test_completeness_on_the_gpu(gpu_predictor):
    """G(n) on the GPU's own attributions and log-probabilities, the 16 images of the CPU test."""
    g = {n: A.G(gpu_predictor, n) for n in (1, 64)}
    print("completeness gap on the GPU: " + ", ".join(f"G_gpu({n}) = {v:.5f}" for n, v in g.items()))
    assert g[64] <= 0.5 * g[1], g


def test_smoothgrad_is_minus_the_mean_input_gradient(cuda_device, gpu_predictor):
    """(B, n) = (2, 8): SmoothGrad equals -1/n times the sum, in ascending sample order, of
    ``Predictor.input_gradient`` over the same ``smooth_noise`` rows, bit for bit."""
    dev, pr, B, n, sigma, seed = cuda_device, gpu_predictor, 2, 8, 0.15, 11
    u8, labels = _images(B, seed=8)
    a, _ = pr.attribute(u8, labels, SG, steps=n, sigma=sigma, seed=seed)
    rows = Fk.smooth_noise(u8.to(dev), sigma / MNIST_STD, n, seed)
    g, _ = pr.input_gradient(rows.view(B * n, 1, 28, 28), labels.repeat_interleave(n))
    want = Fk.attr_reduce_reference(g.reshape(B * n, 784), B, n, scale=float(np.float32(-1.0) / np.float32(n)))
    assert np.array_equal(a.reshape(B, 784).cpu().numpy(), want) and np.abs(want).sum() > 0


def test_smoothgrad_approaches_cpu_reference_with_more_samples(cuda_device, gpu_predictor):
    """The noise bits differ between the paths, so no elementwise cap: the distance to the CPU reference of the
    same n must shrink from n = 4 to n = 256.  Both are printed (docs/COVERAGE.md)."""
    imgs, labels = generate(4, seed=5)
    cpu = Predictor(A.trained_net())
    err = {}
    for n in (4, 256):
        a_ref, _ = cpu.attribute(imgs, labels, SG, steps=n, sigma=0.15, seed=3)
        a, _ = gpu_predictor.attribute(imgs.to(cuda_device), labels, SG, steps=n, sigma=0.15, seed=3)
        err[n] = rel_err(a.cpu(), a_ref)
    print(f"SmoothGrad rel_err against the CPU reference: n = 4: {err[4]:.4f}, n = 256: {err[256]:.4f}")
    assert err[256] < err[4], err


# ---------------------------------------------------------------------------- e. the command line
@pytest.mark.parametrize("method", [IG, SG])
def test_predict_cli_attribution_on_gpu(gpu_box, tmp_path, method):
    torch.manual_seed(5)
    ckpt, out, log = str(tmp_path / "mnist_cnn.pt"), str(tmp_path / "attr.npy"), str(tmp_path / "log.jsonl")
    save_state_dict(Net(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "64", "--checkpoint", ckpt, "--batch-size", "40", "--json-log", log, "--saliency", out,
                        "--saliency-method", method, "--saliency-steps", "8"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert got.shape == (64, 28, 28) and got.dtype == np.float32 and np.isfinite(got).all() and got.any()
    with open(log) as f:
        rec = [json.loads(ln) for ln in f if ln.strip()]
    assert len(rec) == 1 and rec[0]["device"].startswith("cuda")
    assert rec[0]["saliency_method"] == method and rec[0]["saliency_steps"] == 8
    if method == IG:
        gap = rec[0]["saliency_completeness_gap"]
        assert rec[0]["saliency_baseline"] == 0.0 and gap >= 0.0 and gap == gap and gap != float("inf")
    else:
        assert rec[0]["saliency_sigma"] == 0.15 and rec[0]["saliency_seed"] == 0
