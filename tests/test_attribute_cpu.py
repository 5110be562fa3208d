"""Attribution on the CPU side: ``reference_attribution`` against a written-out autograd loop, the numpy emulations
of ``attr_path`` / ``attr_reduce`` (chunking, the mutation proofs of the comparators), completeness of integrated
gradients on the trained test net, the argument checks, and the ``--saliency-method`` options end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import (PIXEL_LO, _PIXEL_LUT, Predictor, build_predict_parser,
                                             reference_attribution)
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import attr_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _grad_rows(net, rows, label):
    """d sum-NLL_label / d rows by plain autograd over forward_reference in eval mode: numpy [ns, 784]."""
    was = net.training
    net.eval()
    xg = rows.clone().requires_grad_()
    lp = net.forward_reference(xg.view(-1, 1, 28, 28))
    g, = torch.autograd.grad(F.nll_loss(lp, torch.full((rows.shape[0],), int(label)), reduction='sum'), xg)
    net.train(was)
    return g.numpy()


def _written_out(net, x0, labels, method, n, base=PIXEL_LO, sigma_n=0.0, seed=0, variant=None):
    """The definitions spelled out: one autograd call per image over its n rows, a float32 add per sample in
    ascending order, then * float32(-1/n) [* (x - b)].  ``variant`` names a deliberate mistake (mutation proofs)."""
    B = x0.shape[0]
    out = np.zeros((B, 784), dtype=f32)
    for j in range(B):
        x = x0[j].numpy()
        if method == "integrated_gradients":
            off = f32(0.0) if variant == "left_endpoint" else f32(0.5)
            alpha = (np.arange(n).astype(f32) + off) / f32(n)
            d = x - f32(base)
            rows = torch.from_numpy(f32(base) + (alpha[:, None] * d[None, :]).astype(f32))
        else:
            gen = torch.Generator().manual_seed((seed * 0x9E3779B97F4A7C15 + j) & (2 ** 63 - 1))
            rows = x0[j] + sigma_n * torch.randn(n, 784, generator=gen, dtype=torch.float32)
        g = _grad_rows(net, rows, labels[j])
        t = np.zeros(784, dtype=f32)
        for s in range(n - 1 if variant == "last_dropped" else n):
            t = t + g[s]
        t = t * (f32(1.0) / f32(n) if variant == "no_sign" else f32(-1.0) / f32(n))
        if method == "integrated_gradients" and variant != "no_difference":
            t = t * (x - f32(base))
        out[j] = t
    return out


def _seeded(B=3):
    torch.manual_seed(3)
    net = Net().train()                                      # inference semantics whatever the mode
    imgs, labels = generate(B, seed=5)
    return net, imgs, labels, _PIXEL_LUT[imgs.reshape(B, 784).long()]


@pytest.mark.parametrize("method,n", [("integrated_gradients", 1), ("integrated_gradients", 5), ("smoothgrad", 4)])
def test_reference_attribution_is_the_written_out_loop_bitwise(method, n):
    net, imgs, labels, x0 = _seeded()
    sigma = 0.15
    want = _written_out(net, x0, labels, method, n, sigma_n=sigma / MNIST_STD, seed=7)
    got = reference_attribution(net, x0, labels, method, n, PIXEL_LO, sigma / MNIST_STD, 7)
    assert got.dtype == torch.float32 and got.shape == (3, 784)
    assert np.array_equal(got.numpy(), want) and np.abs(want).sum() > 0
    pr = Predictor(net)
    assert not pr.native
    for inp in (imgs, imgs.reshape(3, 784), x0.view(3, 1, 28, 28)):
        a, lp = pr.attribute(inp, labels, method, steps=n, sigma=sigma, seed=7)
        assert a.shape == (3, 1, 28, 28) and a.dtype == torch.float32 and not a.requires_grad
        assert np.array_equal(a.reshape(3, 784).numpy(), want)
        assert torch.equal(lp, pr.log_probs(inp))
    a_pred, _ = pr.attribute(imgs, None, method, steps=n, sigma=sigma, seed=7)      # labels None: the predicted class
    a_same, _ = pr.attribute(imgs, pr.predict(imgs), method, steps=n, sigma=sigma, seed=7)
    assert torch.equal(a_pred, a_same)
    assert net.training and all(p.grad is None for p in net.parameters())
    # the mutation proofs: each mistake in the written-out loop is seen by this comparison
    if method == "integrated_gradients":
        for variant in ("left_endpoint", "no_sign", "no_difference") + (("last_dropped",) if n > 1 else ()):
            assert not np.array_equal(_written_out(net, x0, labels, method, n, variant=variant), want), variant
    else:
        for variant in ("no_sign", "last_dropped"):
            bad = _written_out(net, x0, labels, method, n, sigma_n=sigma / MNIST_STD, seed=7, variant=variant)
            assert not np.array_equal(bad, want), variant
        ids, _ = pr.attribute(imgs[1:2], labels[1:2], method, steps=n, sigma=sigma, seed=7, ids=[1])
        assert np.array_equal(ids.reshape(784).numpy(), want[1])                    # ids name the draw


def test_baseline_equal_to_the_image_gives_zeros_and_baseline_forms():
    net, imgs, labels, x0 = _seeded()
    pr = Predictor(net)
    for base in (imgs, x0.view(3, 1, 28, 28)):
        a, _ = pr.attribute(imgs, labels, steps=1, baseline=base)
        assert a.shape == (3, 1, 28, 28) and not a.any()
    black, _ = pr.attribute(imgs, labels, steps=4)
    zero, _ = pr.attribute(imgs, labels, steps=4, baseline=0.0)
    tens, _ = pr.attribute(imgs, labels, steps=4, baseline=torch.zeros(3, 28, 28, dtype=torch.uint8))
    assert torch.equal(black, zero) and torch.equal(black, tens) and black.any()
    grey, _ = pr.attribute(imgs, labels, steps=4, baseline=0.5)
    assert not torch.equal(grey, black)


def test_attr_path_reference_properties():
    _, imgs, _, x0 = _seeded()
    for n in (1, 2, 5, 32, 257):
        rows = Fk.attr_path_reference(x0, n, base=PIXEL_LO).reshape(3, n, 784)
        # alpha spans (0, 1) symmetrically: alpha_s + alpha_{n-1-s} = 1, seen on the pixel that moves most
        d = x0.numpy() - f32(PIXEL_LO)
        j = int(np.abs(d[0]).argmax())
        alpha = (rows[0, :, j].astype(np.float64) - PIXEL_LO) / float(d[0, j])
        assert (alpha > 0).all() and (alpha < 1).all() and (np.diff(alpha) > 0).all()
        assert np.allclose(alpha + alpha[::-1], 1.0, atol=1e-5) and abs(alpha[0] - 0.5 / n) < 1e-5
        # sample_base chunks concatenate to the whole, bit for bit; uint8 source = the LUT rows
        k = n // 3 + 1
        if k < n:
            lo = Fk.attr_path_reference(x0, n, 0, k, PIXEL_LO).reshape(3, k, 784)
            hi = Fk.attr_path_reference(x0, n, k, None, PIXEL_LO).reshape(3, n - k, 784)
            assert np.array_equal(np.concatenate([lo, hi], axis=1), rows)
        assert np.array_equal(Fk.attr_path_reference(imgs.reshape(3, 784), n, base=PIXEL_LO).reshape(3, n, 784), rows)
    tens = Fk.attr_path_reference(x0, 4, base=torch.full((3, 784), PIXEL_LO))
    assert np.array_equal(tens, Fk.attr_path_reference(x0, 4, base=PIXEL_LO))
    # mutation: left-endpoint alpha is another set of rows
    left = f32(PIXEL_LO) + ((np.arange(4).astype(f32) / f32(4))[None, :, None] * d[:, None, :]).astype(f32)
    assert not np.array_equal(left.reshape(12, 784), Fk.attr_path_reference(x0, 4, base=PIXEL_LO))
    for bad in (dict(n_total=0), dict(n_total=4, sample_base=2, ns=3), dict(n_total=4, sample_base=-1)):
        with pytest.raises(ValueError):
            Fk.attr_path_reference(x0, **bad)


def test_attr_reduce_reference_chunking_and_mutations():
    rng = np.random.default_rng(5)
    M, n = 3, 257
    dx = (rng.standard_normal((M, n, 784)) * 10.0 ** rng.uniform(-6, 2, (M, n, 1))).astype(f32)
    flat = dx.reshape(M * n, 784)
    whole = Fk.attr_reduce_reference(flat, M, n)
    loop = np.zeros((M, 784), dtype=f32)
    for s in range(n):
        loop = loop + dx[:, s]
    assert np.array_equal(whole, loop)
    assert not np.array_equal(whole, dx.astype(np.float64).sum(axis=1).astype(f32))    # (an order, not the exact sum)
    first = Fk.attr_reduce_reference(np.ascontiguousarray(dx[:, :100]).reshape(-1, 784), M, 100)
    both = Fk.attr_reduce_reference(np.ascontiguousarray(dx[:, 100:]).reshape(-1, 784), M, 157, acc=first)
    assert np.array_equal(both, whole)                                   # chunked accumulation = one pass, bitwise
    # mutations: accumulate ignored, last sample dropped
    assert not np.array_equal(Fk.attr_reduce_reference(np.ascontiguousarray(dx[:, 100:]).reshape(-1, 784), M, 157), whole)
    assert not np.array_equal(Fk.attr_reduce_reference(np.ascontiguousarray(dx[:, :-1]).reshape(-1, 784), M, n - 1), whole)
    # the finish forms
    scale = float(f32(-1.0) / f32(n))
    x = rng.standard_normal((M, 784)).astype(f32)
    assert np.array_equal(Fk.attr_reduce_reference(flat, M, n, scale=scale), whole * f32(scale))
    path = Fk.attr_reduce_reference(flat, M, n, scale=scale, x=x, base=0.25)
    assert np.array_equal(path, (whole * f32(scale)) * (x - f32(0.25)))
    assert not np.array_equal(Fk.attr_reduce_reference(flat, M, n, scale=-scale), whole * f32(scale))   # the sign
    assert not np.array_equal(path, whole * f32(scale))                                                # (x - b)


def test_completeness_on_the_trained_net():
    """G(n) = sum over the 16 completeness images of |sum attr - (log p_y(x) - log p_y(black))| on the CPU
    reference; measured 40.20, 0.455, 0.0639, 0.0237 at n = 1, 16, 64, 256 (docs/COVERAGE.md)."""
    pr = Predictor(A.trained_net())
    g = {n: A.G(pr, n) for n in (1, 16, 64, 256)}
    print("completeness gap G(n) on the CPU reference: " + ", ".join(f"G({n}) = {v:.5f}" for n, v in g.items()))
    assert g[64] <= 0.5 * g[1], g
    assert g[256] <= g[16], g


def test_attribute_value_errors():
    net, imgs, labels, _ = _seeded()
    pr = Predictor(net)
    for kw in (dict(method="gradient"), dict(steps=0), dict(steps=2.5), dict(steps=-3),
               dict(method="smoothgrad", sigma=0.0), dict(method="smoothgrad", sigma=-1.0),
               dict(labels=labels[:2]), dict(labels=torch.tensor([0, 10, 3])), dict(labels=torch.tensor([0, -1, 3])),
               dict(baseline=torch.zeros(2, 28, 28)), dict(baseline="black"),
               dict(method="smoothgrad", ids=[0, 1])):
        args = dict(labels=labels)
        args.update(kw)
        with pytest.raises(ValueError):
            pr.attribute(imgs, **args)
    with pytest.raises(ValueError):
        pr.attribute(torch.zeros(2, 3, 28, 28))
    with pytest.raises(ValueError):
        reference_attribution(net, torch.zeros(1, 784), torch.zeros(1), "gradient", 2)


def test_predict_parser_saliency_method_defaults():
    ap = build_predict_parser()
    a = ap.parse_args([])
    assert (a.saliency_method, a.saliency_steps, a.saliency_sigma, a.saliency_baseline, a.saliency_seed) == \
        ("gradient", 32, 0.15, None, 0)
    a = ap.parse_args(["--saliency", "o.npy", "--saliency-method", "smoothgrad", "--saliency-steps", "8",
                       "--saliency-sigma", "0.3", "--saliency-seed", "5", "--saliency-baseline", "0.5"])
    assert (a.saliency_method, a.saliency_steps, a.saliency_sigma, a.saliency_baseline, a.saliency_seed) == \
        ("smoothgrad", 8, 0.3, 0.5, 5)
    with pytest.raises(SystemExit):
        ap.parse_args(["--saliency-method", "lime"])


def _run_predict(tmp_path, *extra, size=64):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    if os.path.exists(log):
        os.remove(log)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", str(size), "--checkpoint", ckpt, "--batch-size", "40",
                        "--json-log", log, *extra],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(log) as f:
        rec = [json.loads(ln) for ln in f if ln.strip()]
    assert len(rec) == 1
    return net, r.stdout, rec[0]


def test_predict_cli_gradient_saliency_is_unchanged(tmp_path):
    out0, out1 = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    net, stdout0, rec0 = _run_predict(tmp_path, "--saliency", out0)
    _, stdout1, rec1 = _run_predict(tmp_path, "--saliency", out1, "--saliency-method", "gradient",
                                    "--saliency-steps", "7")
    assert stdout0 == stdout1 and rec0 == rec1
    assert set(rec0) == {"checkpoint", "device", "source", "test_loss", "correct", "n"}
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=64, verbose=False)
    pr = Predictor(net)
    want = np.empty((64, 28, 28), dtype=np.float32)
    for i in (0, 40):
        want[i:i + 40] = pr.input_gradient(data.images[i:i + 40], data.targets[i:i + 40])[0].reshape(-1, 28, 28).numpy()
    ref = str(tmp_path / "want.npy")
    with open(ref, "wb") as f:
        np.save(f, want)
    with open(ref, "rb") as f, open(out0, "rb") as g, open(out1, "rb") as h:
        blob = f.read()
        assert g.read() == blob and h.read() == blob                     # byte-identical files


@pytest.mark.parametrize("method", ["integrated_gradients", "smoothgrad"])
def test_predict_cli_attribution_on_cpu(tmp_path, method):
    out = str(tmp_path / "attr.npy")
    net, stdout, rec = _run_predict(tmp_path, "--saliency", out, "--saliency-method", method, "--saliency-steps", "4",
                                    "--saliency-sigma", "0.2", "--saliency-seed", "3")
    assert len([ln for ln in stdout.splitlines() if ln.startswith("Test set:")]) == 1
    got = np.load(out)
    assert got.shape == (64, 28, 28) and got.dtype == np.float32
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=64, verbose=False)
    pr = Predictor(net)
    want, lp = pr.attribute(data.images, data.targets, method, steps=4, sigma=0.2, seed=3, ids=range(64))
    assert np.array_equal(got, want.reshape(64, 28, 28).numpy())         # image ids are the split indices
    assert rec["saliency_method"] == method and rec["saliency_steps"] == 4
    if method == "smoothgrad":
        assert rec["saliency_sigma"] == 0.2 and rec["saliency_seed"] == 3
        assert "saliency_baseline" not in rec and "saliency_completeness_gap" not in rec
    else:
        assert rec["saliency_baseline"] == 0.0 and "saliency_sigma" not in rec and "saliency_seed" not in rec
        y = data.targets.long().view(-1, 1)
        lp_b = pr.log_probs(torch.full((1, 1, 28, 28), PIXEL_LO))[0]
        delta = lp.gather(1, y)[:, 0].double() - lp_b[y[:, 0]].double()
        gap = float((want.reshape(64, 784).double().sum(1) - delta).abs().mean())
        assert abs(rec["saliency_completeness_gap"] - gap) <= 1e-4       # (float32 log-probs: the CLI's batches are 40)
