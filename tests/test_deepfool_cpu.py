"""Minimum-norm adversarial examples (L2 DeepFool) on the CPU side: ``reference_minimum_norm`` and
``deepfool_step_reference`` against the step written out per image, the properties of the result on the trained test
net, the mutation proofs of the comparator the GPU tests use, the operands of those tests, the argument checks, and the
``--min-norm`` options of ``mnist_predict.py`` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist
from pytorch_mnist_ddp_amd.inference import (_PIXEL_LUT, Predictor, build_predict_parser, minimum_norm_line,
                                             minimum_norm_stats, reference_minimum_norm)
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict
from pytorch_mnist_ddp_amd.utils.logging import test_line as _test_line

import deepfool_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _written_out(net, x0, labels, steps, overshoot=D.OVERSHOOT):
    """DeepFool spelled out: per iteration one autograd pass over the ten rows of every image, labelled 0 .. 9, then
    ``deepfool_ref.step_one`` image by image; stops once no image is still running.  Also returns every iteration's
    operands and results (for the per-step comparison)."""
    B = x0.shape[0]
    was = net.training
    net.eval()
    lab10 = torch.arange(10).repeat(B)
    state = D._blank(B, x0)
    trace = []
    for _ in range(steps):
        rows = state["x"].repeat_interleave(10, dim=0).requires_grad_()
        lp = net.forward_reference(rows.view(10 * B, 1, 28, 28))
        g, = torch.autograd.grad(F.nll_loss(lp, lab10, reduction='sum'), rows)
        ops = dict(state, dx=g, loss=-lp.detach()[torch.arange(10 * B), lab10], y=labels.to(torch.int32))
        new = D.step_images(ops)
        trace.append((ops, new))
        state = dict(state, **{k: new[k] for k in D.KEYS})
        if not (state["status"] == 0).any():
            break
    net.train(was)
    return state, trace


@pytest.mark.parametrize("steps", [2, 50])
def test_reference_minimum_norm_is_the_written_out_loop_bitwise(steps):
    net = D.trained_net()
    imgs, labels = D.trained_case()
    x0 = _PIXEL_LUT[imgs[:6].reshape(6, 784).long()]
    y = labels[:6].clone()
    y[5] = (y[5] + 1) % 10                                   # one image that is outside its label on entry
    want, trace = _written_out(net, x0, y, steps)
    x_adv, norm, iters, status = reference_minimum_norm(net, x0, y, steps, D.OVERSHOOT, D.LO, D.HI)
    assert x_adv.dtype == torch.float32 and iters.dtype == torch.int32 and status.dtype == torch.int32
    assert torch.equal(x_adv, want["x"]) and torch.equal(norm, want["norm"])
    assert torch.equal(iters, want["iters"]) and torch.equal(status, want["status"])
    assert int(status[5]) == 1 and int(iters[5]) == 0 and float(norm[5]) == 0.0 and torch.equal(x_adv[5], x0[5])
    assert (iters[:5] >= 1).all() and (norm[:5] > 0).all()
    if steps == 2:
        assert (status == 0).any(), "steps = 2 was meant to leave an image running"
    else:
        assert (status == 1).all() and len(trace) < 50       # every image crossed, and the loop ended early
    # deepfool_step_reference in fp32 equals the written-out step, iteration by iteration
    for ops, new in trace:
        got = D.reference_step(ops)
        for k in D.KEYS:
            assert torch.equal(got[k], new[k]), k
    # the Predictor's CPU path is that loop; its own forward judges the result
    pr = Predictor(net)
    assert not pr.native
    xa, radii, lp, found = pr.minimum_norm(imgs[:6], y, steps=steps)
    assert xa.shape == (6, 1, 28, 28) and radii.shape == (6,) and lp.shape == (6, 10) and found.dtype == torch.bool
    assert torch.equal(xa.reshape(6, 784), want["x"]) and torch.equal(radii, want["norm"] * MNIST_STD)
    assert torch.equal(lp, pr.log_probs(xa)) and torch.equal(found, lp.argmax(1) != y)
    assert bool(found[5]) and float(radii[5]) == 0.0
    assert not net.training and all(p.grad is None for p in net.parameters())


def test_minimum_norm_on_the_trained_net():
    """64 correctly classified images, steps = 50, overshoot 0.02, on the CPU reference: found 64 / 64 (100%),
    median radius 1.4711, largest 3.7809 (pixel units); every ``x_adv`` is misclassified by ``forward_reference``,
    lies in the box, and ``radii`` is the float64 norm of ``x_adv - x0`` within 4 fp32 ulps."""
    imgs, labels = D.trained_case()
    xa, radii, lp, found = D.cpu_minimum_norm()
    net = D.trained_net()
    print(f"CPU DeepFool: found {int(found.sum())}/64, median radius {float(radii[found].median()):.4f}, "
          f"max {float(radii.max()):.4f}")
    with torch.no_grad():
        pred = net.forward_reference(xa).argmax(1)
    assert torch.equal(pred != labels.long(), found)
    assert found.any()
    assert (pred[found] != labels.long()[found]).all()
    assert (xa >= D.LO).all() and (xa <= D.HI).all() and torch.isfinite(xa).all()
    x0 = _PIXEL_LUT[imgs.reshape(64, 784).long()]
    want = (xa.reshape(64, 784).double() - x0.double()).square().sum(1).sqrt() * MNIST_STD
    ulps = ((radii.double() - want).abs() / (want * D.ULP)).max().item()
    print(f"radii against the float64 norm: {ulps:.2f} ulps")
    assert (radii > 0).all() and ulps <= 4.0, ulps
    # labels None: the class predicted on the clean input, here the true one
    xb, rb, _, fb = Predictor(net).minimum_norm(imgs[:8], steps=50)
    assert torch.equal(xb, xa[:8]) and torch.equal(rb, radii[:8]) and torch.equal(fb, found[:8])


def test_step_reference_on_the_hand_made_images():
    ops = D.hand_cases()
    got, one = D.reference_step(ops), D.step_images(ops)
    for k in D.KEYS:
        assert torch.equal(got[k], one[k]) or (k != "status" and k != "iters" and
                                               torch.equal(torch.nan_to_num(got[k], nan=7.0),
                                                           torch.nan_to_num(one[k], nan=7.0))), k
    D.check_step(got, ops)
    at, y = D.HAND.index, 3
    kept = lambda i: all(torch.equal(got[k][i], ops[k][i]) for k in D.KEYS if k != "status")   # noqa: E731
    for name in ("crossed", "equal_loss_k_below_y"):
        assert int(got["status"][at(name)]) == 1 and kept(at(name)), name
    assert int(got["status"][at("all_unselectable")]) == 2 and kept(at("all_unselectable"))
    assert int(got["status"][at("frozen")]) == 1 and kept(at("frozen"))
    for name, l in (("equal_loss_k_above_y", 7), ("identical_twins", 2), ("mirrored_tie", 2), ("zero_class", 1),
                    ("both_clamps", 0), ("plain", 0), ("nan_in_unchosen", 0)):
        i = at(name)
        assert int(one["l"][i]) == l and int(got["status"][i]) == 0 and int(got["iters"][i]) == 1, name
        assert float(got["norm"][i]) > 0 and not kept(i), name
    i = at("mirrored_tie")                                   # the step lies along w_2, not along w_6 = -w_2
    w2 = ops["dx"].view(-1, 10, 784)[i, y] - ops["dx"].view(-1, 10, 784)[i, 2]
    assert float((got["r_tot"][i] * w2).sum()) > 0
    i = at("both_clamps")
    assert (got["x"][i] == np.float32(D.LO)).any() and (got["x"][i] == np.float32(D.HI)).any()
    i = at("nan_in_g_y")
    assert torch.isnan(got["x"][i]).all() and torch.isnan(got["r_tot"][i]).all() and torch.isnan(got["norm"][i])
    assert int(got["status"][i]) == 0 and int(got["iters"][i]) == 1
    others = [j for j in range(len(D.HAND)) if j != i]
    assert all(torch.isfinite(got[k][others]).all() for k in ("r_tot", "x", "norm"))
    i, j = at("nan_in_unchosen"), at("plain")
    assert all(torch.equal(got[k][i], got[k][j]) for k in D.KEYS)


@pytest.mark.parametrize("variant", D.MUTATIONS)
def test_each_mistake_fails_the_comparator_on_the_hand_made_images(variant):
    ops = D.hand_cases()
    D.check_step(D.step_images(ops), ops)                    # the stand-in itself passes
    with pytest.raises(AssertionError):
        D.check_step(D.step_images(ops, variant=variant), ops)


@pytest.mark.parametrize("M", [1, 3, 33])
def test_random_operands_have_a_clear_nearest_class(M):
    """The operands of the GPU step test: the float64 oracle's best and second-best ratio are at least 1e-3 apart
    (relative) for every image, y takes all ten values at M = 33, and the fp32 reference meets its own cap."""
    ops = D.operands(M)
    gap = D.ratio_gap(ops)
    assert gap.shape == (M,) and float(gap.min()) >= 1e-3, gap
    assert M < 33 or sorted(set(ops["y"].tolist())) == list(range(10))
    loss, y = ops["loss"].view(M, 10), ops["y"].long()
    assert (loss.gather(1, y[:, None]) <= loss).all()
    got = D.reference_step(ops)
    worst = D.check_step(got, ops)
    assert max(worst.values()) <= 0.125 + 1e-12 and (got["status"] == 0).all()
    want, one = D.reference_step(ops, torch.float64), D.step_images(ops, torch.float64)
    assert all(torch.equal(want[k], one[k]) for k in D.KEYS)
    scale = ops["dx"].abs().view(M, -1).max(1).values
    assert M < 3 or (float(scale.min()) < 1e-5 and float(scale.max()) > 1e2)


def test_minimum_norm_value_errors():
    imgs, labels = D.trained_case()
    pr = Predictor(D.trained_net())
    x, y = imgs[:3], labels[:3]
    for kw in (dict(steps=0), dict(steps=-2), dict(steps=2.5), dict(overshoot=-0.1), dict(overshoot=float("nan")),
               dict(check_every=-1), dict(check_every=1.5), dict(labels=y[:2]), dict(labels=torch.tensor([0, 10, 3])),
               dict(labels=torch.tensor([0, -1, 3]))):
        args = dict(labels=y)
        args.update(kw)
        with pytest.raises(ValueError, match="minimum_norm"):
            pr.minimum_norm(x, **args)
    with pytest.raises(ValueError):
        pr.minimum_norm(torch.zeros(2, 3, 28, 28))


def test_minimum_norm_stats_and_line():
    radii = torch.tensor([0.5, 1.5, 1.0, 0.0, 2.0, 3.0])
    found = torch.tensor([True, True, True, True, False, True])
    clean = torch.tensor([True, True, True, False, True, True])
    n, median, mean, acc = minimum_norm_stats(radii, found, clean, (0.0, 1.0, 2.5))
    assert n == 5 and median == 1.25 and mean == 1.5         # over images 0, 1, 2, 5: found and clean
    assert acc == [5, 3, 2]                                  # clean and (not found or radius > R)
    assert minimum_norm_line(50, 0.02, 6, n, median, mean) == \
        "Minimum-norm set (L2 DeepFool, steps=50, overshoot=0.02): Found: 5/6 (83%), median radius: 1.2500, " \
        "mean radius: 1.5000"
    assert minimum_norm_stats(radii, ~clean, clean)[1:] == (None, None, [])


def test_predict_parser_min_norm_options():
    ap = build_predict_parser()
    a = ap.parse_args([])
    assert (a.min_norm, a.min_norm_steps, a.min_norm_overshoot, a.min_norm_count, a.min_norm_radii) == \
        (False, 50, 0.02, None, ())
    a = ap.parse_args(["--min-norm", "--min-norm-steps", "7", "--min-norm-overshoot", "0.1", "--min-norm-count", "9",
                       "--min-norm-radii", "0.5,1,2"])
    assert (a.min_norm, a.min_norm_steps, a.min_norm_overshoot, a.min_norm_count, a.min_norm_radii) == \
        (True, 7, 0.1, 9, (0.5, 1.0, 2.0))
    with pytest.raises(SystemExit):
        ap.parse_args(["--min-norm-radii", "-1"])


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


def test_predict_cli_without_the_flag_is_unchanged(tmp_path):
    net, stdout, rec = _run_predict(tmp_path)
    _, stdout2, rec2 = _run_predict(tmp_path, "--min-norm-steps", "3", "--min-norm-radii", "0.5")   # options alone
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=64, verbose=False)
    loss, correct, n = Predictor(net).evaluate(data.images, data.targets, 40)
    assert stdout == _test_line(loss / n, correct, n) + "\n" and stdout2 == stdout
    want = {"checkpoint": rec["checkpoint"], "device": "cpu", "source": data.source, "test_loss": loss / n,
            "correct": correct, "n": n}
    assert rec == want and rec2 == want and list(rec) == list(want)


def test_predict_cli_min_norm_on_cpu(tmp_path):
    net, stdout, rec = _run_predict(tmp_path, "--min-norm", "--min-norm-steps", "5", "--min-norm-count", "48",
                                    "--min-norm-radii", "0.01,0.5")
    lines = stdout.splitlines()
    assert len([ln for ln in lines if ln.startswith("Test set:")]) == 1
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=64, verbose=False)
    pr = Predictor(net)
    radii, found, clean = torch.empty(48), torch.empty(48, dtype=torch.bool), torch.empty(48, dtype=torch.bool)
    for i, j in ((0, 40), (40, 48)):                         # the CLI's batches
        _, radii[i:j], _, found[i:j] = pr.minimum_norm(data.images[i:j], data.targets[i:j], steps=5)
        clean[i:j] = pr.predict(data.images[i:j]) == data.targets[i:j].long()
    n, median, mean, acc = minimum_norm_stats(radii, found, clean, (0.01, 0.5))
    at = lines.index(minimum_norm_line(5, 0.02, 48, n, median, mean))
    assert lines[at + 1:] == [f"Accuracy at radius {r:g}: {c}/48 ({100.0 * c / 48:.0f}%)"
                              for r, c in zip((0.01, 0.5), acc)]
    assert at == len(lines) - 3 and lines[at].startswith("Minimum-norm set (L2 DeepFool, steps=5, overshoot=0.02): ")
    assert rec["min_norm_steps"] == 5 and rec["min_norm_overshoot"] == 0.02 and rec["min_norm_count"] == 48
    assert rec["min_norm_found"] == n and rec["min_norm_median_radius"] == median
    assert rec["min_norm_mean_radius"] == mean and rec["min_norm_accuracy_at"] == {"0.01": acc[0], "0.5": acc[1]}
    assert n >= int((~clean).sum())                          # an image wrong on the clean input is found at radius 0
