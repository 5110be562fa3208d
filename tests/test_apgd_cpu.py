"""Auto-PGD on the CPU side: the checkpoint schedule, ``apgd_step_reference`` against the per-image oracle of
tests/apgd_ref.py (linf: bit for bit; l2: within the derived bound; every deliberate mistake is caught),
``reference_auto_pgd`` on the trained test net, ``Predictor.auto_pgd`` / ``robust_evaluate_apgd`` and the
``mnist_predict.py --apgd-eps`` line."""
import functools
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
from pytorch_mnist_ddp_amd import _build
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import (Predictor, auto_pgd_line, build_predict_parser, reference_auto_pgd)
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = R.LO, R.HI
# the launches every step test makes: first, middle without and with a closing window, last; either sign; eps = 0
LAUNCHES = [dict(first=True), dict(), dict(window=R.WINDOW), dict(last=True, window=R.WINDOW)]
CASES = [(sign, None, kw) for sign in (1, -1) for kw in LAUNCHES] + [(1, 0.0, dict(window=R.WINDOW)), (1, 0.0, dict(first=True))]


def test_checkpoint_schedule():
    assert Fk.apgd_checkpoints(100) == ((22, 22), (41, 19), (57, 16), (70, 13), (80, 10), (87, 7), (93, 6), (99, 6))
    assert Fk.apgd_checkpoints(1) == ((1, 1),)
    assert Fk.apgd_checkpoints(5) == tuple((i, 1) for i in range(1, 6))
    assert Fk.apgd_checkpoints(17)[:4] == ((3, 3), (5, 2), (6, 1), (7, 1)) and Fk.apgd_checkpoints(17)[-1] == (17, 1)
    for n in (1, 2, 5, 17, 33, 100, 1000):
        cp = Fk.apgd_checkpoints(n)
        its = [i for i, _ in cp]
        assert its == sorted(set(its)) and its[-1] <= n and n - its[-1] < cp[-1][1] + 1
        assert [b - a for a, b in zip([0] + its, its)] == [k for _, k in cp]          # each window closes k later
    with pytest.raises(ValueError):
        Fk.apgd_checkpoints(0)


def test_scenarios_force_every_branch():
    """The generator's images take the branches they are built for (read off the float64 oracle)."""
    case = R.make_case("linf", 33, seed=1)
    (_, x_old, x_best, g_best, fs, ist), _ = R.step_oracle(case, "linf", window=R.WINDOW)
    restarted = ist[:11, Fk.APGD_RESTARTED].tolist()
    assert restarted == [1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    assert ist[:11, Fk.APGD_REDUCED].tolist() == restarted and not ist[:, Fk.APGD_N_UP].any()
    improved = [bool((x_best[i] == case["x"][i].numpy()).all()) for i in range(11)]
    assert improved == [True, False, False, True, False, False, False, False, False, False, True]
    assert (x_old[0] == case["x"][0].numpy()).all()                  # 0: restart after its own improvement: from x
    assert (x_old[1] == case["x_best"][1].numpy()).all()             # 1: from the stored best
    assert (x_old[2] == case["x"][2].numpy()).all()
    assert bool(torch.isnan(case["loss_rows"][9])) and fs[9, Fk.APGD_LOSS_BEST] == case["fstate"][9, 1]
    (_, _, _, _, _, ist0), _ = R.step_oracle(case, "linf", window=0)
    assert ist0[:7, Fk.APGD_N_UP].tolist() == [6, 7, 7, 8, 6, 7, 7]  # the increments; 6 is 4 n_up == 3 k
    x0 = case["x0"][10]
    assert (x0 == LO).any() and (x0 == HI).any()


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_step_reference_against_the_oracle(norm):
    worst = 0.0
    for n, (sign, eps, kw) in enumerate(CASES):
        case = R.make_case(norm, 33, seed=10 + n, sign=sign, eps=eps)
        got32 = R.reference_step(case, torch.float32, **kw)
        want64, bound = R.step_oracle(case, norm, **kw)
        if norm == "linf":                                   # no reductions: per-operation float32, bit for bit
            want32, _ = R.step_oracle(case, norm, dtype=np.float32, **kw)
            assert R.mismatches(got32, want32) == [], (sign, eps, kw)
            assert R.mismatches(R.reference_step(case, torch.float64, **kw), want64) == []
        else:
            assert R.mismatches(got32, want64, bound) == [], (sign, eps, kw)
            if not kw.get("last"):
                ok = np.isfinite(want64[0]).all(axis=1)
                dev = np.abs(got32[0].astype(np.float64) - want64[0])[ok].max(axis=1)
                worst = max(worst, float((dev / bound[ok]).max()))
                assert (bound[ok] > 0).all() and (bound[ok] < 1e-3).all()      # the bound is a bound on rounding
        # the inputs are not modified, NaNs stay in their image
        nan_rows = np.isnan(got32[0]).any(axis=1)
        if not (kw.get("last") or kw.get("first")):
            assert nan_rows.tolist() == [i % 11 == 8 for i in range(33)]
            if norm == "l2":
                assert np.isnan(got32[0][8]).all()
            else:
                assert np.isnan(got32[0][8]).sum() == 1
        if eps == 0.0:
            ok = ~nan_rows
            assert np.array_equal(got32[0][ok], case["x0"].numpy()[ok])
    if norm == "l2":
        print(f"\nl2: largest float32 deviation / derived bound {worst:.3f}")


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_mutation_is_caught(norm, variant):
    """The comparator has teeth: the oracle with one deliberate mistake no longer matches the reference on the same
    operands, in at least one of the launches (and the unmutated oracle matches in all of them: the test above)."""
    caught = []
    for n, (sign, eps, kw) in enumerate(CASES):
        case = R.make_case(norm, 33, seed=10 + n, sign=sign, eps=eps)
        got32 = R.reference_step(case, torch.float32, **kw)
        if norm == "linf":
            want, bound = R.step_oracle(case, norm, dtype=np.float32, variant=variant, **kw)
        else:
            _, bound = R.step_oracle(case, norm, **kw)       # the bound of the true step
            want, _ = R.step_oracle(case, norm, variant=variant, **kw)
        if R.mismatches(got32, want, bound):
            caught.append((sign, eps, tuple(kw)))
    assert caught, variant
    if variant == "first_momentum":
        assert all(c[2] == ("first",) for c in caught)
    if variant == "last_moves_x":
        assert all("last" in c[2] for c in caught)
    if variant == "sign_loss_only":
        assert all(c[0] == -1 for c in caught)


@functools.lru_cache(maxsize=None)
def _case64():
    imgs, labels = generate(64, seed=5)
    return trained_net(), normalize_u8(imgs).reshape(64, 784), labels.long()


def _nll(net, x, y):
    with torch.no_grad():
        return F.nll_loss(net.forward_reference(x.view(-1, 1, 28, 28)), y, reduction='none')


@pytest.mark.parametrize("norm,eps,targeted", [("linf", 0.1, False), ("l2", 1.5, False), ("linf", 0.1, True)])
def test_reference_auto_pgd_on_the_trained_net(norm, eps, targeted):
    net, x0, y = _case64()
    lab = (y + 3) % 10 if targeted else y
    eps_n = eps / MNIST_STD
    x_adv, loss_best = reference_auto_pgd(net, x0, lab, eps_n, 20, LO, HI, norm=norm, targeted=targeted)
    assert x_adv.shape == (64, 784) and loss_best.shape == (64,) and not net.training
    assert (x_adv >= LO).all() and (x_adv <= HI).all()
    d = (x_adv - x0).double()
    if norm == "linf":                                       # x0 -+ eps are rounded once each
        assert (d.abs() <= eps_n + 2.0 ** -23 * max(abs(LO), abs(HI))).all()
    else:                                                    # test_attack_l2_cpu.py ball_slack
        assert (d.norm(dim=1) <= eps_n * (1.0 + 4 * 2.0 ** -23 * (784 / 8 + 1)) + 28 * 2.0 ** -24 * max(abs(LO), abs(HI))).all()
    start = _nll(net, x0, lab)
    assert (loss_best <= start).all() if targeted else (loss_best >= start).all()
    assert (loss_best < start).sum() >= 60 if targeted else (loss_best > start).sum() >= 60
    # the loss of the best point, recomputed: the same float32 forward on another batch composition
    assert torch.allclose(_nll(net, x_adv, lab), loss_best, rtol=1e-5, atol=1e-6)
    a = reference_auto_pgd(net, x0[:16], lab[:16], eps_n, 20, LO, HI, norm=norm, targeted=targeted)
    b = reference_auto_pgd(net, x0[16:], lab[16:], eps_n, 20, LO, HI, norm=norm, targeted=targeted)
    assert torch.equal(torch.cat((a[0], b[0])), x_adv) and torch.equal(torch.cat((a[1], b[1])), loss_best)
    assert all(p.grad is None for p in net.parameters())


def test_auto_pgd_beats_fixed_step_pgd_on_the_loss():
    """Not a property of the step, a sanity check of the whole: at the same budget the summed best loss of Auto-PGD
    is at least that of the fixed-step PGD end point minus nothing - it keeps the best of its iterates and starts
    with the larger step."""
    net, x0, y = _case64()
    pr = Predictor(net)
    _, lp, loss_best = pr.auto_pgd(x0.view(64, 1, 28, 28), y, eps=0.1, steps=20)
    _, lp_pgd = pr.adversarial(x0.view(64, 1, 28, 28), y, eps=0.1, steps=20)
    apgd, pgd = F.nll_loss(lp, y, reduction='sum'), F.nll_loss(lp_pgd, y, reduction='sum')
    print(f"\nsummed NLL after 20 steps at eps 0.1: Auto-PGD {float(apgd):.3f}, PGD {float(pgd):.3f}")
    assert apgd >= 0.9 * pgd
    assert torch.allclose(F.nll_loss(lp, y, reduction='none'), loss_best, rtol=1e-5, atol=1e-6)


def test_predictor_auto_pgd_refusals_and_restarts():
    net, x0, y = _case64()
    pr = Predictor(net)
    x = x0[:6].view(6, 1, 28, 28)
    for kw in (dict(norm="l1"), dict(eps=-0.1), dict(steps=0), dict(steps=2.5), dict(restarts=0), dict(restarts=2),
               dict(targeted=True, labels=None), dict(labels=torch.tensor([0, 1, 2, 3, 4, 10])),
               dict(labels=torch.tensor([0, 1]))):
        args = dict(labels=y[:6], steps=3)
        args.update(kw)
        with pytest.raises(ValueError):
            pr.auto_pgd(x, **args)
    gen = lambda: torch.Generator().manual_seed(4)                                          # noqa: E731
    one = pr.auto_pgd(x, y[:6], eps=0.1, steps=4, random_start=True, generator=gen())
    two = pr.auto_pgd(x, y[:6], eps=0.1, steps=4, random_start=True, restarts=2, generator=gen())
    g = gen()
    _ = pr.auto_pgd(x, y[:6], eps=0.1, steps=4, random_start=True, generator=g)
    second = pr.auto_pgd(x, y[:6], eps=0.1, steps=4, random_start=True, generator=g)         # the second draw
    assert (two[2] >= one[2]).all() and (two[2] >= second[2]).all()
    assert torch.equal(two[2], torch.maximum(one[2], second[2]))
    pick = second[2] > one[2]
    assert torch.equal(two[0], torch.where(pick.view(6, 1, 1, 1), second[0], one[0]))
    assert one[0].shape == (6, 1, 28, 28) and one[1].shape == (6, 10) and one[2].shape == (6,)
    # labels None: the class predicted on the clean input; uint8 images are normalised first
    imgs, _ = generate(64, seed=5)
    a = pr.auto_pgd(imgs[:6], None, eps=0.1, steps=3)
    b = pr.auto_pgd(x, pr.predict(x), eps=0.1, steps=3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    zero = pr.auto_pgd(x, y[:6], eps=0.0, steps=3)
    assert torch.equal(zero[0], x) and torch.equal(zero[1], pr.log_probs(x))


def test_robust_evaluate_apgd_cpu():
    net, _, y = _case64()
    imgs, labels = generate(64, seed=5)
    pr = Predictor(net)
    one = pr.robust_evaluate_apgd(imgs, labels, 0.1, steps=5, batch_size=64)
    parts = pr.robust_evaluate_apgd(imgs.reshape(64, 784), labels, 0.1, steps=5, batch_size=24)
    assert one[1:] == parts[1:] and one[2] == 64 and one[0] == pytest.approx(parts[0], rel=1e-5)
    _, lp, _ = pr.auto_pgd(imgs, labels, eps=0.1, steps=5)
    assert one[0] == pytest.approx(F.nll_loss(lp, y, reduction='sum').item(), rel=1e-5)
    assert one[1] == int((lp.argmax(1) == y).sum())
    clean = pr.evaluate(imgs, labels)
    assert one[0] > clean[0] and one[1] <= clean[1]
    assert pr.robust_evaluate(imgs, labels, 0.1, 5) != one                     # the fixed-step path is its own
    for kw in (dict(norm="l0"), dict(batch_size=0), dict(restarts=0)):
        with pytest.raises(ValueError):
            pr.robust_evaluate_apgd(imgs, labels, 0.1, steps=2, **kw)
    with pytest.raises(TypeError):
        pr.robust_evaluate_apgd(imgs, labels, 0.1, steps=2, step_size=0.01)     # there is no step size to give


def test_native_extension_has_apgd_step():
    _build.build()
    C = native.load(build_if_missing=False)
    assert callable(C.apgd_step)
    ok = dict(dx=16, loss_rows=16, x0=16, x=16, x_old=16, x_best=16, g_best=16, fstate=16, istate=16, sign=1.0, eps=0.1,
              lo=0.0, hi=1.0, l2=False, first=False, last=False, window=0, M=4, stream=0)
    # the launcher's own checks come before any launch
    bad = [dict(M=0), dict(M=-1), dict(M=(1 << 20) + 1), dict(eps=-0.1), dict(eps=float("nan")), dict(sign=0.0),
           dict(sign=2.0), dict(x=20), dict(fstate=24), dict(istate=4), dict(loss_rows=18), dict(window=-1),
           dict(first=True, last=True)] + [{k: 0} for k in list(ok)[:9]]
    for l2 in (False, True):
        for kw in bad:
            with pytest.raises(RuntimeError):
                C.apgd_step(**dict(ok, l2=l2, **kw))
    with pytest.raises(ValueError):                          # the functional wrapper wants GPU tensors
        z = torch.zeros(2, 784)
        Fk.apgd_step(z, torch.zeros(2), z, z, z, z, z, torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32),
                     1, 0.1, 0.0, 1.0)


def test_predict_parser_and_line():
    ap = build_predict_parser()
    d = ap.parse_args([])
    assert (d.apgd_eps, d.apgd_steps, d.apgd_norm, d.apgd_restarts, d.apgd_seed) == (None, 100, "linf", 1, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--apgd-norm", "l1"])
    assert auto_pgd_line(0.1, 100, 1, 0.12344, 9876, 10000) == \
        "Auto-PGD set (Linf eps=0.1, steps=100, restarts=1): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"
    assert auto_pgd_line(2, 5, 3, 0.12344, 9876, 10000, "l2").startswith("Auto-PGD set (L2 eps=2, steps=5, restarts=3): ")


def test_predict_cli_apgd_line_on_cpu(tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    base = [sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic", "--synthetic-test-size",
            "40", "--checkpoint", ckpt, "--batch-size", "24", "--json-log", log, "--attack-eps", "0.1",
            "--attack-steps", "2"]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT),     # noqa: E731
                                       capture_output=True, text=True, timeout=240)
    plain, with_apgd = run([]), run(["--apgd-eps", "0.1", "--apgd-steps", "4"])
    assert plain.returncode == 0 and with_apgd.returncode == 0, with_apgd.stderr[-2000:]
    with open(log) as f:
        rec0, rec = (json.loads(ln) for ln in f.read().splitlines())
    lines0, lines = ([ln for ln in r.stdout.splitlines() if ln.strip()] for r in (plain, with_apgd))
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    loss, correct, n = Predictor(net).robust_evaluate_apgd(data.images, data.targets, 0.1, steps=4, batch_size=24)
    assert lines[:-1] == lines0 and len(lines0) == 2                           # both lines of today, then the new one
    assert lines[-1] == auto_pgd_line(0.1, 4, 1, loss / n, correct, n)
    new = {"apgd_eps": 0.1, "apgd_steps": 4, "apgd_norm": "linf", "apgd_restarts": 1, "apgd_correct": correct}
    assert {k: rec[k] for k in new} == new and rec["apgd_loss"] == pytest.approx(loss / n, rel=1e-6)
    assert {k: v for k, v in rec.items() if not k.startswith("apgd_")} == rec0     # without the flag: today's record
    assert not any(k.startswith("apgd_") for k in rec0) and rec["apgd_correct"] <= rec["correct"]
