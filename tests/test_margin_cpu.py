"""The margin / DLR losses on the host (no GPU): the float64 oracle of ``head_margin`` and the proof that its check
fails on subtly wrong outputs (tests/margin_ref.py), ``margin_loss_reference``, the ``GradChain`` call sequence, the
``Predictor`` interface, the command line, and the worst-case ensemble."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import margin_ref as M
import refmodel as R
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import (Predictor, adversarial_line, auto_pgd_line, build_predict_parser,
                                             ensemble_line, reference_auto_pgd)
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import chain
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict
from test_chain_cpu import STREAM, FakeC, FakeState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows_case(B):
    """The checked rows of the seeded case of B rows: (rows, z1part, labels, targets) restricted to them."""
    z, y, t = M.margin_case(B)
    rows = R.check_rows(B)
    n = torch.tensor(rows)
    return rows, z[:, n], y[n], t[n]


# ------------------------------------------------------------------ the oracle and the proof of the check
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("B", M.SIZES)
def test_the_oracle_alone_leaves_out_no_row(B, kind):
    _, z, y, t = _rows_case(B)
    hp = M.head_params()
    a = (z, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], y, kind, t, 1.0)
    r64, r32 = M.stage_head_margin(*a), M.stage_head_margin(*a, dtype=R.F32)
    tau = R.stage_eps(r32["logits"], r64["logits"], head=True)
    assert (r64["gap"] >= tau).all()                          # committed seeds: every selection is decided
    assert tau < 1e-4 and float(r64["gap"].min()) > 100 * tau
    if kind != "cw":
        assert (r64["d"] >= 1e-2 * r64["d"].median()).all()   # ... and no row's denominator is an outlier
    assert (r64["z1"] > 0).any() and (r64["z1"] < 0).any()


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("B", M.SIZES)
def test_fp32_standin_passes(B, kind):
    rows, z, y, t = _rows_case(B)
    hp = M.head_params()
    full = M.standin(z, hp, y, kind, t, 1.0, B, rows)
    st = M.check_all(B, z, hp, y, kind, t, 1.0, full, rows)
    assert st["rows_excluded"][0] == 0.0
    for k in ("loss_rows", "dl_bf", "dz1", "h_bf"):
        assert st[k][0] <= st[k][1]


@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_scale_is_carried(scale):
    z, y, t = M.margin_case(33)
    hp = M.head_params()
    for kind in M.KINDS:
        M.check_all(33, z, hp, y, kind, t, scale, M.standin(z, hp, y, kind, t, scale, 33))
        with pytest.raises(AssertionError):
            M.check_all(33, z, hp, y, kind, t, scale, M.standin(z, hp, y, kind, t, 1.5 * scale, 33))


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_every_mutation_is_caught(mut):
    z, y, t = M.margin_case(33)
    hp = M.head_params()
    for kind in M.MUT_KINDS.get(mut, M.KINDS):
        with pytest.raises(AssertionError):
            M.check_all(33, z, hp, y, kind, t, 1.0, M.standin(z, hp, y, kind, t, 1.0, 33, mut=mut))


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("bias,pairs", [(M.TIE_BIAS, M.TIE_ROWS), (M.TOP3_BIAS, M.TOP3_ROWS)])
def test_tie_rows_and_last_of_equals_is_caught(bias, pairs, kind):
    z, hp, y, t = M.tie_inputs(bias, pairs)
    a = (z, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], y, kind, t, 1.0)
    r = M.stage_head_margin(*a, dtype=R.F32)
    assert torch.equal(r["logits"], torch.tensor(bias).expand(len(pairs), 10)) and (r["dz1"] == 0).all()
    dl = torch.zeros(len(pairs), 16, dtype=torch.bfloat16)
    dl[:, :10] = R.bf16_round(r["dl"])
    M.check_tie_rows(bias, pairs, kind, r["loss"], dl)
    bad = M.stage_head_margin(*a, dtype=R.F32, mut="last_of_equals")
    dl[:, :10] = R.bf16_round(bad["dl"])
    with pytest.raises(AssertionError):
        M.check_tie_rows(bias, pairs, kind, bad["loss"], dl)


def test_tie_rules_on_hand_rows():
    z = torch.tensor([M.TIE_BIAS, M.TIE_BIAS, M.TOP3_BIAS])
    y = torch.tensor([1, 0, 3])
    o, p1, p2, p3, p4 = Fk.margin_selections(z, y)
    assert o.tolist() == [2, 1, 0]                            # the label is one of the equals; the first of equals
    assert (p1.tolist(), p2.tolist(), p3.tolist(), p4.tolist()) == ([1, 1, 0], [2, 2, 1], [3, 3, 2], [4, 4, 3])
    # a NaN never wins over an earlier class, and a later class is compared with the value held, not with the NaN
    zn = torch.tensor([[1.0, float("nan"), 0.5, 2.0, 0, 0, 0, 0, 0, 0]])
    assert Fk.first_max_excluding(zn, torch.zeros(1, 10, dtype=torch.bool)).tolist() == [3]
    L, dl = M.tie_expected(M.TOP3_BIAS, 3, 0, "dlr")
    assert np.isfinite(L) and np.isfinite(dl).all() and L == np.float32(np.float32(4.0) / np.float32(1e-12))


# ------------------------------------------------------------------ margin_loss_reference / head_margin_reference
def _sort_loss(z, y, kind, t=None):
    """The losses over ``torch.sort`` (the authors' formulation); equal to the explicit selection on tie-free rows."""
    srt, ind = z.sort(dim=1, descending=True)
    zy = z.gather(1, y[:, None])[:, 0]
    top_is_y = ind[:, 0] == y
    zo = torch.where(top_is_y, srt[:, 1], srt[:, 0])
    if kind == "cw":
        return zo - zy
    if kind == "dlr":
        return (zo - zy) / ((srt[:, 0] - srt[:, 2]) + 1e-12)
    return (zy - z.gather(1, t[:, None])[:, 0]) / ((srt[:, 0] - 0.5 * (srt[:, 2] + srt[:, 3])) + 1e-12)


@pytest.mark.parametrize("kind", M.KINDS)
def test_margin_loss_reference_gradient_is_autograd_over_sort(kind):
    g = torch.Generator().manual_seed(11)
    z = torch.randn(64, 10, generator=g, dtype=torch.float64)
    y = torch.randint(0, 10, (64,), generator=g)
    t = (y + torch.randint(1, 10, (64,), generator=g)) % 10
    za, zb = z.clone().requires_grad_(), z.clone().requires_grad_()
    la, lb = Fk.margin_loss_reference(za, y, kind, t), _sort_loss(zb, y, kind, t)
    assert torch.allclose(la, lb, rtol=0, atol=1e-12)
    ga, = torch.autograd.grad(la.sum(), za)
    gb, = torch.autograd.grad(lb.sum(), zb)
    assert torch.allclose(ga, gb, rtol=1e-12, atol=1e-12) and (ga != 0).any(dim=1).all()
    # shift invariance: the log-probs give the same loss
    assert torch.allclose(Fk.margin_loss_reference(F.log_softmax(z, 1), y, kind, t), la.detach(), atol=1e-9)
    # head_margin_reference's explicit dl is that gradient, scaled
    hp = M.head_params()
    zp, yy, tt = M.margin_case(33)
    r = Fk.head_margin_reference(zp.double(), hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], yy, kind, tt, scale=-0.5)
    zl = r["logits"].clone().requires_grad_()
    gl, = torch.autograd.grad(Fk.margin_loss_reference(zl, yy, kind, tt).sum(), zl)
    assert torch.allclose(r["dl"], -0.5 * gl, rtol=1e-12, atol=1e-12)
    o = M.stage_head_margin(zp, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], yy, kind, tt, -0.5)
    for k in ("loss", "dl", "dz1", "h"):
        assert torch.allclose(r[k], o[k], rtol=1e-12, atol=1e-12), k


def test_reference_refusals():
    z = torch.zeros(2, 10)
    with pytest.raises(ValueError):
        Fk.margin_loss_reference(z, torch.tensor([0, 1]), "ce")
    with pytest.raises(ValueError):
        Fk.margin_loss_reference(z, torch.tensor([0, 1]), "dlr_t")
    with pytest.raises(ValueError):
        Fk.head_margin(None, None, None, "nll")


# ------------------------------------------------------------------ GradChain
@pytest.fixture
def fake(monkeypatch):
    C = FakeC()
    monkeypatch.setattr(chain.native, "load", lambda *a, **k: C)
    monkeypatch.setattr(chain.native, "stream_handle", lambda *a, **k: STREAM)
    return C


@pytest.mark.parametrize("loss,code", [("cw", 0), ("dlr", 1), ("dlr_t", 2)])
def test_grad_chain_margin_is_trunk_fc1_head_margin_fc_bwd(fake, loss, code):
    st = FakeState()
    gc = chain.GradChain(st, 40, loss)
    b, w = st.taken[0], chain.param_ptrs(st.ms)
    gc.run(600, 500, 33, 400)
    assert [c[0] for c in fake.calls] == ["trunk_fwd", "fc1_fwd", "head_margin", "fc_bwd"]
    head = fake.calls[2]
    assert head[1:] == ((b.z1part.addr, w.f1b, w.f2w, w.f2b, 500, 400, code, 1.0, b.loss_rows.addr, b.dz1.addr,
                         b.h_bf.addr, b.dl_bf.addr, 33, 64, STREAM), {})
    ce_st = FakeState()
    ce = chain.GradChain(ce_st, 40)
    fake.calls.clear()
    ce.run(600, 500, 33)
    assert [c[0] for c in fake.calls] == ["trunk_fwd", "fc1_fwd", "head_train", "fc_bwd"]
    other = list(fake.calls)
    fake.calls.clear()
    gc.run(600, 500, 33, 400)
    for k in (0, 1, 3):                                       # everything but the head launch is the same call
        assert fake.calls[k][0] == other[k][0] and fake.calls[k][2] == other[k][2]
        assert len(fake.calls[k][1]) == len(other[k][1])
    with pytest.raises(ValueError):
        chain.GradChain(FakeState(), 8, "nll")
    assert chain.chain_loss("x", "dlr", True) == "dlr_t" and chain.chain_loss("x", "dlr", False) == "dlr"
    assert chain.chain_loss("x", "cw", True) == "cw" and chain.chain_loss("x", "ce", True) == "ce"
    with pytest.raises(ValueError):
        chain.chain_loss("x", "dlr_t", False)


def test_grad_chain_ce_explicit_is_the_default(fake):
    a, b = chain.GradChain(FakeState(), 40), chain.GradChain(FakeState(), 40, loss="ce")
    strip = lambda gc: [(c[0], tuple(0 if v == gc._state.data_ptr() else v for v in c[1]), c[2])      # noqa: E731
                        for c in fake.calls]                    # (each chain's own step state apart)
    a.run(600, 500, 31)
    first = strip(a)
    fake.calls.clear()
    b.run(600, 500, 31, 0)
    assert strip(b) == first and [c[0] for c in first] == ["trunk_fwd", "fc1_fwd", "head_train", "fc_bwd"]


# ------------------------------------------------------------------ Predictor
@functools.lru_cache(maxsize=None)
def _case64():
    torch.manual_seed(3)
    net = Net().train()
    imgs, labels = generate(64, seed=5)
    return net, imgs, labels


def test_predictor_validation_errors():
    net, imgs, labels = _case64()
    pr = Predictor(net)
    x, y = imgs[:4], labels[:4]
    tgt = (y + 1) % 10
    for fn in (pr.auto_pgd,):
        with pytest.raises(ValueError):
            fn(x, y, loss="dlr_t")
        with pytest.raises(ValueError):
            fn(x, y, loss="nll")
        with pytest.raises(ValueError):                       # a target equal to its row's true label
            fn(x, tgt, steps=2, targeted=True, loss="dlr", true_labels=torch.cat((y[:3], tgt[3:])))
        with pytest.raises(ValueError):
            fn(x, tgt, steps=2, targeted=True, loss="dlr", true_labels=y[:3])
        with pytest.raises(ValueError):
            fn(x, tgt, steps=2, targeted=True, loss="dlr", true_labels=torch.tensor([0, 1, 2, 10]))
        fn(x, tgt, steps=2, targeted=True, loss="cw", true_labels=tgt)       # read by targeted DLR only
    with pytest.raises(ValueError):
        pr.robust_evaluate_apgd(x, y, 0.1, steps=2, loss="margin")
    for kw in (dict(n_targets=10), dict(n_targets=-1), dict(queries=-1), dict(steps=0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            pr.robust_evaluate_ensemble(x, y, 0.1, **kw)
    # the default true_labels is the class predicted on the clean input
    pred = pr.predict(x)
    with pytest.raises(ValueError):
        pr.auto_pgd(x, pred, steps=2, targeted=True, loss="dlr")
    a = pr.auto_pgd(x, (pred + 1) % 10, steps=2, targeted=True, loss="dlr")
    b = pr.auto_pgd(x, (pred + 1) % 10, steps=2, targeted=True, loss="dlr", true_labels=pred)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("loss,targeted", [("cw", False), ("dlr", False), ("cw", True), ("dlr", True)])
def test_reference_auto_pgd_margin_never_lowers_the_loss(loss, targeted):
    net, imgs, labels = _case64()
    x0 = normalize_u8(imgs).reshape(64, 784)
    y = labels.long()
    lab = (y + 3) % 10 if targeted else y
    true = y if targeted and loss == "dlr" else None
    eps_n = 0.1 / MNIST_STD
    lo, hi = normalize_u8(torch.tensor([[0, 255]], dtype=torch.uint8)).flatten().tolist()
    xb, lb = reference_auto_pgd(net, x0, lab, eps_n, 6, lo, hi, targeted=targeted, loss=loss, true_labels=true)
    pr = Predictor(net)
    kind = chain.chain_loss("t", loss, targeted)
    rows = lambda x: (Fk.margin_loss_reference(pr.log_probs(x.view(64, 1, 28, 28)), true, kind, lab) if kind == "dlr_t"      # noqa: E731
                      else Fk.margin_loss_reference(pr.log_probs(x.view(64, 1, 28, 28)), lab, kind))
    start = rows(x0)
    assert ((lb <= start) if targeted else (lb >= start)).all()           # loss_best starts at the start's loss
    # (an untargeted DLR row whose label ranks third has L = 1 identically: no gradient, it stays where it is)
    assert ((lb < start) if targeted else (lb > start)).float().mean() > 0.5
    assert torch.allclose(rows(xb), lb, atol=1e-5)                          # loss_best is the chosen loss at x_best
    assert (xb >= x0 - eps_n).all() and (xb <= x0 + eps_n).all() and (xb >= lo).all() and (xb <= hi).all()
    # Predictor.auto_pgd is that loop, and eps = 0 returns the clean images
    xa, _, la = pr.auto_pgd(imgs, lab, eps=0.1, steps=6, targeted=targeted, loss=loss, true_labels=true)
    assert torch.equal(xa.view(64, 784), xb) and torch.equal(la, lb)
    xz, _, _ = pr.auto_pgd(imgs, lab, eps=0.0, steps=2, targeted=targeted, loss=loss, true_labels=true)
    assert torch.equal(xz.view(64, 784), x0)


@pytest.mark.parametrize("loss", ["cw", "dlr"])
def test_robust_evaluate_apgd_loss_sum_stays_the_nll(loss):
    net, imgs, labels = _case64()
    pr = Predictor(net)
    y = labels.long()
    one = pr.robust_evaluate_apgd(imgs, labels, 0.1, steps=3, loss=loss)
    _, lp, _ = pr.auto_pgd(imgs, labels, eps=0.1, steps=3, loss=loss)
    assert one[0] == pytest.approx(F.nll_loss(lp, y, reduction='sum').item(), rel=1e-5)
    assert one[1] == int((lp.argmax(1) == y).sum()) and one[2] == 64
    assert one[0] > pr.evaluate(imgs, labels)[0]


# ------------------------------------------------------------------ the ensemble
@functools.lru_cache(maxsize=None)
def _case16():
    from attr_ref import trained_net
    net = trained_net()
    imgs, labels = generate(16, seed=21)
    return net, imgs, labels


ENS = dict(steps=5, n_targets=2, queries=20)


def ensemble_by_hand(pr, imgs, labels, eps, steps, n_targets, queries, seed=0):
    """The surviving set as the AND of every attack of the ensemble run on ALL the images with the same arguments."""
    y = labels.long().to(pr.device)
    n = y.shape[0]
    lp0 = pr.log_probs(imgs)
    alive = lp0.argmax(1) == y
    order = lp0.clone().scatter_(1, y[:, None], float("-inf")).sort(dim=1, descending=True, stable=True)[1]
    alive &= pr.auto_pgd(imgs, y, eps, steps)[1].argmax(1) == y
    for k in range(n_targets):
        alive &= pr.auto_pgd(imgs, order[:, k], eps, steps, targeted=True, loss="dlr", true_labels=y)[1].argmax(1) == y
    if queries:
        alive &= pr.square_attack(imgs, y, eps, queries, 0.8, seed, ids=range(n))[1].argmax(1) == y
    return alive


def test_ensemble_is_the_and_of_its_attacks():
    net, imgs, labels = _case16()
    pr = Predictor(net)
    eps = 0.15
    correct, n, after = pr.robust_evaluate_ensemble(imgs, labels, eps, **ENS)
    want = ensemble_by_hand(pr, imgs, labels, eps, **ENS)
    assert n == 16 and correct == int(want.sum()) == after["square"]
    assert list(after) == ["clean", "apgd_ce", "apgd_t", "square"]
    counts = list(after.values())
    assert counts == sorted(counts, reverse=True) and counts[0] == pr.evaluate(imgs, labels)[1]
    assert counts[0] > counts[-1]                              # the attacks break something at this radius
    parts = pr.robust_evaluate_ensemble(imgs, labels, eps, batch_size=7, **ENS)
    assert parts == (correct, n, after)                        # per-image independence: the batching does not matter
    zero = pr.robust_evaluate_ensemble(imgs, labels, eps, steps=5, n_targets=0, queries=0)
    assert zero[2]["apgd_t"] == zero[2]["apgd_ce"] == zero[2]["square"]


def test_ensemble_skips_a_stage_without_survivors(monkeypatch):
    net, imgs, labels = _case16()
    pr = Predictor(net)
    calls = []
    for name in ("auto_pgd", "square_attack"):
        real = getattr(pr, name)
        monkeypatch.setattr(pr, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, a[0].shape[0])), _r(*a, **k))[1])
    wrong = (pr.predict(imgs) + 1) % 10                       # no image is right on the clean input
    assert pr.robust_evaluate_ensemble(imgs, wrong, 0.1, **ENS) == (0, 16, dict(clean=0, apgd_ce=0, apgd_t=0, square=0))
    assert calls == []
    pr.robust_evaluate_ensemble(imgs, labels, 0.15, **ENS)
    assert [c[0] for c in calls] == ["auto_pgd"] * 3 + ["square_attack"]
    assert all(0 < c[1] <= 16 for c in calls) and [c[1] for c in calls] == sorted((c[1] for c in calls), reverse=True)


# ------------------------------------------------------------------ the command line
def test_predict_parser_and_lines():
    ap = build_predict_parser()
    a = ap.parse_args([])
    assert (a.apgd_loss, a.ensemble_eps) == ("ce", None)
    assert (a.ensemble_steps, a.ensemble_targets, a.ensemble_queries, a.ensemble_seed) == (100, 9, 5000, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--apgd-loss", "dlr_t"])
    assert auto_pgd_line(0.1, 100, 1, 0.12344, 9876, 10000, loss_name="cw").startswith(
        "Auto-PGD set (Linf eps=0.1, steps=100, restarts=1, loss=cw): ")
    assert auto_pgd_line(0.1, 100, 1, 0.12344, 9876, 10000, loss_name="dlr") == \
        "Auto-PGD set (Linf eps=0.1, steps=100, restarts=1, loss=dlr): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"
    assert auto_pgd_line(0.1, 100, 1, 0.12344, 9876, 10000) == \
        "Auto-PGD set (Linf eps=0.1, steps=100, restarts=1): Average loss: 0.1234, Accuracy: 9876/10000 (99%)"
    assert ensemble_line(0.1, 9, 12, 40) == "Ensemble set (Linf eps=0.1: apgd-ce, apgd-t x 9, square): Accuracy: 12/40 (30%)"


def _run_predict(tmp_path, *extra):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    if os.path.exists(log):
        os.remove(log)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic",
                        "--synthetic-test-size", "24", "--checkpoint", ckpt, "--batch-size", "24",
                        "--json-log", log, *extra],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(log) as f:
        return net, r.stdout, json.loads(f.read())


def test_predict_cli_loss_flags_and_ensemble_on_cpu(tmp_path):
    base = ("--attack-eps", "0.1", "--attack-steps", "2", "--apgd-eps", "0.1", "--apgd-steps", "3")
    _, out0, rec0 = _run_predict(tmp_path, *base)
    _, out1, rec1 = _run_predict(tmp_path, *base, "--apgd-loss", "ce")
    assert out0 == out1 and rec0 == rec1                       # the defaults, spelled out: byte for byte
    assert not any(k.endswith("_loss_name") or k.startswith("ensemble") for k in rec0)
    assert "loss=" not in out0 and "Ensemble" not in out0
    net, out, rec = _run_predict(tmp_path, *base, "--apgd-loss", "dlr", "--ensemble-eps", "0.1",
                                 "--ensemble-steps", "3", "--ensemble-targets", "2", "--ensemble-queries", "10",
                                 "--ensemble-seed", "4")
    lines = [ln for ln in out.splitlines() if ln.strip()]
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=24, verbose=False)
    pr = Predictor(net)
    adv = pr.robust_evaluate(data.images, data.targets, 0.1, steps=2, batch_size=24)
    ap = pr.robust_evaluate_apgd(data.images, data.targets, 0.1, steps=3, batch_size=24, loss="dlr")
    ens = pr.robust_evaluate_ensemble(data.images, data.targets, 0.1, steps=3, n_targets=2, queries=10, batch_size=24,
                                      seed=4)
    assert len(lines) == 4 and lines[0] == [ln for ln in out0.splitlines() if ln.strip()][0]
    assert lines[1] == adversarial_line(0.1, 2, adv[0] / 24, adv[1], 24) and "loss=" not in lines[1]
    assert lines[2] == auto_pgd_line(0.1, 3, 1, ap[0] / 24, ap[1], 24, loss_name="dlr")
    assert lines[3] == ensemble_line(0.1, 2, ens[0], 24)
    assert ", loss=dlr): " in lines[2]
    assert rec["apgd_loss_name"] == "dlr" and "adv_loss_name" not in rec
    assert (rec["ensemble_eps"], rec["ensemble_steps"], rec["ensemble_targets"], rec["ensemble_queries"],
            rec["ensemble_seed"], rec["ensemble_correct"], rec["ensemble_after"]) == (0.1, 3, 2, 10, 4, ens[0], ens[2])
    assert set(rec) - set(rec0) == {"apgd_loss_name", "ensemble_eps", "ensemble_steps",
                                    "ensemble_targets", "ensemble_queries", "ensemble_seed", "ensemble_correct",
                                    "ensemble_after"}
