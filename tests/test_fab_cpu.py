"""The FAB attack without a GPU: the projection's properties, the torch reference against the float64 oracle, the
mutations the oracle comparison catches, ``reference_fab`` on the trained test net, and the interface."""
import json

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd import inference as I
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import deepfool_ref as D
import fab_ref as R


@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("M", [1, 3, 33])
def test_projection_properties(M, norm):
    """``fab_projection_reference`` in float64 on the GPU test's operands: inside the box exactly, on the hyperplane
    within the rounding of a 784-term sum of its operands, never longer than a feasible competitor and equal to the
    unconstrained projection where that one stays inside the box; at its bounds where the hyperplane misses the box."""
    ops, lo, hi = R.operands(M), R.f32(R.LO), R.f32(R.HI)
    want = R.step_images(ops, norm)
    w_all = ops["dx"].double().view(M, 10, 784)
    for i, o in enumerate(want["raw"]):
        y, l = int(ops["y"][i]), o["l"]
        w = (w_all[i, y] - w_all[i, l])[None, :]
        for p, v in enumerate((ops["x"][i].double(), ops["x0"][i].double())):
            r = torch.tensor([o["r"][p]], dtype=torch.float64)
            assert abs(o["r"][p]) <= 0.5 * o["g_inf"][p], (i, p)         # the crossing segment is not the tail
            d = Fk.fab_projection_reference(w, v[None, :], r, R.LO, R.HI, norm)[0]
            assert ((v + d) >= lo).all() and ((v + d) <= hi).all()
            bound = 784 * 2.0 ** -52 * float((w[0].abs() * d.abs()).sum() + abs(r))
            assert abs(float(r + (w[0] * d).sum())) <= 4 * bound, (i, p)
            assert np.allclose(d.numpy(), o["proj"][p], rtol=1e-9, atol=0)
            free = -r * (w[0].sign() / w[0].abs().sum() if norm == "linf" else w[0] / w[0].square().sum())
            scaled = (v + 0.5 * (free + d)).clamp(lo, hi) - v            # feasible competitors, put on the hyperplane
            for other in (free, scaled):
                if ((v + other) >= lo).all() and ((v + other) <= hi).all() and abs(float(r + (w[0] * other).sum())) <= 4 * bound:
                    assert R.pnorm(d.numpy(), norm) <= R.pnorm(other.numpy(), norm) * (1 + 1e-12)
            # far outside the box: every element with a weight sits on its bound
            far = Fk.fab_projection_reference(w, v[None, :], r * 1e9, R.LO, R.HI, norm)[0]
            room = torch.where(-r.sign() * w[0].sign() > 0, hi - v, v - lo)
            assert torch.equal(far.abs()[w[0] != 0], room[w[0] != 0]) and not far[w[0] == 0].any()
    # the unconstrained projection where the box is far away
    w, v = torch.randn(2, 784, dtype=torch.float64), torch.zeros(2, 784, dtype=torch.float64)
    r = torch.tensor([0.5, -0.25], dtype=torch.float64)
    d = Fk.fab_projection_reference(w, v, r, -1e6, 1e6, norm)
    free = -r[:, None] * (w.sign() / w.abs().sum(1, keepdim=True) if norm == "linf" else w / w.square().sum(1, keepdim=True))
    assert torch.allclose(d, free, rtol=1e-9, atol=0)


@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("M", [1, 3, 33, "hand"])
def test_reference_against_the_oracle(M, norm):
    """The torch reference in float64 is the oracle (another formulation of the same definitions) to rounding; in
    float32 it chooses the oracle's classes and stays within the eps rule's floor x 2^10 (a sanity bound: the rule's
    own cap is 8 x this very deviation) - on the random operands, the hand-made images and a ``last`` round."""
    ops = R.hand_cases() if M == "hand" else R.operands(M)
    for last in (False, True):
        want, r64, r32 = R.step_images(ops, norm, last), R.reference_step(ops, norm, torch.float64, last), \
            R.reference_step(ops, norm, torch.float32, last)
        for k in R.KEYS:
            fin = torch.isfinite(want[k])
            assert torch.equal(torch.isnan(r64[k].double()), torch.isnan(want[k])), k
            assert torch.allclose(r64[k].double()[fin], want[k][fin], rtol=1e-9, atol=1e-300 if k == "proj" else 1e-12), k
        assert torch.equal(r32["status"], r64["status"]) and torch.equal(r32["iters"], r64["iters"])
        R.check_step(r32, ops, norm, last)
        scale = want["proj"].abs().amax(dim=(1, 2)).clamp_min(1e-30)
        dev = (r32["proj"].double() - want["proj"]).abs().amax(dim=(1, 2)) / scale
        assert float(torch.nan_to_num(dev, nan=0.0).max()) <= 2.0 ** -13, dev


@pytest.mark.parametrize("variant", R.MUTATIONS)
def test_mutations_are_caught(variant):
    """Each single mistake, made in the oracle, leaves the float32 reference outside the eps rule's cap somewhere."""
    caught = False
    for norm in R.NORMS:
        for ops in (R.operands(3), R.hand_cases()):
            want, bad, ref = R.step_images(ops, norm), R.step_images(ops, norm, variant=variant), \
                R.reference_step(ops, norm)
            for k in ("x", "x_best", "norm_best", "proj"):
                fin = torch.isfinite(want[k]) & torch.isfinite(bad[k])
                caught |= not torch.equal(torch.isfinite(want[k]), torch.isfinite(bad[k]))
                if not fin.any():
                    continue
                eps = max(8.0 * float((ref[k].double() - want[k])[fin].abs().max()), 4 * R.ULP * float(want[k][fin].abs().max()))
                caught |= float((ref[k].double() - bad[k])[fin].abs().max()) > eps
    assert caught


@pytest.mark.parametrize("norm", R.NORMS)
def test_reference_fab_on_the_trained_net(norm):
    imgs, labels = D.trained_case()
    xa, radii, lp, found = R.cpu_fab(norm)
    x0 = _PIXEL_LUT[imgs.reshape(64, 784).long()]
    assert int(found.sum()) >= 32 and torch.equal(found, lp.argmax(1) != labels.long())
    assert (xa >= R.LO).all() and (xa <= R.HI).all() and torch.isfinite(radii[found]).all()
    assert torch.equal(xa.reshape(64, 784)[torch.isinf(radii)], x0[torch.isinf(radii)])
    diff = (xa.reshape(64, 784).double() - x0.double())
    want = (diff.abs().amax(1) if norm == "linf" else diff.square().sum(1).sqrt()) * MNIST_STD
    fin = torch.isfinite(radii) & (want > 0)
    assert ((radii.double() - want).abs()[fin] <= 4 * R.ULP * want[fin]).all()
    history = []
    I.reference_fab(D.trained_net(), x0[:16], labels[:16], norm, 8, *R.PAR, history=history)
    assert len(history) == 9 and all((b <= a).all() for a, b in zip(history, history[1:]))
    if norm == "l2":
        _, r_df, _, f_df = D.cpu_minimum_norm()
        both = found & f_df
        print(f"L2 median radius on {int(both.sum())} images: FAB ({R.STEPS} steps) {float(radii[both].median()):.4f}, "
              f"DeepFool {float(r_df[both].median()):.4f}")


def test_interface(tmp_path, capsys):
    pr = Predictor(D.trained_net())
    imgs, labels = D.trained_case()
    for kw in (dict(norm="l1"), dict(steps=0), dict(steps=True), dict(alpha_max=1.5), dict(eta=0.9), dict(beta=0.0),
               dict(beta=1.5), dict(labels=labels[:3])):
        with pytest.raises(ValueError, match="fab"):
            pr.fab(imgs[:4], **{"labels": labels[:4], **kw})
    with pytest.raises(ValueError, match="fab_steps"):
        pr.robust_evaluate_ensemble(imgs[:4], labels[:4], 0.1, fab_steps=-1)
    # the ensemble: fab_steps = 0 is today's result; > 0 is the AND of its stages
    x, y, eps = imgs[:16], labels[:16], 0.15
    base = pr.robust_evaluate_ensemble(x, y, eps, steps=5, n_targets=1, queries=0)
    assert base == pr.robust_evaluate_ensemble(x, y, eps, steps=5, n_targets=1, queries=0, fab_steps=0)
    assert list(base[2]) == ["clean", "apgd_ce", "apgd_t", "square"]
    got = pr.robust_evaluate_ensemble(x, y, eps, steps=5, n_targets=1, queries=0, fab_steps=10)
    assert list(got[2]) == ["clean", "apgd_ce", "apgd_t", "fab", "square"]
    assert {k: v for k, v in got[2].items() if k not in ("fab", "square")} == {k: v for k, v in base[2].items() if k != "square"}
    alive = pr.predict(x) == y.long()
    alive &= pr.auto_pgd(x, y, eps, 5, loss="ce")[1].argmax(1) == y.long()
    order = pr.log_probs(x).clone().scatter_(1, y.long()[:, None], float("-inf")).sort(dim=1, descending=True, stable=True)[1]
    at = alive.nonzero()[:, 0]
    alive[at] = pr.auto_pgd(x[at], order[at, 0], eps, 5, targeted=True, loss="dlr", true_labels=y[at])[1].argmax(1) == y[at].long()
    at = alive.nonzero()[:, 0]
    _, radii, _, found = pr.fab(x[at], y[at], "linf", 10)
    alive[at] = ~(found & (radii <= eps))
    assert got[0] == got[2]["square"] == got[2]["fab"] == int(alive.sum()) and got[2]["fab"] <= base[0]
    # the command line
    args = I.build_predict_parser().parse_args([])
    assert (args.fab, args.fab_norm, args.fab_steps, args.fab_count, args.fab_radii, args.ensemble_fab_steps) == \
        (False, "linf", 100, None, (), 0)
    assert I.ensemble_line(0.1, 9, 3, 4) == "Ensemble set (Linf eps=0.1: apgd-ce, apgd-t x 9, square): Accuracy: 3/4 (75%)"
    assert I.ensemble_line(0.1, 9, 3, 4, True).startswith("Ensemble set (Linf eps=0.1: apgd-ce, apgd-t x 9, fab, square): ")
    assert I.fab_line("l2", 7, 8, 4, 0.5, None) == "FAB set (L2, steps=7): Found: 4/8 (50%), median radius: 0.5000, mean radius: n/a"
    torch.manual_seed(5)
    ckpt, log = str(tmp_path / "net.pt"), str(tmp_path / "log.jsonl")
    save_state_dict(Net(), ckpt)
    common = ["--no-cuda", "--synthetic", "--synthetic-test-size", "16", "--checkpoint", ckpt, "--json-log", log]
    assert I.predict_main(common) == 0
    plain = capsys.readouterr().out
    assert I.predict_main(common + ["--fab", "--fab-norm", "l2", "--fab-steps", "3", "--fab-count", "8", "--fab-radii",
                                    "0.5", "--ensemble-eps", "0.1", "--ensemble-steps", "2", "--ensemble-targets", "1",
                                    "--ensemble-queries", "0", "--ensemble-fab-steps", "2"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert [lines[0]] == [ln for ln in plain.splitlines() if ln.strip()]
    assert lines[1].startswith("FAB set (L2, steps=3): Found: ") and lines[2].startswith("Accuracy at radius 0.5: ")
    assert lines[3].startswith("Ensemble set (Linf eps=0.1: apgd-ce, apgd-t x 1, fab, square): ")
    with open(log) as f:
        rec = [json.loads(ln) for ln in f]
    assert not any(k.startswith("fab_") or k == "ensemble_fab_steps" for k in rec[0])
    assert rec[1]["fab_norm"] == "l2" and rec[1]["fab_steps"] == 3 and rec[1]["fab_count"] == 8 and \
        set(rec[1]["fab_accuracy_at"]) == {"0.5"} and rec[1]["ensemble_fab_steps"] == 2 and "fab" in rec[1]["ensemble_after"]
