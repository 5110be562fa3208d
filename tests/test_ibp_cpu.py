"""Interval bound propagation on the CPU side: ``ibp_reference`` (centre / radius, float32) against the float64 lower /
upper oracle, the eps = 0 identity, soundness against sampled points of the box, and the command line."""
import json

import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import inference as I
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import ibp_ref as R

STAGES = ("pl", "pu", "z1c", "z1r", "lb")


def _margins64(net, x, y):
    """z_y - z_j of the float64 forward (inference semantics) at the rows ``x``."""
    P = {k: v.detach().double() for k, v in net.named_parameters()}
    h = F.relu(F.conv2d(x.double().view(-1, 1, 28, 28), P["conv1.weight"], P["conv1.bias"]))
    h = F.max_pool2d(F.relu(F.conv2d(h, P["conv2.weight"], P["conv2.bias"])), 2).flatten(1)
    z = F.relu(h @ P["fc1.weight"].t() + P["fc1.bias"]) @ P["fc2.weight"].t() + P["fc2.bias"]
    return z.gather(1, y[:, None]) - z


@pytest.mark.parametrize("kind", ["random", "trained"])
def test_reference_against_oracle(kind):
    """Every stage of the float32 reference within 64 float32 ulps of its row's largest float64 value: the stages are
    sums of 9 to 9216 float32 products, whose blocked summation errs by a few ulps of the largest partial sum, and a
    bound is the difference of two such sums.  M = 3, each of the four eps rows used."""
    net = R.net(kind)
    x, y, _ = R.case(3)
    for eps in (R.EPS_ROWS[:3], R.EPS_ROWS[1:]):
        eps = torch.tensor(eps)
        want, got = R.oracle(net, x, y, eps), Fk.ibp_reference(net, x, y, eps)
        for k in STAGES:
            for i in range(3):
                dev, scale = R.worst(got[k][i], want[k][i])
                print(f"ibp_reference {kind} eps={float(eps[i]):g} {k}: deviation {dev:.3e}, scale {scale:.3e}")
                assert dev <= 64 * R.ulp(scale), (k, i, dev, scale)


def test_eps_zero_is_the_forward():
    net = R.net("trained")
    x, y, _ = R.case(3)
    lb = R.oracle(net, x, y, torch.zeros(3))["lb"]
    want = _margins64(net, x, y)
    off = torch.isfinite(lb)
    assert int(off.sum()) == 27 and float((lb[off] - want[off]).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("eps", [0.002, 0.05])
def test_soundness_on_sampled_points(eps):
    """No float64 forward margin of the box centre or of 64 random box corners falls below the float32 ``lb`` by more
    than that image's own deviation of the float32 reference from the oracle."""
    net = R.net("trained")
    x, y, _ = R.case(8)
    e = torch.full((8,), eps)
    got, want = Fk.ibp_reference(net, x, y, e)["lb"], R.oracle(net, x, y, e)["lb"]
    l = (x.double() - R.f32(eps) / R.f32(MNIST_STD)).clamp(min=R.f32(PIXEL_LO))
    u = (x.double() + R.f32(eps) / R.f32(MNIST_STD)).clamp(max=R.f32(PIXEL_HI))
    gen = torch.Generator().manual_seed(0)
    points = [(l + u) / 2] + [torch.where(torch.rand(8, 784, generator=gen) < 0.5, l, u) for _ in range(64)]
    for i in range(8):
        slack = R.worst(got[i], want[i])[0]
        for pt in points:
            m = _margins64(net, pt[i:i + 1], y[i:i + 1])[0]
            off = torch.isfinite(got[i])
            assert bool((m[off] >= got[i][off].double() - slack).all()), (i, eps)


def test_search_reference_and_cli(tmp_path, capsys):
    rec = torch.tensor([[0.1, 0.0, 0.1, 0.0]] * 3)
    lb = torch.tensor([[1.0] * 10, [-1.0] + [2.0] * 9, [float("nan")] + [2.0] * 9])
    out = Fk.ibp_search_reference(rec, lb)
    assert out[0].tolist() == [pytest.approx(0.1)] * 3 + [1.0] and out[1, :3].tolist() == [pytest.approx(0.05), 0.0, pytest.approx(0.1)]
    assert out[2, 2] == out[1, 2] and torch.isnan(out[2, 3])                   # a NaN is not certified
    pr = I.Predictor(R.net("trained"))
    x, y, _ = R.case(3)
    radii, cert, _ = pr.certified_radius_linf(x.view(3, 1, 28, 28), y, 0.1, 6)
    assert bool(pr.verify_linf(x.view(3, 1, 28, 28), y, 0.0)[0].all()) and torch.equal(cert, radii > 0)
    torch.manual_seed(5)
    ckpt, log = str(tmp_path / "net.pt"), str(tmp_path / "log.jsonl")
    save_state_dict(Net(), ckpt)
    common = ["--no-cuda", "--synthetic", "--synthetic-test-size", "16", "--checkpoint", ckpt, "--json-log", log]
    assert I.predict_main(common) == 0
    plain = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert I.predict_main(common + ["--ibp-eps", "0.001", "--ibp-radius", "--ibp-eps-max", "0.05", "--ibp-search-steps",
                                    "3", "--ibp-count", "8", "--ibp-radii", "0.001"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert lines[:1] == plain and len(plain) == 1 and len(lines) == 4
    assert lines[1].startswith("Verified set (Linf eps=0.001, IBP): Accuracy: ") and "/16 (" in lines[1]
    assert lines[2].startswith("IBP set (Linf, eps_max=0.05, search=3): Certified: ") and "/8 (" in lines[2]
    assert lines[3].startswith("Certified accuracy at radius 0.001: ")
    with open(log) as f:
        rec = [json.loads(ln) for ln in f]
    assert not any(k.startswith("ibp_") for k in rec[0])
    assert {"ibp_eps", "ibp_verified", "ibp_eps_max", "ibp_search_steps", "ibp_count", "ibp_certified",
            "ibp_median_radius", "ibp_mean_radius", "ibp_accuracy_at"} <= set(rec[1]) and rec[1]["ibp_count"] == 8
