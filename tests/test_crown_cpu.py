"""CROWN-IBP on the CPU side: ``crown_ibp_reference`` (float32, the kernels' formulas) against the float64 oracle of
``crown_ref``, the eps = 0 identity, soundness against sampled points of the box, what the bound buys over IBP, and
``method=`` on the ``Predictor`` and the command line."""
import json

import pytest
import torch

from pytorch_mnist_ddp_amd import inference as I
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import crown_ref as CR
import ibp_ref as R


@pytest.mark.parametrize("kind", ["random", "trained"])
def test_reference_against_oracle(kind):
    """Every continuous stage within 64 float32 ulps of its row's largest float64 value (the bound of
    ``test_ibp_cpu.test_reference_against_oracle``); the record's discrete fields equal off the near-tie units.
    M = 3, each of the four eps rows used."""
    net = R.net(kind)
    x, y, _ = R.case(3)
    for eps in (CR.EPS_ROWS[:3], CR.EPS_ROWS[1:]):
        eps = torch.tensor(eps)
        want, got = CR.oracle(net, x, y, eps), Fk.crown_ibp_reference(net, x, y, eps)
        hold = CR.check_record(got, want, 3)
        for k in ("pl", "pu", "lb_ibp", "sU", "bU") + CR.CONTINUOUS:
            for i in range(3):
                g, w = (got[k][i][hold[i]], want[k][i][hold[i]]) if k in ("sU", "bU") else (got[k][i], want[k][i])
                dev, scale = R.worst(g, w)
                print(f"crown_ibp_reference {kind} eps={float(eps[i]):g} {k}: deviation {dev:.3e}, scale {scale:.3e}")
                assert dev <= 64 * R.ulp(scale), (k, i, dev, scale)


def test_eps_zero_is_the_forward():
    net = R.net("trained")
    x, y, _ = R.case(3)
    lb = CR.oracle(net, x, y, torch.zeros(3))["lb_crown"]
    want = CR.margins64(net, x, y)
    off = torch.isfinite(lb)
    assert int(off.sum()) == 27 and float((lb[off] - want[off]).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("eps", [0.002, 0.02])
def test_soundness_and_never_below_ibp(eps):
    """No float64 forward margin of the box centre or of 64 random box corners falls below the float32 ``lb`` by more
    than that image's own deviation of the float32 reference from the oracle; ``lb >= lb_ibp`` element-wise."""
    net = R.net("trained")
    x, y, _ = R.case(8)
    e = torch.full((8,), eps)
    got, want = Fk.crown_ibp_reference(net, x, y, e), CR.oracle(net, x, y, e)["lb"]
    assert bool((got["lb"] >= got["lb_ibp"]).all())
    l = (x.double() - R.f32(eps) / R.f32(MNIST_STD)).clamp(min=R.f32(PIXEL_LO))
    u = (x.double() + R.f32(eps) / R.f32(MNIST_STD)).clamp(max=R.f32(PIXEL_HI))
    gen = torch.Generator().manual_seed(0)
    points = [(l + u) / 2] + [torch.where(torch.rand(8, 784, generator=gen) < 0.5, l, u) for _ in range(64)]
    margins = torch.stack([CR.margins64(net, pt, y) for pt in points]).min(dim=0).values
    for i in range(8):
        off = torch.isfinite(got["lb"][i])
        slack = R.worst(got["lb"][i], want[i])[0]
        assert bool((margins[i][off] >= got["lb"][i][off].double() - slack).all()), (i, eps)


def test_certifies_more_than_ibp():
    """The float64 oracle on the first 32 ``trained_case`` images (counts recorded in docs/COVERAGE.md)."""
    x, y, _ = R.case(32)
    for eps in (0.001, 0.003):
        o = CR.oracle(R.net("trained"), x, y, torch.full((32,), eps))
        ibp, crown = (int((o[k].min(dim=1).values > 0).sum()) for k in ("lb_ibp", "lb"))
        print(f"eps {eps:g}: IBP certifies {ibp}/32, CROWN-IBP {crown}/32")
        assert crown > ibp and bool((o["lb_crown"] >= o["lb_ibp"]).all())


def test_predictor_method_and_cli(tmp_path, capsys):
    pr = I.Predictor(R.net("trained"))
    x, y, _ = R.case(3)
    x4 = x.view(3, 1, 28, 28)
    for plain, kw in ((pr.verify_linf(x4, y, 0.002), pr.verify_linf(x4, y, 0.002, method="ibp")),
                      (pr.certified_radius_linf(x4, y, 0.1, 4), pr.certified_radius_linf(x4, y, 0.1, 4, method="ibp"))):
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(plain, kw))
    for call in (lambda: pr.verify_linf(x4, y, 0.002, method="crown"), lambda: pr.certified_radius_linf(x4, y, method="")):
        with pytest.raises(ValueError):
            call()
    cert, lb = pr.verify_linf(x4, y, 0.002, method="crown-ibp")
    assert torch.equal(lb, Fk.crown_ibp_reference(R.net("trained"), x, y, 0.002)["lb"]) and bool(cert.all())
    radii, ibp = pr.certified_radius_linf(x4, y, 0.1, 6, method="crown-ibp")[0], pr.certified_radius_linf(x4, y, 0.1, 6)[0]
    assert bool((radii >= ibp).all()) and bool((radii > ibp).any())
    torch.manual_seed(5)
    ckpt, log = str(tmp_path / "net.pt"), str(tmp_path / "log.jsonl")
    save_state_dict(Net(), ckpt)
    args = ["--no-cuda", "--synthetic", "--synthetic-test-size", "8", "--checkpoint", ckpt, "--json-log", log, "--ibp-eps",
            "0.001", "--ibp-radius", "--ibp-eps-max", "0.05", "--ibp-search-steps", "2", "--ibp-count", "4"]
    assert I.predict_main(args) == 0 and I.predict_main(args + ["--ibp-method", "ibp"]) == 0
    plain, same = (ln.strip() for ln in capsys.readouterr().out.split("Test set")[1:])
    assert plain == same and "CROWN" not in plain
    assert I.predict_main(args + ["--ibp-method", "crown-ibp"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert lines[1].startswith("Verified set (Linf eps=0.001, CROWN-IBP): Accuracy: ")
    assert lines[2].startswith("CROWN-IBP set (Linf, eps_max=0.05, search=2): Certified: ") and "/4 (" in lines[2]
    with open(log) as f:
        rec = [json.loads(ln) for ln in f]
    assert rec[0] == rec[1] and "ibp_method" not in rec[0] and rec[2]["ibp_method"] == "crown-ibp"
    assert set(rec[2]) == set(rec[0]) | {"ibp_method"}
