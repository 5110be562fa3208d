"""Randomized smoothing off the GPU: the confidence bound and ``certify_from_counts`` against scipy, the float64
emulation of the noise generator (counters, moments), ``Predictor.certify`` on the CPU, ``--noise-train-sigma`` on
the module path against a loop written out here, ``mnist_predict.py --certify-*``, and the mutation proofs of the
comparators the GPU tests use (``smooth_ref``)."""
import json
from statistics import NormalDist

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import cli, driver
from pytorch_mnist_ddp_amd import inference as inf
from pytorch_mnist_ddp_amd.data import consume_loader_base_seed
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.trainer import FusedTrainer, noise_config
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import smooth as S
from pytorch_mnist_ddp_amd.optim import Adadelta
from pytorch_mnist_ddp_amd.utils.checkpoint import load_state_dict
from pytorch_mnist_ddp_amd.utils.logging import train_line

import smooth_ref as SR

PHI_INV = NormalDist().inv_cdf


# ---------------------------------------------------------------------------- the confidence bound
@pytest.mark.parametrize("alpha", [1e-3, 0.05])
@pytest.mark.parametrize("n", [1, 100, 100000])
def test_lower_bound_equals_scipy(n, alpha):
    beta = pytest.importorskip("scipy.stats").beta
    for k in sorted({0, 1, n // 2, n - 1, n, n // 3, (9 * n) // 10} & set(range(n + 1))):
        got = S.lower_confidence_bound(k, n, alpha)
        want = 0.0 if k == 0 else float(beta.ppf(alpha, k, n - k + 1))
        assert abs(got - want) <= 1e-9, (k, n, alpha, got, want)
        assert 0.0 <= got < 1.0
    assert S.lower_confidence_bound(n, n, alpha) == alpha ** (1.0 / n)       # exactly
    assert S.lower_confidence_bound(0, n, alpha) == 0.0


def test_certify_from_counts():
    sigma, alpha, n = 0.5, 0.001, 1000
    sel = [0, 0, 0, 7, 0, 0, 0, 3, 0, 0]

    def est(k, cls=3):
        c = [0] * 10
        c[cls], c[(cls + 1) % 10] = k, n - k
        return c

    assert S.certify_from_counts(sel, est(n // 2), sigma, alpha) == (-1, 0.0)          # k = n / 2 abstains
    assert S.certify_from_counts(sel, est(0), sigma, alpha) == (-1, 0.0)
    assert S.certify_from_counts(sel, est(n, cls=7), sigma, alpha) == (-1, 0.0)        # all votes for another class
    last = 0.0
    for k in range(n // 2, n + 1, 10):                                                 # monotone in k
        cls, rad = S.certify_from_counts(sel, est(k), sigma, alpha)
        p_l = S.lower_confidence_bound(k, n, alpha)
        if p_l > 0.5:
            assert cls == 3 and rad == sigma * PHI_INV(p_l) and rad > last
            last = rad
        else:
            assert (cls, rad) == (-1, 0.0) and last == 0.0
    assert last == sigma * PHI_INV(alpha ** (1.0 / n))                                 # the unanimous vote
    assert S.certify_from_counts([5, 5, 0, 0, 0, 0, 0, 0, 0, 0], est(n, cls=0), sigma, alpha)[0] == 0   # first max
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            S.lower_confidence_bound(5, 10, bad)
    with pytest.raises(ValueError):
        S.lower_confidence_bound(11, 10, 0.05)


# ---------------------------------------------------------------------------- the generator, emulated
def test_noise_generator_counters_and_moments():
    """M = 4, n = 320: 1 003 520 normals.  Standard errors under the Gaussian hypothesis, N elements: mean
    1 / sqrt(N); variance sqrt(2 / N) (Var z^2 = 2); excess kurtosis sqrt(24 / N) (the classical large-sample value;
    the 5.77 sigma cut lowers E z^4 by 1e-5 of itself, far inside it); lag-1 correlation of neighbours 1 / sqrt(N - 1)
    (products of independent unit normals have variance 1)."""
    M, n, seed = 4, 320, 0x1234ABCD5678
    c0, c1, c2, c3 = SR.smooth_counters(M, n, sample_base=7, id_base=100)
    assert c0.size == M * n * 196
    packed = np.stack([c0, c2, c3], axis=1)
    assert np.unique(packed, axis=0).shape[0] == c0.size                     # every counter is distinct
    assert (c1 != 0).all() and (c1 != SR.ADV_PHILOX_DOMAIN).all() and (c1 == SR.SMOOTH_PHILOX_DOMAIN).all()
    z = SR.box_muller(SR.smooth_words(M, n, seed, 7, 100), SR.F64)
    assert z.shape == (M * n, 784) and np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2.0))
    flat = z.ravel()
    N = flat.size
    mean, var = flat.mean(), flat.var()
    kurt = ((flat - mean) ** 4).mean() / var ** 2 - 3.0
    lag1 = float(((flat[:-1] - mean) * (flat[1:] - mean)).mean() / var)
    print(f"N={N}: mean {mean:.3e} (se {N ** -0.5:.3e}), var-1 {var - 1:.3e} (se {(2 / N) ** 0.5:.3e}), "
          f"excess kurtosis {kurt:.3e} (se {(24 / N) ** 0.5:.3e}), lag-1 {lag1:.3e} (se {(N - 1) ** -0.5:.3e})")
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / N)
    assert abs(kurt) < 5 * np.sqrt(24.0 / N)
    assert abs(lag1) < 5 / np.sqrt(N - 1)
    # float32 emulation: the same numbers to fp32 accuracy
    z32 = SR.box_muller(SR.smooth_words(1, 3, seed), SR.F32)
    assert z32.dtype == np.float32 and np.abs(z32 - SR.box_muller(SR.smooth_words(1, 3, seed), SR.F64)).max() < 1e-5


# ---------------------------------------------------------------------------- Predictor.certify on the CPU
def _biased_net(cls=4, bias=50.0):
    torch.manual_seed(0)
    net = Net()
    with torch.no_grad():
        net.fc2.bias[cls] += bias
    return net


def test_cpu_certify():
    torch.manual_seed(2)
    net = Net()
    net.train()
    pr = Predictor(net)
    imgs, _ = generate(3, seed=4)
    a = pr.certify(imgs, 0.25, n0=20, n=60, alpha=0.01, seed=9)
    before = torch.get_rng_state()
    b = pr.certify(imgs, 0.25, n0=20, n=60, alpha=0.01, seed=9)
    assert torch.equal(torch.get_rng_state(), before)                        # its own generator
    assert all(torch.equal(p, q) for p, q in zip(a, b))                      # reproducible for one seed
    classes, radii, counts = a
    assert classes.dtype == torch.int64 and radii.dtype == torch.float64 and counts.dtype == torch.int32
    assert counts.shape == (3, 10) and (counts.sum(dim=1) == 60).all()
    assert net.training and all(p.grad is None for p in net.parameters())
    c0 = pr.smoothed_counts(imgs, 0.25, 20, seed=9)
    c1 = pr.smoothed_counts(imgs, 0.25, 60, seed=9, sample_base=20)
    assert torch.equal(c1, counts)
    for j in range(3):
        assert (int(classes[j]), float(radii[j])) == S.certify_from_counts(c0[j].tolist(), c1[j].tolist(), 0.25, 0.01)
    assert not torch.equal(pr.smoothed_counts(imgs, 0.25, 60, seed=9), c1)   # [0, 60) is another draw than [20, 80)
    assert torch.equal(pr.smoothed_counts(imgs[1:], 0.25, 20, seed=9, ids=[1, 2]), c0[1:])   # the id names the draw
    # a net biased towards one class: a unanimous vote, the largest radius n and alpha allow
    cls, rad, cnt = Predictor(_biased_net(4)).certify(imgs, 0.5, n0=10, n=200, alpha=0.001)
    assert (cls == 4).all() and (cnt[:, 4] == 200).all()
    assert torch.equal(rad, torch.full((3,), 0.5 * PHI_INV(0.001 ** (1.0 / 200)), dtype=torch.float64))


def test_certify_value_errors():
    pr = Predictor(Net())
    x = torch.zeros(2, 28, 28, dtype=torch.uint8)
    for kw in (dict(sigma=0.0), dict(sigma=-0.5), dict(sigma=0.5, n0=0), dict(sigma=0.5, n=0),
               dict(sigma=0.5, alpha=0.0), dict(sigma=0.5, alpha=1.0), dict(sigma=0.5, ids=[0]),
               dict(sigma=0.5, ids=[0, 1, 2])):
        with pytest.raises(ValueError):
            pr.certify(x, **kw)
    with pytest.raises(ValueError):
        pr.smoothed_counts(x, 0.0, 10)
    with pytest.raises(ValueError):
        pr.smoothed_counts(x, 0.5, 0)
    with pytest.raises(ValueError):
        pr.smoothed_counts(x, 0.5, 10, ids=[3])


# ---------------------------------------------------------------------------- --noise-train-sigma
@pytest.mark.parametrize("ddp", [False, True])
def test_noise_flag_parses_and_excludes_adversarial(ddp, capsys):
    assert cli.parse_args(ddp=ddp, argv=[]).noise_train_sigma is None
    assert cli.parse_args(ddp=ddp, argv=["--noise-train-sigma", "0.25"]).noise_train_sigma == 0.25
    argv = "--batch-size 200 --epochs 3 --synthetic".split()
    with_flag, without = vars(cli.parse_args(ddp=ddp, argv=argv + ["--noise-train-sigma", "0.5"])), \
        vars(cli.parse_args(ddp=ddp, argv=argv))
    assert {k: v for k, v in with_flag.items() if k != "noise_train_sigma"} == \
        {k: v for k, v in without.items() if k != "noise_train_sigma"}
    for bad in (["--noise-train-sigma", "0.25", "--adv-train-eps", "0.1"], ["--noise-train-sigma", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(ddp=ddp, argv=bad)
        assert e.value.code == 2
    assert "mutually exclusive" in capsys.readouterr().err


def test_noise_config_and_trainer_checks():
    assert noise_config(None) is None and noise_config(0.0) == 0.0 and noise_config(0.5) == 0.5
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            noise_config(bad)
    with pytest.raises(ValueError, match="mutually exclusive"):
        noise_config(0.5, adversarial={"eps": 0.1})
    with pytest.raises(ValueError, match="world size 1"):
        noise_config(0.5, world_size=2)
    with pytest.raises(ValueError, match="bf16"):
        noise_config(0.5, fp32=True)
    for kw in (dict(noise_sigma=-1.0), dict(noise_sigma=0.5, adversarial={"eps": 0.1}),
               dict(noise_sigma=0.5, world_size=2), dict(noise_sigma=0.5, fp32=True)):
        with pytest.raises(ValueError):                       # no model state, no GPU: the check comes first
            FusedTrainer(None, None, None, 64, 64, 128, **kw)


ARGV = ["--no-cuda", "--synthetic", "--synthetic-size", "128", "--synthetic-test-size", "64", "--batch-size", "64",
        "--epochs", "1", "--log-interval", "1", "--save-model"]


def _run_mnist(tmp_path, monkeypatch, capsys, *extra, json_log=None):
    monkeypatch.chdir(tmp_path)
    argv = ARGV + list(extra) + (["--json-log", str(json_log)] if json_log else [])
    assert driver.run(argv, ddp_script=False) == 0
    rng = torch.get_rng_state()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    net = Net()
    load_state_dict(net, str(tmp_path / "mnist_cnn.pt"), map_location="cpu")
    recs = []
    if json_log:
        with open(json_log) as f:
            recs = [json.loads(ln) for ln in f if ln.strip()]
    return lines, net, rng, recs


def test_cpu_noise_training_equals_the_written_out_loop_bitwise(tmp_path, monkeypatch, capsys):
    lines, net, _, recs = _run_mnist(tmp_path, monkeypatch, capsys, "--noise-train-sigma", "0.25",
                                     json_log=tmp_path / "noise.jsonl")
    # the same two steps written out: seed, model init, the loader's base seed, then per step the noise draw
    # (before model(data)), dropout1 and dropout2
    torch.manual_seed(1)
    train = load_mnist("./data", True, True, 128, verbose=False)
    ref = Net()
    opt = Adadelta(ref.parameters(), lr=1.0)
    consume_loader_base_seed()
    ref.train()
    want = []
    for s in range(2):
        data, target = normalize_u8(train.images[64 * s:64 * s + 64]), train.targets[64 * s:64 * s + 64]
        noisy = data + (0.25 / MNIST_STD) * torch.randn(data.shape, dtype=torch.float32)
        opt.zero_grad()
        loss = F.nll_loss(ref(noisy), target)
        loss.backward()
        opt.step()
        want.append(train_line(1, s * 64, 128, s, 2, loss.item()).rstrip("\n"))
    for (n, p), (m, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert n == m and torch.equal(p, q), n
    assert lines[:2] == want and len(lines) == 3 and lines[2].startswith("Test set: Average loss: ")
    assert len(recs) == 1 and recs[0]["noise_train_sigma"] == 0.25 and "adv_train_eps" not in recs[0]
    with pytest.raises(ValueError, match="mutually exclusive"):     # the driver's config check, past the parser
        args = cli.parse_args(ddp=False, argv=ARGV + ["--noise-train-sigma", "0.25"])
        args.adv_train_eps = 0.1
        noise_config(args.noise_train_sigma, cli.adversarial_from_args(args))


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch, capsys):
    """A run without the flag: the RNG draws and printed lines of the loop written out without any noise draw, and
    the JSON record's keys of today."""
    lines, net, rng_after, recs = _run_mnist(tmp_path, monkeypatch, capsys, json_log=tmp_path / "plain.jsonl")
    torch.manual_seed(1)
    train = load_mnist("./data", True, True, 128, verbose=False)
    test = load_mnist("./data", False, True, 64, verbose=False)
    ref = Net()
    opt = Adadelta(ref.parameters(), lr=1.0)
    consume_loader_base_seed()
    ref.train()
    want = []
    for s in range(2):
        data, target = normalize_u8(train.images[64 * s:64 * s + 64]), train.targets[64 * s:64 * s + 64]
        opt.zero_grad()
        loss = F.nll_loss(ref(data), target)
        loss.backward()
        opt.step()
        want.append(train_line(1, s * 64, 128, s, 2, loss.item()).rstrip("\n"))
    assert lines[:2] == want and len(lines) == 3
    for (n, p), (m, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(p, q), n
    consume_loader_base_seed()
    ref.eval()
    with torch.no_grad():
        ref(normalize_u8(test.images))
    assert torch.equal(torch.get_rng_state(), rng_after)                     # nothing else was drawn
    assert len(recs) == 1 and sorted(recs[0]) == ["correct", "epoch", "test_loss", "train_s"]


# ---------------------------------------------------------------------------- mnist_predict.py
def test_predict_flags_and_line_format():
    a = inf.build_predict_parser().parse_args([])
    assert (a.certify_sigma, a.certify_n, a.certify_n0, a.certify_alpha, a.certify_radii, a.certify_count,
            a.certify_seed) == (None, 1000, 100, 0.001, (0.0, 0.25, 0.5), None, 0)
    b = inf.build_predict_parser().parse_args("--certify-sigma 0.5 --certify-n 200 --certify-n0 20 --certify-alpha 0.01 "
                                              "--certify-radii 0,0.1,1.5 --certify-count 7 --certify-seed 3".split())
    assert (b.certify_sigma, b.certify_n, b.certify_n0, b.certify_alpha, b.certify_radii, b.certify_count,
            b.certify_seed) == (0.5, 200, 20, 0.01, (0.0, 0.1, 1.5), 7, 3)
    with pytest.raises(SystemExit):
        inf.build_predict_parser().parse_args(["--certify-radii", "0,-1"])
    assert inf.certified_line(0.5, 1000, 0.001, 0.25, 17, 32, 3) == \
        "Certified set (L2 sigma=0.5, n=1000, alpha=0.001, radius=0.25): Accuracy: 17/32 (53%), abstained 3"


def test_predict_cli_end_to_end_on_the_cpu(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    torch.save(_biased_net(4).state_dict(), tmp_path / "mnist_cnn.pt")
    base = ["--no-cuda", "--synthetic", "--synthetic-test-size", "32", "--batch-size", "16"]
    assert inf.predict_main(base + ["--json-log", "plain.jsonl"]) == 0
    plain_out = capsys.readouterr().out
    assert inf.predict_main(base + ["--json-log", "cert.jsonl", "--certify-sigma", "0.5", "--certify-n", "40",
                                    "--certify-n0", "10", "--certify-alpha", "0.01", "--certify-count", "20"]) == 0
    out = capsys.readouterr().out
    plain = json.loads((tmp_path / "plain.jsonl").read_text())
    cert = json.loads((tmp_path / "cert.jsonl").read_text())
    assert sorted(plain) == ["checkpoint", "correct", "device", "n", "source", "test_loss"]         # today's record
    assert [ln for ln in plain_out.splitlines() if ln.strip()][0].startswith("Test set: Average loss: ")
    assert len([ln for ln in plain_out.splitlines() if ln.strip()]) == 1
    assert out.startswith(plain_out) and {k: cert[k] for k in plain} == plain
    targets = load_mnist("./data", False, True, 32, verbose=False).targets[:20]
    fours = int((targets == 4).sum())
    lines = out[len(plain_out):].splitlines()
    assert lines == [inf.certified_line(0.5, 40, 0.01, r, fours if r <= 0.5 * PHI_INV(0.01 ** (1 / 40)) else 0, 20, 0)
                     for r in (0.0, 0.25, 0.5)]
    assert {k for k in cert if k not in plain} == {"certify_sigma", "certify_n", "certify_n0", "certify_alpha",
                                                   "certify_seed", "certify_count", "certify_radii",
                                                   "certify_correct", "certify_abstained"}
    assert (cert["certify_sigma"], cert["certify_n"], cert["certify_n0"], cert["certify_alpha"], cert["certify_count"],
            cert["certify_radii"], cert["certify_abstained"]) == (0.5, 40, 10, 0.01, 20, [0.0, 0.25, 0.5], 0)


# ---------------------------------------------------------------------------- mutation proofs of the comparators
def _noise_case():
    imgs, _ = generate(3, seed=21)
    x0 = _PIXEL_LUT[imgs.reshape(3, 784).long()].numpy()
    return x0, np.float32(0.5 / MNIST_STD)


def _noise_passes(candidate, x0, sigma, n=5):
    """The GPU test's comparison: every element within ``noise_eps`` of the float64 oracle."""
    want64 = SR.noise_emulation(x0, sigma, n, 77, 3, 11, SR.F64)
    eps = SR.noise_eps(SR.noise_emulation(x0, sigma, n, 77, 3, 11, SR.F32), want64)
    return bool((np.abs(candidate.astype(np.float64) - want64) <= eps).all())


def test_noise_comparator_passes_the_stand_in_and_fails_each_mutation():
    x0, sigma = _noise_case()
    assert _noise_passes(SR.noise_emulation(x0, sigma, 5, 77, 3, 11, SR.F32), x0, sigma)       # the numpy stand-in
    for mut in ("swap", "u1", "sincos", "sigma2"):                                           # mutations 1 to 4
        bad = SR.noise_emulation(x0, sigma, 5, 77, 3, 11, SR.F32, mut=frozenset([mut]))
        assert np.isfinite(bad).all() or mut == "u1"
        assert not _noise_passes(bad, x0, sigma), mut


def test_u1_mutation_is_caught_even_where_it_stays_finite():
    """Without the + 1, u1 = 0 gives an infinite radius only once in 2^24 draws; the comparator catches the
    mutation on every draw, because log(u1) moves by 1 / (w >> 8) relative - far above eps for small words."""
    x0, sigma = _noise_case()
    bad = SR.noise_emulation(x0, sigma, 5, 77, 3, 11, SR.F32, mut=frozenset(["u1"]))
    want64 = SR.noise_emulation(x0, sigma, 5, 77, 3, 11, SR.F64)
    assert np.isfinite(bad).all() and not _noise_passes(bad, x0, sigma)
    assert np.abs(bad - want64).max() > 0


def test_vote_comparator_passes_the_stand_in_and_fails_each_mutation():
    M, n = 3, 257
    lp = SR.hand_logp(M, n, seed=5)
    want = SR.vote_reference(lp, M, n)
    assert np.array_equal(SR.vote_reference(lp.copy(), M, n), want)
    for mut in ("last", "nan0"):                                                             # mutations 5, 6
        assert not np.array_equal(SR.vote_reference(lp, M, n, mut=frozenset([mut])), want), mut
    k = 100
    parts = lp.reshape(M, n, 10)
    first = SR.vote_reference(parts[:, :k].reshape(-1, 10), M, k)
    second = parts[:, k:].reshape(-1, 10)
    assert np.array_equal(SR.vote_reference(second, M, n - k, counts=first, accumulate=True), want)
    assert not np.array_equal(SR.vote_reference(second, M, n - k, counts=first, accumulate=True,
                                                mut=frozenset(["overwrite"])), want)         # mutation 7


def test_estimation_samples_reusing_the_selection_samples_is_caught():
    """Mutation 8: the estimation counts drawn from [0, n) instead of [n0, n0 + n).  The comparison the GPU test
    makes (``certify``'s counts == ``smoothed_counts(sample_base = n0)``) tells them apart: the two ranges give
    other rows, so on a net with no strong preference other counts."""
    torch.manual_seed(2)
    pr = Predictor(Net())
    imgs, _ = generate(3, seed=4)
    _, _, counts = pr.certify(imgs, 0.5, n0=30, n=60, alpha=0.01, seed=9)
    assert torch.equal(counts, pr.smoothed_counts(imgs, 0.5, 60, seed=9, sample_base=30))
    assert not torch.equal(counts, pr.smoothed_counts(imgs, 0.5, 60, seed=9, sample_base=0))
    # and in the emulation of the kernel's draw: the rows of [0, n) and [n0, n0 + n) share only their overlap
    x0, sigma = _noise_case()
    a = SR.noise_emulation(x0[:1], sigma, 6, 77, 0, 0, SR.F32)
    b = SR.noise_emulation(x0[:1], sigma, 6, 77, 4, 0, SR.F32)
    assert np.array_equal(a[4:], b[:2]) and not np.array_equal(a[:2], b[:2])
