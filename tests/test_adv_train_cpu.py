"""Adversarial training off the GPU: the ``--adv-train-*`` flags, the module path (``driver.craft_adversarial``
before ``model(data)``) against a loop written out here, argument checking, the JSON record's keys, and the numpy
emulation of ``adv_init``'s random start that the GPU test compares the kernel with."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import cli, driver
from pytorch_mnist_ddp_amd.data import consume_loader_base_seed
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.trainer import FusedTrainer, adversarial_config
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.optim import Adadelta
from pytorch_mnist_ddp_amd.utils.checkpoint import load_state_dict
from pytorch_mnist_ddp_amd.utils.logging import test_line as fmt_test_line
from pytorch_mnist_ddp_amd.utils.logging import train_line

from advtrain_ref import adv_init_emulation, plain_pgd

ADV_DEFAULTS = {"adv_train_eps": None, "adv_train_steps": 1, "adv_train_step_size": None,
                "adv_train_random_start": False}


# ---------------------------------------------------------------------------- parser
@pytest.mark.parametrize("ddp", [False, True])
def test_parser_flags_and_defaults(ddp):
    a = vars(cli.parse_args(ddp=ddp, argv=[]))
    for k, v in ADV_DEFAULTS.items():
        assert a[k] == v and type(a[k]) is type(v), k
    assert cli.adversarial_from_args(cli.parse_args(ddp=ddp, argv=[])) is None
    b = cli.parse_args(ddp=ddp, argv="--adv-train-eps 0.1 --adv-train-steps 7 --adv-train-step-size 0.02 "
                                     "--adv-train-random-start".split())
    assert (b.adv_train_eps, b.adv_train_steps, b.adv_train_step_size, b.adv_train_random_start) == (0.1, 7, 0.02, True)
    assert cli.adversarial_from_args(b) == {"eps": 0.1, "steps": 7, "step_size": 0.02, "random_start": True}
    # every other flag parses to what it parses to without them: today's namespace plus the new defaults
    argv = "--batch-size 200 --epochs 3 --synthetic --dtype fp32".split()
    with_flags = vars(cli.parse_args(ddp=ddp, argv=argv + ["--adv-train-eps", "0.3"]))
    without = vars(cli.parse_args(ddp=ddp, argv=argv))
    assert set(with_flags) == set(without)
    assert {k: v for k, v in with_flags.items() if k not in ADV_DEFAULTS} == \
        {k: v for k, v in without.items() if k not in ADV_DEFAULTS}
    assert {k: without[k] for k in ADV_DEFAULTS} == ADV_DEFAULTS


# ---------------------------------------------------------------------------- argument checking
def test_adversarial_config_defaults_and_errors():
    assert adversarial_config(None) is None
    assert adversarial_config({"eps": 0.1}) == {"eps": 0.1, "steps": 1, "step_size": 0.1, "random_start": False}
    c = adversarial_config({"eps": 0.1, "steps": 4, "random_start": True})
    assert c["step_size"] == 2.5 * 0.1 / 4 and c["random_start"] is True       # Predictor.adversarial's rule
    assert adversarial_config({"eps": 0.2, "steps": 3, "step_size": 0.05})["step_size"] == 0.05
    assert adversarial_config({"eps": 0.0})["eps"] == 0.0                       # a zero radius is allowed
    for bad in ({"eps": -0.1}, {"eps": float("nan")}, {"eps": 0.1, "steps": 0}, {"eps": 0.1, "steps": -1},
                {"eps": 0.1, "steps": 1.5}, {"eps": 0.1, "step_size": 0.0}, {"eps": 0.1, "step_size": -0.01},
                {"steps": 2}, {"eps": 0.1, "norm": "l2"}):
        with pytest.raises(ValueError):
            adversarial_config(bad)
    with pytest.raises(ValueError, match="world size 1"):
        adversarial_config({"eps": 0.1}, world_size=2)
    with pytest.raises(ValueError, match="bf16"):
        adversarial_config({"eps": 0.1}, fp32=True)


def test_fused_trainer_checks_its_arguments_before_it_builds_anything():
    # no model state, no data, no GPU: the check comes first
    for kw in (dict(adversarial={"eps": -0.1}), dict(adversarial={"eps": 0.1, "steps": 0}),
               dict(adversarial={"eps": 0.1, "step_size": 0.0}), dict(adversarial={"eps": 0.1}, world_size=2),
               dict(adversarial={"eps": 0.1}, fp32=True)):
        with pytest.raises(ValueError, match="adversarial"):
            FusedTrainer(None, None, None, 64, 64, 128, **kw)


def test_driver_refuses_bad_flags_before_training():
    for extra in (["--adv-train-eps", "-0.1"], ["--adv-train-eps", "0.1", "--adv-train-steps", "0"],
                  ["--adv-train-eps", "0.1", "--adv-train-step-size", "0"]):
        with pytest.raises(ValueError, match="adversarial"):
            driver.run(["--no-cuda", "--synthetic", "--synthetic-size", "64", *extra], ddp_script=False)


# ---------------------------------------------------------------------------- CPU module path
ARGV = ["--no-cuda", "--synthetic", "--synthetic-size", "128", "--synthetic-test-size", "64", "--batch-size", "64",
        "--epochs", "1", "--log-interval", "1", "--save-model"]


def _run_mnist(tmp_path, monkeypatch, capsys, *extra, json_log=None):
    """mnist.py's main flow in-process on the CPU (the dry run's sizes: two steps of 64): (stdout lines, final
    net, global RNG state afterwards, JSON records)."""
    monkeypatch.chdir(tmp_path)
    argv = ARGV + list(extra) + (["--json-log", str(json_log)] if json_log else [])
    assert driver.run(argv, ddp_script=False) == 0
    rng = torch.get_rng_state()
    lines =[ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    net = Net()
    load_state_dict(net, str(tmp_path / "mnist_cnn.pt"), map_location="cpu")
    recs = []
    if json_log:
        with open(json_log) as f:
            recs = [json.loads(ln) for ln in f if ln.strip()]
    return lines, net, rng, recs


def test_cpu_module_path_equals_the_written_out_loop_bitwise(tmp_path, monkeypatch, capsys):
    lines, net, rng_after, _ = _run_mnist(tmp_path, monkeypatch, capsys, "--adv-train-eps", "0.1",
                                          "--adv-train-steps", "2")
    # the same two steps written out: RNG draws in the driver's order (seed, model init, the loader's base seed,
    # then per step dropout1 and dropout2 of the training forward - the attack, in eval mode, draws nothing)
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
        x_adv = plain_pgd(ref, data, target, 0.1, 2)
        assert ref.training and not torch.equal(x_adv, data)
        assert (x_adv - data).abs().max().item() <= 0.1 / MNIST_STD * (1 + 1e-6)
        opt.zero_grad()
        loss = F.nll_loss(ref(x_adv), target)
        loss.backward()
        opt.step()
        want.append(train_line(1, s * 64, 128, s, 2, loss.item()).rstrip("\n"))
    for (n, p), (m, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert n == m and torch.equal(p, q), n
    # the reference's lines, in its format: two train lines (the attacked batches' losses), one test line
    assert lines[:2] == want and len(lines) == 3 and lines[2].startswith("Test set: Average loss: ")
    consume_loader_base_seed()
    ref.eval()
    with torch.no_grad():
        out = ref(normalize_u8(test.images))
    tl = F.nll_loss(out, test.targets, reduction='sum').item() / 64
    assert lines[2] == fmt_test_line(tl, int((out.argmax(1) == test.targets).sum()), 64).strip("\n")
    assert torch.equal(torch.get_rng_state(), rng_after)          # and nothing else was drawn

    # a clean run draws the same numbers in the same order (the attack consumes no RNG) and prints the same kinds
    # of lines; its losses and parameters differ
    clean_lines, clean_net, clean_rng, _ = _run_mnist(tmp_path, monkeypatch, capsys)
    assert torch.equal(clean_rng, rng_after)
    assert [ln.split("Loss:")[0] for ln in clean_lines[:2]] == [ln.split("Loss:")[0] for ln in lines[:2]]
    assert clean_lines[:2] != lines[:2]
    assert not torch.equal(clean_net.fc2.weight, net.fc2.weight)


def test_craft_adversarial_leaves_mode_and_gradients_alone():
    torch.manual_seed(3)
    net = Net()
    imgs, labels = generate(9, seed=5)
    data = normalize_u8(imgs)
    cfg = adversarial_config({"eps": 0.1, "steps": 3})
    for mode in (True, False):
        net.train(mode)
        before = torch.get_rng_state()
        x = driver.craft_adversarial(net, data, labels, cfg)
        assert net.training is mode and all(p.grad is None for p in net.parameters())
        assert torch.equal(torch.get_rng_state(), before)                     # no dropout, no random start: no draw
        assert x.shape == data.shape and not x.requires_grad
        assert torch.equal(x, plain_pgd(net, data, labels, 0.1, 3))
    # random start: drawn with torch from the given generator; inside the ball and the valid range
    rs = adversarial_config({"eps": 0.1, "steps": 1, "step_size": 0.01, "random_start": True})
    xa = driver.craft_adversarial(net, data, labels, rs, generator=torch.Generator().manual_seed(7))
    xb = driver.craft_adversarial(net, data, labels, rs, generator=torch.Generator().manual_seed(7))
    xc = driver.craft_adversarial(net, data, labels, rs, generator=torch.Generator().manual_seed(8))
    assert torch.equal(xa, xb) and not torch.equal(xa, xc)
    eps_n = 0.1 / MNIST_STD
    assert (xa >= data - eps_n).all() and (xa <= data + eps_n).all()
    assert (xa >= PIXEL_LO).all() and (xa <= PIXEL_HI).all()


def test_json_log_keys(tmp_path, monkeypatch, capsys):
    _, _, _, plain = _run_mnist(tmp_path, monkeypatch, capsys, json_log=tmp_path / "plain.jsonl")
    _, _, _, adv = _run_mnist(tmp_path, monkeypatch, capsys, "--adv-train-eps", "0.1", "--adv-train-random-start",
                              json_log=tmp_path / "adv.jsonl")
    new = {"adv_train_eps", "adv_train_steps", "adv_train_step_size", "adv_train_random_start"}
    assert len(plain) == 1 and sorted(plain[0]) == ["correct", "epoch", "test_loss", "train_s"]    # no new keys
    assert len(adv) == 1 and set(adv[0]) == set(plain[0]) | new
    assert (adv[0]["adv_train_eps"], adv[0]["adv_train_steps"], adv[0]["adv_train_step_size"],
            adv[0]["adv_train_random_start"]) == (0.1, 1, 0.1, True)


# ---------------------------------------------------------------------------- adv_init's random start, emulated
def test_random_start_emulation_is_sane():
    imgs, _ = generate(40, seed=11)
    u8 = imgs.reshape(40, 784).numpy()
    n = u8.size
    lo, hi = np.float32(PIXEL_LO), np.float32(PIXEL_HI)
    for eps_px, seed, step in ((0.1, 1, 0), (0.3, 0x1234ABCD5678, 5)):
        eps = np.float32(eps_px / MNIST_STD)
        x0, x, u = adv_init_emulation(u8, seed, step, eps, lo, hi, True)
        assert x0.dtype == x.dtype == u.dtype == np.float32 and x.shape == (40, 784)
        assert (u >= 0).all() and (u < 1).all()
        assert abs(float(u.mean(dtype=np.float64)) - 0.5) < 4 / np.sqrt(n)
        assert (x >= np.maximum(x0 - eps, lo)).all() and (x <= np.minimum(x0 + eps, hi)).all()
        # the lower clamp binds on dark pixels (a negative draw at pixel 0 stays pixel 0); most pixels move
        assert ((x == lo) & (x0 + (2 * u - 1) * eps < lo)).any() and (x != x0).mean() > 0.5
        # another step or seed is another draw; off, the iterate is the clean image
        assert not np.array_equal(adv_init_emulation(u8, seed, step + 1, eps, lo, hi, True)[1], x)
        assert not np.array_equal(adv_init_emulation(u8, seed + 1, step, eps, lo, hi, True)[1], x)
        x0b, xb, _ = adv_init_emulation(u8, seed, step, eps, lo, hi, False)
        assert np.array_equal(xb, x0b) and np.array_equal(x0b, x0)
    # the draw is in a counter domain of its own: not the dropout stream's words under the same seed and step
    import refmodel as R
    from advtrain_ref import ADV_PHILOX_DOMAIN, adv_uniform_words
    w = adv_uniform_words(1, 1, 0)
    assert tuple(int(v) for v in w[0, :4]) == R.philox4x32((0, ADV_PHILOX_DOMAIN, 0, 0), (1, 0))
    assert tuple(int(v) for v in w[0, :4]) != R.philox4x32((0, 0, 0, 0), (1, 0))
