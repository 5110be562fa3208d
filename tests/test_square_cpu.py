"""Square Attack on the CPU: the side schedule, the numpy Philox, the package's torch references against the
per-image emulation of tests/square_ref.py (bit for bit), the emulation's deliberate mistakes, ``reference_square_attack``
on the trained net, ``Predictor.square_attack``'s refusals and the ``mnist_predict.py --square-eps`` line."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refmodel
import square_ref as R
from pytorch_mnist_ddp_amd import _build
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, build_predict_parser, reference_square_attack, square_line
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.philox import philox4x32
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict
from pytorch_mnist_ddp_amd.utils.logging import test_line as _test_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = R.LO, R.HI
SIDES = (25, 18, 13, 9, 6, 4, 3, 2, 2, 1)
TOPS = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)


def _band(it: int) -> int:
    return next((k for k, top in enumerate(TOPS) if it <= top), 9)


@pytest.mark.parametrize("queries", [10000, 100])
def test_side_schedule(queries):
    sides = Fk.square_sides(0.8, queries)
    assert len(sides) == queries - 1
    seen = set()
    for q in range(1, queries):
        band = _band(int(q / queries * 10000))
        seen.add(band)
        assert sides[q - 1] == SIDES[band], (q, band)
    # every range of the table is reached; rescaled to 100 queries, query 1 is already at it = 100: the third range
    assert seen == (set(range(10)) if queries == 10000 else set(range(2, 10)))
    assert sides[0] == (25 if queries == 10000 else 13) and sides[-1] == 1
    if queries == 10000:                                     # the borders of the table themselves
        for it, band in ((10, 0), (11, 1), (50, 1), (51, 2), (8000, 8), (8001, 9), (9999, 9)):
            assert sides[it - 1] == SIDES[band]


def test_sides_stay_in_range():
    for p in (0.05, 0.8, 1.0):
        for queries in (1, 2, 7, 100, 5000):
            sides = Fk.square_sides(p, queries)
            assert len(sides) == queries - 1 and all(1 <= s <= 27 for s in sides)
            assert list(sides) == sorted(sides, reverse=True)
    assert Fk.square_sides(1.0, 10000)[0] == 27              # sqrt(784) = 28 is capped: a window never fills the image
    for bad in (dict(p_init=0.0, queries=5), dict(p_init=1.5, queries=5), dict(p_init=0.5, queries=0)):
        with pytest.raises(ValueError):
            Fk.square_sides(**bad)


def test_numpy_philox_equals_the_reference_model():
    g = np.random.default_rng(3)
    ctr = g.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    ctr[0], ctr[1] = 0, 2 ** 32 - 1
    for seed in (0, 1, 0xDEADBEEF12345678, 2 ** 64 - 1):
        got = philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
        assert got.dtype == np.uint32 and got.shape == (64, 4)
        for r in range(64):
            want = refmodel.philox4x32(tuple(int(v) for v in ctr[r]), (seed & 0xFFFFFFFF, seed >> 32))
            assert tuple(int(v) for v in got[r]) == want
    assert philox4x32(5, R.DOMAIN, np.arange(3)[:, None], np.arange(7)[None, :], 9).shape == (3, 7, 4)
    assert Fk.SQUARE_PHILOX_DOMAIN == R.DOMAIN == int.from_bytes(b"SQR1", "big")
    assert Fk.SQUARE_PHILOX_DOMAIN not in (0, Fk.SMOOTH_PHILOX_DOMAIN, 0x41445631)


def _t(case, key):
    return torch.from_numpy(case[key])


def reference_step(case, dev="cpu", **kw):
    """``functional.square_step_reference`` on ``case``: (x_best, x_cand, state) as numpy."""
    first = kw.get("first", False)
    out = Fk.square_step_reference(_t(case, "logp").to(dev), _t(case, "y").to(dev), _t(case, "x0").to(dev),
                                   None if first else _t(case, "x_best").to(dev), _t(case, "x_cand").to(dev),
                                   None if first else _t(case, "state").to(dev), case["eps"], LO, HI, case["seed"],
                                   ids=case["ids"], targeted=case["targeted"], **kw)
    return tuple(t.cpu().numpy() for t in out)


FORMS = [dict(first=True), dict(), dict(last=True), dict(first=True, last=True)]


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("M", [1, 3, 33])
def test_package_references_equal_the_emulation(M, targeted):
    n = 0
    for side in (1, 2, 13, 27):
        for kw in FORMS:
            n += 1
            case = R.make_case(M, seed=10 * M + n, targeted=targeted)
            q = 1 + 97 * n
            want = R.step_oracle(case, side=side, q=q, **kw)
            assert R.mismatches(reference_step(case, side=side, q=q, **kw), want) == [], (side, kw)
            if not kw.get("first"):                          # frozen images: nothing of them moved
                frozen = case["state"][:, 2] != 0
                assert frozen.any() or M == 1
                for got, was in zip(want, (case["x_best"], case["x_cand"], case["state"])):
                    assert np.array_equal(got[frozen].view(np.int32), was[frozen].view(np.int32))
            if kw.get("last"):
                assert np.array_equal(want[1].view(np.int32), case["x_cand"].view(np.int32))
    case = R.make_case(M, seed=M)
    init = Fk.square_init_reference(_t(case, "x0"), case["eps"], LO, HI, case["seed"], case["ids"]).numpy()
    assert not R.init_mismatch(init, R.init_oracle(case["x0"], case["eps"], case["seed"], case["ids"]))
    base = int(case["ids"][0])                               # id_base + i is the same thing
    again = Fk.square_init_reference(_t(case, "x0"), case["eps"], LO, HI, case["seed"], id_base=base).numpy()
    assert not R.init_mismatch(again, init)
    x = case["x0"].reshape(M, 28, 28)                        # vertical stripes: a column has one sign
    with np.errstate(invalid="ignore"):
        sign = np.where((x > LO + 1.0) & (x < HI - 1.0), np.sign(init.reshape(M, 28, 28) - x), 0)   # (clamp inactive)
    for i in range(M):
        assert all(len(set(sign[i, :, c][sign[i, :, c] != 0])) <= 1 for c in range(28))
        assert len(set(sign[i][sign[i] != 0])) == 2


def test_hand_case_forces_every_branch():
    case = R.make_case(33, seed=2)
    xb, xc, st = R.step_oracle(case, side=5, q=3)
    was = case["state"]
    frozen = was[:, 2] != 0
    margin, old = st[:, 0].copy().view(np.float32), was[:, 0].copy().view(np.float32)
    accepted = ~frozen & (margin != old) & ~np.isnan(margin)
    L = np.array([R.margin(case["logp"][i], int(case["y"][i]), False) for i in range(33)])
    assert frozen.any() and (~frozen).any() and accepted.any()
    assert (~frozen & ~accepted & (L == old)).any()          # an exact tie that is not accepted
    assert np.isnan(L[~frozen]).any() and np.isnan(old[~frozen]).any()
    became = ~frozen & (st[:, 2] == 1)
    assert became.any() and (~frozen & (st[:, 2] == 0)).any()
    assert all(np.array_equal(xc[i], xb[i]) for i in np.nonzero(became)[0])         # x_cand = x_best, once
    assert (st[~frozen, 1] == was[~frozen, 1] + 1).all() and (st[frozen] == was[frozen]).all()
    assert (st[:, 3] == was[:, 3]).all()


@pytest.mark.parametrize("mut", R.STEP_MUTATIONS)
def test_every_step_mutation_is_caught(mut):
    caught = []
    for n, side in enumerate((1, 2, 13, 27)):
        case = R.make_case(33, seed=40 + n)
        want = R.step_oracle(case, side=side, q=5 + n)
        assert R.mismatches(R.step_oracle(case, side=side, q=5 + n), want) == []
        caught += R.mismatches(R.step_oracle(case, side=side, q=5 + n, mut=mut), want)
    assert caught, mut


@pytest.mark.parametrize("mut", R.INIT_MUTATIONS)
def test_every_init_mutation_is_caught(mut):
    case = R.make_case(3, seed=9)
    want = R.init_oracle(case["x0"], case["eps"], case["seed"], case["ids"])
    assert not R.init_mismatch(R.init_oracle(case["x0"], case["eps"], case["seed"], case["ids"]), want)
    assert R.init_mismatch(R.init_oracle(case["x0"], case["eps"], case["seed"], case["ids"], mut=mut), want)


def test_all_ten_mutations_are_listed():
    assert len(R.MUTATIONS) == 10 and set(R.MUTATIONS) == set(R.INIT_MUTATIONS) | set(R.STEP_MUTATIONS)


@functools.lru_cache(maxsize=None)
def _case64():
    net = refmodel.trained_net()
    imgs, labels = generate(64, seed=5)
    return net, normalize_u8(imgs).reshape(64, 784).contiguous(), labels.long()


@functools.lru_cache(maxsize=None)
def _attack64(check_every=64, seed=0):
    net, x0, y = _case64()
    return reference_square_attack(net, x0, y, 0.3 / MNIST_STD, 32, LO, HI, seed=seed, check_every=check_every)


def _margin_of(lp, y):
    return Fk.square_margin_reference(lp, y)


def test_reference_square_attack_on_the_trained_net():
    """64 synthetic test images of the trained net, eps 0.3, 32 queries, seed 0: CLEAN_CORRECT of 64 are correct on
    the clean input and ADV_CORRECT after the attack (the counts measured on the CPU are in the asserts below)."""
    net, x0, y = _case64()
    eps = 0.3 / MNIST_STD
    x_adv, margin, used = _attack64()
    up, down = R.vertex(x0.numpy(), True, eps), R.vertex(x0.numpy(), False, eps)
    got = x_adv.numpy().view(np.int32)
    assert ((got == up.view(np.int32)) | (got == down.view(np.int32))).all()      # a vertex of the box, bitwise
    with torch.no_grad():
        lp = net.forward_reference(x_adv.view(64, 1, 28, 28))
        clean = int((net.forward_reference(x0.view(64, 1, 28, 28)).argmax(1) == y).sum())
    assert torch.equal(_margin_of(lp, y).view(torch.int32), margin.view(torch.int32))
    assert used.dtype == torch.int32 and int(used.min()) >= 1 and int(used.max()) <= 32
    frozen = used < 32
    assert frozen.any() and (margin[frozen] < 0).all()
    correct = int((lp.argmax(1) == y).sum())
    print(f"\nsquare attack on the CPU: clean {clean}/64, after the attack {correct}/64, broken {int((margin < 0).sum())}")
    assert (clean, correct) == (CLEAN_CORRECT, ADV_CORRECT)
    assert correct < clean
    assert net.training is False


CLEAN_CORRECT, ADV_CORRECT = 51, 23                          # measured: see the test above


def test_reference_square_attack_is_the_same_under_batchings_and_check_every():
    """The draws depend on (seed, id, query) alone, so a batching changes a result only through the forward.  torch's
    CPU matrix product picks its kernel by the row count: in batches that are multiples of 16 a row's log-probabilities
    are the same bits, and the whole result is compared bit for bit there.  With cuts of 1 or 8 rows (1, 31, 32 and
    24, 8, 32 were tried) x_best and queries_used were still the same, and one image's margin moved by one ulp: that
    bit is torch's, so for an odd cut only the draws - the stripe start - are compared."""
    net, x0, y = _case64()
    eps = 0.3 / MNIST_STD
    whole = _attack64()
    start = Fk.square_init_reference(x0, eps, LO, HI, 0)
    for at, c in ((0, 1), (1, 31), (32, 8), (40, 24)):
        part = Fk.square_init_reference(x0[at:at + c], eps, LO, HI, 0, ids=range(at, at + c))
        assert torch.equal(part.view(torch.int32), start[at:at + c].view(torch.int32))
    for cuts in ((16, 48), (32, 32)):
        parts, at = [], 0
        for c in cuts:
            parts.append(reference_square_attack(net, x0[at:at + c], y[at:at + c], eps, 32, LO, HI,
                                                 ids=range(at, at + c)))
            at += c
        for k in range(3):
            assert torch.equal(torch.cat([p[k] for p in parts]).view(torch.int32), whole[k].view(torch.int32)), (cuts, k)
    for check_every in (0, 1, 7):
        again = _attack64(check_every)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, whole)), check_every
    shifted = reference_square_attack(net, x0, y, eps, 32, LO, HI, ids=range(100, 164))
    assert not torch.equal(shifted[0], whole[0])             # the id is part of the draw
    assert not torch.equal(_attack64(seed=1)[0], whole[0])   # and so is the seed


def test_targeted_reference_reaches_targets():
    net, x0, y = _case64()
    tgt = (y + 1) % 10
    x_adv, margin, used = reference_square_attack(net, x0, tgt, 0.3 / MNIST_STD, 32, LO, HI, targeted=True)
    with torch.no_grad():
        lp = net.forward_reference(x_adv.view(64, 1, 28, 28))
    assert torch.equal(Fk.square_margin_reference(lp, tgt, True).view(torch.int32), margin.view(torch.int32))
    reached = lp.argmax(1) == tgt
    assert ((margin < 0) <= reached).all()                   # a negative targeted margin: the target is the arg-max


def test_predictor_square_attack_on_the_cpu_and_its_refusals():
    net, x0, y = _case64()
    imgs, _ = generate(64, seed=5)
    pr = Predictor(net)
    x_adv, lp, margin, used = pr.square_attack(imgs, y, eps=0.3, queries=32)
    whole = _attack64()
    assert x_adv.shape == (64, 1, 28, 28) and lp.shape == (64, 10) and margin.shape == used.shape == (64,)
    assert torch.equal(x_adv.reshape(64, 784), whole[0]) and torch.equal(used, whole[2])
    assert torch.equal(lp, pr.log_probs(x_adv))
    own = pr.square_attack(imgs[:8], None, eps=0.3, queries=4)               # labels: the clean prediction
    same = pr.square_attack(imgs[:8], pr.predict(imgs[:8]), eps=0.3, queries=4)
    assert all(torch.equal(a, b) for a, b in zip(own, same))
    one = pr.square_attack(imgs[:8], y[:8], eps=0.3, queries=1)              # one query: the stripe start itself
    assert torch.equal(one[0].reshape(8, 784), Fk.square_init_reference(x0[:8], 0.3 / MNIST_STD, LO, HI))
    assert one[3].tolist() == [1] * 8
    zero = pr.square_attack(imgs[:8], y[:8], eps=0.0, queries=3)
    assert torch.equal(zero[0].reshape(8, 784), x0[:8])
    for bad in (dict(eps=-0.1), dict(eps=float("nan")), dict(queries=0), dict(queries=2.5), dict(queries=True),
                dict(p_init=0.0), dict(p_init=1.01), dict(check_every=-1), dict(ids=[1, 2, 3]),
                dict(labels=None, targeted=True), dict(labels=torch.full((8,), 10))):
        kw = dict(labels=y[:8], eps=0.3, queries=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            pr.square_attack(imgs[:8], **kw)


def test_robust_evaluate_square_cpu():
    net, _, y = _case64()
    imgs, labels = generate(64, seed=5)
    pr = Predictor(net)
    one = pr.robust_evaluate_square(imgs, labels, 0.3, queries=32, batch_size=64)
    parts = pr.robust_evaluate_square(imgs.reshape(64, 784), labels, 0.3, queries=32, batch_size=24)
    assert one[1:] == parts[1:] and one[2] == 64 and one[0] == pytest.approx(parts[0], rel=1e-5)
    _, lp, _, used = pr.square_attack(imgs, labels, eps=0.3, queries=32)
    assert one[0] == pytest.approx(F.nll_loss(lp, y, reduction='sum').item(), rel=1e-5)
    assert one[1] == int((lp.argmax(1) == y).sum())
    clean = pr.predict(imgs) == y
    broken = clean & (lp.argmax(1) != y)
    assert one[3] == float(used[broken].double().quantile(0.5))
    none = pr.robust_evaluate_square(imgs[:4], labels[:4], 0.0, queries=2)
    assert none[3] is None and none[1] == int(clean[:4].sum())
    for kw in (dict(batch_size=0), dict(queries=0), dict(p_init=2.0)):
        with pytest.raises(ValueError):
            pr.robust_evaluate_square(imgs, labels, 0.3, **dict(dict(queries=2), **kw))


def test_native_extension_has_the_square_kernels():
    _build.build()
    C = native.load(build_if_missing=False)
    assert C.SQUARE_PHILOX_DOMAIN == Fk.SQUARE_PHILOX_DOMAIN
    ok = dict(logp=16, y=16, x0=16, x_best=16, x_cand=32, state=16, eps=0.1, lo=0.0, hi=1.0, seed=1, q=1, id_base=0,
              side=3, first=False, last=False, targeted=False, M=4, stream=0)
    # the launcher's own checks come before any launch
    bad = [dict(M=0), dict(M=-1), dict(M=(1 << 20) + 1), dict(eps=-0.1), dict(eps=float("nan")), dict(side=0),
           dict(side=28), dict(x_cand=20), dict(state=24), dict(logp=18), dict(y=18), dict(q=1 << 32), dict(q=-1),
           dict(id_base=1 << 32), dict(id_base=(1 << 32) - 3)] + [{k: 0} for k in list(ok)[:6]]
    for kw in bad:
        with pytest.raises(RuntimeError):
            C.square_step(**dict(ok, **kw))
    ok = dict(x0=16, x_cand=32, eps=0.1, lo=0.0, hi=1.0, seed=1, id_base=0, M=4, stream=0)
    for kw in (dict(M=0), dict(M=(1 << 20) + 1), dict(eps=-0.1), dict(x0=0), dict(x_cand=0), dict(x0=8),
               dict(id_base=-1), dict(id_base=(1 << 32) - 3)):
        with pytest.raises(RuntimeError):
            C.square_init(**dict(ok, **kw))
    z = torch.zeros(2, 784)
    with pytest.raises(ValueError):                          # the functional wrappers want GPU tensors
        Fk.square_init(z, 0.1, 0.0, 1.0)
    with pytest.raises(ValueError):
        Fk.square_step(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int32), z, z.clone(), z.clone(),
                       torch.zeros(2, 4, dtype=torch.int32), 0.1, 0.0, 1.0)


def test_predict_parser_and_line():
    ap = build_predict_parser()
    d = ap.parse_args([])
    assert (d.square_eps, d.square_queries, d.square_p_init, d.square_seed) == (None, 1000, 0.8, 0)
    d = ap.parse_args(["--square-eps", "0.3", "--square-queries", "50", "--square-p-init", "0.1", "--square-seed", "4"])
    assert (d.square_eps, d.square_queries, d.square_p_init, d.square_seed) == (0.3, 50, 0.1, 4)
    assert d.attack_eps is None and d.apgd_eps is None       # independent of the gradient attacks' flags
    assert square_line(0.3, 1000, 0.8, 0.12344, 9876, 10000, 17.5) == \
        "Square set (Linf eps=0.3, queries=1000, p_init=0.8): Average loss: 0.1234, Accuracy: 9876/10000 (99%), " \
        "median queries: 17.5"
    assert square_line(0.1, 5, 0.05, 1.0, 3, 4, None).endswith("Accuracy: 3/4 (75%), median queries: n/a")


def test_predict_cli_square_line_on_cpu(tmp_path):
    torch.manual_seed(5)
    net = Net()
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(net, ckpt)
    log = str(tmp_path / "log.jsonl")
    base = [sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--no-cuda", "--synthetic", "--synthetic-test-size",
            "40", "--checkpoint", ckpt, "--batch-size", "24", "--json-log", log]
    run = lambda extra: subprocess.run(base + extra, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT),     # noqa: E731
                                       capture_output=True, text=True, timeout=240)
    plain, with_sq = run([]), run(["--square-eps", "0.3", "--square-queries", "6", "--square-seed", "2"])
    assert plain.returncode == 0 and with_sq.returncode == 0, with_sq.stderr[-2000:]
    with open(log) as f:
        rec0, rec = (json.loads(ln) for ln in f.read().splitlines())
    lines0, lines = ([ln for ln in r.stdout.splitlines() if ln.strip()] for r in (plain, with_sq))
    data = load_mnist(train=False, synthetic_data=True, synthetic_size=40, verbose=False)
    pr = Predictor(net)
    clean = pr.evaluate(data.images, data.targets, 24)
    # without the flag: the one line and the six keys the tool has always written
    assert lines0 == [_test_line(clean[0] / 40, clean[1], 40).strip()]
    assert set(rec0) == {"checkpoint", "device", "source", "test_loss", "correct", "n"}
    loss, correct, n, median = pr.robust_evaluate_square(data.images, data.targets, 0.3, 6, 24, 0.8, 2)
    assert lines[:-1] == lines0
    assert lines[-1] == square_line(0.3, 6, 0.8, loss / n, correct, n, median)
    new = {"square_eps": 0.3, "square_queries": 6, "square_p_init": 0.8, "square_seed": 2, "square_correct": correct,
           "square_median_queries": median}
    assert {k: rec[k] for k in new} == new and rec["square_loss"] == pytest.approx(loss / n, rel=1e-6)
    assert {k: v for k, v in rec.items() if not k.startswith("square_")} == rec0
