"""L2 Square Attack on the GPU: ``square_l2_step`` / ``square_l2_init`` (csrc/kernels/square.hip) against the float64
emulation of tests/square_l2_ref.py - the record, ``x_best`` and the frozen images bit for bit, ``x_cand`` in the
convention of tests/test_gpu_attack_l2.py (EPS_MARGIN x the deviation of the torch float32 reference on the CPU from
the float64 oracle over the launch, not below FLOOR_ULPS ulps of the largest output); the native loop against its
launches made by hand; ``Predictor.square_attack(norm="l2")`` on the trained net and against the CPU reference; the
``mnist_predict.py --square-norm l2`` line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refmodel
import square_l2_ref as L2
import square_ref as R
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD
from pytorch_mnist_ddp_amd.inference import Predictor, reference_square_attack
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.chain import EvalChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.ops.square import fused_square_attack
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict
from test_gpu_square import (FORMS, ISENTINEL, NAN_BITS, ROOT, _bits, _images, _images_cpu, _nan_rows, _same,
                             _trained)      # the guards, the trained net and the 128 images of the L-inf tests

pytestmark = pytest.mark.gpu

LO, HI = R.LO, R.HI
EPS_MARGIN, FLOOR_ULPS = 8.0, 4.0                           # tests/test_gpu_attack_l2.py
EPS_N = 2.0 / MNIST_STD


def _launch(case, dev, M, side, q, **kw):
    """One ``square_l2_step`` on guard-filled buffers of M + 1 images: ((x_best, x_cand, state) of the M images as
    numpy, whether the guards and the read-only operands are intact)."""
    def rows(key, width=784):
        t = _nan_rows(M + 1, dev, width)
        t[:M] = torch.from_numpy(case[key]).to(dev)
        return t
    x0, x_best, x_cand, logp = rows("x0"), rows("x_best"), rows("x_cand"), rows("logp", 10)
    y = torch.full((M + 1,), ISENTINEL, dtype=torch.int32, device=dev)
    y[:M] = torch.from_numpy(case["y"]).to(dev)
    state = torch.full((M + 1, 4), ISENTINEL, dtype=torch.int32, device=dev)
    if kw.get("first"):                                      # the first launch reads neither: give it the guards
        x_best = _nan_rows(M + 1, dev)
    else:
        state[:M] = torch.from_numpy(case["state"]).to(dev)
    before = (x0.clone(), logp.clone(), y.clone())
    Fk.square_l2_step(logp, y, x0, x_best, x_cand, state, case["eps"], LO, HI, case["seed"], q, side,
                      id_base=int(case["ids"][0]), targeted=case["targeted"], M=M, **kw)
    ok = all(bool((_bits(t[M:]) == NAN_BITS).all()) for t in (x_best, x_cand)) and bool((state[M] == ISENTINEL).all())
    ok = ok and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (x0, logp, y)))
    return tuple(t[:M].cpu().numpy() for t in (x_best, x_cand, state)), ok


def _reference(case, side, q, **kw):
    t = {k: torch.from_numpy(v) for k, v in case.items() if isinstance(v, np.ndarray) and k != "ids"}
    return Fk.square_l2_step_reference(t["logp"], t["y"], t["x0"], None if kw.get("first") else t["x_best"],
                                       t["x_cand"], None if kw.get("first") else t["state"], case["eps"], LO, HI,
                                       case["seed"], q, side, case["ids"], targeted=case["targeted"], **kw)[1].numpy()


def _check_cand(got, ref32, want, what):
    """``got`` against the float64 ``want``: NaN where it is NaN, else within the module's tolerance."""
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(np.isnan(ref32), ~ok), what
    if not ok.any():
        return 0.0
    dev32 = float(np.abs(ref32[ok] - want[ok]).max())
    tol = max(EPS_MARGIN * dev32, FLOOR_ULPS * 2.0 ** (int(np.frexp(np.abs(want[ok]).max())[1]) - 24))
    dev = float(np.abs(got[ok] - want[ok]).max())
    print(f"\n{what}: dev {dev:.3e}  torch fp32 {dev32:.3e}  tolerance {tol:.3e}", end="")
    assert dev <= tol, (what, dev, tol)
    return dev


def _check_step(case, dev, M, side, q, **kw):
    got, intact = _launch(case, dev, M, side, q, **kw)
    what = f"M {M} side {side} q {q} {kw} targeted {case['targeted']}"
    assert intact, what                                      # the guard image and record, the read-only operands
    want = L2.step_oracle(case, side=side, q=q, **kw)
    assert R.mismatches((got[0], got[0], got[2]), (want[0], want[0], want[2])) == [], what
    worst = _check_cand(got[1], _reference(case, side, q, **kw), want[1], what)
    if not kw.get("first"):                                  # frozen images: x_best, x_cand and the record untouched
        frozen = case["state"][:, 2] != 0
        for out, was in zip(got, (case["x_best"], case["x_cand"], case["state"])):
            assert np.array_equal(out[frozen].view(np.int32), was[frozen].view(np.int32)), what
    if kw.get("last"):
        assert np.array_equal(got[1].view(np.int32), case["x_cand"].view(np.int32)), what
    return got, worst


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("M", [1, 3, 33])
def test_square_l2_step_kernel_against_the_emulation(cuda_device, M, targeted):
    """Measured on the MI355X: the worst deviation of x_cand from the float64 oracle was 5.2e-7 (M 33, side 3,
    targeted, first) against a tolerance of 2.6e-6 there; the torch float32 reference's own worst was 1.0e-6."""
    n, worst = 0, 0.0
    for side in (3, 5, 13, 25):
        for kw in FORMS:
            n += 1
            case = L2.make_case(M, seed=10 * M + n, targeted=targeted)
            q = 1 + 97 * n
            got, dev = _check_step(case, cuda_device, M, side, q, **kw)
            worst = max(worst, dev)
            with torch.cuda.stream(torch.cuda.Stream(cuda_device)):     # another stream: the same bits
                again, intact = _launch(case, cuda_device, M, side, q, **kw)
                torch.cuda.current_stream().synchronize()
            assert intact and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))
    case = L2.make_case(M, seed=77, targeted=targeted)       # the top of the counter words: nothing wraps
    case["ids"] = np.arange(M, dtype=np.int64) + (2 ** 32 - M)
    _check_step(case, cuda_device, M, 5, 2 ** 32 - 1)
    case = L2.make_case(M, seed=78, targeted=targeted, eps=0.0)        # eps = 0: the candidate is x_best, bit for bit
    got, intact = _launch(case, cuda_device, M, 3, 9)
    live = (case["state"][:, 2] == 0) & ~np.isnan(case["x0"]).any(1)
    assert intact and np.array_equal(got[1][live].view(np.int32), got[0][live].view(np.int32))
    assert np.array_equal(got[0][live].view(np.int32), case["x0"][live].view(np.int32))
    print(f"\nworst x_cand deviation, M {M}: {worst:.3e}")


@pytest.mark.parametrize("M", [1, 3, 33])
def test_square_l2_init_kernel_against_the_emulation(cuda_device, M):
    dev = cuda_device
    for n, eps in enumerate((L2.EPS, 0.5 / MNIST_STD, 0.0)):
        case = L2.make_case(M, seed=5 * M + n, eps=eps)
        x0 = _nan_rows(M + 1, dev)
        x0[:M] = torch.from_numpy(case["x0"]).to(dev)
        out, keep, base = _nan_rows(M + 1, dev), x0.clone(), int(case["ids"][0])
        Fk.square_l2_init(x0, eps, LO, HI, case["seed"], base, out=out, M=M)
        assert bool((_bits(out[M:]) == NAN_BITS).all()) and torch.equal(_bits(x0), _bits(keep))
        got = out[:M].cpu().numpy()
        ref = Fk.square_l2_init_reference(x0[:M].cpu(), eps, LO, HI, case["seed"], id_base=base).numpy()
        _check_cand(got, ref, L2.init_oracle(case["x0"], eps, case["seed"], case["ids"]), f"init M {M} eps {eps:g}")
        assert not R.init_mismatch(got, ref)                 # no sum: the package's reference bit for bit
        with torch.cuda.stream(torch.cuda.Stream(dev)):
            again = Fk.square_l2_init(x0, eps, LO, HI, case["seed"], base, M=M)
            torch.cuda.current_stream().synchronize()
        assert not R.init_mismatch(again.cpu().numpy(), got)
        if eps == 0.0:
            ok = ~np.isnan(case["x0"])
            assert np.array_equal(got[ok], case["x0"][ok])


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    M = 4
    case = L2.make_case(M, seed=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items() if isinstance(v, np.ndarray) and k != "ids"}
    t["state"][:, 2] = 0                                     # every image live: a launch would store
    keep = {k: v.clone() for k, v in t.items()}
    C, p, s = native.load(), native.ptr, native.stream_handle()
    tab = p(Fk.square_l2_tables(dev))
    ok = dict(logp=p(t["logp"]), y=p(t["y"]), x0=p(t["x0"]), x_best=p(t["x_best"]), x_cand=p(t["x_cand"]),
              state=p(t["state"]), table=tab, eps=0.1, lo=LO, hi=HI, seed=1, q=1, id_base=0, side=3, first=False,
              last=False, targeted=False, M=M, stream=s)
    for kw in (dict(side=4), dict(side=1), dict(side=29), dict(table=0), dict(table=tab + 2), dict(x_cand=0),
               dict(state=0), dict(logp=0), dict(x_cand=ok["x_cand"] + 4), dict(state=ok["state"] + 4),
               dict(x_best=ok["x_best"] + 8), dict(side=0), dict(q=1 << 32), dict(id_base=1 << 32),
               dict(id_base=(1 << 32) - M + 1), dict(M=0), dict(M=(1 << 20) + 1), dict(eps=-0.1)):
        with pytest.raises(RuntimeError):
            C.square_l2_step(**dict(ok, **kw))
    oki = dict(x0=ok["x0"], x_cand=ok["x_cand"], table=tab, eps=0.1, lo=LO, hi=HI, seed=1, id_base=0, M=M, stream=s)
    for kw in (dict(table=0), dict(table=tab + 2), dict(x_cand=0), dict(x0=0), dict(x_cand=ok["x_cand"] + 4),
               dict(id_base=1 << 32), dict(id_base=(1 << 32) - M + 1), dict(M=0), dict(M=(1 << 20) + 1),
               dict(eps=-0.1)):
        with pytest.raises(RuntimeError):
            C.square_l2_init(**dict(oki, **kw))
    args = (t["logp"], t["y"], t["x0"], t["x_best"], t["x_cand"], t["state"])
    for bad in (dict(eps=-1.0), dict(side=4), dict(side=1), dict(side=29), dict(q=1 << 32), dict(M=5),
                dict(id_base=(1 << 32) - 1), dict(lo=1.0, hi=0.0), dict(tables=t["x0"][0])):
        with pytest.raises(ValueError):
            Fk.square_l2_step(*args, **dict(dict(eps=0.1, lo=LO, hi=HI), **bad))
    with pytest.raises(ValueError):
        Fk.square_l2_init(t["x0"], 0.1, LO, HI, out=t["x0"])
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t[k]), _bits(v)) for k, v in keep.items())     # nothing ran


def _by_hand(net, x0, y, queries, seed, ids):
    """The launches of ``fused_square_attack(norm="l2")``, one by one through the checked entry points."""
    dev, M = x0.device, x0.shape[0]
    st = fused_state(net)
    st.sync()
    buf = Fk.EvalBuffers.allocate(M, dev)
    chain = EvalChain(st.ms, buf)
    lab = y.to(torch.int32)
    x_best = _nan_rows(M, dev)
    state = torch.full((M, 4), ISENTINEL, dtype=torch.int32, device=dev)
    sides = Fk.square_sides_l2(0.8, queries)
    x_cand = Fk.square_l2_init(x0, EPS_N, LO, HI, seed, ids[0])
    for j in range(queries):
        last = j == queries - 1
        chain.run(M, xin=native.ptr(x_cand))
        Fk.square_l2_step(buf.logp, lab, x0, x_best, x_cand, state, EPS_N, LO, HI, seed, j + 1,
                          3 if last else sides[j], id_base=ids[0], first=j == 0, last=last)
    return x_best, Fk.square_state_margin(state), state[:, Fk.SQUARE_QUERIES].clone()


def test_fused_loop_equals_its_launches_by_hand(cuda_device):
    dev = cuda_device
    net = _trained(dev)
    x0, y = _images(dev, 5)
    ids = list(range(40, 45))
    want = _by_hand(net, x0, y, 12, 3, ids)
    for check_every in (0, 1, 5):
        got = fused_square_attack(net, x0, y, EPS_N, 12, LO, HI, seed=3, ids=ids, check_every=check_every, norm="l2")
        assert _same(got, want), check_every
    for chunk in (1, 2, 5):
        parts = [fused_square_attack(net, x0[i:i + chunk], y[i:i + chunk], EPS_N, 12, LO, HI, seed=3,
                                     ids=ids[i:i + chunk], norm="l2") for i in range(0, 5, chunk)]
        assert _same([torch.cat([q[k] for q in parts]) for k in range(3)], want), chunk
    assert not torch.equal(want[0], x0) and int(want[2].min()) >= 1 and int(want[2].max()) <= 12


def test_predictor_square_attack_l2_on_the_gpu(cuda_device):
    dev = cuda_device
    pr = Predictor(_trained(dev))
    assert pr.native
    x0, y = _images(dev)
    x_adv, lp, margin, used = pr.square_attack(x0.view(128, 1, 28, 28), y, eps=2.0, queries=32, norm="l2")
    xa = x_adv.reshape(128, 784)
    assert (xa >= LO).all() and (xa <= HI).all()
    norms = (xa.double() - x0.double()).square().sum(1).sqrt()
    assert float(norms.max()) <= L2.ball_slack(EPS_N) and float(norms.max()) > 0.5 * EPS_N
    assert torch.equal(_bits(Fk.square_margin_reference(lp, y)), _bits(margin))
    assert torch.equal(lp.argmax(1) != y, margin < 0)
    assert used.dtype == torch.int32 and int(used.min()) >= 1 and int(used.max()) <= 32
    assert (margin[used < 32] < 0).all()
    with pytest.raises(ValueError):
        pr.square_attack(x0.view(128, 1, 28, 28), y, eps=2.0, queries=4, norm="l0")


SEEDS = (0, 1, 2)
SUCCESS_EPS, SUCCESS_QUERIES = 3.0, 32     # chosen on the CPU: at 2.0 / 32 the reference broke only 5, 6 and 7 images


def test_success_rate_against_the_cpu_reference(cuda_device):
    """128 synthetic test images of the trained net, L2 eps 3.0, 32 queries, seeds 0, 1, 2.  The images still correct
    after the attack, CPU reference (100 correct on the clean input): 88, 85, 86 where the parameters were chosen -
    13, 16 and 14 clean-correct images broken - and 88, 84, 83 on the CPU of the MI355X host (torch's CPU forward
    differs by a few ulps between hosts), so there a = 83, b = 88, d = 5 and the GPU counts must lie in [78, 93].
    MI355X (101 correct on the clean input): 88, 84, 83 - that host's CPU counts, seed by seed."""
    dev = cuda_device
    net = refmodel.trained_net()
    x0c, yc = _images_cpu()
    ref = []
    for seed in SEEDS:
        x_adv = reference_square_attack(net, x0c, yc, SUCCESS_EPS / MNIST_STD, SUCCESS_QUERIES, LO, HI, seed=seed,
                                        norm="l2")[0]
        with torch.no_grad():
            ref.append(int((net.forward_reference(x_adv.view(128, 1, 28, 28)).argmax(1) == yc).sum()))
    pr = Predictor(_trained(dev))
    x0, y = _images(dev)
    a, b = min(ref), max(ref)
    d = max(b - a, 2)
    got = []
    for seed in SEEDS:
        lp = pr.square_attack(x0.view(128, 1, 28, 28), y, eps=SUCCESS_EPS, queries=SUCCESS_QUERIES, seed=seed,
                              norm="l2")[1]
        got.append(int((lp.argmax(1) == y).sum()))
    clean = int((pr.predict(x0.view(128, 1, 28, 28)) == y).sum())
    print(f"\nL2 square attack, correct of 128 after the attack: CPU reference {ref}, GPU {got}, clean {clean}")
    assert all(a - d <= c <= b + d for c in got), (ref, got)
    assert max(got) < clean


def test_predict_cli_square_l2_on_gpu(cuda_device, tmp_path):
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(refmodel.trained_net(), ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "200", "--checkpoint", ckpt, "--json-log", log, "--square-eps", "2.0", "--square-norm", "l2",
                        "--square-queries", "20"],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    with open(log) as f:
        rec = json.loads(f.read())
    assert len(lines) == 2 and lines[1].startswith("Square set (L2 eps=2, queries=20, p_init=0.8): Average loss: ")
    assert rec["device"].startswith("cuda") and rec["square_correct"] <= rec["correct"]
    assert f"Accuracy: {rec['square_correct']}/200 ({100.0 * rec['square_correct'] / 200:.0f}%), median queries: " in lines[1]
    assert (rec["square_eps"], rec["square_norm"], rec["square_queries"]) == (2.0, "l2", 20)
