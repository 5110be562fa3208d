"""Square Attack on the GPU: the kernels (csrc/kernels/square.hip) against the per-image emulation of
tests/square_ref.py, bit for bit (there is no reordering to allow for: every operation is an integer operation, a
select, one add and one clamp); the native loop ``ops.square.fused_square_attack`` against its launches made by hand,
under ``check_every`` and under chunkings; ``Predictor.square_attack`` on the trained net and against the CPU
reference; the ``mnist_predict.py --square-eps`` line."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refmodel
import square_ref as R
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, reference_square_attack
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.chain import EvalChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.ops.square import fused_square_attack
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = R.LO, R.HI
NAN_BITS, ISENTINEL = 0x7FC00123, -77                        # the guards: a NaN of a payload nothing computes
FORMS = [dict(first=True), dict(), dict(last=True)]
EPS_N = 0.3 / MNIST_STD


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan_rows(n, dev, width=784):
    return torch.full((n, width), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _guard_ok(t, M):
    return bool((_bits(t[M:]) == NAN_BITS).all())


def _launch(case, dev, M, side, q, **kw):
    """One ``square_step`` on guard-filled buffers of M + 1 images: (x_best, x_cand, state of the M images as numpy,
    guards and read-only operands intact)."""
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
    Fk.square_step(logp, y, x0, x_best, x_cand, state, case["eps"], LO, HI, case["seed"], q, side,
                   id_base=int(case["ids"][0]), targeted=case["targeted"], M=M, **kw)
    ok = _guard_ok(x_best, M) and _guard_ok(x_cand, M) and bool((state[M] == ISENTINEL).all())
    ok = ok and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (x0, logp, y)))
    return tuple(t[:M].cpu().numpy() for t in (x_best, x_cand, state)), ok


@pytest.mark.parametrize("targeted", [False, True])
@pytest.mark.parametrize("M", [1, 3, 33])
def test_square_step_kernel_against_the_emulation(cuda_device, M, targeted):
    n = 0
    for side in (1, 2, 13, 27):
        for kw in FORMS:
            n += 1
            case = R.make_case(M, seed=10 * M + n, targeted=targeted)
            q = 1 + 97 * n
            got, intact = _launch(case, cuda_device, M, side, q, **kw)
            assert intact, (side, kw)                        # the guard image and record, the read-only operands
            assert R.mismatches(got, R.step_oracle(case, side=side, q=q, **kw)) == [], (side, kw)
            if not kw.get("first"):                          # frozen images: x_best, x_cand and the record untouched
                frozen = case["state"][:, 2] != 0
                for out, was in zip(got, (case["x_best"], case["x_cand"], case["state"])):
                    assert np.array_equal(out[frozen].view(np.int32), was[frozen].view(np.int32))
            if kw.get("last"):
                assert np.array_equal(got[1].view(np.int32), case["x_cand"].view(np.int32))
            with torch.cuda.stream(torch.cuda.Stream(cuda_device)):     # another stream: the same bits
                again, intact = _launch(case, cuda_device, M, side, q, **kw)
                torch.cuda.current_stream().synchronize()
            assert intact and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))
    case = R.make_case(M, seed=77, targeted=targeted)        # the top of the counter words: nothing wraps
    case["ids"] = np.arange(M, dtype=np.int64) + (2 ** 32 - M)
    got, intact = _launch(case, cuda_device, M, 4, 2 ** 32 - 1)
    assert intact and R.mismatches(got, R.step_oracle(case, side=4, q=2 ** 32 - 1)) == []


@pytest.mark.parametrize("M", [1, 3, 33])
def test_square_init_kernel_against_the_emulation(cuda_device, M):
    dev = cuda_device
    for n, eps in enumerate((R.EPS, 0.1 / MNIST_STD, 0.0)):
        case = R.make_case(M, seed=5 * M + n, eps=eps)
        x0 = _nan_rows(M + 1, dev)
        x0[:M] = torch.from_numpy(case["x0"]).to(dev)
        out = _nan_rows(M + 1, dev)
        keep = x0.clone()
        base = int(case["ids"][0])
        Fk.square_init(x0, eps, LO, HI, case["seed"], base, out=out, M=M)
        assert _guard_ok(out, M) and torch.equal(_bits(x0), _bits(keep))
        got = out[:M].cpu().numpy()
        assert not R.init_mismatch(got, R.init_oracle(case["x0"], eps, case["seed"], case["ids"]))
        ref = Fk.square_init_reference(x0[:M], eps, LO, HI, case["seed"], id_base=base)     # the package's own, on the GPU
        assert not R.init_mismatch(got, ref.cpu().numpy())
        with torch.cuda.stream(torch.cuda.Stream(dev)):
            again = Fk.square_init(x0, eps, LO, HI, case["seed"], base, M=M)
            torch.cuda.current_stream().synchronize()
        assert not R.init_mismatch(again.cpu().numpy(), got)
        if eps == 0.0:
            ok = ~np.isnan(case["x0"])
            assert np.array_equal(got[ok], case["x0"][ok])


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    M = 4
    case = R.make_case(M, seed=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items() if isinstance(v, np.ndarray) and k != "ids"}
    t["state"][:, 2] = 0                                     # every image live: a launch would store
    keep = {k: v.clone() for k, v in t.items()}
    C, p, s = native.load(), native.ptr, native.stream_handle()
    ok = dict(logp=p(t["logp"]), y=p(t["y"]), x0=p(t["x0"]), x_best=p(t["x_best"]), x_cand=p(t["x_cand"]),
              state=p(t["state"]), eps=0.1, lo=LO, hi=HI, seed=1, q=1, id_base=0, side=3, first=False, last=False,
              targeted=False, M=M, stream=s)
    for kw in (dict(x_cand=0), dict(state=0), dict(logp=0), dict(x_cand=ok["x_cand"] + 4), dict(state=ok["state"] + 4),
               dict(x_best=ok["x_best"] + 8), dict(side=0), dict(side=28), dict(q=1 << 32), dict(id_base=1 << 32),
               dict(id_base=(1 << 32) - M + 1), dict(M=0), dict(M=(1 << 20) + 1), dict(eps=-0.1)):
        with pytest.raises(RuntimeError):
            C.square_step(**dict(ok, **kw))
    oki = dict(x0=ok["x0"], x_cand=ok["x_cand"], eps=0.1, lo=LO, hi=HI, seed=1, id_base=0, M=M, stream=s)
    for kw in (dict(x_cand=0), dict(x0=0), dict(x_cand=ok["x_cand"] + 4), dict(id_base=1 << 32),
               dict(id_base=(1 << 32) - M + 1), dict(M=0), dict(M=(1 << 20) + 1), dict(eps=-0.1)):
        with pytest.raises(RuntimeError):
            C.square_init(**dict(oki, **kw))
    args = (t["logp"], t["y"], t["x0"], t["x_best"], t["x_cand"], t["state"])
    for bad in (dict(eps=-1.0), dict(side=0), dict(side=28), dict(q=1 << 32), dict(q=-1), dict(M=5),
                dict(id_base=(1 << 32) - 1), dict(lo=1.0, hi=0.0)):
        kw = dict(eps=0.1, lo=LO, hi=HI)
        kw.update(bad)
        with pytest.raises(ValueError):
            Fk.square_step(*args, **kw)
    with pytest.raises(ValueError):                          # three buffers
        Fk.square_step(t["logp"], t["y"], t["x0"], t["x_cand"], t["x_cand"], t["state"], 0.1, LO, HI)
    with pytest.raises(ValueError):
        Fk.square_init(t["x0"], 0.1, LO, HI, out=t["x0"])
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t[k]), _bits(v)) for k, v in keep.items())     # nothing ran


def _trained(dev):
    return copy.deepcopy(refmodel.trained_net()).to(dev)


@functools.lru_cache(maxsize=None)
def _images_cpu(n=128):
    imgs, labels = generate(n, seed=5)
    return normalize_u8(imgs).reshape(n, 784).contiguous(), labels.long()


def _images(dev, n=128):
    x, y = _images_cpu()
    return x[:n].to(dev).contiguous(), y[:n].to(dev)


def _by_hand(net, x0, y, queries, seed, ids, targeted=False):
    """The launches of ``fused_square_attack``, one by one through the checked entry points, on buffers of its own."""
    dev = x0.device
    M = x0.shape[0]
    st = fused_state(net)
    st.sync()
    buf = Fk.EvalBuffers.allocate(M, dev)
    chain = EvalChain(st.ms, buf)
    lab = y.to(torch.int32)
    x_best = _nan_rows(M, dev)
    state = torch.full((M, 4), ISENTINEL, dtype=torch.int32, device=dev)
    sides = Fk.square_sides(0.8, queries)
    x_cand = Fk.square_init(x0, EPS_N, LO, HI, seed, ids[0])
    for j in range(queries):
        last = j == queries - 1
        chain.run(M, xin=native.ptr(x_cand))
        Fk.square_step(buf.logp, lab, x0, x_best, x_cand, state, EPS_N, LO, HI, seed, j + 1, 1 if last else sides[j],
                       id_base=ids[0], first=j == 0, last=last, targeted=targeted)
    return x_best, Fk.square_state_margin(state), state[:, Fk.SQUARE_QUERIES].clone()


def _same(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_fused_loop_equals_its_launches_by_hand(cuda_device):
    dev = cuda_device
    net = _trained(dev)
    x0, y = _images(dev, 5)
    ids = list(range(40, 45))
    fused_state(net).sync()                                  # (binds the parameters to the flat buffer, once)
    params = [(q.detach().clone(), q.grad) for q in net.parameters()]
    want = _by_hand(net, x0, y, 12, 3, ids)
    for check_every in (0, 1, 5):
        assert _same(fused_square_attack(net, x0, y, EPS_N, 12, LO, HI, seed=3, ids=ids, check_every=check_every),
                     want), check_every
    for chunk in (1, 2, 5):                                  # every launch below fc1_fwd's 512-row change of split
        parts = [fused_square_attack(net, x0[i:i + chunk], y[i:i + chunk], EPS_N, 12, LO, HI, seed=3,
                                     ids=ids[i:i + chunk]) for i in range(0, 5, chunk)]
        assert _same([torch.cat([q[k] for q in parts]) for k in range(3)], want), chunk
    split = fused_square_attack(net, x0, y, EPS_N, 12, LO, HI, seed=3, ids=[40, 41, 42, 143, 144])   # two runs of ids
    assert _same([t[:3] for t in split], [t[:3] for t in want]) and not torch.equal(split[0][3:], want[0][3:])
    tgt = (y + 1) % 10
    assert _same(fused_square_attack(net, x0, tgt, EPS_N, 12, LO, HI, seed=3, ids=ids, targeted=True),
                 _by_hand(net, x0, tgt, 12, 3, ids, targeted=True))
    assert int(want[2].min()) >= 1 and int(want[2].max()) <= 12
    assert net.training is False                             # the mode, the parameters and their .grad are untouched
    assert all(torch.equal(q, was) and q.grad is g for q, (was, g) in zip(net.parameters(), params))


def test_predictor_square_attack_on_the_gpu(cuda_device):
    dev = cuda_device
    pr = Predictor(_trained(dev))
    assert pr.native
    x0, y = _images(dev)
    x_adv, lp, margin, used = pr.square_attack(x0.view(128, 1, 28, 28), y, eps=0.3, queries=32)
    xa = x_adv.reshape(128, 784)
    assert (xa >= LO).all() and (xa <= HI).all()
    up, down = R.vertex(x0.cpu().numpy(), True, EPS_N), R.vertex(x0.cpu().numpy(), False, EPS_N)
    got = xa.cpu().numpy().view(np.int32)
    assert ((got == up.view(np.int32)) | (got == down.view(np.int32))).all()      # a vertex of the box, bitwise
    assert torch.equal(_bits(Fk.square_margin_reference(lp, y)), _bits(margin))
    found = lp.argmax(1) != y
    assert torch.equal(found, margin < 0)
    assert used.dtype == torch.int32 and int(used.min()) >= 1 and int(used.max()) <= 32
    assert (margin[used < 32] < 0).all() and found.any()
    again = pr.square_attack(x0.view(128, 1, 28, 28), y, eps=0.3, queries=32, check_every=0)
    assert _same(again, (x_adv, lp, margin, used))


SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _cpu_counts():
    net = refmodel.trained_net()
    x0, y = _images_cpu()
    out = []
    for seed in SEEDS:
        x_adv, _, _ = reference_square_attack(net, x0, y, EPS_N, 32, LO, HI, seed=seed)
        with torch.no_grad():
            out.append(int((net.forward_reference(x_adv.view(128, 1, 28, 28)).argmax(1) == y).sum()))
    return tuple(out)


def test_success_rate_against_the_cpu_reference(cuda_device):
    """128 synthetic test images of the trained net (101 correct on the clean input), eps 0.3, 32 queries, seeds 0, 1,
    2.  The images still correct after the attack, as measured: CPU reference 43, 36, 40 (so a = 36, b = 43, d = 7 and
    the GPU counts must lie in [29, 50]); MI355X 43, 36, 40 - the same counts, seed by seed."""
    dev = cuda_device
    pr = Predictor(_trained(dev))
    x0, y = _images(dev)
    ref = _cpu_counts()
    a, b = min(ref), max(ref)
    d = max(b - a, 2)
    got = []
    for seed in SEEDS:
        _, lp, _, _ = pr.square_attack(x0.view(128, 1, 28, 28), y, eps=0.3, queries=32, seed=seed)
        got.append(int((lp.argmax(1) == y).sum()))
    clean = int((pr.predict(x0.view(128, 1, 28, 28)) == y).sum())
    print(f"\nsquare attack, correct of 128 after the attack: CPU reference {ref}, GPU {tuple(got)}, clean {clean}")
    assert all(a - d <= c <= b + d for c in got), (ref, got)
    assert max(got) < clean


def test_predict_cli_square_on_gpu(cuda_device, tmp_path):
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(refmodel.trained_net(), ckpt)
    log = str(tmp_path / "log.jsonl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "200", "--checkpoint", ckpt, "--json-log", log, "--square-eps", "0.3", "--square-queries", "20"],
                       cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    with open(log) as f:
        rec = json.loads(f.read())
    assert len(lines) == 2 and lines[1].startswith("Square set (Linf eps=0.3, queries=20, p_init=0.8): Average loss: ")
    assert rec["device"].startswith("cuda") and rec["square_correct"] < rec["correct"]
    assert f"Accuracy: {rec['square_correct']}/200 ({100.0 * rec['square_correct'] / 200:.0f}%), median queries: " in lines[1]
    assert (rec["square_eps"], rec["square_queries"], rec["square_p_init"], rec["square_seed"]) == (0.3, 20, 0.8, 0)
    # (the attack lowers the margin, not the NLL: the mean loss of a set with misclassified images may fall)
    assert rec["square_loss"] > 0 and 1 <= rec["square_median_queries"] <= 20
