"""The FAB attack on the GPU (MI355X only): ``fab_step`` against the float64 oracle on random operands and on the
hand-made images, the launcher refusals, ``fused_fab`` against its launches made by hand and under other chunkings,
``Predictor.fab`` against the CPU reference on the trained test net, the ensemble stage and the command line."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import fab as FB
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import deepfool_ref as D
import fab_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, ISENT = -7.25, -77
RATIO_MARGIN, FOUND_MARGIN = 0.05, 2                         # test_gpu_deepfool.py's caps for the same comparison
OUT = ("rows", "x", "x_best", "norm_best", "status", "iters", "proj")


def _launch(dev, ops, norm, last=False, state=None):
    """One ``fab_step`` launch of the operand dict on sentinel-guarded buffers (a guard image after the M; ``state``:
    the buffers of an earlier launch instead); the results on the CPU and the device buffers."""
    M = ops["y"].numel()
    if state is None:
        state = {k: torch.full(s, ISENT if k in ("status", "iters") else SENT, device=dev,
                               dtype=torch.int32 if k in ("status", "iters") else torch.float32)
                 for k, s in (("rows", (10 * (M + 1), 784)), ("x", (M + 1, 784)), ("x_best", (M + 1, 784)),
                              ("norm_best", (M + 1,)), ("status", (M + 1,)), ("iters", (M + 1,)), ("proj", (M + 1, 2, 784)))}
        state["rows"][:10 * M] = ops["x"].to(dev).repeat_interleave(10, dim=0)
        for k in ("x", "x_best", "norm_best", "status", "iters"):
            state[k][:M] = ops[k].to(dev)
    dx = torch.cat([ops["dx"], torch.full((10, 784), float("nan"))]).to(dev)           # the guard image's rows: NaN
    loss = torch.cat([ops["loss"], torch.full((10,), float("nan"))]).to(dev)
    y = torch.cat([ops["y"], torch.tensor([3], dtype=torch.int32)]).to(dev)
    x0 = torch.cat([ops["x0"], ops["x0"][:1]]).to(dev)
    Fk.fab_step(dx, loss, y, x0, state["x"], state["x_best"], state["norm_best"], state["rows"], state["status"],
                state["iters"], *R.PAR, norm, last=last, proj=state["proj"], M=M)
    torch.cuda.synchronize()
    assert torch.equal(x0[:M].cpu(), ops["x0"])
    for k in OUT:
        n = 10 * M if k == "rows" else M
        assert (state[k][n:] == (ISENT if k in ("status", "iters") else SENT)).all(), f"{k}: an entry past M was written"
    got = {k: state[k][:M].cpu() for k in R.KEYS}
    stepped = ~(got["proj"].reshape(M, -1) == SENT).all(dim=1)                        # proj is stored by forward steps only
    got["proj"] = torch.where(stepped[:, None, None], got["proj"], torch.zeros(()))
    return got, state


@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("M", [1, 3, 33])
def test_fab_step_against_the_oracle(cuda_device, M, norm):
    """``fab_ref.operands`` (scales 1e-6 .. 1e2, equal breakpoints on lo, pixels on hi, zero weights, the crossing
    segment away from the tail): every element of x, d1 and d2 within the launch's cap (``fab_ref.check_step``), the
    class chosen the oracle's, the ten rows equal x bit for bit, a relaunch the same bits."""
    ops = R.operands(M)
    got, st = _launch(cuda_device, ops, norm)
    worst = R.check_step(got, ops, norm)
    print(f"fab_step {norm} M={M}: largest deviation / eps: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert torch.equal(st["rows"][:10 * M].cpu().view(M, 10, 784), got["x"][:, None, :].expand(M, 10, 784))
    want = R.step_images(ops, norm)
    g, f = ops["dx"].double().view(M, 10, 784), ops["loss"].double().view(M, 10)
    for i in range(M):                                       # d1 moves every weighted pixel along -sgn(f_l) sgn(w_l)
        y, d1 = int(ops["y"][i]), got["proj"][i, 0].double()
        agree = ((-(f[i, y] - f[i]).sign()[:, None] * (g[i, y][None, :] - g[i]).sign() * d1.sign()[None, :]) > 0).sum(1)
        agree[y] = -1
        assert int(agree.argmax()) == int(want["l"][i]) and int(agree.max()) == int((d1 != 0).sum()), i
    again, st2 = _launch(cuda_device, ops, norm)
    assert all(torch.equal(again[k], got[k]) for k in R.KEYS) and torch.equal(st2["rows"], st["rows"])


@pytest.mark.parametrize("norm", R.NORMS)
def test_fab_step_hand_made_images(cuda_device, norm):
    dev, ops, at = cuda_device, R.hand_cases(), R.HAND.index
    M, lo, hi = len(R.HAND), np.float32(R.LO), np.float32(R.HI)
    got, st = _launch(dev, ops, norm)
    R.check_step(got, ops, norm)
    rows = st["rows"][:10 * M].cpu().view(M, 10, 784)
    kept = lambda i, keys: all(torch.equal(got[k][i], ops[k][i]) for k in keys)                    # noqa: E731
    moved = [i for i in range(M) if R.HAND[i] not in ("clean_misclassified", "all_zero", "frozen")]
    assert all(torch.equal(rows[i], got["x"][i].expand(10, 784)) or R.HAND[i] == "nan_in_g_y" for i in range(M))
    assert torch.equal(got["iters"], torch.tensor([int(i in moved) for i in range(M)], dtype=torch.int32) + ops["iters"])
    i = at("crossed_nearer")                                 # recorded, then pulled back towards x0
    assert torch.equal(got["x_best"][i], ops["x"][i]) and float(got["norm_best"][i]) > 0 and int(got["status"][i]) == 0
    assert ((got["x"][i] - ops["x0"][i]).abs() <= (ops["x"][i] - ops["x0"][i]).abs()).all() and not kept(i, ("x",))
    i = at("crossed_farther")                                # not recorded, still pulled back
    assert kept(i, ("x_best", "norm_best")) and not kept(i, ("x",))
    i = at("clean_misclassified")
    assert int(got["status"][i]) == Fk.FAB_DONE and float(got["norm_best"][i]) == 0.0 and kept(i, ("x", "iters"))
    assert torch.equal(got["x_best"][i], ops["x0"][i])
    i = at("misses_box")                                     # every weighted element on its bound, bit for bit
    w = (ops["dx"].view(M, 10, 784)[i, 3] - ops["dx"].view(M, 10, 784)[i, int(R.step_images(ops, norm)["l"][i])])
    for p, v in enumerate((ops["x"][i], ops["x0"][i])):
        d = got["proj"][i, p]
        assert torch.equal(d[w != 0], torch.where(d > 0, hi - v, -(v - lo))[w != 0]) and not d[w == 0].any()
    i = at("x_is_x0")
    assert torch.equal(got["proj"][i, 0], got["proj"][i, 1]) and got["proj"][i, 0].any()
    i = at("r_zero")
    assert not got["proj"][i, 0].any() and got["proj"][i, 1].any()
    assert int(got["status"][at("all_zero")]) == Fk.FAB_STUCK and kept(at("all_zero"), ("x", "x_best", "norm_best", "iters"))
    i = at("both_clamps")
    assert (got["x"][i] == lo).any() and (got["x"][i] == hi).any() and (got["x"][i] >= lo).all() and (got["x"][i] <= hi).all()
    i = at("nan_in_g_y")                                     # fills its image, and only it
    assert torch.isnan(got["x"][i]).all() and torch.isnan(rows[i]).all() and torch.isnan(got["proj"][i]).all()
    others = [j for j in range(M) if j != i]
    assert torch.isfinite(got["x"][others]).all() and torch.isfinite(rows[others]).all()
    assert all(torch.equal(got[k][at("nan_in_unchosen")], got[k][at("plain")]) for k in ("x", "proj"))
    assert kept(at("frozen"), R.KEYS[:5]) and torch.equal(rows[at("frozen")], ops["x"][at("frozen")].expand(10, 784))
    # a `last` round on the results moves no iterate; frozen images (done, stuck) keep every bit over a further round
    before = {k: v.clone() for k, v in st.items()}
    ops2 = dict(ops, **{k: got[k] for k in ("x", "x_best", "norm_best", "status", "iters")})
    for last in (True, False):
        got2, _ = _launch(dev, ops2, norm, last=last, state=st)
        if last:
            assert all(torch.equal(st[k].view(torch.int32), before[k].view(torch.int32))          # (bits: an image is NaN)
                       for k in ("x", "rows", "iters", "status"))
        for i in (at("clean_misclassified"), at("all_zero"), at("frozen")):
            assert all(torch.equal(st[k][i], before[k][i]) for k in OUT if k != "rows"), i
            assert torch.equal(st["rows"][10 * i:10 * i + 10], before["rows"][10 * i:10 * i + 10]), i
    assert int(st["iters"][at("plain")]) == 2


def test_fab_launcher_refusals(cuda_device):
    dev, M = cuda_device, 2
    ops = R.operands(3)
    f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=dev)              # noqa: E731
    b = dict(x=f(M, 784), x_best=f(M, 784), norm_best=f(M), rows=f(10 * M, 784), proj=f(M, 2, 784),
             status=torch.full((M,), ISENT, dtype=torch.int32, device=dev),
             iters=torch.full((M,), ISENT, dtype=torch.int32, device=dev))
    dx, loss, y, x0 = (ops[k][:n].to(dev) for k, n in (("dx", 10 * M), ("loss", 10 * M), ("y", M), ("x0", M)))
    good = dict(dx=dx, loss_rows=loss, y=y, x0=x0, x=b["x"], x_best=b["x_best"], norm_best=b["norm_best"], rows=b["rows"],
                status=b["status"], iters=b["iters"], alpha_max=0.1, eta=1.05, beta=0.9, lo=R.LO, hi=R.HI, norm="linf",
                proj=b["proj"])
    for kw in (dict(dx=dx.double()), dict(dx=dx[:19]), dict(dx=dx.cpu()), dict(loss_rows=loss[:19]), dict(y=y.long()),
               dict(y=y[:1], M=2), dict(x0=x0[:1]), dict(x0=b["x"]), dict(x_best=b["x_best"][:1]),
               dict(norm_best=b["norm_best"].double()), dict(rows=b["rows"][:19]), dict(status=b["status"].long()),
               dict(iters=b["iters"][:1]), dict(proj=b["proj"][:1]), dict(norm="l1"), dict(eta=0.9), dict(beta=0.0),
               dict(beta=1.1), dict(alpha_max=-0.1), dict(alpha_max=float("nan")), dict(lo=1.0, hi=0.0), dict(M=0)):
        with pytest.raises(ValueError, match="fab_step"):
            Fk.fab_step(**{**good, **kw})
    C, p, s = Fk.native.load(), Fk.native.ptr, Fk.native.stream_handle()
    st = (p(dx), p(loss), p(y), p(x0), p(b["x"]), p(b["x_best"]), p(b["norm_best"]), p(b["rows"]), p(b["status"]),
          p(b["iters"]), p(b["proj"]))
    tail = (0.1, 1.05, 0.9, R.LO, R.HI, C.FAB_LINF, False)
    bad = [st[:k] + (0,) + st[k + 1:] + tail + (M, s) for k in range(10)]             # each required pointer null
    bad += [st[:k] + (st[k] + 4,) + st[k + 1:] + tail + (1, s) for k in (0, 3, 4, 5, 7, 10)]      # misaligned rows
    bad += [st[:k] + (st[k] + 2,) + st[k + 1:] + tail + (1, s) for k in (1, 2, 6, 8, 9)]          # misaligned vectors
    bad += [st + t + (M, s) for t in ((1.5,) + tail[1:], (float("nan"),) + tail[1:], (0.1, 0.99) + tail[2:],
                                      (0.1, 1.05, 0.0) + tail[3:], (0.1, 1.05, 1.5) + tail[3:], tail[:5] + (2, False))]
    bad += [st + tail + (0, s), st + tail + (Fk.DF_MAX_M + 1, s)]
    for args in bad:
        with pytest.raises(RuntimeError, match="fab_step"):
            C.fab_step(*args)
    torch.cuda.synchronize()
    assert all((v == (ISENT if k in ("status", "iters") else SENT)).all() for k, v in b.items())
    assert (C.FAB_LINF, C.FAB_L2, C.FAB_RUNNING, C.FAB_DONE, C.FAB_STUCK) == (0, 1, 0, 1, 2)


def _by_hand(net, src, labels, norm, steps):
    """``deepfool_init`` and ``steps`` + 1 times the six launches, through ``ops.functional``, on buffers of their own."""
    st = fused_state(net)
    st.sync()
    ms, dev, M = st.ms, src.device, src.shape[0]
    buf = Fk.StepBuffers.allocate(10 * M, dev)
    state = torch.tensor([1 << 32, 0, 0], dtype=torch.int64).to(dev)     # step 0 | NO_DROPOUT, zero seed / counter
    lab10 = torch.arange(10, dtype=torch.int32, device=dev).repeat(M)
    rows, x, x0, x_best, status, iters, _ = Fk.deepfool_init(src)
    norm_best = torch.full((M,), float("inf"), device=dev)
    for it in range(steps + 1):
        Fk.trunk_fwd(ms, None, None, buf, True, state=state, xin=rows)
        Fk.fc1_fwd(ms, buf)
        Fk.head_train(ms, lab10, None, buf, state=state, inv_batch=1.0)
        Fk.fc_bwd(ms, buf, role=Fk.FC_ROLE_B, state=state)
        dx = Fk.input_grad(ms, buf)
        Fk.fab_step(dx, buf.loss_rows, labels.to(dev, torch.int32), x0, x, x_best, norm_best, rows, status, iters,
                    *R.PAR, norm, last=it == steps)
    return torch.where(torch.isinf(norm_best)[:, None], x0, x_best), norm_best, iters, status


@pytest.mark.parametrize("norm", R.NORMS)
def test_fused_fab_equals_hand_launches(cuda_device, norm):
    """The loop equals ``deepfool_init`` plus its six launches a round made by hand, bit for bit, under other chunkings
    (every launch below fc1_fwd's 512-row split change), reuses its buffers and leaves the net as it was."""
    dev, steps, B = cuda_device, 6, 33
    net = copy.deepcopy(D.trained_net()).to(dev).train()
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    st = fused_state(net)
    grads = {k: None if v.grad is None else v.grad.clone() for k, v in net.named_parameters()}
    offset = st.rng_offset
    imgs, labels = D.trained_case()
    u8, y = imgs[:B].reshape(B, 784).contiguous().to(dev), labels[:B].clone()
    y[1] = (y[1] + 1) % 10                                   # an image outside its label on entry
    same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a, b))                  # noqa: E731
    want = _by_hand(net, u8, y, norm, steps)
    assert torch.isfinite(want[0]).all() and int(want[3][1]) == Fk.FAB_DONE and float(want[1][1]) == 0.0
    assert same(_by_hand(net, _PIXEL_LUT.to(dev)[u8.long()].contiguous(), y, norm, steps), want)   # fp32 source form
    got = FB.fused_fab(net, u8, y.to(dev), norm, steps, *R.PAR)
    assert same(got, want) and got[0].shape == (B, 784) and got[2].dtype == torch.int32
    buf = st.deepfool_buf
    ptrs = (buf.x.data_ptr(), buf.dx.data_ptr())
    for rpl in (110, 330, 110):
        if rpl == 330:
            pooled = sum(len(v) for v in st.pool.values())       # (both sizes' activation sets are in the pool by now)
        assert same(FB.fused_fab(net, u8, y.to(dev), norm, steps, *R.PAR, rows_per_launch=rpl), want), rpl
    assert st.deepfool_buf is buf and (buf.x.data_ptr(), buf.dx.data_ptr()) == ptrs
    assert sum(len(v) for v in st.pool.values()) == pooled
    for kw in (dict(norm="l1"), dict(steps=0), dict(eta=0.5), dict(beta=0.0), dict(alpha_max=2.0), dict(rows_per_launch=9)):
        args = dict(norm=norm, steps=steps, alpha_max=0.1, eta=1.05, beta=0.9, lo=R.LO, hi=R.HI)
        with pytest.raises(ValueError, match="fused_fab"):
            FB.fused_fab(net, u8, y.to(dev), **{**args, **kw})
    assert st.rng_offset == offset and net.training
    assert all(torch.equal(v, before[k]) for k, v in net.named_parameters())
    for k, v in net.named_parameters():
        assert (v.grad is None) == (grads[k] is None) and (v.grad is None or torch.equal(v.grad, grads[k])), k


@pytest.fixture(scope="module")
def gpu_predictor(cuda_device):
    return Predictor(copy.deepcopy(D.trained_net()).to(cuda_device).train())   # train mode: must not matter


@pytest.mark.parametrize("norm", R.NORMS)
def test_fab_matches_cpu_reference(cuda_device, gpu_predictor, norm):
    """The 64 images of ``deepfool_ref.trained_case``, ``fab_ref.STEPS`` iterations: the bf16 forward moves the
    boundary, so the found count and the median-radius ratio GPU / CPU are held at ``test_gpu_deepfool.py``'s caps."""
    dev, pr = cuda_device, gpu_predictor
    imgs, labels = D.trained_case()
    _, r_ref, _, f_ref = R.cpu_fab(norm)
    assert pr.native
    xa, radii, lp, found = pr.fab(imgs.to(dev), labels.to(dev), norm, steps=R.STEPS)
    assert xa.shape == (64, 1, 28, 28) and xa.is_cuda and radii.shape == (64,) and lp.shape == (64, 10)
    assert torch.equal(found, pr.predict(xa) != labels.to(dev).long())
    assert (xa >= R.LO).all() and (xa <= R.HI).all() and torch.isfinite(xa).all()
    diff = xa.cpu().reshape(64, 784).double() - _PIXEL_LUT[imgs.reshape(64, 784).long()].double()
    want = (diff.abs().amax(1) if norm == "linf" else diff.square().sum(1).sqrt()) * MNIST_STD
    fin = torch.isfinite(radii.cpu()) & (want > 0)
    assert ((radii.cpu().double() - want).abs()[fin] <= 4 * R.ULP * want[fin]).all()
    both = found.cpu() & f_ref
    ratio = float(radii.cpu()[both].median()) / float(r_ref[both].median())
    print(f"GPU FAB ({norm}): found {int(found.sum())}/64 (CPU {int(f_ref.sum())}), median radius "
          f"{float(radii.cpu()[both].median()):.4f} (CPU {float(r_ref[both].median()):.4f}), ratio {ratio:.4f}")
    assert abs(ratio - 1.0) <= RATIO_MARGIN, ratio
    assert abs(int(found.sum()) - int(f_ref.sum())) <= FOUND_MARGIN
    assert pr.net.training and all(p.grad is None or not p.grad.any().item() for p in pr.net.parameters())


def test_ensemble_stage_and_cli_on_gpu(cuda_device, gpu_predictor, gpu_box, tmp_path):
    pr = gpu_predictor
    imgs, labels = D.trained_case()
    x, y = imgs[:16].to(cuda_device), labels[:16]
    base = pr.robust_evaluate_ensemble(x, y, 0.15, steps=5, n_targets=1, queries=0)
    got = pr.robust_evaluate_ensemble(x, y, 0.15, steps=5, n_targets=1, queries=0, fab_steps=10)
    assert list(got[2]) == ["clean", "apgd_ce", "apgd_t", "fab", "square"] and got[2]["apgd_t"] == base[2]["apgd_t"]
    assert got[0] == got[2]["fab"] <= base[0]
    torch.manual_seed(5)
    ckpt, log = str(tmp_path / "mnist_cnn.pt"), str(tmp_path / "log.jsonl")
    save_state_dict(Net(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size",
                        "64", "--checkpoint", ckpt, "--batch-size", "40", "--json-log", log, "--fab", "--fab-steps", "10",
                        "--fab-count", "64", "--fab-radii", "0.1,0.3"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[0].startswith("Test set:") and len(lines) == 4
    assert lines[1].startswith("FAB set (Linf, steps=10): Found: ") and "/64 (" in lines[1] and "median radius: " in lines[1]
    assert lines[2].startswith("Accuracy at radius 0.1: ") and lines[3].startswith("Accuracy at radius 0.3: ")
    with open(log) as f:
        rec = [json.loads(ln) for ln in f if ln.strip()]
    assert len(rec) == 1 and rec[0]["device"].startswith("cuda") and rec[0]["fab_steps"] == 10
    assert 0 <= rec[0]["fab_found"] <= 64 and set(rec[0]["fab_accuracy_at"]) == {"0.1", "0.3"}
