"""The Carlini-Wagner L2 attack on the GPU (MI355X only): ``cw_step`` against the float64 evaluation of its formulas,
the launcher refusals, ``fused_carlini_wagner`` against its launches made by hand and under other chunkings,
``Predictor.carlini_wagner`` against the CPU reference on the trained test net, and the command line."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import cw as CW
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
from pytorch_mnist_ddp_amd.utils.checkpoint import save_state_dict

import cw_ref as R
import deepfool_ref as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, ISENT = -7.25, -77
# test_matches_cpu_reference: the first measured deviations (one run) and the floors they are held above
RATIO_FIRST, FOUND_DIFF_FIRST, RATIO_FLOOR, FOUND_FLOOR = 0.0002, 0, 0.05, 2
_bits = lambda t: t.contiguous().view(torch.int32)                                          # noqa: E731


def _launch(dev, ops, sign, kappa, t, search, kind):
    """One ``cw_step`` launch of the case on buffers with a sentinel-filled guard image after the M; the results on
    the CPU.  With ``first`` the state buffers hold sentinels throughout (the launch reads none of them)."""
    M = ops["x"].shape[0]
    pad = lambda q, fill: torch.cat([q, torch.full((1, *q.shape[1:]), fill, dtype=q.dtype)]).to(dev)     # noqa: E731
    b = {k: pad(v, ISENT if k == "istate" else SENT) for k, v in ops.items()}
    if kind == "first":
        for k in ("w", "m1", "v", "x_best", "fstate", "istate"):
            b[k].fill_(ISENT if k == "istate" else SENT)
    keep = {k: b[k].clone() for k in ("dx", "loss", "x0")}
    Fk.cw_step(b["dx"], b["loss"], b["x0"], b["w"], b["m1"], b["v"], b["x"], b["x_best"], b["fstate"], b["istate"],
               sign, kappa, R.LR, R.C_INIT, t, search, R.LO, R.HI, first=kind == "first",
               search_end=kind == "search_end", last=kind == "last", M=M)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(b[k]), _bits(keep[k])) for k in keep)                     # the read-only operands
    for k in R.ROWS + ("fstate", "istate"):
        assert (b[k][M:] == (ISENT if k == "istate" else SENT)).all(), f"{k}: the guard image was written"
    return {k: b[k][:M].cpu() for k in R.ROWS + ("fstate", "istate")}


def _check(dev, ops, sign, kappa, kind, t=4, search=2):
    """One case: the float32 reference decides as the float64 form does (CPU), then the kernel against both.  Returns
    the largest kernel and reference deviations from float64 over d_best, w, m1, v, x, relative to each value's scale."""
    M = ops["x"].shape[0]
    w64, r32 = R.step64(ops, sign, kappa, t, search, kind), R.reference32(ops, sign, kappa, t, search, kind)
    dec64 = torch.from_numpy(w64["fstate"][:, :3]).float()
    assert torch.equal(r32["istate"].long(), torch.from_numpy(w64["istate"])) and torch.equal(_bits(r32["fstate"][:, :3]), _bits(dec64))
    got = _launch(dev, ops, sign, kappa, t, search, kind)
    again = _launch(dev, ops, sign, kappa, t, search, kind)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got)                   # the same operands: the same bits
    rdev = R.reference32({k: v.to(dev) for k, v in ops.items()}, sign, kappa, t, search, kind)   # the device's own tanh / atanh
    assert torch.equal(got["istate"], r32["istate"]) and torch.equal(_bits(got["fstate"][:, :3]), _bits(dec64))
    improved = torch.from_numpy(w64["istate"][:, 1] == search + 1)
    old_best = ops["x0"] if kind == "first" else ops["x_best"]
    assert torch.equal(_bits(got["x_best"]), _bits(torch.where(improved[:, None], ops["x"], old_best)))
    if kind == "search_end":
        assert torch.equal(_bits(got["x"]), _bits(ops["x0"])) and torch.equal(_bits(got["w"]), _bits(rdev["w"].cpu()))
        assert not got["m1"].any() and not got["v"].any()
    if kind == "last":
        assert all(torch.equal(_bits(got[k]), _bits(ops[k])) for k in ("w", "m1", "v", "x"))
    worst = [0.0, 0.0]
    for k in ("d_best", "w", "m1", "v", "x"):
        pick = (lambda q: np.asarray(q["fstate"])[:, 3]) if k == "d_best" else (lambda q: np.asarray(q[k]))
        want, fin = pick(w64), np.isfinite(pick(w64))
        assert (np.isfinite(pick(got)) == fin).all() and (pick(got)[~fin] == want[~fin]).all(), k
        scale = float(np.abs(want[fin]).max()) if fin.any() else 0.0
        dk, dr = (float(np.abs(pick(q)[fin].astype(np.float64) - want[fin]).max()) if fin.any() else 0.0 for q in (got, r32))
        print(f"cw_step {kind} M={M} sign={sign} kappa={kappa} {k}: kernel {dk:.3e} reference {dr:.3e} scale {scale:.3e}")
        assert dk <= max(4 * dr, float(np.spacing(np.float32(scale)))), (k, dk, dr)
        if scale:
            worst = [max(worst[0], dk / scale), max(worst[1], dr / scale)]
    return worst


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M", [1, 3, 33])
def test_cw_step_against_float64(cuda_device, M, kind):
    """Largest deviations from the float64 values measured once, relative to each quantity's largest value: kernel
    6.1e-6 (w after a reset: atanh at a background pixel), ``cw_step_reference`` (torch float32, CPU) 6.1e-6."""
    worst = [_check(cuda_device, R.make_case(M, sign, kappa, kind), sign, kappa, kind)
             for sign in (1, -1) for kappa in (0.0, 0.5)]
    print(f"cw_step {kind} M={M}: largest relative deviation kernel {max(w[0] for w in worst):.3e}, "
          f"reference {max(w[1] for w in worst):.3e}")


def test_nan_gradient_stays_in_its_image(cuda_device):
    ops = R.make_case(3, 1, 0.5, "plain")
    base = _launch(cuda_device, ops, 1, 0.5, 4, 2, "plain")
    ops["dx"][1, 5] = float("nan")
    got = _launch(cuda_device, ops, 1, 0.5, 4, 2, "plain")
    assert torch.isnan(got["w"][1, 5]) and torch.isnan(got["x"][1, 5])
    for k in got:
        assert torch.equal(_bits(got[k][[0, 2]]), _bits(base[k][[0, 2]])), k


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    t = {k: v.to(dev) for k, v in R.make_case(4, 1, 0.0, "plain").items()}
    keep = {k: v.clone() for k, v in t.items()}
    C, p, s = native.load(), native.ptr, native.stream_handle()
    ok = dict(dx=p(t["dx"]), loss_rows=p(t["loss"]), x0=p(t["x0"]), w=p(t["w"]), m1=p(t["m1"]), v=p(t["v"]), x=p(t["x"]),
              x_best=p(t["x_best"]), fstate=p(t["fstate"]), istate=p(t["istate"]), sign=1.0, kappa=0.0, lr=0.05,
              c_init=1.0, beta1=0.9, beta2=0.999, adam_eps=1e-8, bc1=0.1, bc2=0.001, dist_scale=0.09, lo=R.LO, hi=R.HI,
              search=0, first=False, search_end=False, last=False, M=4, stream=s)
    for kw in (dict(M=0), dict(M=(1 << 20) + 1), dict(sign=0.0), dict(kappa=-0.1), dict(lr=0.0), dict(x=ok["x"] + 4),
               dict(first=True, c_init=0.0), dict(first=True, last=True), dict(fstate=ok["fstate"] + 4), dict(w=0),
               dict(loss_rows=ok["loss_rows"] + 2), dict(x_best=0)):
        with pytest.raises(RuntimeError):
            C.cw_step(**dict(ok, **kw))
    args = tuple(t[k] for k in ("dx", "loss", "x0", "w", "m1", "v", "x", "x_best", "fstate", "istate"))
    for bad in (dict(sign=0), dict(kappa=-1.0), dict(lr=0.0), dict(first=True, c_init=0.0), dict(first=True, last=True),
                dict(M=5), dict(t=0), dict(search=-1), dict(lo=1.0, hi=0.0)):
        kw = dict(sign=1, kappa=0.0, lr=0.05, c_init=1.0, t=1, search=0, lo=R.LO, hi=R.HI)
        kw.update(bad)
        with pytest.raises(ValueError):
            Fk.cw_step(*args, **kw)
    with pytest.raises(ValueError):                          # seven buffers
        Fk.cw_step(*args[:4], t["w"], *args[5:], 1, 0.0, 0.05, 1.0, 1, 0, R.LO, R.HI)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t[k]), _bits(v)) for k, v in keep.items())     # nothing ran


def _by_hand(net, x0, y, search_steps, steps, sign=1, kappa=0.0):
    """The launches of ``fused_carlini_wagner``, one by one through ``GradChain`` and the checked entry point."""
    dev, M = x0.device, x0.shape[0]
    st = fused_state(net)
    st.sync()
    lab = y.to(dev, torch.int32)
    w, m1, v, dx, x_best = (torch.full((M, 784), float("nan"), device=dev) for _ in range(5))
    x = x0.clone()
    fstate = torch.full((M, 4), float("nan"), device=dev)
    istate = torch.full((M, 4), ISENT, dtype=torch.int32, device=dev)
    chain = GradChain(st, M, "cw")
    loss = chain._buf.loss_rows
    for k in range(search_steps):
        for j in range(steps + 1):
            end, final = j == steps, k == search_steps - 1
            chain.run(native.ptr(x), native.ptr(lab), M)
            chain.input_grad(native.ptr(dx), M)
            Fk.cw_step(dx, loss, x0, w, m1, v, x, x_best, fstate, istate, sign, kappa, R.LR, R.C_INIT, min(j + 1, steps),
                       k, R.LO, R.HI, first=k == 0 and j == 0, search_end=end and not final, last=end and final, M=M)
    chain.release()
    return x_best, fstate[:, Fk.CW_D_BEST].clone(), istate[:, Fk.CW_FOUND_SEARCH].clone(), fstate[:, Fk.CW_C].clone()


def test_fused_loop_equals_its_launches_by_hand(cuda_device):
    dev, B = cuda_device, 5
    net = copy.deepcopy(D.trained_net()).to(dev).train()
    imgs, labels = D.trained_case()
    x0 = _PIXEL_LUT[imgs[:B].reshape(B, 784).long()].to(dev).contiguous()
    y = labels[:B].clone()
    y[1] = (y[1] + 1) % 10                                   # an image outside its label on entry
    same = lambda a, b: all(torch.equal(_bits(u), _bits(q)) for u, q in zip(a, b))            # noqa: E731
    fused_state(net)
    before = [(q.detach().clone(), None if q.grad is None else q.grad.clone()) for q in net.parameters()]
    want = _by_hand(net, x0, y, 2, 3)
    assert float(want[1][1]) == 0.0 and int(want[2][1]) == 1 and torch.equal(want[0][1], x0[1])
    for rpl in (8192, 2, 8192):
        assert same(CW.fused_carlini_wagner(net, x0, y.to(dev), 2, 3, R.LR, R.C_INIT, 0.0, 1, R.LO, R.HI, rows_per_launch=rpl), want), rpl
    assert net.training
    for q, (val, grad) in zip(net.parameters(), before):
        assert torch.equal(q, val) and (q.grad is None) == (grad is None) and (grad is None or torch.equal(q.grad, grad))


def test_matches_cpu_reference(cuda_device):
    """``D.trained_case`` (image 1 mislabelled), search_steps = 3, steps = 30.  The bf16 forward flips near-ties, so the
    median-radius ratio GPU / CPU over the images found by both and the count of images whose ``found`` differs are
    held to twice their first measured deviations (floors 0.05 and 2).  Measured once: ratio 1.0002, 0 images
    differ; median CW radius 1.4645 beside DeepFool's 1.4314 on the same images (reported, not asserted)."""
    dev = cuda_device
    pr = Predictor(copy.deepcopy(D.trained_net()).to(dev).train())
    imgs, _ = D.trained_case()
    labels, ref = R.cpu_carlini_wagner()
    out = pr.carlini_wagner(imgs.to(dev), labels.to(dev), search_steps=3, steps=30)
    assert pr.native and out[0].shape == (64, 1, 28, 28) and out[0].is_cuda
    R.check_invariants(_PIXEL_LUT[imgs.reshape(64, 784).long()], labels.long(), out, pr.predict(imgs.to(dev)).cpu())
    radii, found = out[1].cpu(), out[3].cpu()
    both = found & ref[3]
    ratio = float(radii[both].median()) / float(ref[1][both].median())
    differ = int((found != ref[3]).sum())
    _, r_df, _, f_df = pr.minimum_norm(imgs.to(dev), labels.to(dev))
    on = both & f_df.cpu()
    print(f"GPU CW: found {int(found.sum())}/64 (CPU {int(ref[3].sum())}, {differ} differ), median radius "
          f"{float(radii[both].median()):.4f} (CPU {float(ref[1][both].median()):.4f}), ratio {ratio:.4f}; on the "
          f"{int(on.sum())} images DeepFool found too: CW {float(radii[on].median()):.4f}, DeepFool {float(r_df.cpu()[on].median()):.4f}")
    assert abs(ratio - 1.0) <= max(2 * RATIO_FIRST, RATIO_FLOOR), ratio
    assert differ <= max(2 * FOUND_DIFF_FIRST, FOUND_FLOOR), differ


def test_cli_on_gpu(cuda_device, gpu_box, tmp_path):
    torch.manual_seed(5)
    ckpt = str(tmp_path / "mnist_cnn.pt")
    save_state_dict(Net(), ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT, MNIST_AMD_NO_BUILD="1")
    base = [sys.executable, os.path.join(ROOT, "mnist_predict.py"), "--synthetic", "--synthetic-test-size", "64",
            "--checkpoint", ckpt]
    for cw in (True, False):
        log = str(tmp_path / f"log{int(cw)}.jsonl")
        flags = ["--cw", "--cw-count", "32", "--cw-search-steps", "2", "--cw-steps", "10", "--cw-radii", "0.5"] if cw else []
        r = subprocess.run(base + ["--json-log", log] + flags, cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        with open(log) as f:
            rec = json.loads(f.read())
        keys = {"cw_search_steps", "cw_steps", "cw_lr", "cw_c", "cw_kappa", "cw_count", "cw_found", "cw_median_radius",
                "cw_mean_radius", "cw_accuracy_at"}
        if cw:
            assert len(lines) == 3 and lines[1].startswith("CW set (L2, search=2, steps=10): Found: ") and "/32 (" in lines[1]
            assert lines[2].startswith("Accuracy at radius 0.5: ") and keys <= set(rec) and rec["cw_count"] == 32
        else:
            assert len(lines) == 1 and not any(k.startswith("cw_") for k in rec) and "CW set" not in r.stdout
