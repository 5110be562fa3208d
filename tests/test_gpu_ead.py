"""EAD, the elastic-net L1 attack, on the GPU (MI355X only): ``ead_step`` against the float64 evaluation of its formulas
and the float32 reference, the launcher refusals, ``fused_elastic_net`` against its launches made by hand and under
other chunkings, and ``Predictor.elastic_net`` against the CPU reference on the trained test net."""
import copy

import numpy as np
import pytest
import torch

from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.ops import ead as EAD
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

import deepfool_ref as D
import ead_ref as R

pytestmark = pytest.mark.gpu
SENT, ISENT = -7.25, -77
# test_matches_cpu_reference: the first measured deviations (one run) and the floors they are held above
RATIO_FIRST, FOUND_DIFF_FIRST, RATIO_FLOOR, FOUND_FLOOR = 0.0056, 0, 0.05, 2
OUT = R.ROWS + ("fstate", "istate")
_bits = lambda t: t.contiguous().view(torch.int32)                                          # noqa: E731


def _launch(dev, ops, sign, kappa, k, search, kind, rule):
    """One ``ead_step`` launch of the case on buffers with a sentinel-filled guard image after the M (``loss``: a guard
    entry after the 2 M); the results on the CPU.  With ``first`` x_best and the records hold sentinels (not read)."""
    M = ops["x"].shape[0]
    pad = lambda q, fill: torch.cat([q, torch.full((1, *q.shape[1:]), fill, dtype=q.dtype)]).to(dev)     # noqa: E731
    b = {n: pad(v, ISENT if n == "istate" else SENT) for n, v in ops.items()}
    if kind == "first":
        for n in ("x_best", "fstate", "istate"):
            b[n].fill_(ISENT if n == "istate" else SENT)
    keep = {n: b[n].clone() for n in ("dx", "loss", "x0")}
    Fk.ead_step(b["dx"], b["loss"], b["x0"], b["y"], b["x"], b["x_best"], b["fstate"], b["istate"], sign, kappa, R.LR,
                R.C_INIT, R.BETA, k, R.STEPS, search, R.LO, R.HI, rule, first=kind == "first",
                search_end=kind == "search_end", last=kind == "last", M=M)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(b[n]), _bits(keep[n])) for n in keep)                     # the read-only operands
    for n in OUT:
        assert (b[n][M:] == (ISENT if n == "istate" else SENT)).all(), f"{n}: the guard image was written"
    return {n: b[n][:M].cpu() for n in OUT}


def _check(dev, ops, sign, kappa, kind, rule, k=4, search=2):
    """One case: the kernel's records, resets, best-point copies and a second launch bit for bit against the float32
    reference; y, x and d_best within 4 x the reference's own deviation from float64, not below one ulp of the scale."""
    M = ops["x"].shape[0]
    w64, r32 = R.step64(ops, sign, kappa, k, search, kind, rule), R.reference32(ops, sign, kappa, k, search, kind, rule)
    got = _launch(dev, ops, sign, kappa, k, search, kind, rule)
    again = _launch(dev, ops, sign, kappa, k, search, kind, rule)
    assert all(torch.equal(_bits(got[n]), _bits(again[n])) for n in got)                   # the same operands: the same bits
    assert torch.equal(got["istate"], r32["istate"]) and torch.equal(_bits(got["fstate"]), _bits(r32["fstate"]))
    assert torch.equal(got["istate"].long(), torch.from_numpy(w64["istate"]))
    improved = torch.from_numpy(w64["istate"][:, 1] == search + 1)
    old_best = ops["x0"] if kind == "first" else ops["x_best"]
    assert torch.equal(_bits(got["x_best"]), _bits(torch.where(improved[:, None], ops["x"], old_best)))
    if kind == "search_end":
        assert torch.equal(_bits(got["x"]), _bits(ops["x0"])) and torch.equal(_bits(got["y"]), _bits(ops["x0"]))
    if kind == "last":
        assert all(torch.equal(_bits(got[n]), _bits(ops[n])) for n in ("y", "x"))
    if "branch" in w64:
        on_clean = torch.from_numpy(w64["branch"] == 0)
        assert torch.equal(_bits(got["x"])[on_clean], _bits(ops["x0"])[on_clean])
    worst = [0.0, 0.0]
    for n in ("d_best", "y", "x"):
        pick = (lambda q: np.asarray(q["fstate"])[:, 3]) if n == "d_best" else (lambda q: np.asarray(q[n]))
        want, fin = pick(w64), np.isfinite(pick(w64))
        assert (np.isfinite(pick(got)) == fin).all() and (pick(got)[~fin] == want[~fin]).all(), n
        scale = float(np.abs(want[fin]).max()) if fin.any() else 0.0
        dk, dr = (float(np.abs(pick(q)[fin].astype(np.float64) - want[fin]).max()) if fin.any() else 0.0 for q in (got, r32))
        print(f"ead_step {kind} {rule} M={M} sign={sign} kappa={kappa} {n}: kernel {dk:.3e} reference {dr:.3e} scale {scale:.3e}")
        assert dk <= max(4 * dr, float(np.spacing(np.float32(scale)))), (n, dk, dr)
        if scale:
            worst = [max(worst[0], dk / scale), max(worst[1], dr / scale)]
    return worst


@pytest.mark.parametrize("rule", ["en", "l1"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M", [1, 3, 33])
def test_ead_step_against_float64(cuda_device, M, kind, rule):
    """Largest deviations from the float64 values measured once, relative to each quantity's largest value: kernel
    1.7e-7 (x and y of a plain launch), ``ead_step_reference`` (torch float32, CPU) 1.7e-7: the two agreed bit for bit."""
    worst = [_check(cuda_device, R.make_case(M, sign, kappa, kind, rule), sign, kappa, kind, rule)
             for sign in (1, -1) for kappa in (0.0, 0.5)]
    print(f"ead_step {kind} {rule} M={M}: largest relative deviation kernel {max(w[0] for w in worst):.3e}, "
          f"reference {max(w[1] for w in worst):.3e}")


def test_nan_gradient_stays_in_its_image(cuda_device):
    ops = R.make_case(3, 1, 0.5, "plain", "en")
    base = _launch(cuda_device, ops, 1, 0.5, 4, 2, "plain", "en")
    ops["dx"][1, 5] = float("nan")
    got = _launch(cuda_device, ops, 1, 0.5, 4, 2, "plain", "en")
    for n in got:
        assert torch.equal(_bits(got[n][[0, 2]]), _bits(base[n][[0, 2]])), n
    rest = torch.arange(784) != 5                            # the image's own other elements and records too
    assert all(torch.equal(_bits(got[n][1, rest]), _bits(base[n][1, rest])) for n in R.ROWS)
    assert torch.equal(_bits(got["fstate"]), _bits(base["fstate"])) and torch.equal(got["istate"], base["istate"])


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    t = {n: v.to(dev) for n, v in R.make_case(4, 1, 0.0, "plain", "en").items()}
    keep = {n: v.clone() for n, v in t.items()}
    C, p, s = native.load(), native.ptr, native.stream_handle()
    ok = dict(dx=p(t["dx"]), loss_rows=p(t["loss"]), x0=p(t["x0"]), y=p(t["y"]), x=p(t["x"]), x_best=p(t["x_best"]),
              fstate=p(t["fstate"]), istate=p(t["istate"]), sign=1.0, kappa=0.0, c_init=1.0, lr_k=0.01, zeta_k=0.5,
              beta=0.01, beta_n=0.03, std=0.3, dist_scale=0.09, lo=R.LO, hi=R.HI, search=0, rule=0, first=False,
              search_end=False, last=False, M=4, stream=s)
    for kw in (dict(M=0), dict(M=(1 << 19) + 1), dict(sign=0.0), dict(kappa=-0.1), dict(lr_k=-1.0), dict(zeta_k=1.0),
               dict(x=ok["x"] + 4), dict(first=True, c_init=0.0), dict(first=True, last=True), dict(beta=-0.01),
               dict(fstate=ok["fstate"] + 4), dict(y=0), dict(loss_rows=ok["loss_rows"] + 2), dict(x_best=0), dict(rule=2)):
        with pytest.raises(RuntimeError):
            C.ead_step(**dict(ok, **kw))
    args = tuple(t[n] for n in ("dx", "loss", "x0", "y", "x", "x_best", "fstate", "istate"))
    for bad in (dict(sign=0), dict(kappa=-1.0), dict(lr=0.0), dict(first=True, c_init=0.0), dict(first=True, last=True),
                dict(M=5), dict(k=R.STEPS), dict(search=-1), dict(lo=1.0, hi=0.0), dict(beta=-1.0), dict(rule="l2")):
        kw = dict(sign=1, kappa=0.0, lr=0.01, c_init=1.0, beta=0.01, k=1, steps=R.STEPS, search=0, lo=R.LO, hi=R.HI)
        kw.update(bad)
        with pytest.raises(ValueError):
            Fk.ead_step(*args, **kw)
    with pytest.raises(ValueError):                          # five buffers
        Fk.ead_step(*args[:4], t["y"], *args[5:], 1, 0.0, 0.01, 1.0, 0.01, 1, R.STEPS, 0, R.LO, R.HI)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t[n]), _bits(v)) for n, v in keep.items())     # nothing ran


def _by_hand(net, x0, y, search_steps, steps, rule, sign=1, kappa=0.0):
    """The launches of ``fused_elastic_net``, one by one through ``GradChain`` and the checked entry point."""
    dev, M = x0.device, x0.shape[0]
    st = fused_state(net)
    st.sync()
    lab = torch.cat((y, y)).to(dev, torch.int32)
    xin = torch.cat((x0, x0))
    dx, x_best = (torch.full((M, 784), float("nan"), device=dev) for _ in range(2))
    fstate = torch.full((M, 4), float("nan"), device=dev)
    istate = torch.full((M, 4), ISENT, dtype=torch.int32, device=dev)
    chain = GradChain(st, 2 * M, "cw")
    loss = chain._buf.loss_rows
    for k in range(search_steps):
        for j in range(steps + 1):
            end, final = j == steps, k == search_steps - 1
            chain.run(native.ptr(xin), native.ptr(lab), 2 * M)
            chain.input_grad(native.ptr(dx), M)
            Fk.ead_step(dx, loss, x0, xin[:M], xin[M:], x_best, fstate, istate, sign, kappa, R.LR, R.C_INIT, R.BETA,
                        min(j, steps - 1), steps, k, R.LO, R.HI, rule, first=k == 0 and j == 0,
                        search_end=end and not final, last=end and final, M=M)
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
    want = _by_hand(net, x0, y, 2, 3, "en")
    assert float(want[1][1]) == 0.0 and int(want[2][1]) == 1 and torch.equal(want[0][1], x0[1])
    for rpl in (8192, 2, 8192):
        got = EAD.fused_elastic_net(net, x0, y.to(dev), 2, 3, R.LR, R.C_INIT, R.BETA, 0.0, "en", 1, R.LO, R.HI,
                                    rows_per_launch=rpl)
        assert same(got, want), rpl
    assert net.training
    for q, (val, grad) in zip(net.parameters(), before):
        assert torch.equal(q, val) and (q.grad is None) == (grad is None) and (grad is None or torch.equal(q.grad, grad))


def test_matches_cpu_reference(cuda_device):
    """``D.trained_case`` (image 1 mislabelled), search_steps = 3, steps = 30, rule l1.  The bf16 forward flips
    near-ties, so the median-L1-radius ratio GPU / CPU over the images found by both and the count of images whose
    ``found`` differs are held to twice their first measured deviations (floors 0.05 and 2).  Measured once: ratio 0.9944
    (median L1 radius 9.3712 against 9.4238), found 64 / 64 on both, 0 images differ."""
    dev = cuda_device
    pr = Predictor(copy.deepcopy(D.trained_net()).to(dev).train())
    imgs, _ = D.trained_case()
    labels, ref = R.cpu_elastic_net()
    out = pr.elastic_net(imgs.to(dev), labels.to(dev), search_steps=3, steps=30, decision_rule="l1")
    assert pr.native and out[0].shape == (64, 1, 28, 28) and out[0].is_cuda
    R.check_invariants(_PIXEL_LUT[imgs.reshape(64, 784).long()], labels.long(), out, pr.predict(imgs.to(dev)).cpu())
    radii, found = out[1].cpu(), out[3].cpu()
    both = found & ref[3]
    ratio = float(radii[both].median()) / float(ref[1][both].median())
    differ = int((found != ref[3]).sum())
    print(f"GPU EAD: found {int(found.sum())}/64 (CPU {int(ref[3].sum())}, {differ} differ), median L1 radius "
          f"{float(radii[both].median()):.4f} (CPU {float(ref[1][both].median()):.4f}), ratio {ratio:.4f}")
    assert abs(ratio - 1.0) <= max(2 * RATIO_FIRST, RATIO_FLOOR), ratio
    assert differ <= max(2 * FOUND_DIFF_FIRST, FOUND_FLOOR), differ
