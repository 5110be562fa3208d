"""CROWN-IBP on the GPU (MI355X only): each kernel alone against the float64 oracle from the oracle's float32-rounded
inputs (the backward kernels from the float32 record), batch independence, and ``certified_radius_linf(method=
"crown-ibp")`` end to end against the oracle."""
import copy
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.ops import crown as CROWN
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

import crown_ref as CR
import ibp_ref as R

pytestmark = pytest.mark.gpu
SENT = -7.25
_bits = lambda t: t.contiguous().view(torch.int32)                                          # noqa: E731


def _hold(name, got, ref, want):
    """The project's rule: the kernel's deviation from float64 at most 4 x the float32 CPU reference's on the same
    inputs, or one ulp of the quantity's largest value."""
    (dk, scale), (dr, _) = R.worst(got, want), R.worst(ref, want)
    print(f"{name}: kernel {dk:.3e} reference {dr:.3e} scale {scale:.3e}")
    assert dk <= max(4 * dr, R.ulp(scale)), (name, dk, dr, scale)


@functools.lru_cache(maxsize=None)
def _inputs(M, kind):
    """The oracle at ``CR.case(M)`` and its float32-rounded stage inputs, shared by the kernels' cases; never modified."""
    x, y, eps = CR.case(M)
    n = R.net(kind)
    want = CR.oracle(n, x, y, eps)
    b1 = R._P(n)["fc1.bias"]
    i = dict(x=x, y=y, eps=eps, want=want, rec={k: want[k].float() for k in ("sL", "sU", "bU")},
             z1c=((want["l3"] + want["u3"]) / 2 - b1).float(), z1r=((want["u3"] - want["l3"]) / 2).float(),
             lam=want["lam"].float(), v=want["v"].float(), fcb=want["fcb"].float(), sp=want["sp"].float(),
             vb=want["vb"].float(), lb_ibp=want["lb_ibp"].float())
    i["rec"]["istar"] = want["istar"]
    i["rec4"] = torch.stack((i["rec"]["sL"], i["rec"]["sU"], i["rec"]["bU"], want["istar"].int().view(torch.float32)), dim=2)
    return i


def _run(kernel, i, M, kind, dev, param):
    """One launch of ``kernel`` with a sentinel image past M: {output: (kernel rows [M + 1], reference, oracle)}."""
    n, y32 = R.net(kind), torch.cat([i["y"], torch.zeros(1, dtype=torch.long)]).to(dev, torch.int32)
    g = lambda t: torch.cat([t.float(), torch.full((1,) + t.shape[1:], SENT)]).to(dev).contiguous()   # noqa: E731
    s = lambda *shape: torch.full((M + 1,) + shape, SENT, device=dev)                                 # noqa: E731
    rec = g(torch.stack((i["eps"],) + (torch.zeros(M),) * 3, dim=1))
    P = Fk._ibp_setup(n, torch.float32, None, None)[0]
    if kernel == "relax":
        pl, pu, rx = Fk.crown_relax(param, g(i["x"]), rec, s(9216), s(9216), s(9216, 4), M=M)
        ref, want = Fk.crown_ibp_reference(n, i["x"], i["y"], i["eps"]), i["want"]
        got = Fk._crown_rec(rx[:M].cpu())
        hold = CR.check_record(got, want, M)
        out = {k: (torch.cat([got[k] * hold, rx[M:, :, 0].cpu()]), ref[k] * hold, want[k] * hold) for k in ("sU", "bU")}
        return dict(out, pl=(pl, ref["pl"], want["pl"]), pu=(pu, ref["pu"], want["pu"]), rx=(rx, None, None))
    if kernel == "lambda":
        part = torch.zeros(Fk.IBP_SPLITS, M, 2, 128)
        part[0, :, 0], part[0, :, 1] = i["z1c"], i["z1r"]
        lam, fcb = Fk.crown_lambda(param, part.to(dev), y32, s(16, 128), s(2, 16), M=M)
        b1 = R._P(n)["fc1.bias"]
        w = CR.fc_part(n, i["z1c"].double() - i["z1r"].double() + b1, i["z1c"].double() + i["z1r"].double() + b1, i["y"])
        r = Fk.crown_lambda_reference(P, i["z1c"], i["z1r"], i["y"])
        ibp = R.from_fc1(n, i["z1c"], i["z1r"], i["y"])
        ribp = Fk.ibp_head_reference(n, part, i["y"])
        return dict(lam=(lam, r[0], w[0]), fcb=(fcb[:, 0, :10], r[1], w[1]), lb_ibp=(fcb[:, 1, :10], ribp, ibp))
    if kernel == "fc":
        v, vb = Fk.crown_fc(param, g(i["rec4"]), g(i["lam"]), s(10, 9216), s(576, 16), M=M)
        w, r = CR.pool_part(n, i["lam"], i["rec"]), Fk.crown_fc_reference(P, i["lam"], *(i["rec"][k] for k in ("sL", "sU", "bU")))
        assert (vb[:, :, 10:] == SENT).all()
        return dict(v=(v, r[0], w[0]), vb=(vb[:, :, :10], r[1], w[1]))
    if kernel == "bwd":
        sp = Fk.crown_bwd(param, g(i["x"]), rec, g(i["rec4"]), g(i["v"]), y32, s(7, 10, 2), M=M)
        _, xl, xu, pre1 = Fk.crown_box_reference(n, i["x"], i["eps"])
        return dict(sp=(sp, Fk.crown_bwd_reference(P, xl, xu, pre1, i["v"], i["rec"]["istar"]),
                        CR.trunk_part(n, i["want"], i["v"], i["rec"]["istar"])))
    fcb = torch.zeros(M, 2, 16)
    fcb[:, 0, :10], fcb[:, 1, :10] = i["fcb"], i["lb_ibp"]
    lbc, lb = s(10), s(10)
    Fk.crown_head(g(fcb), g(torch.nn.functional.pad(i["vb"], (0, 6))), g(i["sp"]), y32, rec, lb, lbc, M=M)
    w, r = CR.head_part(i["fcb"], i["vb"], i["sp"], i["lb_ibp"], i["y"]), Fk.crown_head_reference(i["fcb"], i["vb"], i["sp"], i["lb_ibp"], i["y"])
    assert torch.equal(_bits(rec), _bits(g(torch.stack((i["eps"],) + (torch.zeros(M),) * 3, dim=1))))
    return dict(lb_crown=(lbc, r[0], w[0]), lb=(lb, r[1], w[1]))


@pytest.mark.parametrize("kind", ["random", "trained"])
@pytest.mark.parametrize("M", [1, 3, 17])
@pytest.mark.parametrize("kernel", ["relax", "lambda", "fc", "bwd", "head"])
def test_kernel_against_float64(cuda_device, kernel, M, kind):
    """Largest deviations measured once (kernel / float32 CPU reference, absolute): see docs/COVERAGE.md."""
    dev = cuda_device
    net = copy.deepcopy(R.net(kind)).to(dev)
    param = fused_state(net).ms.param
    i = _inputs(M, kind)
    first, again = _run(kernel, i, M, kind, dev, param), _run(kernel, i, M, kind, dev, param)
    for k, (got, ref, want) in first.items():
        assert torch.equal(_bits(got), _bits(again[k][0])) and (got[M] == SENT).all(), k
        if ref is not None:
            _hold(f"crown_{kernel} M={M} {kind} {k}", got[:M], ref, want)


def test_bound_does_not_depend_on_the_batch(cuda_device):
    dev = cuda_device
    net = copy.deepcopy(R.net("trained")).to(dev)
    x, y, _ = R.case(40)
    rows = torch.tensor([0, 7, 16, 23, 39])
    big = CROWN.fused_crown_ibp_radius(net, x.to(dev), y.to(dev), 0.1, 4)
    small = CROWN.fused_crown_ibp_radius(net, x[rows].to(dev), y[rows].to(dev), 0.1, 4, rows_per_launch=2)
    assert torch.equal(_bits(small), _bits(big[rows.to(dev)]))
    big = CROWN.fused_crown_ibp(net, x.to(dev), y.to(dev), 0.003)
    small = CROWN.fused_crown_ibp(net, x[rows].to(dev), y[rows].to(dev), 0.003, rows_per_launch=2)
    assert torch.equal(_bits(small), _bits(big[rows.to(dev)]))


def test_certified_radius_end_to_end(cuda_device):
    """``trained_case``, eps_max = 0.1, 10 bisections: the oracle (from the float32 reference's record at that eps) at
    the GPU's own ``lo`` gives min lb >= -tau and at its own ``hi`` min lb <= tau for every image, tau = 4 x the float32
    reference's deviation from the oracle at that eps, or an ulp of the bounds' scale; no radius below IBP's; the
    median (a measurement, see the README) above IBP's."""
    dev = cuda_device
    net = copy.deepcopy(R.net("trained")).to(dev)
    imgs, labels = R.trained_case()
    x, y, _ = R.case(64)
    pr = Predictor(net, dtype="fp32")
    radii, cert, _ = pr.certified_radius_linf(imgs.to(dev), labels.to(dev), 0.1, 10, method="crown-ibp")
    ibp = pr.certified_radius_linf(imgs.to(dev), labels.to(dev), 0.1, 10, method="ibp")[0]
    rec = CROWN.fused_crown_ibp_radius(net, x.to(dev), y.to(dev), 0.1, 10).cpu()
    assert torch.equal(radii.cpu(), rec[:, 1]) and torch.equal(cert.cpu(), rec[:, 1] > 0)
    for col, sign in ((1, 1.0), (2, -1.0)):
        eps = rec[:, col]
        ref = Fk.crown_ibp_reference(R.net("trained"), x, y, eps)
        want = CR.oracle(R.net("trained"), x, y, eps, rec=ref)["lb"]
        for i in range(64):
            dr, scale = R.worst(ref["lb"][i], want[i])
            tau = max(4 * dr, R.ulp(scale))
            assert sign * float(want[i].min()) >= -tau, (i, col, float(eps[i]), float(want[i].min()), tau)
    print(f"CROWN-IBP certified radius: median {float(radii.median()):.5f} (IBP {float(ibp.median()):.5f}), "
          f"certified {int(cert.sum())}/64")
    assert bool((radii >= ibp).all()) and float(radii.median()) > float(ibp.median())
