"""Interval bound propagation on the GPU (MI355X only): each kernel alone against the float64 oracle from the oracle's
float32-rounded inputs, the record update, batch independence of the radius search, ``Predictor.certified_radius_linf``
end to end against the oracle, and the launcher refusals."""
import copy

import pytest
import torch

from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import ibp as IBP
from pytorch_mnist_ddp_amd.ops import native
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

import ibp_ref as R

pytestmark = pytest.mark.gpu
SENT = -7.25
_bits = lambda t: t.contiguous().view(torch.int32)                                          # noqa: E731
S = Fk.IBP_SPLITS


def _gpu_net(kind, dev):
    net = copy.deepcopy(R.net(kind)).to(dev)
    return net, fused_state(net).ms.param


def _guarded(t, dev, extra):
    """``t`` flattened on the GPU with ``extra`` sentinel entries after it."""
    return torch.cat([t.reshape(-1).float(), torch.full((extra,), SENT)]).to(dev)


def _hold(name, got, ref, want):
    """The project's rule: the kernel's deviation from float64 at most 4 x the float32 CPU reference's on the same
    launch, or one ulp of the quantity's largest value."""
    (dk, scale), (dr, _) = R.worst(got, want), R.worst(ref, want)
    print(f"{name}: kernel {dk:.3e} reference {dr:.3e} scale {scale:.3e}")
    assert dk <= max(4 * dr, R.ulp(scale)), (name, dk, dr, scale)


@pytest.mark.parametrize("kind", ["random", "trained"])
@pytest.mark.parametrize("M", [1, 3, 17])
def test_stages_against_float64(cuda_device, M, kind):
    """Largest deviations measured once (kernel / float32 CPU reference, absolute): see the README's IBP section."""
    dev = cuda_device
    net, param = _gpu_net(kind, dev)
    x, y, eps = R.case(M)
    want = R.oracle(R.net(kind), x, y, eps)
    rec = torch.zeros(M + 1, 4)
    rec[:M, 0], rec[M] = eps, SENT
    rec_d = rec.to(dev)

    def trunk():
        pl, pu = (torch.full((M + 1, 9216), SENT, device=dev) for _ in range(2))
        Fk.ibp_trunk(param, _guarded(x, dev, 784).view(M + 1, 784), rec_d, pl, pu, M=M)
        return pl, pu
    (pl, pu), again = trunk(), trunk()
    ref = Fk.ibp_trunk_reference(R.net(kind), x, eps)
    for k, g, a, r in (("pl", pl, again[0], ref[0]), ("pu", pu, again[1], ref[1])):
        assert (g[M] == SENT).all() and torch.equal(_bits(g), _bits(a))
        _hold(f"ibp_trunk M={M} {kind} {k}", g[:M], r, want[k])
    assert torch.equal(_bits(rec_d), _bits(rec.to(dev)))

    pl32, pu32 = want["pl"].float(), want["pu"].float()                      # fc1 from the oracle's rounded bounds
    w1 = R.from_pool(R.net(kind), pl32, pu32, y)

    def fc1():
        part = torch.full((S * M * 256 + 256,), SENT, device=dev)
        Fk.ibp_fc1(param, _guarded(pl32, dev, 9216), _guarded(pu32, dev, 9216), part, M=M)
        return part
    part, again = fc1(), fc1()
    assert (part[S * M * 256:] == SENT).all() and torch.equal(_bits(part), _bits(again))
    z = part[:S * M * 256].view(S, M, 2, 128).double().sum(dim=0).cpu()        # (the float64 sum of the float32 partials)
    ref = Fk.ibp_fc1_reference(R.net(kind), pl32, pu32)
    _hold(f"ibp_fc1 M={M} {kind} z1c", z[:, 0], ref[0], w1["z1c"])
    _hold(f"ibp_fc1 M={M} {kind} z1r", z[:, 1], ref[1], w1["z1r"])

    p32 = torch.zeros(S, M, 2, 128)                                            # the head from the oracle's rounded sums
    p32[0, :, 0], p32[0, :, 1] = w1["z1c"].float(), w1["z1r"].float()
    w2 = R.from_fc1(R.net(kind), p32[0, :, 0], p32[0, :, 1], y)

    def head():
        lb = torch.full((M + 1, 10), SENT, device=dev)
        Fk.ibp_head(param, p32.to(dev), _guarded(y, dev, 1).to(torch.int32), rec_d, lb, M=M)
        return lb
    lb, again = head(), head()
    assert (lb[M] == SENT).all() and torch.equal(_bits(lb), _bits(again)) and torch.equal(_bits(rec_d), _bits(rec.to(dev)))
    _hold(f"ibp_head M={M} {kind} lb", lb[:M], Fk.ibp_head_reference(R.net(kind), p32, y), w2)


def test_record_update_is_the_reference_on_the_kernels_own_lb(cuda_device):
    """First and later rounds; certified, uncertified and NaN rows: a pure function of ``lb``, bit for bit."""
    dev = cuda_device
    net, param = _gpu_net("trained", dev)
    x, y, _ = R.case(4)
    x = x.clone()
    x[3, 100] = float("nan")
    rec = torch.tensor([[0.1, 0.0, 0.1, 0.0], [0.0, 0.0, 0.00625, 1.0], [0.05, 0.0, 0.1, -3.0], [1e-4, 0.0, 0.1, 0.0],
                        [SENT] * 4]).to(dev)
    pl, pu = Fk.ibp_trunk(param, x.to(dev), rec, M=4)
    part = Fk.ibp_fc1(param, pl, pu, M=4)
    before = rec.clone()
    lb = Fk.ibp_head(param, part, y.to(dev, torch.int32), rec, search=True, M=4)
    want = Fk.ibp_search_reference(before[:4].cpu(), lb.cpu())
    cert = lb.cpu().min(dim=1).values > 0
    assert cert.tolist() == [False, True, False, False] and torch.isnan(lb[3]).any() and not torch.isnan(lb[:3]).any()
    got = rec[:4].cpu()
    assert torch.equal(_bits(got[:3]), _bits(want[:3])) and torch.equal(_bits(got[3, :3]), _bits(want[3, :3]))
    assert torch.isnan(got[3, 3]) and torch.isnan(want[3, 3]) and (rec[4] == SENT).all()    # (a NaN's payload is not held)


def test_radius_search_does_not_depend_on_the_batch(cuda_device):
    dev = cuda_device
    net, _ = _gpu_net("trained", dev)
    x, y, _ = R.case(40)
    big = IBP.fused_ibp_radius(net, x.to(dev), y.to(dev), 0.1, 4)
    rows = torch.tensor([0, 7, 16, 23, 39])
    small = IBP.fused_ibp_radius(net, x[rows].to(dev), y[rows].to(dev), 0.1, 4, rows_per_launch=2)
    assert torch.equal(_bits(small), _bits(big[rows.to(dev)]))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_certified_radius_end_to_end(cuda_device, dtype):
    """``trained_case``, eps_max = 0.1, 10 bisections: the oracle at the GPU's own ``lo`` gives min lb >= -tau and at its
    own ``hi`` min lb <= tau for every image, tau = 4 x the float32 reference's deviation from the oracle at that eps,
    or an ulp of the bounds' scale.  Median radius measured once: see the README (float64 on the CPU: 0.0021)."""
    dev = cuda_device
    net = copy.deepcopy(R.net("trained")).to(dev)
    imgs, labels = R.trained_case()
    x, y, _ = R.case(64)
    radii, cert, _ = Predictor(net, dtype=dtype).certified_radius_linf(imgs.to(dev), labels.to(dev), 0.1, 10)
    rec = IBP.fused_ibp_radius(net, x.to(dev), y.to(dev), 0.1, 10).cpu()
    assert torch.equal(radii.cpu(), rec[:, 1]) and torch.equal(cert.cpu(), rec[:, 1] > 0)
    for col, sign in ((1, 1.0), (2, -1.0)):
        eps = rec[:, col]
        want = R.oracle(R.net("trained"), x, y, eps)["lb"]
        ref = Fk.ibp_reference(R.net("trained"), x, y, eps)["lb"]
        for i in range(64):
            dr, scale = R.worst(ref[i], want[i])
            tau = max(4 * dr, R.ulp(scale))
            assert sign * float(want[i].min()) >= -tau, (i, col, float(eps[i]), float(want[i].min()), tau)
    print(f"IBP certified radius ({dtype} predictor): median {float(radii.median()):.5f}, certified {int(cert.sum())}/64")


def test_launcher_refusals_make_no_launch(cuda_device):
    dev = cuda_device
    _, param = _gpu_net("trained", dev)
    t = {k: torch.full(shape, SENT, device=dev) for k, shape in
         (("x", (2, 784)), ("rec", (2, 4)), ("pl", (2, 9216)), ("pu", (2, 9216)), ("part", (S * 512,)), ("lb", (2, 10)))}
    lab = torch.zeros(2, dtype=torch.int32, device=dev)
    C, s = native.load(), native.stream_handle()
    a = {k: native.ptr(v) for k, v in dict(t, param=param, labels=lab).items()}
    trunk = dict(param=a["param"], x0=a["x"], rec=a["rec"], pl=a["pl"], pu=a["pu"], pix_std=0.3081, lo=-0.5, hi=3.0, B=2, stream=s)
    fc1 = dict(param=a["param"], pl=a["pl"], pu=a["pu"], part=a["part"], B=2, stream=s)
    head = dict(param=a["param"], part=a["part"], labels=a["labels"], lb=a["lb"], rec=a["rec"], search=True, B=2, stream=s)
    for fn, ok, bad in ((C.ibp_trunk, trunk, (dict(B=0), dict(x0=0), dict(pl=a["pl"] + 4), dict(rec=0), dict(lo=4.0))),
                        (C.ibp_fc1, fc1, (dict(B=0), dict(B=1 << 16), dict(part=0), dict(pu=a["pu"] + 4))),
                        (C.ibp_head, head, (dict(B=-1), dict(labels=0), dict(labels=a["labels"] + 2), dict(rec=a["rec"] + 4)))):
        for kw in bad:
            with pytest.raises(RuntimeError):
                fn(**dict(ok, **kw))
    with pytest.raises(ValueError):
        Fk.ibp_trunk(param, t["x"], t["rec"], t["pl"], t["pl"])
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in t.values())
