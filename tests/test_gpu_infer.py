"""The single-launch fused inference forward (csrc/kernels/infer_fwd.hip) and the Predictor on the GPU.

Model and data: ``test_gpu_numerics._setup``'s seeded ``Net()`` and ``generate(B, seed=5)``, except that
the net first takes 32 seeded Adadelta steps on the CPU (batch 64 of ``generate(1024, seed=11)``).  The
freshly initialised net puts 87-100 % of the rows under the 0.1 top-2 margin for every data seed tried
(5, 6, 7), so the argmax rule below would check almost nothing; after the 32 steps 0-7 % of the rows are
under it at every batch size used here (checked on the CPU; ``_check`` asserts the 10 % cap on the
reference itself).  Tolerances are the existing eval path's (test_eval_forward_matches_fp32_reference);
rounding a1 / w2 / p / w1 to bf16 in an fp32 CPU forward of this net moves the log-probs by at most
0.009, so they are no looser for it than for the untrained net.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd import inference
from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk

from refmodel import reference_forward, rel_err

pytestmark = pytest.mark.gpu

MARGIN = 0.1            # twice the absolute log-prob tolerance: a different argmax above it is a real error


@functools.lru_cache(maxsize=None)
def _trained_net():
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(1024, seed=11)
    x, y = normalize_u8(imgs), labels.long()
    opt = torch.optim.Adadelta(net.parameters(), lr=1.0)
    net.train()
    with torch.enable_grad():
        for step in range(32):
            i = (step * 64) % 1024
            opt.zero_grad()
            F.nll_loss(net.forward_reference(x[i:i + 64]), y[i:i + 64]).backward()
            opt.step()
    return net.eval()


@functools.lru_cache(maxsize=None)
def _case(B, n=None):
    """uint8 images [n or B, 28, 28], labels, and the fp32 CPU reference log-probs (computed once)."""
    imgs, labels = generate(n or B, seed=5)
    with torch.no_grad():
        lp_ref = reference_forward(_trained_net(), normalize_u8(imgs), train=False)
    return imgs, labels, lp_ref


@pytest.fixture(scope="module")
def ms(cuda_device):
    return ModelState(copy.deepcopy(_trained_net()), cuda_device)


def _check(lp, pred, lp_ref, labels=None, loss_rows=None, correct=None):
    lp, pred = lp.cpu(), pred.cpu().long()
    assert torch.isfinite(lp).all()
    err = (lp - lp_ref).abs().max().item()
    rel = rel_err(lp, lp_ref)
    top2 = lp_ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > MARGIN
    print(f"B={lp.shape[0]} max|dlogp|={err:.5f} rel_err={rel:.6f} rows under margin={int((~clear).sum())}")
    assert err < 5e-2, err
    assert rel < 1e-2, rel
    assert (~clear).float().mean().item() <= 0.10
    assert torch.equal(pred[clear], lp_ref.argmax(1)[clear])
    if labels is not None:
        nll_ref = -lp_ref.gather(1, labels.view(-1, 1).long()).squeeze(1)
        assert (loss_rows.cpu() - nll_ref).abs().max().item() < 5e-2
        assert torch.equal(correct.cpu().long(), (pred == labels.long()).long())


def _run(ms, buf, B, dev, form="u8", labels=True):
    imgs, lab, lp_ref = _case(B)
    kw = {}
    if form == "u8":
        kw["u8"] = imgs.reshape(B, 784).contiguous().to(dev)
    else:
        kw["x"] = normalize_u8(imgs).reshape(B, 784).contiguous().to(dev)
    if labels:
        kw["labels"] = lab.to(torch.int32).to(dev)
    Fk.infer_forward(ms, buf, B, **kw)
    torch.cuda.synchronize()
    return lab, lp_ref


@pytest.mark.parametrize("B,form", [(1, "u8"), (2, "u8"), (15, "u8"), (16, "u8"), (17, "u8"), (17, "x"),
                                    (33, "u8"), (200, "u8"), (345, "x")])
def test_infer_forward_matches_fp32_reference(cuda_device, ms, B, form):
    # 33: two images per workgroup with a one-image last group; 200: ten per workgroup; 345: sixteen,
    # with nine in the last group
    buf = Fk.InferBuffers.allocate(B, cuda_device)
    lab, lp_ref = _run(ms, buf, B, cuda_device, form)
    _check(buf.logp[:B], buf.pred[:B], lp_ref, lab, buf.loss_rows[:B], buf.correct[:B])


@pytest.mark.parametrize("B", [17, 200])
def test_infer_forward_agrees_with_three_launch_path(cuda_device, ms, B):
    imgs, lab, lp_ref = _case(B)
    u8 = imgs.reshape(B, 784).contiguous().to(cuda_device)
    lab32 = lab.to(torch.int32).to(cuda_device)
    old = Fk.StepBuffers.allocate(B, cuda_device)
    Fk.eval_forward(ms, u8, lab32, torch.arange(B, dtype=torch.int32, device=cuda_device), old)
    buf = Fk.InferBuffers.allocate(B, cuda_device)
    Fk.infer_forward(ms, buf, B, u8=u8, labels=lab32)
    torch.cuda.synchronize()
    _check(buf.logp[:B], buf.pred[:B], lp_ref, lab, buf.loss_rows[:B], buf.correct[:B])
    _check(old.logp, old.logp.argmax(1), lp_ref)
    clear = (lp_ref.topk(2, dim=1).values @ torch.tensor([1.0, -1.0])) > MARGIN
    assert torch.equal(buf.pred[:B].cpu().long()[clear], old.logp.argmax(1).cpu()[clear])


def test_infer_forward_invariants(cuda_device, ms):
    """(a) partials written, not accumulated; (b) same bits on every launch; (c) tickets back to zero
    with no host reset; (d) rows >= B untouched; (e) ragged groups and B = 1."""
    maxB, pad = 33, 8
    buf = Fk.InferBuffers.allocate(maxB + pad, cuda_device)
    buf.z1part.fill_(float("nan"))
    buf.logp.fill_(-777.0); buf.loss_rows.fill_(-777.0)
    buf.pred.fill_(-777); buf.correct.fill_(-777)
    first = None
    for B in (17, 1, 33, 17):
        lab, lp_ref = _run(ms, buf, B, cuda_device)
        assert int(buf.tickets.abs().sum().item()) == 0
        _check(buf.logp[:B], buf.pred[:B], lp_ref, lab, buf.loss_rows[:B], buf.correct[:B])
        if B == 17:
            got = (buf.logp[:B].clone(), buf.pred[:B].clone(), buf.loss_rows[:B].clone(), buf.correct[:B].clone())
            if first is None:
                first = got
            else:
                assert all(torch.equal(a, b) for a, b in zip(first, got))
    # rows past the largest batch were never written (sentinels), by any of the four launches
    assert (buf.logp[maxB:] == -777.0).all() and (buf.loss_rows[maxB:] == -777.0).all()
    assert (buf.pred[maxB:] == -777).all() and (buf.correct[maxB:] == -777).all()
    # ... and a launch leaves the rows past its own B alone
    buf.logp.fill_(-777.0); buf.pred.fill_(-777); buf.loss_rows.fill_(-777.0); buf.correct.fill_(-777)
    _run(ms, buf, 17, cuda_device)
    assert (buf.logp[17:] == -777.0).all() and (buf.pred[17:] == -777).all()
    assert (buf.loss_rows[17:] == -777.0).all() and (buf.correct[17:] == -777).all()
    assert torch.isfinite(buf.logp[:17]).all()


def test_infer_forward_graph_replay(cuda_device, ms):
    B = 17
    imgs, _, _ = _case(B, n=4 * B)
    rows = imgs.reshape(4 * B, 784).contiguous().to(cuda_device)
    eager = Fk.InferBuffers.allocate(B, cuda_device)
    want = []
    for r in range(1, 4):
        Fk.infer_forward(ms, eager, B, u8=rows[r * B:(r + 1) * B])
        torch.cuda.synchronize()
        want.append((eager.logp.clone(), eager.pred.clone()))
    buf = Fk.InferBuffers.allocate(B, cuda_device)
    u8 = rows[:B].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        Fk.infer_forward(ms, buf, B, u8=u8)                   # warm-up launch on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            Fk.infer_forward(ms, buf, B, u8=u8)               # one kernel node: a chain with no branches
    torch.cuda.current_stream().wait_stream(side)
    for r in range(1, 4):
        u8.copy_(rows[r * B:(r + 1) * B])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.logp, want[r - 1][0]) and torch.equal(buf.pred, want[r - 1][1])
        assert int(buf.tickets.abs().sum().item()) == 0


def test_infer_forward_index_form(cuda_device, ms):
    imgs, lab, _ = _case(64)
    rows = imgs.reshape(64, 784).contiguous().to(cuda_device)
    lab32 = lab.to(torch.int32).to(cuda_device)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0))[:40]
    idx = perm.to(torch.int32).to(cuda_device)
    a = Fk.InferBuffers.allocate(40, cuda_device)
    b = Fk.InferBuffers.allocate(40, cuda_device)
    Fk.infer_forward(ms, a, 40, u8=rows, idx=idx, labels=lab32)                    # labels per data row
    Fk.infer_forward(ms, b, 40, u8=rows[perm.to(cuda_device)].contiguous(), labels=lab32[idx.long()].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(a.logp).all()
    assert torch.equal(a.logp, b.logp) and torch.equal(a.pred, b.pred)
    assert torch.equal(a.loss_rows, b.loss_rows) and torch.equal(a.correct, b.correct)


@pytest.mark.parametrize("edge", ["shipped", 32])
def test_predictor_dispatch(cuda_device, monkeypatch, edge):
    """Both sides of INFER_FUSED_MAX_B: the shipped constant (patched down to 32 above 272; at 0 only the
    three-launch side exists), and 32 so that the fused side runs through the Predictor whatever ships."""
    if edge != "shipped" or inference.INFER_FUSED_MAX_B > 272:
        monkeypatch.setattr(inference, "INFER_FUSED_MAX_B", 32)
    net = copy.deepcopy(_trained_net()).to(cuda_device)
    pr = Predictor(net)
    assert pr.native
    edge = inference.INFER_FUSED_MAX_B
    for B in ([edge, edge + 1] if edge > 0 else [1]):
        imgs, lab, lp_ref = _case(B)
        for x in (imgs, normalize_u8(imgs)):                   # uint8 [B,28,28] and float [B,1,28,28]
            _check(pr.log_probs(x), pr.predict(x), lp_ref)
        assert (pr._infer_buf is not None) == (edge > 0) and (pr._eval_buf is not None) == (B > edge)
        loss_sum, correct, n = pr.evaluate(imgs, lab, batch_size=B)
        nll_ref = -lp_ref.gather(1, lab.view(-1, 1).long()).sum().item()
        assert n == B and abs(loss_sum - nll_ref) < 5e-2 * B
        assert correct == int((pr.predict(imgs).cpu() == lab.long()).sum())
    # a live Net: an in-place parameter edit is picked up by the next call
    imgs, _, _ = _case(17)
    before = pr.log_probs(imgs)
    net.fc2.bias.data.add_(1.0)
    net.fc2.bias.data[3] += 4.0
    ref = Net()
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    with torch.no_grad():
        lp_ref = reference_forward(ref, normalize_u8(imgs), train=False)
    after = pr.log_probs(imgs)
    assert not torch.equal(before, after)
    assert (after.cpu() - lp_ref).abs().max().item() < 5e-2
