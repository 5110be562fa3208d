"""T1: every bf16 forward kernel on its own against the float64 stage oracle (MI355X only).

trunk_fwd, fc1_fwd, head_train, head_eval and head_fwd are launched one at a time; each is compared
with tests/refmodel.py's oracle applied to that kernel's own device inputs, copied back, so nothing
cascades.  Rounded outputs are held element by element to the bf16 rounding of the oracle
(assert_rounded_bf16, nothing excluded), discrete outputs wherever the oracle's margin decides them
(assert_decisions, at most 1e-3 excluded), with every eps measured at run time as 8 x the deviation of
torch's fp32 CPU op from float64 on the same operands.  tests/test_forward_oracle_cpu.py proves on the
CPU that these checks fail on subtly wrong outputs.  Each test prints `stage B tensor deviation eps`
(docs/COVERAGE.md 2.4 records the table).
"""
import copy
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.engine.state import FLAG_NO_DROPOUT, ModelState
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native

import refmodel as R
from refmodel import FWD_RNG_BASE, FWD_SEED, FWD_STEP, bf16_round

pytestmark = pytest.mark.gpu

OFF1 = FWD_RNG_BASE + 2 * FWD_STEP           # dropout-1 offset at step 3; dropout-2 draws at OFF1 + 1
SENT = 0x7FC1                                # bf16 NaN sentinel bits


def _report(stage, B, stats):
    for name, (dev, eps) in stats.items():
        print(f"\n{stage:22s} B={B:<5d} {name:18s} dev {dev:10.3e}  eps {eps:10.3e}", end="")


def _sentinel(*tensors):
    for t in tensors:
        if t.dtype == torch.bfloat16:
            t.view(torch.int16).fill_(SENT)
        elif t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(0xAA)
        else:
            t.fill_(-0x55555556)             # 0xAAAAAAAA


def _is_sentinel(t):
    return bool((t.view(torch.int16) == SENT).all())


class Box:
    """Model state, dataset, index vector and buffers of one batch size on the device, and the kernels'
    own operands copied back (fp32 parameters, the bf16 shadows in torch layouts)."""

    def __init__(self, dev, B, trained=False, step=FWD_STEP, flags=0):
        if trained:
            net = copy.deepcopy(R.trained_net())
        else:
            torch.manual_seed(1)
            net = Net()
        self.dev, self.B = dev, B
        self.ms = ModelState(net, dev)
        self.ms.set_state(step, seed=FWD_SEED, rng_base=FWD_RNG_BASE, flags=flags)
        self.step = step
        self.imgs, self.labels, self.idx = R.forward_case(B)
        self.u8 = self.imgs.reshape(-1, 784).contiguous().to(dev)
        self.lab_d = self.labels.to(torch.int32).to(dev)
        self.idx_d = self.idx.to(torch.int32).to(dev)
        self.buf = Fk.StepBuffers.allocate(B, dev)
        self.rows = R.check_rows(B)
        self.rows_d = torch.tensor(self.rows, device=dev)
        self.d = {n: v.detach().cpu().clone() for n, v in self.ms.views(self.ms.param).items()}
        self.d["w2q"] = self.ms.w2f.cpu().view(64, 3, 3, 32).permute(0, 3, 1, 2).contiguous()   # [co][tap][ci]
        self.d["w1q"] = self.ms.w1.cpu().view(128, 9216)
        assert torch.equal(self.d["w2q"], bf16_round(self.d["conv2.weight"]))
        self.ks = R.fc1_ksplit(B)
        self.inv = float(torch.tensor(1.0 / B, dtype=torch.float32))

    def src_rows(self, step=None):
        """Dataset rows that the checked batch rows read at `step` with idx_stride = B."""
        return self.idx[(self.step if step is None else step) * self.B + torch.tensor(self.rows)]

    def x_rows(self, src):
        return normalize_u8(self.imgs[src]).reshape(len(src), 784)

    def keep1(self):
        return R.keep_rows(OFF1, self.rows, 9216, 192)

    def keep2(self):
        return R.keep_rows(OFF1 + 1, self.rows, 128, 128)

    # ---- launches: sentinel first, one kernel, copy the checked rows back
    def trunk(self, train=True, idx=True, stride=None, xin=None):
        buf, B = self.buf, self.B
        _sentinel(buf.a1, buf.p, buf.pmask)
        stride = B if stride is None else stride
        if xin is None:
            Fk.trunk_fwd(self.ms, self.u8, self.idx_d if idx else None, buf, train, stride)
        else:                                 # the module-API entry: fp32 normalised rows, no wrapper
            p, o, ms = native.ptr, self.ms.offsets, self.ms
            native.load().trunk_fwd(0, 0, 0, p(ms.state), p(ms.param) + 4 * o["conv1.weight"],
                                    p(ms.param) + 4 * o["conv1.bias"], p(ms.w2f), p(ms.param) + 4 * o["conv2.bias"],
                                    p(buf.a1) if train else 0, p(buf.p), p(buf.pmask) if train else 0, B, train,
                                    native.stream_handle(), xin=p(xin))
        torch.cuda.synchronize()
        assert _is_sentinel(buf.p[B:]), "trunk_fwd wrote p rows past B"
        out = dict(p=buf.p[self.rows_d].cpu())
        if train:
            out["a1"] = buf.a1[self.rows_d].cpu()
            out["pm"] = Fk.pmask_flat(buf.pmask)[self.rows_d].cpu()
        else:                                 # null a1 / pmask pointers: nothing may be stored
            assert _is_sentinel(buf.a1) and bool((buf.pmask == 0xAA).all())
        return out

    def fc1(self):
        buf, B = self.buf, self.B
        buf.p[B:].zero_()
        _sentinel(buf.z1part)
        Fk.fc1_fwd(self.ms, buf)
        torch.cuda.synchronize()
        flat = buf.z1part.view(-1)
        assert torch.isnan(flat[self.ks * B * 128:]).all(), "fc1_fwd wrote past [ksplit][B][128]"
        return flat[:self.ks * B * 128].view(self.ks, B, 128)[:, self.rows_d].cpu()

    def head_train(self, idx=True):
        buf, B = self.buf, self.B
        _sentinel(buf.loss_rows, buf.dz1, buf.h_bf, buf.dl_bf)
        if idx:
            Fk.head_train(self.ms, self.lab_d, self.idx_d, buf, B)
        else:                                 # pre-gathered labels: row b of step s reads labels[s*B + b]
            Fk.head_train(self.ms, self.lab_d[self.idx_d.long()].contiguous(), None, buf, B)
        torch.cuda.synchronize()
        return dict(loss_rows=buf.loss_rows[self.rows_d].cpu(), dz1=buf.dz1.cpu(), h_bf=buf.h_bf.cpu(),
                    dl_bf=buf.dl_bf.cpu())

    def check_trunk(self, out, x, keep1, stage, a1=None):
        d = self.d
        st = R.check_trunk(x, d["conv1.weight"], d["conv1.bias"], d["w2q"], d["conv2.bias"], out["p"],
                           out["a1"] if a1 is None else a1, pm=out.get("pm"), keep1=keep1, check_a1=a1 is None,
                           name=stage)
        _report(stage, self.B, st)


@functools.lru_cache(maxsize=None)
def _train_run(dev, B):
    """trunk_fwd -> fc1_fwd -> head_train at step 3 with dropout, rows by index with stride B; every kernel's
    inputs and outputs for the checked rows (each stage is then checked on its own inputs)."""
    bx = Box(dev, B)
    t = bx.trunk()
    z = bx.fc1()
    h = bx.head_train()
    return bx, t, z, h


# ------------------------------------------------------------------ trunk
@pytest.mark.parametrize("B", R.TRUNK_B)
def test_trunk_train_form(cuda_device, B):
    bx, t, _, _ = _train_run(cuda_device, B)
    bx.check_trunk(t, bx.x_rows(bx.src_rows()), bx.keep1(), "trunk train idx")


def test_trunk_no_dropout_flag(cuda_device):
    bx = Box(cuda_device, 33, flags=FLAG_NO_DROPOUT)
    t = bx.trunk()
    assert bool((((t["pm"] >> 2) & 1) == 1).all())
    bx.check_trunk(t, bx.x_rows(bx.src_rows()), None, "trunk train nodrop")


def test_trunk_pregathered_rows(cuda_device):
    bx = Box(cuda_device, 33, step=2)
    t = bx.trunk(idx=False)                                     # row b reads dataset row 2*B + b
    src = 2 * 33 + torch.tensor(bx.rows)
    bx.check_trunk(t, bx.x_rows(src), R.keep_rows(FWD_RNG_BASE + 4, bx.rows, 9216, 192), "trunk train pre")


@pytest.mark.parametrize("B", [7, 257])
def test_trunk_fp32_module_input(cuda_device, B):
    bx = Box(cuda_device, B)
    x = normalize_u8(bx.imgs[bx.idx[:B]]).reshape(B, 784).contiguous()
    t = bx.trunk(xin=x.to(cuda_device))
    bx.check_trunk(t, x[bx.rows], bx.keep1(), "trunk train xin")


@pytest.mark.parametrize("B", [7, 257])
def test_trunk_eval_form(cuda_device, B):
    """Null a1 / pmask pointers as eval_forward passes them: p is the no-dropout oracle's on the a1 that the
    train form stored for the same images (checked there), and bitwise the train form's p under
    FLAG_NO_DROPOUT - the two forms differ in what they store, not in what they compute."""
    bx = Box(cuda_device, B, flags=FLAG_NO_DROPOUT)
    tr = bx.trunk()
    ev = bx.trunk(train=False)
    x = bx.x_rows(bx.src_rows())
    bx.check_trunk(tr, x, None, "trunk train nodrop")
    bx.check_trunk(ev, x, None, "trunk eval", a1=tr["a1"])
    assert torch.equal(ev["p"].view(torch.int16), tr["p"].view(torch.int16))
    bx.ms.set_state(FWD_STEP, seed=FWD_SEED, rng_base=FWD_RNG_BASE)          # eval ignores the dropout state
    assert torch.equal(bx.trunk(train=False)["p"].view(torch.int16), ev["p"].view(torch.int16))


# ------------------------------------------------------------------ fc1
@pytest.mark.parametrize("B", R.FC1_B)
def test_fc1_partials(cuda_device, B):
    bx, t, z, _ = _train_run(cuda_device, B)
    _report("fc1", B, R.check_fc1(t["p"], bx.d["w1q"], z, bx.ks))


@pytest.mark.parametrize("B", [33, 513])
def test_fc1_hand_made_rows(cuda_device, B):
    bx = Box(cuda_device, B)
    ks, kc = bx.ks, 9216 // bx.ks
    g = torch.Generator().manual_seed(B)
    p = bf16_round(torch.randn(B, 9216, generator=g))
    cols = {2: 5, 3: 9216 // 2 + 7, 4: 9215}                    # one-hot rows: first, a middle, the last chunk
    p[1] = 0
    for r, k in cols.items():
        p[r] = 0
        p[r, k] = 1.75 * (r - 3.5)
    bx.buf.p.zero_()
    bx.buf.p[:B].copy_(p)
    bx.rows = sorted(set(bx.rows) | {1, 2, 3, 4})
    bx.rows_d = torch.tensor(bx.rows, device=cuda_device)
    z = bx.fc1()
    _report("fc1 hand-made", B, R.check_fc1(p[bx.rows], bx.d["w1q"], z, ks))
    at = {r: i for i, r in enumerate(bx.rows)}
    assert bool((z[:, at[1]] == 0).all())
    for r, k in cols.items():
        want = torch.zeros(ks, 128)
        want[k // kc] = bx.d["w1q"][:, k].float() * float(p[r, k])           # one product: exact in fp32
        assert torch.equal(z[:, at[r]], want), (r, k)


# ------------------------------------------------------------------ head, training form
def _check_head_train(bx, z, h, stage):
    n = torch.tensor(bx.rows)
    y = bx.labels[bx.src_rows()]
    st = R.check_head_train(z, bx.d, y, bx.keep2(), bx.inv, h["loss_rows"], h["h_bf"][n], h["dz1"][n], h["dl_bf"][n],
                            name=stage)
    R.check_head_padding(bx.B, h["dz1"], h["h_bf"], h["dl_bf"], SENT, name=stage)
    _report(stage, bx.B, st)


@pytest.mark.parametrize("B", R.HEAD_B)
def test_head_train(cuda_device, B):
    bx, _, z, h = _train_run(cuda_device, B)
    _check_head_train(bx, z, h, "head_train idx")


def test_head_train_pregathered_labels(cuda_device):
    bx, _, z, h = _train_run(cuda_device, 33)
    h2 = bx.head_train(idx=False)
    _check_head_train(bx, z, h2, "head_train pre")
    for k in h:
        assert torch.equal(h[k].view(torch.int16 if h[k].dtype == torch.bfloat16 else h[k].dtype),
                           h2[k].view(torch.int16 if h2[k].dtype == torch.bfloat16 else h2[k].dtype)), k


# ------------------------------------------------------------------ head_eval / head_fwd
@pytest.mark.parametrize("B", R.EVAL_B)
def test_head_eval_and_head_fwd(cuda_device, B):
    bx = Box(cuda_device, B, trained=True)
    buf, ms, dev = bx.buf, bx.ms, cuda_device
    bx.trunk(train=False)
    z = bx.fc1()
    rows = bx.rows_d
    # head_eval reads labels[idx[b]] (no step, no stride)
    y = bx.labels[bx.idx[torch.tensor(bx.rows)]]
    _sentinel(buf.loss_rows, buf.correct, buf.logp)
    Fk.head_eval(ms, bx.lab_d, bx.idx_d, buf)
    torch.cuda.synchronize()
    logp_all = buf.logp.clone()
    assert torch.isfinite(logp_all).all()
    st = R.check_head_logp(z, bx.d, buf.logp[rows].cpu(), labels=y, loss_rows=buf.loss_rows[rows].cpu(),
                           correct=buf.correct[rows].cpu(), name="head_eval")
    _report("head_eval", B, st)
    assert len(set(buf.logp.argmax(1).tolist())) > 1            # the trained net decides between classes
    # no labels: loss_rows and correct are 0, the log-probs the same bits
    _sentinel(buf.loss_rows, buf.correct, buf.logp)
    Fk.head_eval(ms, None, None, buf)
    torch.cuda.synchronize()
    assert bool((buf.loss_rows == 0).all()) and bool((buf.correct == 0).all())
    assert torch.equal(buf.logp, logp_all)
    # head_fwd (module-API entry, unwrapped): eval form bitwise head_eval's log-probs
    p, o = native.ptr, ms.offsets
    args = (p(buf.z1part), p(ms.param) + 4 * o["fc1.bias"], p(ms.param) + 4 * o["fc2.weight"],
            p(ms.param) + 4 * o["fc2.bias"], p(ms.state), p(buf.logp), B)
    _sentinel(buf.logp)
    native.load().head_fwd(*args, False, native.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(buf.logp, logp_all)
    # train form: dropout-2 drawn as head_train draws it
    _sentinel(buf.logp)
    native.load().head_fwd(*args, True, native.stream_handle())
    torch.cuda.synchronize()
    assert torch.isfinite(buf.logp).all()
    st = R.check_head_logp(z, bx.d, buf.logp[rows].cpu(), keep2=bx.keep2(), name="head_fwd train")
    _report("head_fwd train", B, {"logp": st["logp"]})


# ------------------------------------------------------------------ launch geometry must not show
def test_trunk_geometry_invariance_bitwise(cuda_device):
    """Rows 0..6 of a B = 257 launch (one workgroup per strip) == the B = 7 launch (one per image) on the same
    seven images, seed, step and rng_base: a1, p and pmask bit for bit."""
    small, big = Box(cuda_device, 7), Box(cuda_device, 257)
    seven = small.imgs[small.idx[FWD_STEP * 7:FWD_STEP * 7 + 7]].reshape(7, 784)
    data = big.imgs.reshape(-1, 784).clone()
    data[:7] = seven
    big.u8 = data.contiguous().to(cuda_device)
    idx = big.idx.clone()
    idx[FWD_STEP * 257:FWD_STEP * 257 + 7] = torch.arange(7)
    big.idx_d = idx.to(torch.int32).to(cuda_device)
    a = small.trunk()                                             # small.rows is every row 0..6
    big.trunk()
    got = {"a1": big.buf.a1[:7].cpu(), "p": big.buf.p[:7].cpu(), "pm": Fk.pmask_flat(big.buf.pmask)[:7].cpu()}
    for k, t in got.items():
        bits = (lambda v: v.view(torch.int16)) if t.dtype == torch.bfloat16 else (lambda v: v)
        assert torch.equal(bits(a[k]), bits(t)), k


def test_split_k_geometry_row0(cuda_device):
    """Row 0 at B = 512 (4-way split) against B = 511 (32-way) on the same row: not bitwise - the split
    differs - but the z1part sums and head outputs agree within the stages' eps."""
    outs = []
    img0, lab0 = R.forward_case(511)[0][0], R.forward_case(511)[1][0]
    for B in (511, 512):
        bx = Box(cuda_device, B)
        bx.imgs, bx.labels, bx.idx = bx.imgs.clone(), bx.labels.clone(), bx.idx.clone()
        bx.imgs[0], bx.labels[0] = img0, lab0                    # dataset row 0: the same image and label
        bx.idx[FWD_STEP * B] = 0                                 # row 0 of the step reads dataset row 0
        bx.u8 = bx.imgs.reshape(-1, 784).contiguous().to(cuda_device)
        bx.lab_d = bx.labels.to(torch.int32).to(cuda_device)
        bx.idx_d = bx.idx.to(torch.int32).to(cuda_device)
        t = bx.trunk()
        z = bx.fc1()
        h = bx.head_train()
        outs.append((bx, t, z, h))
    (b1, t1, z1, h1), (b2, t2, z2, h2) = outs
    assert torch.equal(b1.imgs[0], b2.imgs[0]) and b1.labels[0] == b2.labels[0]
    assert torch.equal(t1["p"][0].view(torch.int16), t2["p"][0].view(torch.int16))
    ref = R.stage_fc1_partials(t1["p"][:1], b1.d["w1q"], 1)[0]
    eps = max(R.stage_eps(R.stage_fc1_partials(t1["p"][:1], b1.d["w1q"], k, R.F32).sum(0), ref[0:1]) for k in (32, 4))
    for z in (z1, z2):                                            # each within eps of the exact sum
        R.assert_within(z[:, 0].double().sum(0, keepdim=True), ref, eps, "split-K row 0 sum")
    # per-row NLL (independent of inv_batch).  Each kernel is within the head eps of the oracle on its own
    # z1part; the two z1 differ by at most 2 eps per unit, which moves a logit by at most 2 (dropout scale) x
    # sum_o |w_fc2[c][o]| x 2 eps and the NLL by at most twice the largest logit move
    y = b1.labels[:1]
    k2 = R.keep_rows(OFF1 + 1, [0], 128, 128)
    args = (z1[:, :1], b1.d["fc1.bias"], b1.d["fc2.weight"], b1.d["fc2.bias"], y, k2, 1.0)
    e = 2 * R.stage_eps(R.stage_head(*args, dtype=R.F32)["nll"], R.stage_head(*args)["nll"], head=True) \
        + 8 * eps * float(b1.d["fc2.weight"].abs().sum(1).max())
    diff = abs(float(h1["loss_rows"][0]) - float(h2["loss_rows"][0]))
    print(f"\nsplit-K row 0           B=511/512 nll difference    dev {diff:10.3e}  eps {e:10.3e}", end="")
    assert diff <= e
