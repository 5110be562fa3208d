"""T1: every Adadelta update path on its own against the float64 stage oracle (MI355X only).

adadelta_step (regions ALL / FC / CONV, the fc region on 1, 144, 576 and 577 workgroups, write-through stores on
and off), refresh_shadows, the conv reduce fused with the update (whole launch, the conv2 and the conv1 parts,
adadelta_c1) and the fc weight gradients fused with the update are launched one at a time over sentinel-filled
buffers.  ``param``, ``square_avg`` and ``acc_delta`` are held to tests/refmodel.py's stage_adadelta in float64 on
the launch's own inputs, copied back, within eps = 8 x max |fp32 CPU - float64| measured here per tensor and
step (fp32 CPU: the op-by-op numpy emulation of Ada::step and one step of torch.optim.Adadelta), and bit for bit
to that emulation; the four bf16 shadows to stage_shadows of the launch's own ``param``.  Three consecutive steps
run from the seeded state of refmodel.ada_case, each checked from the kernel's own previous state, with the
device lr rewritten before the third.  Paths that the source claims equal are compared bit for bit with the one
that was held to the oracle on the same inputs.  tests/test_optimizer_oracle_cpu.py proves on the CPU that these
checks fail on subtly wrong updates.  Each test prints `stage B tensor deviation eps` (docs/COVERAGE.md 2.4).
"""
import pytest
import torch

from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native

import refmodel as R
from refmodel import ADA_ALL, ADA_CONV, ADA_FC, OFF_CONV, PARAM_TOTAL
from test_gpu_backward_stages import LOG_N, BwdBox, _conv_ready
from test_gpu_forward_stages import _report, _sentinel

pytestmark = pytest.mark.gpu

FLAT = ("param", "grad", "square_avg", "acc_delta")
ALL_BUFS = FLAT + R.ADA_SHADOWS


def _dbits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _deq(a, b, sel=None):
    a, b = _dbits(a.reshape(-1)), _dbits(b.reshape(-1))
    return bool(torch.equal(a, b) if sel is None else torch.equal(a[sel], b[sel]))


class AdaState:
    """The seeded flat state of refmodel.ada_case in a ModelState, with snapshots on either side of the bus."""

    def __init__(self, ms, dev):
        self.ms, self.dev = ms, dev
        C = native.load()
        assert dict(C.PARAM_OFFSETS) == R.ADA_OFFS and C.PARAM_TOTAL == PARAM_TOTAL and C.BUCKET_SPLIT == OFF_CONV
        assert (C.RED_W2_PARTS, C.RED_ALL_PARTS) == (R.RED_W2_PARTS, R.RED_ALL_PARTS) == (Fk.RED_W2_PARTS, Fk.RED_ALL_PARTS)
        assert C.ADA_FC_LEAN_GRID == 144 and (ms.rho, ms.eps) == (R.ADA_RHO, R.ADA_EPS)
        case = R.ada_case()
        self.init = {k: case[k].to(dev) for k in R.ADA_STATE}
        self.grads = [g.to(dev) for g in case["grads"]]

    def config(self, lr, wd):
        self.ms.lr.fill_(lr)
        self.ms.weight_decay = wd

    def load(self):
        for k in R.ADA_STATE:
            getattr(self.ms, k).copy_(self.init[k])

    def bufs(self):
        return {k: getattr(self.ms, k) for k in ALL_BUFS}

    def snap(self):                      # device clones: bit comparisons stay on the device
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.bufs().items()}

    def restore(self, snap):
        for k, v in self.bufs().items():
            v.copy_(snap[k])

    def sentinel_outside(self, own_d):
        """R.ADA_SENTINEL into the three state tensors outside the device mask ``own_d`` (finite: an update that
        strays there changes it, where a NaN would stay a NaN), the NaN sentinel into every shadow."""
        for k in R.ADA_STATE:
            getattr(self.ms, k).masked_fill_(~own_d, R.ADA_SENTINEL)
        _sentinel(*[getattr(self.ms, k) for k in R.ADA_SHADOWS])


def _cpu(snap):
    return {k: v.cpu() for k, v in snap.items()}


def _box(dev, lr=1.0, wd=0.0):
    torch.manual_seed(1)
    st = AdaState(ModelState(Net(), dev, lr=lr, weight_decay=wd), dev)
    st.load()
    return st


def _lr_at(lr, s):
    return lr * R.ADA_LR_GAMMA if s == 2 else lr


def _check_mismatch(stats, what):
    """Measured on an MI355X before it was asserted: in every path no element of param, square_avg or acc_delta
    differs from the op-by-op fp32 emulation (the device's sqrtf and / are correctly rounded, denormals are kept)."""
    for k in R.ADA_STATE:
        n = stats[f"mismatch {k}"][0]
        assert n == 0, f"{what}: {int(n)} elements of {k} differ from the fp32 emulation"


REGION_OWN = {r: R.own_mask(*R.ADA_RANGE[r]) for r in (ADA_ALL, ADA_FC, ADA_CONV)}
REGION_SHADOWS = {ADA_ALL: R.ADA_SHADOWS, ADA_FC: ("w1", "w1t"), ADA_CONV: ("w2f", "w2d")}
# region, grid, write-through: every launch form of adadelta_kernel<true> besides (ALL, full grid, plain stores)
STEP_PATHS = [(ADA_ALL, 0, True), (ADA_FC, 0, False), (ADA_FC, 0, True), (ADA_CONV, 0, False), (ADA_CONV, 0, True)] + \
             [(ADA_FC, g, wt) for g in (1, 144, 576, 577) for wt in (False, True)]


# ------------------------------------------------------------------ 1. adadelta_step: regions and grids
@pytest.mark.parametrize("lr,wd", R.ADA_CONFIGS)
def test_adadelta_step_regions_and_grids(cuda_device, lr, wd):
    st = _box(cuda_device, lr, wd)
    ms = st.ms
    ms.set_state(5, seed=1, rng_base=0)
    ref = []                                             # (before, after) of the whole update, per step
    for s in range(3):                                   # ADA_ALL, full grid, plain stores: against the oracle
        ms.grad.copy_(st.grads[s])
        ms.lr.fill_(_lr_at(lr, s))                       # the third step reads a new lr from device memory
        _sentinel(*[getattr(ms, k) for k in R.ADA_SHADOWS])
        before, step0 = st.snap(), ms.get_step()
        Fk.adadelta_step(ms, ADA_ALL, advance_step=(s == 1))
        after = st.snap()
        assert ms.get_step() == step0 + (s == 1), "the step counter advances by exactly 1, and only when asked"
        b, a = _cpu(before), _cpu(after)
        stats = R.check_adadelta_update(b, a, REGION_OWN[ADA_ALL], _lr_at(lr, s), wd, name=f"ADA_ALL step {s}")
        _report(f"adadelta ALL s{s} lr{lr} wd{wd}", 0, stats)
        _check_mismatch(stats, f"ADA_ALL step {s}")
        R.check_ownership(b, a, REGION_OWN[ADA_ALL], R.ADA_SHADOWS, name=f"ADA_ALL step {s}")
        if s == 2 and lr != _lr_at(lr, s):               # the old lr would be off by (1 - gamma) lr |d|
            old = R.stage_adadelta(b["param"], b["grad"], b["square_avg"], b["acc_delta"], lr, R.ADA_RHO, R.ADA_EPS, wd)[0]
            assert float((old - a["param"].double()).abs().max()) > 100 * stats["param"][1]
        ref.append((before, after))
    own_d = {r: m.to(cuda_device) for r, m in REGION_OWN.items()}
    for region, grid, wt in STEP_PATHS:                  # the same inputs: the same bits in what the launch owns
        what = f"region {region} grid {grid} wt {wt}"
        own = own_d[region]
        for s in range(3):
            st.restore(ref[s][0])                        # the kernel's own previous state = the reference's, asserted below
            ms.lr.fill_(_lr_at(lr, s))
            st.sentinel_outside(own)
            before, step0 = st.snap(), ms.get_step()
            Fk.adadelta_step(ms, region, advance_step=(s == 0), grid=grid, wt=wt)
            after = st.snap()
            assert ms.get_step() == step0 + (s == 0), what
            for k in R.ADA_STATE:
                assert _deq(after[k], ref[s][1][k], own), f"{what} step {s}: {k} differs from the full grid"
                assert _deq(after[k], before[k], ~own), f"{what} step {s}: {k} written outside the region"
            assert _deq(after["grad"], before["grad"]), f"{what}: grad was written"
            for k in R.ADA_SHADOWS:
                want = ref[s][1][k] if k in REGION_SHADOWS[region] else before[k]
                assert _deq(after[k], want), f"{what} step {s}: shadow {k}"


def test_adadelta_step_refuses_a_grid_outside_the_fc_region(cuda_device):
    st = _box(cuda_device)
    for region, grid in ((ADA_ALL, 144), (ADA_CONV, 8), (ADA_FC, 578)):
        with pytest.raises(RuntimeError, match="reduced grid"):
            Fk.adadelta_step(st.ms, region, grid=grid)


# ------------------------------------------------------------------ 2. isolation of a non-finite gradient
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_adadelta_step_isolates_a_non_finite_gradient(cuda_device, poison):
    lr, wd = 0.7, 0.01
    st = _box(cuda_device, lr, wd)
    ms, case = st.ms, R.ada_case()
    for region, grid, wt in ((ADA_ALL, 0, False), (ADA_FC, 144, True), (ADA_FC, 0, True), (ADA_CONV, 0, True)):
        own = REGION_OWN[region]
        idx = torch.tensor([e for e in R.ADA_POISON if own[e]])
        runs = []
        for dirty in (False, True):
            st.load()
            ms.grad.copy_(st.grads[0])
            if dirty:
                ms.grad[idx.to(cuda_device)] = poison
            st.sentinel_outside(own.to(cuda_device))
            Fk.adadelta_step(ms, region, grid=grid, wt=wt)
            runs.append(_cpu(st.snap()))
        g = torch.full((len(idx),), poison)
        emu = R.stage_adadelta(case["param"][idx], g, case["square_avg"][idx], case["acc_delta"][idx], lr, R.ADA_RHO,
                               R.ADA_EPS, wd, dtype=R.F32)
        R.check_isolation(runs[0], runs[1], idx, emu, name=f"region {region} grid {grid} wt {wt}")


# ------------------------------------------------------------------ 3. refresh_shadows
def test_refresh_shadows_writes_the_shadows_and_nothing_else(cuda_device):
    st = _box(cuda_device, 0.7, 0.01)
    ms = st.ms
    ms.set_state(7, seed=1, rng_base=0)
    sp = R.shadow_specials()
    for name, at in R.SHADOW_SPECIAL_AT.items():
        ms.param[(R.ADA_OFFS[name] + torch.tensor(at)).to(cuda_device)] = sp.to(cuda_device)
    ms.grad.fill_(float("nan"))                          # neither read nor written
    _sentinel(*[getattr(ms, k) for k in R.ADA_SHADOWS])
    before = _cpu(st.snap())
    ms.refresh_shadows()
    after = _cpu(st.snap())
    assert ms.get_step() == 7
    R.check_ownership(before, after, R.own_mask(), R.ADA_SHADOWS, name="refresh_shadows")
    src = R.shadow_sources()
    for name, shadows in (("fc1.weight", ("w1", "w1t")), ("conv2.weight", ("w2f", "w2d"))):
        for k in shadows:                                # the hand-placed values, against bits written down by hand
            flat = after[k].reshape(-1).view(torch.int16).long() & 0xFFFF
            for e, want in zip(R.SHADOW_SPECIAL_AT[name], R.SHADOW_SPECIAL_BITS):
                pos = (src[k] == R.ADA_OFFS[name] + e).nonzero()
                assert pos.numel() == 1
                got = int(flat[pos[0, 0]])
                assert (got & 0x7F80) == 0x7F80 and got & 0x7F if want is None else got == want, (k, e, hex(got), want)


# ------------------------------------------------------------------ 4. conv reduce fused with the update
def _conv_forms():
    p2, pa = R.RED_W2_PARTS, R.RED_ALL_PARTS
    c2, c1 = R.own_mask(idx=R.conv_sink_elements(0, p2)), R.own_mask(idx=R.conv_sink_elements(p2, pa))
    return {"whole": (Fk.UPD_WHOLE, c2 | c1, ("w2f", "w2d", "w1", "w1t")),
            "parts conv2": (("parts", 0, p2), c2, ("w2f", "w2d")),
            "parts conv1": (("parts", p2, pa), c1, ()),
            "c1": (Fk.UPD_C1, c1, ())}


@pytest.mark.parametrize("B", [2, 86, 341])
def test_conv_reduce_update_forms(cuda_device, B):
    dev = cuda_device
    bx = _conv_ready(dev, B, hand=B != 341)
    pre = B == 341                                       # the real chain, the reduce reading the c1red group sums
    ms, buf = bx.ms, bx.buf
    _sentinel(buf.c1part, buf.w2part, bx.c1red)
    kw = dict(c1red=bx.c1red if pre else None)
    Fk.conv_bwd(ms, bx.u8, bx.idx_d, buf, 1.0, B, stages=Fk.CONV_DGRAD | Fk.CONV_WGRAD, **kw)   # the slabs, once
    torch.cuda.synchronize()
    slabs, c1rows = buf.w2part[:bx.G].cpu(), (bx.c1red[:R.C1_PRE_SLABS] if pre else buf.c1part[:4 * B]).cpu()
    st = AdaState(ms, dev)
    fc = R.own_mask(0, OFF_CONV)
    conv_d = R.own_mask(OFF_CONV, PARAM_TOTAL).to(dev)
    for lr, wd in R.ADA_CONFIGS:
        st.config(lr, wd)
        for form, (update, sink, shadows) in _conv_forms().items():
            what = f"conv reduce+update {form}"
            own = sink | fc if form == "whole" else sink
            own_d, sink_d = own.to(dev), sink.to(dev)
            st.load()
            for s in range(3):
                ms.grad.copy_(st.grads[s])               # the fc region's gradient (read by the whole launch only)
                ms.grad.masked_fill_(conv_d, float("nan"))
                ms.lr.fill_(_lr_at(lr, s))
                _sentinel(*[getattr(ms, k) for k in R.ADA_SHADOWS])
                start = st.snap()
                # the two-kernel path from the same state: conv_grad_reduce, then adadelta_step.  It also updates the
                # padding elements (from whatever grad holds there), which the fused launches leave alone.
                Fk.conv_bwd(ms, bx.u8, bx.idx_d, buf, 1.0, B, stages=Fk.CONV_REDUCE, **kw)
                Fk.adadelta_step(ms, ADA_ALL if form == "whole" else ADA_CONV)
                two = st.snap()
                st.restore(start)
                st.sentinel_outside(own_d)
                before = st.snap()
                Fk.conv_bwd(ms, bx.u8, bx.idx_d, buf, 1.0, B, stages=Fk.CONV_REDUCE, update=update, **kw)
                after = st.snap()
                for k in FLAT:
                    assert _deq(after[k], two[k], own_d), f"{what} step {s}: {k} differs from reduce + adadelta_step"
                for k in R.ADA_SHADOWS:
                    assert _deq(after[k], two[k] if k in shadows else before[k]), f"{what} step {s}: shadow {k}"
                b, a = _cpu(before), _cpu(after)
                R.check_ownership(b, a, own, shadows, grad_own=sink, name=what)
                stats = R.check_adadelta_update(b, a, sink, _lr_at(lr, s), wd, grad=a["grad"], name=what)
                _check_mismatch(stats, what)
                if form == "whole" and s == 0:
                    grads = {n: a["grad"][R.ADA_OFFS[n]:R.ADA_OFFS[n] + R.ADA_NUMEL[n]].view(v.shape)
                             for n, v in ms.views(ms.grad).items()}
                    stats.update(R.check_conv_reduce(slabs, c1rows, 1.0, grads, name=what))
                if s == 0:
                    _report(f"{form} lr{lr} wd{wd}", B, stats)
                st.restore(after)                        # the next step starts from the kernel's own state
                for k in R.ADA_STATE:                    # (sentinels outside: refill what the next reference reads)
                    getattr(ms, k).copy_(torch.where(own_d, after[k], two[k]))


# ------------------------------------------------------------------ 5. fc weight gradients fused with the update
@pytest.mark.parametrize("B", [33, 1024])
def test_fc_wgrad_update(cuda_device, B):
    dev = cuda_device
    bx = BwdBox(dev, B, trained=False).load_fc_hand()
    ms, buf = bx.ms, bx.buf
    st = AdaState(ms, dev)
    own = R.own_mask(0, OFF_CONV)
    own[R.ada_padding()] = False                         # the fused launch updates parameters, not the padding
    own_d = own.to(dev)
    op = bx.fc_operands()
    for ci, (lr, wd) in enumerate(R.ADA_CONFIGS):
        st.config(lr, wd)
        for wt in (False, True):
            what = f"fc_wgrad_update wt {wt}"
            st.load()
            for s in range(3):
                ms.grad.fill_(float("nan"))
                ms.lr.fill_(_lr_at(lr, s))
                _sentinel(*[getattr(ms, k) for k in R.ADA_SHADOWS], bx.loss_log)
                start = st.snap()
                Fk.fc_bwd(ms, buf, 1.0, bx.loss_log, role=Fk.FC_ROLES_CA)        # roles C + A, then the fc update
                Fk.adadelta_step(ms, ADA_FC)
                two, log2 = st.snap(), bx.loss_log.clone()
                st.restore(start)
                st.sentinel_outside(own_d)
                _sentinel(bx.loss_log)
                before = st.snap()
                Fk.fc_bwd(ms, buf, 1.0, bx.loss_log, update=True, wt=wt)
                after = st.snap()
                for k in FLAT:
                    assert _deq(after[k], two[k], own_d), f"{what} step {s}: {k} differs from fc_bwd + adadelta_step"
                for k in R.ADA_SHADOWS:
                    assert _deq(after[k], two[k] if k in ("w1", "w1t") else before[k]), f"{what} step {s}: shadow {k}"
                assert _deq(bx.loss_log, log2), f"{what}: loss_log"
                log = bx.loss_log.cpu()
                assert torch.isnan(log[:bx.step]).all() and torch.isnan(log[bx.step + 1:]).all() and LOG_N > bx.step
                for k in R.ADA_STATE:                    # the next step starts from the kernel's own state
                    getattr(ms, k).copy_(torch.where(own_d, after[k], two[k]))
                if wt:                                   # the same bits as the plain-store launch, held to the oracle
                    continue
                b, a = _cpu(before), _cpu(after)
                R.check_ownership(b, a, own, ("w1", "w1t"), grad_own=own, name=what)
                stats = R.check_adadelta_update(b, a, own, _lr_at(lr, s), wd, grad=a["grad"], name=what)
                _check_mismatch(stats, what)
                if ci == 0 and s == 0:
                    grads = {n: a["grad"][R.ADA_OFFS[n]:R.ADA_OFFS[n] + R.ADA_NUMEL[n]].view(v.shape)
                             for n, v in ms.views(ms.grad).items()}
                    stats.update(R.check_fc_wgrads(op["dz1"], op["p"], op["h_bf"], op["dl_bf"], 1.0, grads,
                                                   op["loss_rows"], log[bx.step], name=what))
                if s == 0:
                    _report(f"fc_wgrad_update lr{lr} wd{wd}", B, stats)


def test_fc_wgrad_update_refuses_two_splits(cuda_device):
    """B = 1025: a host-side throw of the launcher, no kernel launch."""
    torch.manual_seed(1)
    ms = ModelState(Net(), cuda_device)
    buf = Fk.StepBuffers.allocate(1025, cuda_device)
    before = ms.param.clone()
    with pytest.raises(RuntimeError, match="fc_wgrad_update: one split"):
        Fk.fc_bwd(ms, buf, 1.0, None, update=True)
    with pytest.raises(RuntimeError, match="fc_wgrad_update: one split"):
        Fk.fc_bwd(ms, Fk.StepBuffers.allocate(33, cuda_device), 0.5, None, update=True)      # grad scale != 1
    torch.cuda.synchronize()
    assert _deq(ms.param, before)
