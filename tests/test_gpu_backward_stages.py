"""T1: every bf16 backward kernel on its own against the float64 stage oracle (MI355X only).

fc_bwd (roles C, A, B, alone and together), fc_bwd_dw1, fc_grad_reduce, conv2_wgrad (both forms), conv2_dgrad,
c1_prereduce and conv_grad_reduce are launched one at a time over sentinel-filled outputs; each is compared with
tests/refmodel.py's backward oracle applied to that kernel's own device inputs, copied back.  The comparators,
the sentinels and the eps rule (8 x the deviation of torch's fp32 CPU op from float64 on the same operands,
measured here) are the forward test's.  Inputs are either the real chain (trained net, dropout on, step 3,
rows by index with stride B, the forward kernels run once) or hand-made operands (refmodel.fc_hand_case /
conv_hand_case).  tests/test_backward_oracle_cpu.py proves on the CPU that these checks fail on subtly wrong
outputs.  Each test prints `stage B tensor deviation eps` (docs/COVERAGE.md 2.4 records the table).
"""
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.engine.state import FLAG_NO_DROPOUT
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native

import refmodel as R
from test_gpu_forward_stages import Box, _report, _sentinel

pytestmark = pytest.mark.gpu

LOG_N = 8                                    # loss_log entries; the step writes entry Box.step = 3


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class BwdBox(Box):
    """Box with one spare row on every backward output that is indexed by image, group or partial row, so that
    a write past B / G / 4B meets a sentinel."""

    def __init__(self, dev, B, trained=True, flags=0):
        super().__init__(dev, B, trained=trained, flags=flags)
        buf = self.buf
        self.G = native.load().conv_wgrad_groups(B)
        assert self.G == R.conv_wgrad_groups(B)
        buf.dyc = torch.zeros(B + 1, 144 * Fk.DYC_REC, dtype=torch.uint8, device=dev)
        buf.c1part = torch.zeros(4 * B + 1, 320, device=dev)
        buf.w2part = torch.zeros(self.G + 1, 18432 + 64, device=dev)
        self.loss_log = torch.zeros(LOG_N, device=dev)
        self.c1red = torch.zeros(R.C1_PRE_SLABS + 1, 320, device=dev)
        self.dyc_rows = R.dyc_check_rows(B)
        self.dyc_rows_d = torch.tensor(self.dyc_rows, device=dev)

    # ---- inputs
    def forward(self):
        """The forward kernels once (checked by test_gpu_forward_stages.py); p rows [B, round_up(B, 64)) are then
        filled with NaN: fc_bwd must mask them."""
        buf, B = self.buf, self.B
        Fk.trunk_fwd(self.ms, self.u8, self.idx_d, buf, True, B)
        buf.p[B:].zero_()
        Fk.fc1_fwd(self.ms, buf)
        Fk.head_train(self.ms, self.lab_d, self.idx_d, buf, B)
        buf.p[B:].fill_(float("nan"))
        torch.cuda.synchronize()
        return self

    def load_fc_hand(self):
        h, buf, B = R.fc_hand_case(self.B), self.buf, self.B
        for k in ("dz1", "h_bf", "dl_bf", "p", "loss_rows"):
            getattr(buf, k).copy_(h[k])
        buf.pmask.copy_(R.pmask_device(h["pm"]))
        assert torch.equal(Fk.pmask_flat(buf.pmask).cpu(), h["pm"])
        return self

    def load_conv_hand(self):
        h, buf, B = R.conv_hand_case(self.B), self.buf, self.B
        buf.dyc[:B].copy_(R.dyc_pack(h["g"], h["code"]))
        buf.a1.copy_(h["a1"])
        data = self.imgs.reshape(-1, 784).clone()
        data[self.idx[self.step * B:self.step * B + B]] = h["imgs"].reshape(B, 784)   # row b of the step reads image b
        self.u8 = data.contiguous().to(self.dev)
        self.x_all = h["x"]
        return self

    def fc_operands(self):
        buf, B = self.buf, self.B
        return dict(dz1=buf.dz1.cpu(), p=buf.p.cpu(), h_bf=buf.h_bf.cpu(), dl_bf=buf.dl_bf.cpu(),
                    loss_rows=buf.loss_rows.cpu(), pm=Fk.pmask_flat(buf.pmask).cpu())

    def conv_operands(self):
        """dense dy and a1 NCHW of all B images, the input rows of the step."""
        buf, B = self.buf, self.B
        g, code = R.dyc_unpack(buf.dyc[:B].cpu())
        x = getattr(self, "x_all", None)
        if x is None:
            x = normalize_u8(self.imgs[self.idx[self.step * B:self.step * B + B]]).reshape(B, 784)
        return dict(dy=R.dense_dy(g, code), a1=buf.a1.cpu().permute(0, 3, 1, 2).contiguous(), x=x)

    # ---- launches: sentinel first, one launch, copy back
    def fc_bwd(self, role=-1, grad_scale=1.0):
        buf, ms = self.buf, self.ms
        _sentinel(ms.grad, buf.dyc, self.loss_log)
        if role != Fk.FC_REDUCE:
            _sentinel(buf.fcpart)
        Fk.fc_bwd(ms, buf, grad_scale, self.loss_log, role=role)
        torch.cuda.synchronize()
        return dict(grads={n: v.cpu() for n, v in ms.views(ms.grad).items()}, dyc=buf.dyc[self.dyc_rows_d].cpu(),
                    dyc_past=buf.dyc[self.B].cpu(), loss_log=self.loss_log.cpu(), fcpart=buf.fcpart.cpu())

    def conv(self, stages, grad_scale=1.0, src="idx", c1red=False, keep=()):
        """One conv_bwd stage launch.  Every output is sentinel-filled first except those named in ``keep`` (the
        reduce's inputs)."""
        buf, ms, B = self.buf, self.ms, self.B
        outs = dict(grad=ms.grad, c1part=buf.c1part, w2part=buf.w2part, c1red=self.c1red)
        _sentinel(*[t for k, t in outs.items() if k not in keep])
        kw = dict(stages=stages, c1red=self.c1red if c1red else None)
        if src == "idx":
            Fk.conv_bwd(ms, self.u8, self.idx_d, buf, grad_scale, B, **kw)
        elif src == "pre":                     # pre-gathered rows: row b of step s is data row s * B + b
            rows = self.u8[self.idx_d[self.step * B:self.step * B + B].long()]
            pre = torch.zeros((self.step + 1) * B, 784, dtype=torch.uint8, device=self.dev)
            pre[self.step * B:] = rows
            Fk.conv_bwd(ms, pre, None, buf, grad_scale, B, **kw)
        else:                                  # fp32 module input
            xin = self.conv_operands()["x"].contiguous().to(self.dev)
            Fk.conv_bwd(ms, None, None, buf, grad_scale, 0, xin=xin, **kw)
        torch.cuda.synchronize()
        return dict(grads={n: v.cpu() for n, v in ms.views(ms.grad).items()}, c1part=buf.c1part.cpu(),
                    w2part=buf.w2part.cpu(), c1red=self.c1red.cpu())


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _fc_parts(B, fcpart):
    S = R.fc_splits(B)
    if S == 1:
        return None
    stride = native.load().FCB_PART_STRIDE
    slabs = fcpart[:S * stride].view(S, stride)
    return [{k: slabs[s, off:off + max(1, int(torch.tensor(shape).prod()))].reshape(shape)
             for k, (off, shape) in R.FCB_PART.items()} for s in range(S)]


def _check_fc_full(bx, out, grad_scale=1.0, stage="fc_bwd", no_dropout=False):
    B, op = bx.B, bx.fc_operands()
    parts = _fc_parts(B, out["fcpart"])
    st = R.check_fc_wgrads(op["dz1"], op["p"], op["h_bf"], op["dl_bf"], grad_scale, out["grads"], op["loss_rows"],
                           out["loss_log"][bx.step], parts, name=stage)
    rows = torch.tensor(bx.dyc_rows)
    st.update(R.check_fc_dgrad(op["dz1"][rows], bx.d["w1q"], op["pm"][rows], no_dropout, out["dyc"], name=stage))
    _report(stage, B, st)
    log = out["loss_log"]
    assert _all_nan(log[:bx.step]) and _all_nan(log[bx.step + 1:]), f"{stage}: loss_log neighbours were written"
    assert bool((out["dyc_past"] == 0xAA).all()), f"{stage}: records of image B were written"
    assert all(_all_nan(out["grads"][k]) for k in R.CONV_NAMES), f"{stage}: conv gradients were written"
    if parts is None:
        assert _all_nan(out["fcpart"]), f"{stage}: the split workspace was written at one split"
    return op


def _fc_roles(bx, full, op):
    """One role per launch: what it owns equals the whole launch's bits (held to the oracle there), everything
    else keeps the sentinel."""
    B = bx.B
    owns = {Fk.FC_ROLE_C: ("fc2.weight", "fc2.bias"), Fk.FC_ROLE_A: ("fc1.weight", "fc1.bias"), Fk.FC_ROLE_B: ()}
    if R.fc_splits(B) == 1:
        for role, names in owns.items():
            o = bx.fc_bwd(role=role)
            for k in R.FC_NAMES:
                assert _same(o["grads"][k], full["grads"][k]) if k in names else _all_nan(o["grads"][k]), (role, k)
            assert _same(o["loss_log"], full["loss_log"]) if role == Fk.FC_ROLE_C else _all_nan(o["loss_log"]), role
            assert _same(o["dyc"], full["dyc"]) if role == Fk.FC_ROLE_B else bool((o["dyc"] == 0xAA).all()), role
        return
    # B > 1024: the launches of the side schedules leave split partials; fc_grad_reduce sums them
    S, stride = R.fc_splits(B), native.load().FCB_PART_STRIDE
    fp = full["fcpart"][:S * stride].view(S, stride)
    a_lo, a_hi = R.FCB_PART["fc1.weight"][0], R.FCB_PART["fc2.weight"][0]
    c_hi = R.FCB_PART["loss"][0] + 1
    for role, has_a, has_c, has_b in ((Fk.FC_DW1, 1, 0, 0), (Fk.FC_ROLES_CB, 0, 1, 1), (Fk.FC_ROLES_B, 0, 0, 1),
                                      (Fk.FC_ROLES_CA, 1, 1, 0)):
        o = bx.fc_bwd(role=role)
        got = o["fcpart"][:S * stride].view(S, stride)
        assert _same(got[:, a_lo:a_hi], fp[:, a_lo:a_hi]) if has_a else _all_nan(got[:, a_lo:a_hi]), role
        assert _same(got[:, a_hi:c_hi], fp[:, a_hi:c_hi]) if has_c else _all_nan(got[:, a_hi:c_hi]), role
        assert _all_nan(got[:, c_hi:]) and _all_nan(o["fcpart"][S * stride:]), role
        assert _same(o["dyc"], full["dyc"]) if has_b else bool((o["dyc"] == 0xAA).all()), role
        assert all(_all_nan(v) for v in o["grads"].values()) and _all_nan(o["loss_log"]), role
    o = bx.fc_bwd(role=Fk.FC_REDUCE)           # on the partials that roles C | A just left
    for k in R.FC_NAMES:
        assert _same(o["grads"][k], full["grads"][k]), k
    assert _same(o["loss_log"], full["loss_log"]) and bool((o["dyc"] == 0xAA).all())


# ------------------------------------------------------------------ fc_bwd
@pytest.mark.parametrize("B", R.FC_REAL_B)
def test_fc_bwd_real_chain(cuda_device, B):
    bx = BwdBox(cuda_device, B).forward()
    full = bx.fc_bwd()
    op = _check_fc_full(bx, full, stage="fc_bwd chain")
    again = bx.fc_bwd()
    assert all(_same(again["grads"][k], full["grads"][k]) for k in R.FC_NAMES) and _same(again["dyc"], full["dyc"])
    _fc_roles(bx, full, op)


@pytest.mark.parametrize("B", (33,) + R.FC_HAND_B)
def test_fc_bwd_hand_made(cuda_device, B):
    bx = BwdBox(cuda_device, B, trained=False).load_fc_hand()
    full = bx.fc_bwd()
    op = _check_fc_full(bx, full, stage="fc_bwd hand")
    again = bx.fc_bwd()
    assert all(_same(again["grads"][k], full["grads"][k]) for k in R.FC_NAMES) and _same(again["dyc"], full["dyc"])
    assert _same(again["fcpart"], full["fcpart"])
    _fc_roles(bx, full, op)


@pytest.mark.parametrize("B", [33, 1025])
def test_fc_bwd_grad_scale(cuda_device, B):
    bx = BwdBox(cuda_device, B, trained=False).load_fc_hand()
    _check_fc_full(bx, bx.fc_bwd(grad_scale=0.25), 0.25, stage="fc_bwd scale .25")


def test_fc_bwd_no_dropout_flag(cuda_device):
    bx = BwdBox(cuda_device, 33, trained=False, flags=FLAG_NO_DROPOUT).load_fc_hand()
    _check_fc_full(bx, bx.fc_bwd(), stage="fc_bwd nodrop", no_dropout=True)


# ------------------------------------------------------------------ conv backward
def _conv_ready(dev, B, hand=False):
    bx = BwdBox(dev, B)
    if hand:
        return bx.load_conv_hand()
    bx.forward()
    Fk.fc_bwd(bx.ms, bx.buf, 1.0, None)
    torch.cuda.synchronize()
    return bx


def _check_wgrad(bx, op, stage):
    o = bx.conv(Fk.CONV_WGRAD)
    _report(stage, bx.B, R.check_conv2_wgrad(op["a1"], op["dy"], o["w2part"][:bx.G], name=stage))
    assert _all_nan(o["w2part"][bx.G:]), f"{stage}: slab G was written"
    assert _all_nan(o["c1part"]) and _all_nan(o["c1red"]) and all(_all_nan(v) for v in o["grads"].values()), stage
    assert _same(bx.conv(Fk.CONV_WGRAD)["w2part"], o["w2part"]), f"{stage}: a second launch differs"
    return o["w2part"]


def _check_dgrad(bx, op, stage, src="idx", c1red=False):
    B = bx.B
    o = bx.conv(Fk.CONV_DGRAD, src=src, c1red=c1red)
    _report(stage, B, R.check_conv2_dgrad(op["dy"], bx.d["w2q"], op["x"], op["a1"], o["c1part"][:4 * B], name=stage))
    assert _all_nan(o["c1part"][4 * B:]), f"{stage}: partial row 4B was written"
    assert _all_nan(o["w2part"]) and all(_all_nan(v) for v in o["grads"].values()), stage
    if c1red:
        _report(stage, B, R.check_c1red(o["c1part"][:4 * B], o["c1red"][:R.C1_PRE_SLABS], name=stage))
        assert _all_nan(o["c1red"][R.C1_PRE_SLABS:]), f"{stage}: c1red row 256 was written"
    else:
        assert _all_nan(o["c1red"]), f"{stage}: c1red was written without the pre-reduce"
    o2 = bx.conv(Fk.CONV_DGRAD, src=src, c1red=c1red)
    assert _same(o2["c1part"], o["c1part"]) and _same(o2["c1red"], o["c1red"]), f"{stage}: a second launch differs"
    return o


def _check_reduce(bx, w2part, dg, stage, grad_scale=1.0, c1red=False):
    """conv_grad_reduce on the partials that the two launches before left (copied back to the device)."""
    bx.buf.w2part.copy_(w2part)
    bx.buf.c1part.copy_(dg["c1part"])
    bx.c1red.copy_(dg["c1red"])
    o = bx.conv(Fk.CONV_REDUCE, grad_scale=grad_scale, c1red=c1red, keep=("c1part", "w2part", "c1red"))
    c1rows = dg["c1red"][:R.C1_PRE_SLABS] if c1red else dg["c1part"][:4 * bx.B]
    _report(stage, bx.B, R.check_conv_reduce(w2part[:bx.G], c1rows, grad_scale, o["grads"], name=stage))
    assert all(_all_nan(o["grads"][k]) for k in R.FC_NAMES), f"{stage}: fc gradients were written"
    assert _same(o["w2part"], w2part) and _same(o["c1part"], dg["c1part"]), f"{stage}: the reduce wrote its inputs"


@pytest.mark.parametrize("B", R.CONV_B + (1025,))
def test_conv_bwd_real_chain(cuda_device, B):
    bx = _conv_ready(cuda_device, B)
    op = bx.conv_operands()
    pre = B in (5, 341)                          # c1_prereduce: one row per slab / a ragged last slab
    w2part = _check_wgrad(bx, op, "conv2_wgrad chain")
    dg = _check_dgrad(bx, op, "conv2_dgrad chain", c1red=pre)
    _check_reduce(bx, w2part, dg, "conv_reduce chain", c1red=pre)


@pytest.mark.parametrize("B", [2, 86])
def test_conv_bwd_hand_made(cuda_device, B):
    bx = _conv_ready(cuda_device, B, hand=True)
    op = bx.conv_operands()
    w2part = _check_wgrad(bx, op, "conv2_wgrad hand")
    dg = _check_dgrad(bx, op, "conv2_dgrad hand")
    _check_reduce(bx, w2part, dg, "conv_reduce hand .25", grad_scale=0.25)


@pytest.mark.parametrize("B", [86, 342])
def test_conv2_wgrad_both_forms(cuda_device, B):
    """The lean and the staggered form, forced, each against the oracle."""
    bx = _conv_ready(cuda_device, B, hand=True)
    op = bx.conv_operands()
    C = native.load()
    try:
        for form in (0, 1):
            C.set_wgrad_form(form)
            _check_wgrad(bx, op, f"conv2_wgrad form {form}")
    finally:
        C.set_wgrad_form(-1)


def test_conv2_dgrad_grids(cuda_device):
    """B = 129: 516 items on 2 x CUs workgroups by default (ragged rounds), on 37, and one item each."""
    B = 129
    bx = _conv_ready(cuda_device, B, hand=True)
    op = bx.conv_operands()
    C = native.load()
    try:
        for grid in (0, 37, 4 * B):
            C.set_dgrad_grid(grid)
            _check_dgrad(bx, op, f"conv2_dgrad grid {grid}")
    finally:
        C.set_dgrad_grid(0)


@pytest.mark.parametrize("src", ["pre", "xin"])
def test_conv2_dgrad_input_sources(cuda_device, src):
    bx = _conv_ready(cuda_device, 5)
    _check_dgrad(bx, bx.conv_operands(), f"conv2_dgrad {src}", src=src)
