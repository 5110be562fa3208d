"""The shared launch chains on the host (no GPU, no extension): ``ops.chain`` against a fake native module that
notes every call, with stub model / fused-state objects.  The argument tuples below are the launches of the loops
as they were written out in ``ops.attack`` / ``ops.attribute`` / ``ops.smooth`` / ``Predictor._native``."""
from types import SimpleNamespace

import pytest
import torch

from pytorch_mnist_ddp_amd.ops import chain
from pytorch_mnist_ddp_amd.ops.functional import FC_ROLE_B, round_up

STREAM = 77
NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight",
         "fc2.bias")


class FakeC:
    """Stands in for the extension: any attribute is a launch that records (name, args, kwargs)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))


class Mem:
    """Stands in for a device tensor: an address."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def _ms():
    offsets = {n: 1000 * i + 7 * (i + 1) for i, n in enumerate(NAMES)}
    return SimpleNamespace(param=Mem(1 << 20), offsets=offsets, device=torch.device("cpu"),
                           w2f=Mem(2 << 20), w2d=Mem(3 << 20), w1=Mem(4 << 20), w1t=Mem(5 << 20))


class FakeState:
    """Stands in for the fused state: a pool that counts what it hands out and takes back."""

    def __init__(self):
        self.ms, self.seed, self.rng_offset = _ms(), 12345, 40
        self.taken, self.given = [], []

    def take(self, B, device):
        fields = ("a1", "p", "pmask", "z1part", "loss_rows", "dz1", "h_bf", "dl_bf", "dyc", "fcpart")
        buf = SimpleNamespace(B=B, **{f: Mem((16 + i) << 20) for i, f in enumerate(fields)})
        self.taken.append(buf)
        return buf

    def give(self, buf):
        self.given.append(buf)


@pytest.fixture
def fake(monkeypatch):
    C = FakeC()
    monkeypatch.setattr(chain.native, "load", lambda *a, **k: C)
    monkeypatch.setattr(chain.native, "stream_handle", lambda *a, **k: STREAM)
    return C


def test_param_ptrs_are_param_plus_four_times_the_offset_and_the_shadows():
    ms = _ms()
    w = chain.param_ptrs(ms)
    P, o = ms.param.addr, ms.offsets
    assert (w.c1w, w.c1b, w.c2b) == (P + 4 * o["conv1.weight"], P + 4 * o["conv1.bias"], P + 4 * o["conv2.bias"])
    assert (w.f1b, w.f2w, w.f2b) == (P + 4 * o["fc1.bias"], P + 4 * o["fc2.weight"], P + 4 * o["fc2.bias"])
    assert (w.w2f, w.w2d, w.w1, w.w1t) == (ms.w2f.addr, ms.w2d.addr, ms.w1.addr, ms.w1t.addr)
    assert len(w) == 10 and len(set(w)) == 10
    with pytest.raises(AttributeError):
        w.c1w = 0                                            # immutable
    ms.param = Mem(9 << 20)                                  # a re-bind moved the flat buffer: computed per call
    assert chain.param_ptrs(ms).c1w == (9 << 20) + 4 * o["conv1.weight"]


@pytest.mark.parametrize("rows", [1, 31, 33])
def test_eval_chain_is_trunk_fc1_head_eval(fake, rows):
    ms = _ms()
    buf = SimpleNamespace(rows=40, p=Mem(11 << 20), z1part=Mem(12 << 20), loss_rows=Mem(13 << 20),
                          correct=Mem(14 << 20), logp=Mem(15 << 20))
    ev = chain.EvalChain(ms, buf)
    assert fake.calls == []                                  # building a chain launches nothing
    w = chain.param_ptrs(ms)
    ev.run(rows, xin=900)
    ev.run(rows, u8=800, labels=700)
    assert [c[0] for c in fake.calls] == ["trunk_fwd", "fc1_fwd", "head_eval"] * 2
    for k, (u8, xin, labels) in enumerate(((0, 900, 0), (800, 0, 700))):
        trunk, fc1, head = fake.calls[3 * k:3 * k + 3]
        assert trunk[1:] == ((u8, 0, 0, 0, w.c1w, w.c1b, w.w2f, w.c2b, 0, buf.p.addr, 0, rows, False, STREAM),
                             {"xin": xin})
        assert fc1[1:] == ((buf.p.addr, w.w1, buf.z1part.addr, rows, STREAM), {})
        assert head[1:] == ((buf.z1part.addr, w.f1b, w.f2w, w.f2b, labels, 0, buf.loss_rows.addr, buf.correct.addr,
                             buf.logp.addr, rows, STREAM), {})


@pytest.mark.parametrize("rows", [1, 31, 33])
def test_grad_chain_is_trunk_fc1_head_train_fc_bwd_role_b(fake, rows):
    st = FakeState()
    gc = chain.GradChain(st, 40)
    assert fake.calls == [] and len(st.taken) == 1 and st.taken[0].B == 40 and st.given == []
    assert st.rng_offset == 40                               # nothing is drawn: the counter stream stays
    b, w = st.taken[0], chain.param_ptrs(st.ms)
    Bp = round_up(rows, 32)
    assert Bp == {1: 32, 31: 32, 33: 64}[rows]
    gc.run(600, 500, rows)
    assert [c[0] for c in fake.calls] == ["trunk_fwd", "fc1_fwd", "head_train", "fc_bwd"]
    trunk, fc1, head, fcb = fake.calls
    pst = trunk[1][3]
    assert trunk[1:] == ((0, 0, 0, pst, w.c1w, w.c1b, w.w2f, w.c2b, b.a1.addr, b.p.addr, b.pmask.addr, rows, True,
                          STREAM), {"xin": 600})
    assert fc1[1:] == ((b.p.addr, w.w1, b.z1part.addr, rows, STREAM), {})
    assert head[1:] == ((b.z1part.addr, w.f1b, w.f2w, w.f2b, 500, 0, 0, pst, 1.0, b.loss_rows.addr, b.dz1.addr,
                         b.h_bf.addr, b.dl_bf.addr, rows, Bp, STREAM), {})
    assert fcb[1:] == ((b.dz1.addr, b.p.addr, b.pmask.addr, w.w1t, b.h_bf.addr, b.dl_bf.addr, b.loss_rows.addr, pst,
                        0, b.dyc.addr, 0, 1.0, 1.0, rows, Bp, STREAM), {"role": FC_ROLE_B, "part": b.fcpart.addr})
    # the step state: step 0 | STEP_FLAG_NO_DROPOUT, zero seed and counter
    assert pst == gc._state.data_ptr() and gc._state.tolist() == [1 << 32, 0, 0]
    # one launch each for the two forms of the input gradient
    fake.calls.clear()
    gc.input_grad(300, rows)
    gc.input_grad_step(600, 610, 620, 0.25, 0.5, -1.0, 2.0, rows)
    assert fake.calls == [
        ("input_grad", (b.dyc.addr, b.a1.addr, w.w2d, w.c1w, 300, rows, STREAM), {}),
        ("input_grad_step", (b.dyc.addr, b.a1.addr, w.w2d, w.c1w, 600, 610, 620, 0.25, 0.5, -1.0, 2.0, rows, STREAM),
         {})]
    fake.calls.clear()
    gc.release()
    gc.release()                                             # the set goes back exactly once
    assert st.given == [b] and fake.calls == [] and st.rng_offset == 40
