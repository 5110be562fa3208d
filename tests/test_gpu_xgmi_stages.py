"""T1: the four kernels of csrc/kernels/xgmi_allreduce.hip launched one at a time against the oracle (MI355X only),
and the support kernels of comm_kernels.hip bit for bit.

The case list is tests/xgmi_stage_cases.py: plain one-shot and two-shot all-reduces around the one-shot limit, forced
two-shot launches with ragged, short and empty shards at two offsets and on one workgroup, the two-shot and one-shot
kernels with the fused Adadelta step (the fp32 step's buckets, and a small ragged range with ada_base != 0) and
allreduce_fc_fused on its planned grid, 8 and 1 workgroups with write-through stores off and on (the same inputs,
bit for bit equal), and conv_reduce_fused (whole [0, 309) on the planned grid and on 39 workgroups, the engine's parts
[0, 289) and [289, 309) on channels of their own, grad_scale 1 / W, slabs of conv_hand_case at B = 2 and 86 and of the
real chain at 341 with c1red at world 1, three calls).  The fc and conv launches are also held bit for bit to the
separate launches they replace.  Reduced values are
held bit for bit to the rank-ordered fp32 sum and within eps to the float64 sum; param / square_avg / acc_delta to
stage_adadelta on the float64 sum within eps = 8 x max |fp32 emulation - float64| and bit for bit to the emulation;
shadows to stage_shadows of the launch's own param; a NaN and an inf on one rank reach exactly their elements.
Ownership, derived from the kernels and asserted per launch: ``in`` is never written; ``out`` is written in the
launch's range by the plain and the fused two-shot kernel, in this rank's shard of units by allreduce_fc_fused, and not
at all by the fused one-shot kernel and conv_reduce_fused (whose parts update exactly the parameters they sink: part
[0, 289) leaves conv1 alone, part [289, 309) leaves conv2 and w2f / w2d alone); state outside the bucket, the other bucket's shadows, the gradient buffer and
every other channel's flags and staging slots keep their bits; the step counter moves by one when state_inc is
given to the fused two-shot, one-shot and conv kernels, and never in allreduce_fc_fused, which does not read state_inc.

World 1 runs in this process; worlds 2, 3 and 5 share GPU 0 through one spawn each (process set-up of
tools/xgmi_check.py), cached per module.  tests/test_xgmi_oracle_cpu.py proves that these checks fail on subtly wrong
kernels.
"""
import os
import sys
import time

import pytest
import torch

from pytorch_mnist_ddp_amd.ops import functional as Fk

import refmodel as R
import xgmi_stage_cases as XC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parent deadline per world: 3 x the first measured run of the case list (docs/COVERAGE.md 2.6), process start included
DEADLINE_S = {2: 18, 3: 27, 5: 47}
_records = {}


def _world(W, dev=None):
    if W not in _records:
        t0 = time.perf_counter()
        if W == 1:
            _records[W] = {0: (True, XC.run_cases(1, 0, dev))}
        else:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import xgmi_check
            res, codes = xgmi_check.spawn_world(W, XC.worker, None, DEADLINE_S[W])
            _records[W] = {r: res.get(r, (False, f"no result (exit code {codes[r]})")) for r in range(W)}
        print(f"xgmi stages world {W}: {time.perf_counter() - t0:.1f} s")
    return _records[W]


def _assert_world(W, res):
    for r in range(W):
        ok, recs = res[r]
        assert ok, f"world {W} rank {r}: {recs}"
        bad = [f"{c['case']}: {c['msg']}" for c in recs if not c["ok"]]
        for c in recs:
            for k, v in c["stats"].items():
                print(f"W{W} r{r} {c['case']} | {k} {v[0]:.3g} {v[1]:.3g}")
        assert not bad, f"world {W} rank {r}: {len(bad)} of {len(recs)} cases failed: " + " | ".join(bad[:6])
        assert sum(c["case"].startswith("conv fused parts [289") for c in recs) == (3 if W == 1 else 2), f"world {W} rank {r}: the case list stopped early"


def test_world1_cases(cuda_device):
    _assert_world(1, _world(1, cuda_device))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("W", [2, 3, 5])
def test_shared_gpu_world_cases(cuda_device, W):
    _assert_world(W, _world(W))


# ------------------------------------------------------------------ the support kernels of comm_kernels.hip
@pytest.mark.parametrize("s", [1 / 3, 1 / 8])
def test_scale_copy_bitwise(cuda_device, s):
    g = torch.Generator().manual_seed(3)
    for n in (0, 1, 3, 4, 5, 1023, 1024, 1025, 262144 + 3):
        for do in (0, 1):
            for so in (0, 1):                                   # 16-byte aligned, or off by one float: the scalar path
                src = torch.randn(n + 12, generator=g)
                dst = torch.full((n + 12,), R.XG_SENTINEL, device=cuda_device)
                src_d = src.to(cuda_device)
                d, sv = dst[4 + do:], src_d[4 + so:]
                assert d.data_ptr() % 16 == 4 * do and sv.data_ptr() % 16 == 4 * so
                Fk.scale_copy(d, sv, n, s)
                torch.cuda.synchronize()
                got = dst.cpu()
                want = src[4 + so:4 + so + n] * torch.tensor(s, dtype=torch.float32)
                assert torch.equal(got[4 + do:4 + do + n].view(torch.int32), want.view(torch.int32)), (n, do, so)
                assert (got[:4 + do] == R.XG_SENTINEL).all() and (got[4 + do + n:] == R.XG_SENTINEL).all(), (n, do, so)
                assert torch.equal(src_d.cpu().view(torch.int32), src.view(torch.int32))


@pytest.mark.parametrize("value", [0, 0xA5])
def test_fill_bytes_exact(cuda_device, value):
    sent = 0x3C
    sizes = [(a, n) for a in range(16) for n in range(49)] + [(a, n) for a in (0, 5) for n in (4097, (1 << 20) + 5)]
    for a, n in sizes:
        buf = torch.full((n + 64,), sent, dtype=torch.uint8, device=cuda_device)
        assert buf.data_ptr() % 16 == 0
        Fk.fill_bytes(buf[16 + a:], n, value)
        torch.cuda.synchronize()
        got = buf.cpu()
        assert (got[16 + a:16 + a + n] == value).all(), (a, n)
        assert (got[:16 + a] == sent).all() and (got[16 + a + n:] == sent).all(), (a, n)


def test_gather_rows_bitwise(cuda_device):
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, 256, (40, 784), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 10, (40,), generator=g, dtype=torch.int32)
    for n in (1, 3, 4, 5, 257):
        for start in (0, 7):
            rows = start + n + 3
            idx = torch.randint(0, 40, (rows,), generator=g, dtype=torch.int32)
            idx[start:start + min(n, 4)] = torch.tensor([39, 39, 38, 0], dtype=torch.int32)[:min(n, 4)]   # duplicates, descending
            dst = torch.full((rows, 784), 0xEE, dtype=torch.uint8, device=cuda_device)
            dlab = torch.full((rows,), -5, dtype=torch.int32, device=cuda_device)
            Fk.gather_rows(src.to(cuda_device), lab.to(cuda_device), idx.to(cuda_device), start, n, dst, dlab)
            torch.cuda.synchronize()
            got, gl = dst.cpu(), dlab.cpu()
            sel = idx[start:start + n].long()
            assert torch.equal(got[start:start + n], src[sel]) and torch.equal(gl[start:start + n], lab[sel]), (n, start)
            keep = torch.ones(rows, dtype=torch.bool)
            keep[start:start + n] = False
            assert (got[keep] == 0xEE).all() and (gl[keep] == -5).all(), (n, start)
