"""T1: every kernel of the fp32 step (csrc/kernels/f32_net.hip) on its own against the float64 stage oracle
(MI355X only).

f32_prep, f32_conv1, the MFMA GEMM behind its six policies (conv2 forward, fc1, fc1 weight / input gradient, conv2
weight / input gradient), f32_pool, f32_head (train and eval), f32_fc_small, f32_conv1w and f32_conv_reduce are
launched one at a time through the stage mask of launch_f32_forward and the backward launchers, over
sentinel-filled buffers that each carry a guard row or slab (ops.functional.F32Buffers).  Around every launch all
buffers are copied back: what the stage does not own must keep its bits, what it owns is compared element by
element with refmodel's f32o_* oracle on the operands the kernel read, and a second launch must give the same bits
(refmodel.f32_run_stage).  eps = 8 x max |torch fp32 CPU op - float64| on the same operands, not below 4 fp32 ulps
(head tensors 16) of the largest reference value; a measured 0 means exact agreement.  Batch sizes 1, 3, 33 and 65
run the whole chain on the trained net (dropout on, step 3, rows through the index vector); 257 and 1025 run the
fc kernels on hand-made operands.  tests/test_fp32_oracle_cpu.py proves on the CPU that these checks fail on
subtly wrong outputs.  Each test prints `stage B tensor deviation eps measured` (docs/COVERAGE.md 2.4).
"""
import pytest
import torch

from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native

import refmodel as R
from refmodel import F32Cfg

pytestmark = pytest.mark.gpu


def _report(stage, B, stats):
    for name, v in stats.items():
        tail = f"  measured {v[2]:10.3e}{'  floor' if v[0] > v[2] else ''}" if len(v) == 3 else ""
        print(f"\nf32 {stage:14s} B={B:<5d} {name:24s} dev {v[0]:10.3e}  eps {v[1]:10.3e}{tail}", end="")


class GpuMachine(R.F32Machine):
    """The buffers on the device; ``launch`` is one launch of the real kernels."""

    def __init__(self, dev, cfg, hand=False):
        self.buf, t = R.f32_make(cfg, hand, dev)
        super().__init__(cfg, t)

    def _args(self):
        c, t = self.cfg, self.t
        return dict(param=t["param"], data_u8=t["data_u8"], labels=t["labels"], idx=t["idx"] if c.use_idx else None,
                    idx_stride=c.stride, state=t["state"] if c.train else None, inv_batch=c.inv_batch,
                    out_row=R.F32_OUT_ROW)

    def launch(self, stage):
        if stage in R.F32_FWD or isinstance(stage, int):
            mask = stage if isinstance(stage, int) else R.F32_FWD[stage]
            Fk.f32_forward(self.buf, train=self.cfg.train, stages=mask, **self._args())
        else:
            Fk.f32_backward(self.buf, R.F32_BWD[stage], grad=self.t["grad"], loss_log=self.t["loss_log"], **self._args())
        torch.cuda.synchronize()


def test_host_split_rules_and_stage_constants(cuda_device):
    C = native.load()
    assert (C.F32_MAX_SPLITS, C.F32_C1W_BLOCKS, C.F32_STAGE_ALL) == (Fk.F32_MAX_SPLITS, Fk.F32_C1W_BLOCKS, Fk.F32_FWD_ALL)
    assert sum(R.F32_FWD.values()) == Fk.F32_FWD_ALL and R.F32_BWD["conv_reduce"] == Fk.F32_CONV_REDUCE
    for B in R.F32_TRUNK_B + R.F32_HAND_B + (1024, 4096):
        sp = R.f32_splits(B)
        assert (C.f32_fc1_splits(B), C.f32_conv2w_splits(B), C.f32_conv1w_splits(B)) == \
            (sp["fc1"], sp["conv2w"], sp["conv1w"]), B
        assert sp["fc1"] == Fk.f32_fc1_splits(B) and sp["conv2w"] <= C.F32_MAX_SPLITS
    sp = {B: R.f32_splits(B) for B in R.F32_TRUNK_B}
    assert (sp[1]["conv2w_kc"], sp[1]["conv2w"]) == (16, 36) and sp[3]["conv2w"] == 108          # half a k-tile
    assert (sp[33]["conv2w_kc"], sp[33]["conv2w"]) == (160, 119) and 33 * 576 % 160 != 0        # ragged last split
    assert sp[65]["conv2w_kc"] == 304 and 304 % 32 != 0 and 65 * 576 % 304 != 0                 # chunk off the k-tile
    assert C.f32_fc1_splits(1025) == 9 and 1025 % 4 == 1 and 257 > 256
    with pytest.raises(RuntimeError):
        Fk.f32_forward(Fk.F32Buffers.allocate(1, cuda_device), torch.zeros(1), torch.zeros(1), torch.zeros(1), stages=64)


@pytest.mark.parametrize("B", R.F32_TRUNK_B)
def test_every_stage_on_the_real_chain(cuda_device, B):
    """Rows through idx with idx_step_stride = B at step 3, dropout on."""
    R.f32_run_chain(GpuMachine(cuda_device, F32Cfg(B)), R.F32_TRUNK_STAGES, report=_report)


def test_pregathered_rows_without_dropout(cuda_device):
    """idx null (row b of step 3 is dataset row 3B + b) and STEP_FLAG_NO_DROPOUT: p unscaled, every keep bit set
    (nothing is drawn), dscale = 1 in the fc1 input gradient."""
    m = GpuMachine(cuda_device, F32Cfg(33, use_idx=False, flags=1))
    R.f32_run_chain(m, R.F32_TRUNK_STAGES, report=_report, repeat=False)


def test_inv_batch_of_a_world_of_two(cuda_device):
    m = GpuMachine(cuda_device, F32Cfg(33, world=2))
    R.f32_run_chain(m, R.F32_TRUNK_STAGES, report=_report, repeat=False)


@pytest.mark.parametrize("B", (3, 33))
def test_eval_form(cuda_device, B):
    """Null state, stride 0, loss_rows / correct at an offset pointer; w1p and pm keep their sentinels."""
    m = GpuMachine(cuda_device, F32Cfg(B, train=False))
    R.f32_run_chain(m, R.F32_EVAL_STAGES, report=_report)
    after = m.snapshot(("w1p", "pm", "h", "dz1", "dl"))
    assert all(bool((R.f32_bits(v) == (R.F32_SENT_B if v.dtype == torch.uint8 else R.F32_SENT_F)).all())
               for v in after.values())


@pytest.mark.parametrize("B", R.F32_HAND_B)
def test_fc_kernels_on_hand_made_operands(cuda_device, B):
    """257: the second trip of fc_small's 256-row loop; 1025: the 9-way fc1 split (a partial group of 12 in the
    head), M / N one past a tile."""
    R.f32_run_chain(GpuMachine(cuda_device, F32Cfg(B), hand=True), R.F32_HAND_STAGES, hand=True, report=_report)


def test_masked_launches_equal_the_all_stages_launch(cuda_device):
    """Six single-stage launches leave bit for bit what one launch of all stages leaves (train and eval)."""
    for train in (True, False):
        cfg = F32Cfg(33, train=train)
        one, six = GpuMachine(cuda_device, cfg), GpuMachine(cuda_device, cfg)
        one.launch(Fk.F32_FWD_ALL)
        for st in R.F32_EVAL_STAGES:
            six.launch(st)
        a, b = one.snapshot(), six.snapshot()
        for k in a:
            assert torch.equal(R.f32_bits(a[k]), R.f32_bits(b[k])), (train, k)
        assert not torch.isnan(a["loss_rows"][R.F32_OUT_ROW:R.F32_OUT_ROW + 33]).any()
