"""The fp32-path stage oracle and its checks (tests/refmodel.py f32o_* / f32_check), proved on the CPU.

* the float64 stages, chained, give reference_step(dtype=float64)'s parameter gradients and loss;
* a stand-in for the kernels of f32_net.hip built from torch fp32 CPU ops (refmodel.f32_twin, the kernels' own
  layouts) passes every check that tests/test_gpu_fp32_stages.py applies, at that test's shapes and input forms,
  with the share of decisions below margin under the cap;
* each single subtle mutation of the stand-in fails the check of the stage it sits in.
"""
import functools

import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8

import refmodel as R
from refmodel import F64, F32Cfg


def _machine(cfg, hand=False, **kw):
    return R.F32Machine(cfg, R.f32_make(cfg, hand)[1], **kw)


# ------------------------------------------------------------------ the chained oracle == the float64 step
@pytest.mark.parametrize("B,flags", [(3, 0), (3, 1), (33, 0), (33, 1)])
def test_chained_f32_oracle_is_the_float64_step(B, flags):
    cfg = F32Cfg(B, flags=flags)
    net = R.trained_net()
    param = R.f32_flat_params(net)
    data, labels, idx = R.f32_dataset(B)
    src = cfg.rows(idx)
    u8, y = data[src].view(B, 28, 28), labels[src].long()
    x = normalize_u8(u8).reshape(B, 784)
    pr = R.f32o_prep(param)
    a1 = R.f32o_conv1(x, param)
    pool = R.f32o_pool(R.f32o_conv2(a1, pr["w2fwd"], param), cfg)
    S = R.f32_splits(B)["fc1"]
    hd = R.f32o_head(R.stage_fc1_partials(pool["p"], R.f32_params(param)["fc1.weight"], S), param, y, cfg)
    got = R.f32o_fc_small(hd["h"], hd["dl"], hd["dz1"], hd["nll"])
    got["fc1.weight"] = R.f32o_fc1w(hd["dz1"], pool["p"])
    dy2 = R.f32o_fc1x(hd["dz1"], pr["w1p"], pool["pm"], cfg)["dy2"]
    dx1 = R.f32o_conv2x(dy2, pr["w2bwd"], a1)["dx1"]
    got.update(R.f32o_conv_reduce(R.f32o_conv2w(dy2, a1), R.f32o_conv1w(dx1, x)))
    k1 = pool["keep"] if cfg.dropout else None
    loss, _, want = R.reference_step(net, u8, y, k1, hd["keep2"], dtype=F64)
    # the oracle takes the launch's own fp32 scalars (inv_batch = float32(1/B), float32(1/0.75)): 6e-8 relative each
    for k, w in want.items():
        assert R.rel_err(got[k], w) < 2e-7, (k, R.rel_err(got[k], w))
    assert abs(float(got["loss"]) - float(loss)) < 1e-7 * float(loss)
    if cfg.dropout:
        assert 0.70 < float(pool["keep"].mean()) < 0.80 and 0.4 < float(hd["keep2"].mean()) < 0.6
    else:
        assert bool(((pool["pm"] >> 2) & 1 == 1).all())


def test_f32_split_rules_reach_the_edges():
    """The shapes of the GPU test reach the edges they are chosen for."""
    sp = {B: R.f32_splits(B) for B in R.F32_TRUNK_B}
    assert (sp[1]["conv2w_kc"], sp[1]["conv2w"]) == (16, 36) and sp[3]["conv2w"] == 108
    assert (sp[33]["conv2w_kc"], sp[33]["conv2w"]) == (160, 119) and 33 * 576 % 160 != 0
    assert (sp[65]["conv2w_kc"], sp[65]["conv2w"]) == (304, 124) and 304 % 32 != 0 and 65 * 576 % 304 != 0
    assert 676 * 1 < 1024 and (3 * 676) % 128 != 0                      # empty conv1 slabs; a ragged 128-row tile
    b = torch.arange(1025) * (3 * 676) // 1024
    assert bool(((b[:-1] // 676) != ((b[1:] - 1) // 676)).any())        # a conv1 slab straddling two images
    assert R.f32_splits(1024)["fc1"] == 36 and R.f32_splits(1025)["fc1"] == 9 and 257 > 256


# ------------------------------------------------------------------ the stand-in passes, the caps hold
CASES = {
    "idx dropout": dict(),
    "pre-gathered, no dropout": dict(use_idx=False, flags=1),
    "world 2": dict(world=2),
}


@pytest.mark.parametrize("B", R.F32_TRUNK_B)
def test_standin_passes_every_check(B):
    st = R.f32_run_chain(_machine(F32Cfg(B)), R.F32_TRUNK_STAGES)
    assert set(st) == set(R.F32_TRUNK_STAGES)


@pytest.mark.parametrize("form", list(CASES)[1:])
def test_standin_passes_input_forms(form):
    R.f32_run_chain(_machine(F32Cfg(33, **CASES[form])), R.F32_TRUNK_STAGES, repeat=False)


@pytest.mark.parametrize("B", (3, 33))
def test_standin_passes_eval_form(B):
    R.f32_run_chain(_machine(F32Cfg(B, train=False)), R.F32_EVAL_STAGES, repeat=False)


@pytest.mark.parametrize("B", R.F32_HAND_B)
def test_standin_passes_hand_made(B):
    R.f32_run_chain(_machine(F32Cfg(B), hand=True), R.F32_HAND_STAGES, hand=True, repeat=False)


# ------------------------------------------------------------------ single mutations each fail
@functools.lru_cache(maxsize=None)
def _states(B, world=1):
    """The buffers after the forward stages and after the whole chain (fc1x overwrites y2), un-mutated."""
    m = _machine(F32Cfg(B, world=world))
    R.f32_run_chain(m, R.F32_TRUNK_STAGES[:6], repeat=False)
    fwd = m.snapshot()
    for st in R.F32_TRUNK_STAGES[6:]:
        m.launch(st)
    return fwd, m.snapshot()


MUTATIONS = [                                   # (mutation, stage, B, world, the check that must catch it)
    ("bias_wrong_n", "conv2w", 3, 1, "c2part"),
    ("last_slab_dropped", "conv_reduce", 33, 1, "conv2"),
    ("stale_slab", "conv_reduce", 33, 1, "conv2"),
    ("w2bwd_taps_transposed", "prep", 3, 1, "w2bwd is not the permutation"),
    ("w1p_swapped", "prep", 3, 1, "w1p is not the permutation"),
    ("last_max_wins", "pool", 3, 1, "argmax code"),
    ("pooled_geq", "pool", 3, 1, "pooled > 0 bit"),
    ("philox_offset", "pool", 3, 1, "keep bits differ from Philox|p"),
    ("wrong_quadrant", "fc1x", 3, 1, "dy2"),
    ("drop1_scale_missing", "fc1x", 3, 1, "dy2"),
    ("drop2_scale_missing", "head", 3, 1, "dz1"),
    ("inv_batch_no_world", "head", 3, 2, "dz1|dl"),
    ("dl_no_label", "head", 3, 1, "dz1|dl"),
    ("head_12_partials", "head", 3, 1, "loss_rows|h"),
    ("relu_geq", "conv2x_conv1w", 3, 1, "dx1"),
    ("c1w_range_off_by_one", "conv2x_conv1w", 3, 1, "c1part"),
    ("loss_padded_B", "fc_small", 3, 1, "loss_log"),
    ("guard_row_written", "conv1", 3, 1, "outside what the stage owns"),
    ("guard_row_written", "fc1", 3, 1, "outside what the stage owns"),
    ("guard_row_written", "head", 3, 1, "outside what the stage owns"),
    ("guard_row_written", "conv2w", 3, 1, "outside what the stage owns"),
]


@pytest.mark.parametrize("mut,stage,B,world,caught", MUTATIONS, ids=[f"{m[0]}-{m[1]}" for m in MUTATIONS])
def test_single_mutation_fails(mut, stage, B, world, caught):
    fwd, full = _states(B, world)
    base = fwd if stage in R.F32_TRUNK_STAGES[:6] else full
    if stage in ("fc1x",):                      # fc1x reads nothing that it or a later stage overwrites
        base = full
    t = {k: v.clone() for k, v in base.items()}
    good = R.F32Machine(F32Cfg(B, world=world), {k: v.clone() for k, v in t.items()})
    R.f32_run_stage(good, stage, repeat=False)                            # the same state passes un-mutated
    with pytest.raises(AssertionError, match=caught):
        R.f32_run_stage(R.F32Machine(F32Cfg(B, world=world), t, mut=mut), stage, repeat=False)
