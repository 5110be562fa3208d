"""CPU proof of the collective-kernel checks (no GPU).

tests/refmodel.py's XgWorld walks the index sets of the four kernels of csrc/kernels/xgmi_allreduce.hip over W ranks'
buffers in numpy.  Here, for W = 1 .. 8 and the grids tests/test_gpu_xgmi_stages.py may meet (that test repeats the
coverage count for the grid it actually gets before it launches):
  - coverage: every bucket element is reduced and updated exactly once, nothing outside the bucket is touched;
  - the chained model gives, bit for bit, the rank-ordered fp32 sum followed by the emulation of Ada::step and
    stage_shadows, and passes the comparators that the GPU test applies to the kernels;
  - each of the thirteen single mutations of XG_MUTATIONS fails those comparators.
"""
import numpy as np
import pytest
import torch

import refmodel as R
from refmodel import OFF_CONV, PARAM_TOTAL, XG_CONV_N, XG_FC_N, XgWorld

WORLDS = range(1, 9)
NAN = float("nan")
FC_GRIDS = (1, 8, 37, 73, 116, 145, 289, 577)        # capped by the natural grid ceil(577 / W)
CONV_GRIDS = {(0, 309): (39, 40, 77, 155, 309), (0, 289): (37, 39, 145, 289), (289, 309): (3, 7, 20)}
SHADOW_SENTINEL = 0x4000                                       # bf16 2.0 in every shadow before a launch


def _before():
    case = R.ada_case()
    d = {k: case[k].clone() for k in R.ADA_STATE}
    for k, src in R.shadow_sources().items():
        d[k] = torch.full((src.numel(),), SHADOW_SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    d["grad"] = torch.zeros(PARAM_TOTAL)
    return d


def _flat_inputs(W, offset, count, case=0, edges=(), poison=None):
    """Per rank a flat [PARAM_TOTAL] vector: the bucket's values in [offset, offset + count), NaN elsewhere."""
    at = [e - offset for e in R.ADA_POISON if offset <= e < offset + count]
    out = []
    for q in range(W):
        v = torch.full((PARAM_TOTAL,), NAN)
        v[offset:offset + count] = R.xg_bucket(7, case, q, W, count, edges, poison, at)
        out.append(v)
    return out


def _own(offset, count):
    return R.own_mask(offset, offset + count)


def _fused_checks(before, after, own, shadows, ins, lr, wd, name):
    g32 = R.xg_ordered_sum(ins)
    g64 = torch.stack([v.to(R.F64) for v in ins]).sum(0)
    stats = R.xg_check_update(before, after, own, g32, g64, lr, wd, name)
    R.check_ownership(before, after, own, shadows, name=name)
    return stats


# ------------------------------------------------------------------ 1. coverage, pure index arithmetic
def _assert_cover(w, lo, hi, out=None, shadows=(), what=""):
    """Adadelta steps: exactly one per flat element of [lo, hi), none elsewhere; out stores: one per float of
    ``out`` = (lo, hi) or index array, none elsewhere; the named shadows written once per element, the others never."""
    want = np.zeros(PARAM_TOTAL, np.int32)
    want[lo:hi] = 1
    assert np.array_equal(w.n_upd, want), f"{what}: updates {np.flatnonzero(w.n_upd != want)[:8]}"
    want = np.zeros(len(w.n_out), np.int32)
    if out is not None:
        want[out if isinstance(out, np.ndarray) else slice(*out)] = 1
    assert np.array_equal(w.n_out, want), f"{what}: out stores {np.flatnonzero(w.n_out != want)[:8]}"
    for k, n in w.n_shadow.items() if shadows is not None else ():
        assert (n == (1 if k in shadows else 0)).all(), f"{what}: shadow {k}"


@pytest.mark.parametrize("W", WORLDS)
def test_coverage_twoshot_and_oneshot(W):
    nvecs = sorted({1, max(1, W - 1), W, W + 1, 513 * W + 1, 32772 // 4})
    for r in range(W):
        for nvec in nvecs:
            for off in (0, 4, 4096):
                for fuse in (False, True):
                    for G in {1, R.xg_grid("twoshot", W, nvec, fuse)}:
                        w = XgWorld(W, r, None, arith=False)
                        w.twoshot(off, 4 * nvec, G, fuse=fuse)
                        _assert_cover(w, *((off, off + 4 * nvec) if fuse else (0, 0)), out=(off, off + 4 * nvec),
                                      what=f"twoshot W{W} r{r} nvec{nvec} off{off} fuse{fuse} G{G}")
        for count in (4, 1020, 1024, 1028, 4100, 32768, XG_CONV_N):
            nvec = count // 4
            for planned in (XG_CONV_N // 4 // 256 + 1, 8, 1, R.XG_MAX_WG):
                G = R.xg_grid("oneshot", W, nvec, planned=planned)
                assert G * 1024 >= nvec, "the KMAX floor"
                for fuse in (False, True) if OFF_CONV + count <= PARAM_TOTAL else (False,):
                    w = XgWorld(W, r, None, arith=False)
                    w.oneshot(OFF_CONV if fuse else 0, count, G, fuse=fuse)
                    lo = OFF_CONV if fuse else 0
                    _assert_cover(w, *((lo, lo + count) if fuse else (0, 0)), out=None if fuse else (0, count),
                                  shadows=("w2f", "w2d") if fuse and count == XG_CONV_N else None if fuse else (),
                                  what=f"oneshot W{W} r{r} count{count} G{G} fuse{fuse}")


def test_coverage_twoshot_fc_range():
    for W in WORLDS:
        for r in {0, W // 2, W - 1}:
            for G in {R.xg_grid("twoshot", W, XG_FC_N // 4, True), 64, 1}:
                w = XgWorld(W, r, None, arith=False)
                w.twoshot(0, XG_FC_N, G, fuse=True)
                _assert_cover(w, 0, XG_FC_N, out=(0, XG_FC_N), what=f"twoshot fc W{W} r{r} G{G}")


@pytest.mark.parametrize("W", WORLDS)
def test_coverage_fc_fused(W):
    assert [R.xg_fc_lo(p, W) for p in (0, W)] == [0, R.XG_UNITS]
    for r in range(W):
        own = (4 * R.xg_fc_own_f4(r, W)[:, None] + np.arange(4)).reshape(-1)
        for G in sorted({R.xg_grid("fc", W, planned=g) for g in FC_GRIDS}):
            w = XgWorld(W, r, None, arith=False)
            w.fc_fused(G)
            _assert_cover(w, 0, XG_FC_N, out=own, shadows=("w1", "w1t"), what=f"fc_fused W{W} r{r} G{G}")


def test_coverage_conv_fused():
    sink = {(lo, hi): R.conv_sink_elements(lo, hi).numpy() for lo, hi in CONV_GRIDS}
    for (lo, hi), grids in CONV_GRIDS.items():
        for planned in grids:
            for W in WORLDS:                                     # (the partition does not depend on W or the rank)
                G = R.xg_grid("conv", W, planned=planned, lo=lo, hi=hi)
                w = XgWorld(W, W - 1, None, arith=False)
                w.conv_fused(None, G, lo, hi)
                want = np.zeros(PARAM_TOTAL, np.int32)
                want[sink[(lo, hi)]] = 1
                assert np.array_equal(w.n_upd, want), (lo, hi, G, W)
                assert not w.n_out.any()
                for k, n in w.n_shadow.items():
                    assert (n == (1 if lo == 0 and k in ("w2f", "w2d") else 0)).all(), (lo, hi, G, k)
    with pytest.raises(AssertionError, match="virtual blocks"):   # below the launcher's floor the slots run out
        XgWorld(1, 0, None, arith=False).conv_fused(None, 38)


def test_grid_arithmetic():
    assert R.xg_grid("conv", 1, planned=309, max_wg=39) == 39 and R.xg_grid("conv", 1, planned=309, max_wg=1) == 39
    assert R.xg_grid("conv", 1, planned=20, lo=289, hi=309, max_wg=1) == 3
    assert R.xg_grid("fc", 1, planned=577) == 512 and R.xg_grid("fc", 5, planned=577, max_wg=8) == 8
    assert R.xg_grid("fc", 3, planned=100, max_wg=400) == 100, "max_wg never widens the planned grid"
    assert R.xg_grid("oneshot", 2, 8192, planned=512, max_wg=1) == 8
    assert R.xg_grid("twoshot", 3, 513 * 3 + 1, planned=512) == 2 and R.xg_grid("twoshot", 1, 295280, True) == 512


# ------------------------------------------------------------------ 2. the chained model against the straight one
CFGS = ((1.0, 0.0), (0.7, 0.01))


@pytest.mark.parametrize("W", (1, 2, 3, 5, 8))
def test_plain_allreduce_models_give_the_ordered_sum(W):
    for r in {0, W - 1}:
        for kind, off, nvec, G in (("twoshot", 4, 513 * W + 1, 1), ("twoshot", 4096, W + 1, 1), ("twoshot", 0, 2 * W + 1, 3),
                                   ("twoshot", 0, max(1, W - 1), 1), ("oneshot", 0, 1025, 2), ("oneshot", 0, 255, 1)):
            n = off + 4 * nvec + 8
            w = XgWorld(W, r, [torch.zeros(n)] * W)
            for call in range(3):                                    # fresh inputs; both staging parities, a slot's reuse
                ins = [torch.full((n,), NAN) for _ in range(W)]
                for q in range(W):
                    ins[q][off:off + 4 * nvec] = R.xg_bucket(3, call, q, W, 4 * nvec, edges=[4 * _c(nvec, W) * p for p in range(W)])
                w.set_inputs(ins)
                w.out[r][:] = R.XG_SENTINEL
                getattr(w, kind)(off, 4 * nvec, G)
                got = torch.from_numpy(w.out[r].copy())
                R.xg_check_reduce(got[off:off + 4 * nvec], [v[off:off + 4 * nvec] for v in ins], f"{kind} W{W}")
                assert (got[:off] == R.XG_SENTINEL).all() and (got[off + 4 * nvec:] == R.XG_SENTINEL).all()


def _c(a, b):
    return -(-a // b)


def _run_fused(kind, W, r, lr, wd, G, mut=None, poison=None, calls=1, **kw):
    """``calls`` launches of one fused kernel on the seeded state; returns what the comparators need of the last."""
    before = _before()
    if kind == "fc":
        off, count, shadows = 0, XG_FC_N, ("w1", "w1t")
    elif kind in ("twoshot", "oneshot"):
        off, count = kw["offset"], kw["count"]
        shadows = ("w2f", "w2d") if (off, count) == (OFF_CONV, XG_CONV_N) else ()
    else:
        off, count = OFF_CONV, XG_CONV_N
        shadows = ("w2f", "w2d") if kw.get("lo", 0) == 0 else ()
    own = _own(off, count)
    if kind == "conv":
        own = R.own_mask(idx=R.conv_sink_elements(kw.get("lo", 0), kw.get("hi", 309)))
    S4 = _c(count // 4, W)
    edges = [4 * S4 * p for p in range(1, W)] + [4 * int(R.xg_fc_f4(R.xg_fc_lo(p, W), 0)[0]) for p in range(1, W) if kind == "fc"]
    w = None
    for call in range(calls):
        ins = _flat_inputs(W, off, count, case=call, edges=edges, poison=poison if call == calls - 1 else None)
        if w is None:
            w = XgWorld(W, r, ins, before, lr, wd)
        else:                                                       # fresh inputs, the seeded state again
            w.set_inputs(ins)
            w.st = {k: before[k].numpy().copy() for k in R.ADA_STATE}
        if kind == "fc":
            w.fc_fused(G, mut=mut)
        elif kind == "conv":
            w.conv_fused([v[OFF_CONV:].numpy() for v in ins], G, kw.get("lo", 0), kw.get("hi", 309), mut=mut)
        else:
            getattr(w, kind)(off, count, G, fuse=True, mut=mut)
    return before, w.snap(before["grad"]), own, shadows, ins, w


@pytest.mark.parametrize("W", (1, 2, 3, 5, 8))
def test_fused_models_equal_sum_then_update(W):
    r = W // 2
    for lr, wd in CFGS:
        small = dict(offset=OFF_CONV + 64, count=4 * (2 * W + 1))   # ragged (nvec % W != 0), ada_base != 0
        for kind, G, kw in (("twoshot", 1, small), ("twoshot", R.xg_grid("twoshot", W, XG_FC_N // 4, True), dict(offset=0, count=XG_FC_N)),
                            ("oneshot", 5, dict(offset=OFF_CONV, count=XG_CONV_N)), ("fc", R.xg_grid("fc", W, planned=145), {}),
                            ("fc", 8, {}), ("conv", 309, {}), ("conv", 39, {}), ("conv", 37, dict(lo=0, hi=289)),
                            ("conv", 20, dict(lo=289, hi=309))):
            if (kind == "fc" and (lr, wd) != CFGS[1] and G != 8) or (kind == "twoshot" and kw is not small and wd == 0):
                continue                                             # the big buckets once per grid
            before, after, own, shadows, ins, w = _run_fused(kind, W, r, lr, wd, G, calls=2 if kind in ("oneshot", "conv") else 1, **kw)
            _fused_checks(before, after, own, shadows, ins, lr, wd, f"{kind} W{W} G{G}")


@pytest.mark.parametrize("poison", [NAN, float("inf")])
def test_non_finite_gradient_reaches_exactly_its_elements(poison):
    for kind, W, G, kw in (("fc", 3, 64, {}), ("conv", 2, 39, {}), ("oneshot", 3, 5, dict(offset=OFF_CONV, count=XG_CONV_N))):
        before, after, own, shadows, ins, w = _run_fused(kind, W, 0, 0.7, 0.01, G, poison=poison, **kw)
        _fused_checks(before, after, own, shadows, ins, 0.7, 0.01, kind)
        hit = torch.tensor([e for e in R.ADA_POISON if own[e]])
        assert len(hit) and torch.isnan(after["param"][hit]).all()
        assert int(torch.isnan(after["param"]).sum()) == len(hit)


# ------------------------------------------------------------------ 3. every single mutation fails
MUTANTS = {   # mutation -> the launches on which the GPU test's comparators must catch it
    "rank_order_reversed": (("fc", 3, 1, 64, {}), ("conv", 3, 0, 39, {})),
    "peer_skipped": (("fc", 2, 0, 64, {}), ("oneshot", 3, 1, 5, dict(offset=OFF_CONV, count=XG_CONV_N))),
    "peer_twice": (("fc", 5, 4, 8, {}), ("conv", 2, 1, 309, {})),
    "own_shard_not_updated": (("twoshot", 3, 1, 1, dict(offset=OFF_CONV + 64, count=28)),),
    "own_shard_twice": (("twoshot", 3, 1, 1, dict(offset=OFF_CONV + 64, count=28)),),
    "ragged_last_dropped": (("twoshot", 3, 2, 1, dict(offset=OFF_CONV + 64, count=28)),),
    "stale_slot": (("oneshot", 2, 0, 5, dict(offset=OFF_CONV, count=XG_CONV_N, calls=2)), ("conv", 3, 1, 39, dict(calls=2))),
    "shadows_from_old_param": (("fc", 2, 1, 64, {}), ("conv", 1, 0, 39, {}), ("oneshot", 1, 0, 5, dict(offset=OFF_CONV, count=XG_CONV_N))),
    "w1t_untransposed": (("fc", 1, 0, 64, {}),),
    "tail_368_written": (("fc", 1, 0, 64, {}), ("fc", 5, 2, 8, {})),
    "ada_base_off": (("twoshot", 2, 0, 1, dict(offset=OFF_CONV + 64, count=28)), ("oneshot", 2, 0, 1, dict(offset=OFF_CONV, count=320))),
    "conv1_part_touches_conv2": (("conv", 2, 0, 20, dict(lo=289, hi=309)),),
    "wd_before_sum": (("fc", 2, 0, 64, {}), ("conv", 3, 0, 39, {}), ("twoshot", 3, 1, 1, dict(offset=OFF_CONV + 64, count=28))),
}


def test_the_mutation_list_is_complete():
    assert set(MUTANTS) == set(R.XG_MUTATIONS) and len(R.XG_MUTATIONS) == 13


@pytest.mark.parametrize("mut", R.XG_MUTATIONS)
def test_single_mutation_fails(mut):
    lr, wd = CFGS[1]
    for kind, W, r, G, kw in MUTANTS[mut]:
        kw = dict(kw)
        calls = kw.pop("calls", 1)
        before, after, own, shadows, ins, w = _run_fused(kind, W, r, lr, wd, G, calls=calls, **kw)
        _fused_checks(before, after, own, shadows, ins, lr, wd, "unmutated")
        before, after, own, shadows, ins, w = _run_fused(kind, W, r, lr, wd, G, mut=mut, calls=calls, **kw)
        with pytest.raises(AssertionError):
            _fused_checks(before, after, own, shadows, ins, lr, wd, f"{mut} on {kind} W{W}")


@pytest.mark.parametrize("mut", ("rank_order_reversed", "peer_skipped", "peer_twice", "stale_slot"))
def test_single_mutation_fails_the_plain_reduce(mut):
    W, r, nvec = 3, 1, 1025
    for kind, G in (("twoshot", 1), ("oneshot", 2)):
        if mut == "stale_slot" and kind == "twoshot":
            continue
        w = XgWorld(W, r, [torch.zeros(4 * nvec)] * W)
        for call in range(2):
            ins = [R.xg_bucket(5, call, q, W, 4 * nvec, edges=[1368, 2736]) for q in range(W)]
            w.set_inputs(ins)
            getattr(w, kind)(0, 4 * nvec, G, mut=mut)
        with pytest.raises(AssertionError):
            R.xg_check_reduce(torch.from_numpy(w.out[r]), ins, mut)
