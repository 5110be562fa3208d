"""The case list of tests/test_gpu_xgmi_stages.py, run by one rank of a world of W (in the pytest process at W = 1,
in spawned ranks that share GPU 0 at W > 1).  Every rank builds every rank's inputs from (seed, case, call, rank) on
the CPU, so it computes its expectations locally; only the verdict records leave the process.

Rules that keep a mistake here from becoming a spin on a shared machine: the stage timeout is 10 s from before the
first launch; every rank issues the same launch sequence whatever it has seen; checks run after the synchronise and
their failures are collected, never raised between launches; after every launch the ranks agree (host collective)
on the largest error code, and once it is non-zero no rank launches anything more.
"""
import time

import numpy as np
import torch

from pytorch_mnist_ddp_amd.engine.state import ModelState
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops import functional as Fk
from pytorch_mnist_ddp_amd.ops import native

import refmodel as R
from refmodel import ADA_FC, OFF_CONV, PARAM_TOTAL, XG_CONV_N, XG_FC_N

SEED = 11
NAN = float("nan")
CFGS = ((1.0, 0.0), (0.7, 0.01))                       # (lr, weight_decay), alternating by call
POISON = (None, NAN, float("inf"))                     # by call: clean, a NaN on rank W - 1, +inf on rank W - 1
CH_A, CH_B = 24, 24                                    # channels of the two communicators


class Stop(Exception):
    """A rank saw a non-zero error code: nothing more is launched."""


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1))))


class Rig:
    def __init__(self, W, rank, dev):
        from torch.utils.dlpack import from_dlpack

        from pytorch_mnist_ddp_amd.parallel.distributed import create_xgmi_comm
        self.W, self.rank, self.dev, self.records, self.C = W, rank, dev, [], native.load()
        # A: the default one-shot limit.  B: oneshot_max = 0, every count takes the two-shot kernel.
        self.xa = create_xgmi_comm(W, rank, dev, PARAM_TOTAL, channels=CH_A, verify=False, oneshot_max=32768, co_ranks=W)
        self.xb = create_xgmi_comm(W, rank, dev, PARAM_TOTAL, channels=CH_B, verify=False, oneshot_max=0, co_ranks=W)
        assert self.xa is not None and self.xb is not None, "communicator set-up failed"
        self.limit = {id(self.xa): 32768, id(self.xb): 0}
        for x in (self.xa, self.xb):
            x.set_timeout_seconds(10)                   # before the first launch
            x.flags_view = from_dlpack(x.dlpack("flags")).view(torch.int32).view(-1, 2 * 8 * R.XG_MAX_WG)
        self.xa.stage_view = from_dlpack(self.xa.dlpack("stage")).view(CH_A, 2 * 32768)
        # ONE LAUNCH SHAPE PER CHANNEL for a communicator's lifetime: the per-workgroup call counters advance only
        # for workgroups that exist in a launch, so a channel whose kernel, count or grid changed would have
        # workgroups that disagree on the call number (and the one-shot staging parity).  A channel is therefore
        # keyed by (kernel, offset, count, grid) and handed out once per key.
        self.channels = {id(self.xa): {}, id(self.xb): {}}
        torch.manual_seed(1)
        self.ms = ModelState(Net(), dev, lr=1.0)
        case = R.ada_case()
        self.init = {k: case[k].to(dev) for k in R.ADA_STATE}
        self.case_no = 0

    def channel(self, x, key):
        d = self.channels[id(x)]
        if key not in d:
            d[key] = len(d)
            assert d[key] < x.flags_view.shape[0], "more launch shapes than channels"
        return d[key]

    def kind(self, x, count):
        return "oneshot" if count <= self.limit[id(x)] else "twoshot"

    # ---- per launch
    def agree(self, x):
        """After the synchronise: this rank's error code, then the largest over the ranks (which is also the barrier
        that keeps a rank from refilling buffers a peer's kernel still reads)."""
        err = x.error()
        if self.W > 1:
            import torch.distributed as dist
            t = torch.tensor([err], dtype=torch.int64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            worst = int(t)
        else:
            worst = err
        if worst:
            raise Stop(f"error code {err:#x} on rank {self.rank} (largest over ranks {worst:#x}: "
                       f"{self.C.Engine.describe_xgmi_error(worst)})")

    def settle(self):
        """After the post-launch snapshots, before the (slow, rank-dependent) CPU checks: no rank launches again -
        and writes its flags into the peers' blocks of the next channel - while a peer still takes its snapshots."""
        torch.cuda.synchronize()
        if self.W > 1:
            import torch.distributed as dist
            dist.barrier()

    def launched_grid(self, x, ch):
        """The grid the launcher used, read back from this rank's flag block: workgroup b of this rank wrote its call
        number into slot [stage 0][this rank][b], and slots of workgroups that never ran are still 0."""
        return int((x.flags_view[ch].view(2, 8, R.XG_MAX_WG)[0, self.rank] > 0).sum())

    def guard(self, x, ch):
        """Bits of every other channel's flags and staging slots."""
        keep = [c for c in range(x.flags_view.shape[0]) if c != ch]
        out = [x.flags_view[keep].clone()]
        if hasattr(x, "stage_view"):
            out.append(x.stage_view[keep].clone())
        return out

    def snap(self):
        torch.cuda.synchronize()
        return {k: getattr(self.ms, k).clone() for k in ("param", "grad", "square_avg", "acc_delta") + R.ADA_SHADOWS}

    def load_state(self, own_d, lr, wd):
        ms = self.ms
        ms.lr.fill_(lr)
        ms.weight_decay = wd
        for k in R.ADA_STATE:
            getattr(ms, k).copy_(self.init[k])
            getattr(ms, k).masked_fill_(~own_d, R.ADA_SENTINEL)
        for k in R.ADA_SHADOWS:
            getattr(ms, k).view(torch.int16).fill_(0x7FC1)          # a NaN pattern of our own
        ms.grad.fill_(NAN)                                   # the fused launches neither read nor write it

    def run(self, name, fn):
        """One case: its failures are collected; a Stop ends the whole list."""
        t0, fails, stats = time.perf_counter(), [], {}
        try:
            fn(fails, stats)
        except Stop as e:
            self.records.append(dict(case=name, ok=False, msg=str(e), stats=stats, seconds=time.perf_counter() - t0))
            raise
        self.records.append(dict(case=name, ok=not fails, msg="; ".join(fails[:4]), stats=stats,
                                 seconds=round(time.perf_counter() - t0, 2)))


def _check(fails, what, fn):
    try:
        return fn()
    except AssertionError as e:
        fails.append(f"{what}: {str(e)[:300]}")
        return None


def _cover(W, r, kind, offset, count, G, fuse):
    """The coverage count of tests/test_xgmi_oracle_cpu.py for the grid this launch will get: before the launch."""
    w = R.XgWorld(W, r, None, arith=False)
    if kind == "fc":
        w.fc_fused(G)
    else:
        getattr(w, kind)(offset, count, G, fuse=fuse)
    want = np.zeros(PARAM_TOTAL, np.int32)
    if fuse:
        want[offset:offset + count] = 1
    assert np.array_equal(w.n_upd, want), f"{kind} grid {G}: the update does not cover the bucket exactly once"


def _edges(kind, W, count):
    S4 = -(-(count // 4) // W)
    e = [4 * S4 * p for p in range(1, W)]
    if kind == "fc":
        e += [4 * int(R.xg_fc_f4(R.xg_fc_lo(p, W), 0)[0]) for p in range(1, W)] + [R.ADA_OFFS["fc1.bias"], XG_FC_N - 4 * R.XG_TAIL_F4 + 1024]
    return [min(x, count - 1) for x in e]


# ------------------------------------------------------------------ plain all-reduce
def plain(rig, x, offset, count, max_wg=0, calls=2):
    W, r = rig.W, rig.rank
    kind = rig.kind(x, count)
    G = R.xg_grid(kind, W, count // 4, False, x.grids[kind], max_wg)
    ch = rig.channel(x, (kind, offset, count, G))
    name = f"plain {kind} offset {offset} count {count} grid {G}"

    def body(fails, stats):
        _cover(W, r, kind, offset, count, G, False)
        for call in range(calls):
            rig.case_no += 1
            ins = [R.xg_bucket(SEED, rig.case_no, q, W, count, _edges(kind, W, count), POISON[call % 3],
                               sorted({0, count // 2, count - 1})) for q in range(W)]
            x.grad_in.fill_(NAN)
            x.grad_in[offset:offset + count] = ins[r].to(rig.dev)
            x.grad_out.fill_(R.XG_SENTINEL)                 # the guard floats on both sides of the range, too
            gin, guard = x.grad_in.clone(), rig.guard(x, ch)
            torch.cuda.synchronize()
            Fk.xgmi_allreduce(x, ch, offset, count, max_wg=max_wg)
            torch.cuda.synchronize()
            rig.agree(x)
            out, guard1, in_kept, grid = x.grad_out.cpu(), rig.guard(x, ch), _same(x.grad_in, gin), rig.launched_grid(x, ch)
            rig.settle()
            if grid != G:
                fails.append(f"call {call}: the launcher used {grid} workgroups, the model's grid is {G}")
            st = _check(fails, f"call {call}", lambda: R.xg_check_reduce(out[offset:offset + count], ins, name))
            if st:
                stats[f"call {call}"] = st["sum"]
            if not ((out[:offset] == R.XG_SENTINEL).all() and (out[offset + count:] == R.XG_SENTINEL).all()):
                fails.append(f"call {call}: out was written outside the range")
            if not in_kept:
                fails.append(f"call {call}: in was written")
            if not all(_same(a, b) for a, b in zip(guard, guard1)):
                fails.append(f"call {call}: another channel's flags or staging changed")
    rig.run(name, body)


# ------------------------------------------------------------------ fused launches
def fused(rig, kind, x, offset=0, count=XG_FC_N, max_wg=0, calls=2, wt=False, against_separate=False, wt_pair=False):
    """kind: "twoshot" / "oneshot" (allreduce with fuse_ada) or "fc" (allreduce_fc_fused).  ``wt_pair``: every call is
    launched again from the same state and inputs with write-through stores, which must give the same bits."""
    W, r, ms, dev = rig.W, rig.rank, rig.ms, rig.dev
    if kind == "fc":
        G = R.xg_grid("fc", W, planned=x.grids["fc_fused"], max_wg=max_wg)
        shadows = ("w1", "w1t")
        out_own = torch.zeros(PARAM_TOTAL, dtype=torch.bool)       # out: this rank's shard of units only
        out_own[(4 * torch.from_numpy(R.xg_fc_own_f4(r, W))[:, None] + torch.arange(4)).reshape(-1)] = True
    else:
        assert kind == rig.kind(x, count)
        G = R.xg_grid(kind, W, count // 4, True, x.grids[kind], max_wg)
        shadows = ("w2f", "w2d") if (offset, count) == (OFF_CONV, XG_CONV_N) else ()
        assert shadows or offset + count <= R.ADA_OFFS["conv2.weight"] or offset >= R.ADA_OFFS["conv2.bias"]
        out_own = R.own_mask(offset, offset + count) if kind == "twoshot" else torch.zeros(PARAM_TOTAL, dtype=torch.bool)
    ch = rig.channel(x, (kind + " fused", offset, count, G))
    ref_ch = rig.channel(x, ("twoshot", offset, count, R.xg_grid("twoshot", W, count // 4, False, x.grids["twoshot"]))) \
        if against_separate else None
    own = R.own_mask(offset, offset + count)
    own_d = own.to(dev)
    name = f"fused {kind} offset {offset} count {count} grid {G} wt {wt}"

    def body(fails, stats):
        _cover(W, r, kind, offset, count, G, True)
        for call in range(calls):
            rig.case_no += 1
            lr, wd = CFGS[call % 2]
            at = [e - offset for e in R.ADA_POISON if offset <= e < offset + count]
            ins = []
            for q in range(W):
                v = torch.full((PARAM_TOTAL,), NAN)
                v[offset:offset + count] = R.xg_bucket(SEED, rig.case_no, q, W, count, _edges(kind, W, count), POISON[call % 3], at)
                ins.append(v)
            rig.load_state(own_d, lr, wd)
            ms.set_state(5, seed=1, rng_base=0)
            x.grad_in.copy_(ins[r])
            x.grad_out.fill_(R.XG_SENTINEL)
            gin, guard, before = x.grad_in.clone(), rig.guard(x, ch), rig.snap()
            adv = call == 0
            if kind == "fc":
                Fk.xgmi_fc_fused(x, ch, ms, wt=wt, advance_step=adv, max_wg=max_wg)
            else:
                Fk.xgmi_allreduce(x, ch, offset, count, ms=ms, wt=wt, advance_step=adv, max_wg=max_wg)
            torch.cuda.synchronize()
            rig.agree(x)
            after, out, guard1, in_kept, step = rig.snap(), x.grad_out.cpu(), rig.guard(x, ch), _same(x.grad_in, gin), ms.get_step()
            grid = rig.launched_grid(x, ch)
            rig.settle()
            if grid != G:
                fails.append(f"call {call}: the launcher used {grid} workgroups, the model's grid is {G}")
            # xgmi_fc_fused_kernel never reads state_inc (the conv bucket's launch is the engine's end-of-step
            # marker): given or not, the counter stays; the other fused kernels advance it by one when given
            moved = adv and kind != "fc"
            if step != 5 + moved:
                fails.append(f"call {call}: the step counter is {step}, not {5 + moved}")
            b, a = {k: v.cpu() for k, v in before.items()}, {k: v.cpu() for k, v in after.items()}
            g32 = R.xg_ordered_sum(ins)
            g64 = torch.stack([v.to(R.F64) for v in ins]).sum(0)
            what = f"{name} call {call}"
            st = _check(fails, what, lambda: R.xg_check_update(b, a, own, g32, g64, lr, wd, what))
            if st and call == 0:
                stats.update(st)
            _check(fails, what, lambda: R.check_ownership(b, a, own, shadows, name=what))
            if POISON[call % 3] is not None:
                hit = torch.tensor([e for e in R.ADA_POISON if own[e]])
                if len(hit) and not (torch.isnan(a["param"][hit]).all() and int(torch.isnan(a["param"]).sum()) == len(hit)):
                    fails.append(f"{what}: the non-finite gradient did not reach exactly its {len(hit)} elements")
            ok = R.xg_same(out[out_own], g32[out_own]).all() and (out[~out_own] == R.XG_SENTINEL).all()
            if not ok:
                fails.append(f"{what}: out is not the ordered sum where the launch owns it and untouched elsewhere")
            if not in_kept:
                fails.append(f"{what}: in was written")
            if not all(_same(p, q) for p, q in zip(guard, guard1)):
                fails.append(f"{what}: another channel's flags or staging changed")
            if wt_pair:                                          # the same launch with write-through stores
                for k, v in before.items():
                    getattr(ms, k).copy_(v)
                x.grad_out.fill_(R.XG_SENTINEL)
                torch.cuda.synchronize()
                Fk.xgmi_fc_fused(x, ch, ms, wt=not wt, max_wg=max_wg)
                torch.cuda.synchronize()
                rig.agree(x)
                pair, out2 = rig.snap(), x.grad_out.clone()
                rig.settle()
                for k in after:
                    if not _same(after[k], pair[k]):
                        fails.append(f"{what}: {k} differs between wt off and on")
                if not _same(out2.cpu(), out):
                    fails.append(f"{what}: out differs between wt off and on")
            if against_separate:                                 # plain all-reduce + adadelta_step on the same inputs
                for k, v in before.items():
                    getattr(ms, k).copy_(v)
                torch.cuda.synchronize()
                Fk.xgmi_allreduce(x, ref_ch, offset, count)
                torch.cuda.synchronize()
                rig.agree(x)
                ms.grad[offset:offset + count] = x.grad_out[offset:offset + count]
                Fk.adadelta_step(ms, ADA_FC)
                two = rig.snap()
                for k in R.ADA_STATE + shadows:
                    sel = own_d if k in R.ADA_STATE else None
                    ta, tb = _bits(after[k].reshape(-1)), _bits(two[k].reshape(-1))
                    nan = torch.isnan(after[k].reshape(-1)) & torch.isnan(two[k].reshape(-1))
                    eq = (ta == tb) | nan
                    if not bool((eq[sel] if sel is not None else eq).all()):
                        fails.append(f"{what}: {k} differs from plain all-reduce + adadelta_step")
    rig.run(name, body)


# ------------------------------------------------------------------ conv_reduce_fused
class ConvSlabs:
    """The conv gradient slabs of one batch size, made once on this GPU by conv2_dgrad / conv2_wgrad (hand-made operands
    of refmodel.conv_hand_case; ``real``: the forward and fc backward kernels' own outputs, the conv1 partials
    pre-reduced into c1red), and per (call, rank) a seeded elementwise factor in [0.5, 1.5) on them, so that the
    ranks' slabs differ and every rank can make every rank's."""

    def __init__(self, rig, B, real):
        from test_gpu_backward_stages import BwdBox
        bx = BwdBox(rig.dev, B, trained=False)
        if real:
            bx.forward()
            Fk.fc_bwd(bx.ms, bx.buf, 1.0, None)
        else:
            bx.load_conv_hand()
        self.bx, self.B, self.real, self.c1red = bx, B, real, bx.c1red if real else None
        bx.buf.w2part.zero_()
        bx.buf.c1part.zero_()
        bx.c1red.zero_()
        Fk.conv_bwd(bx.ms, bx.u8, bx.idx_d, bx.buf, 1.0, B, stages=Fk.CONV_DGRAD | Fk.CONV_WGRAD, c1red=self.c1red)
        torch.cuda.synchronize()
        self.c1 = bx.c1red if real else bx.buf.c1part       # what the reduce reads for conv1
        self.nc1 = R.C1_PRE_SLABS if real else 4 * B
        self.base = (bx.buf.w2part[:bx.G].clone(), self.c1[:self.nc1].clone())

    def load(self, case_no, q, W, poison):
        """Rank q's slabs of this call into the buffers the reduce reads; returns them (CPU) for the oracle."""
        g = torch.Generator().manual_seed(7919 * (1000003 * SEED + 1009 * case_no + q) + self.B)
        out = []
        for base in self.base:
            f = (0.5 + torch.rand(base.shape, generator=g)).to(base.device)
            out.append(base * f)
        if poison is not None and q == W - 1:               # slab 0 at the columns of the isolation test's elements
            inv = torch.empty(18432, dtype=torch.long)
            inv[R._w2part_index()] = torch.arange(18432)
            o = R.ADA_OFFS
            for e in R.ADA_POISON:
                if o["conv2.weight"] <= e < o["conv2.weight"] + 18432:
                    out[0][0, inv[e - o["conv2.weight"]]] = poison
                elif o["conv2.bias"] <= e < o["conv2.bias"] + 64:
                    out[0][0, 18432 + e - o["conv2.bias"]] = poison
                elif o["conv1.weight"] <= e < o["conv1.weight"] + 288:
                    ci, kk = divmod(e - o["conv1.weight"], 9)
                    out[1][0, ci * 10 + kk] = poison
                elif o["conv1.bias"] <= e < o["conv1.bias"] + 32:
                    out[1][0, (e - o["conv1.bias"]) * 10 + 9] = poison
        self.bx.buf.w2part[:self.bx.G].copy_(out[0])
        self.c1[:self.nc1].copy_(out[1])
        return out[0].cpu(), out[1].cpu()


def conv(rig, x, slabs, lo=0, hi=R.RED_ALL_PARTS, max_wg=0, calls=3):
    """conv_reduce_fused on reduce parts [lo, hi) with grad_scale = 1 / W.  Ownership, from the kernel: it updates
    exactly the parameters that parts [lo, hi) sink (part [0, 289): conv2.weight, conv2.bias and the w2f / w2d shadows;
    part [289, 309): conv1.weight and conv1.bias, no shadow) and nothing else - not the padding elements of the conv
    bucket, not the fc region or its shadows, not the gradient buffer, not ``in`` and not ``out`` (the sums travel
    through the staging slots); the step counter moves by one where state_inc is given (no wait_* here)."""
    W, r, ms, dev, bx, B = rig.W, rig.rank, rig.ms, rig.dev, slabs.bx, slabs.B
    G = R.xg_grid("conv", W, planned=x.grids["conv_fused"], max_wg=max_wg, lo=lo, hi=hi)
    ch = rig.channel(x, ("conv fused", lo, hi, G))
    ref_ch = rig.channel(x, ("oneshot", OFF_CONV, XG_CONV_N, R.xg_grid("oneshot", W, XG_CONV_N // 4, False, x.grids["oneshot"])))
    own = R.own_mask(idx=R.conv_sink_elements(lo, hi))
    own_d = own.to(dev)
    shadows = ("w2f", "w2d") if lo == 0 else ()
    scale = 1.0 / W
    name = f"conv fused parts [{lo}, {hi}) B {B} grid {G}" + (" c1red" if slabs.real else "")

    def body(fails, stats):
        w = R.XgWorld(W, r, None, arith=False)               # coverage for this very grid, before the launch
        w.conv_fused(None, G, lo, hi)
        assert np.array_equal(w.n_upd > 0, own.numpy()) and w.n_upd.max() == 1 and not w.n_out.any(), "conv coverage"
        for call in range(calls):
            rig.case_no += 1
            lr, wd = CFGS[call % 2]
            what = f"{name} call {call}"
            reds = []
            for q in list(range(r)) + list(range(r + 1, W)) + [r]:          # this rank's slabs last: they stay loaded
                cpu_slabs = slabs.load(rig.case_no, q, W, POISON[call % 3])
                ms.grad.fill_(NAN)
                Fk.conv_bwd(ms, bx.u8, bx.idx_d, bx.buf, scale, B, stages=Fk.CONV_REDUCE, c1red=slabs.c1red)
                torch.cuda.synchronize()
                reds.append((q, ms.grad.cpu()))
            reds = [v for _, v in sorted(reds, key=lambda t: t[0])]
            if call == 0:                                    # this rank's reduce against the slab oracle
                grads = {n: reds[r][R.ADA_OFFS[n]:R.ADA_OFFS[n] + R.ADA_NUMEL[n]].view(R.PARAM_SHAPES[n]) for n in R.CONV_NAMES}
                st = _check(fails, what, lambda: R.check_conv_reduce(cpu_slabs[0], cpu_slabs[1], scale, grads, name=what))
                if st:
                    stats.update({f"reduce {k}": v for k, v in st.items()})
            rig.load_state(own_d, lr, wd)
            ms.set_state(5, seed=1, rng_base=0)
            x.grad_in.fill_(NAN)
            x.grad_out.fill_(R.XG_SENTINEL)
            gin, guard, before = x.grad_in.clone(), rig.guard(x, ch), rig.snap()
            adv = call != 1
            Fk.xgmi_conv_reduce_fused(x, ch, ms, bx.u8, bx.idx_d, bx.buf, grad_scale=scale, c1red=slabs.c1red, lo=lo, hi=hi,
                                      advance_step=adv, max_wg=max_wg)
            torch.cuda.synchronize()
            rig.agree(x)
            after, guard1, in_kept, step = rig.snap(), rig.guard(x, ch), _same(x.grad_in, gin), ms.get_step()
            out_kept, grid = bool((x.grad_out == R.XG_SENTINEL).all()), rig.launched_grid(x, ch)
            rig.settle()
            if grid != G:
                fails.append(f"{what}: the launcher used {grid} workgroups, the model's grid is {G}")
            if step != 5 + adv:
                fails.append(f"{what}: the step counter is {step}, not {5 + adv}")
            if not out_kept:
                fails.append(f"{what}: out was written")
            if not in_kept:
                fails.append(f"{what}: in was written")
            if not all(_same(p, q) for p, q in zip(guard, guard1)):
                fails.append(f"{what}: another channel's flags or staging changed")
            b, a = {k: v.cpu() for k, v in before.items()}, {k: v.cpu() for k, v in after.items()}
            g32 = R.xg_ordered_sum(reds)
            g64 = torch.stack([v.to(R.F64) for v in reds]).sum(0)
            st = _check(fails, what, lambda: R.xg_check_update(b, a, own, g32, g64, lr, wd, what))
            if st and call == 0:
                stats.update(st)
            _check(fails, what, lambda: R.check_ownership(b, a, own, shadows, name=what))
            if POISON[call % 3] is not None:
                hit = torch.tensor([e for e in R.ADA_POISON if own[e]])
                if not (torch.isnan(a["param"][hit]).all() and int(torch.isnan(a["param"]).sum()) == len(hit)):
                    fails.append(f"{what}: the non-finite gradient did not reach exactly its {len(hit)} elements")
            # conv_bwd(stages=4) on this rank's slabs (reds[r], above) + plain all-reduce + adadelta_step(ADA_CONV)
            for k, v in before.items():
                getattr(ms, k).copy_(v)
            x.grad_in[OFF_CONV:] = reds[r][OFF_CONV:].to(dev)
            torch.cuda.synchronize()
            Fk.xgmi_allreduce(x, ref_ch, OFF_CONV, XG_CONV_N)
            torch.cuda.synchronize()
            rig.agree(x)
            ms.grad[OFF_CONV:] = x.grad_out[OFF_CONV:]
            Fk.adadelta_step(ms, R.ADA_CONV)
            two = rig.snap()
            rig.settle()
            for k in R.ADA_STATE + shadows:
                ta, tb = after[k].reshape(-1), two[k].reshape(-1)
                eq = (_bits(ta) == _bits(tb)) | (torch.isnan(ta) & torch.isnan(tb))
                if not bool((eq[own_d] if k in R.ADA_STATE else eq).all()):
                    fails.append(f"{what}: {k} differs from conv_bwd(stages=4) + all-reduce + adadelta_step")
    rig.run(name, body)


def run_cases(W, rank, dev):
    """The whole list for a world of W; returns the records (every rank the same launches)."""
    rig = Rig(W, rank, dev)
    xa, xb = rig.xa, rig.xb
    try:
        for count in (4, 1020, 1024, 1028, 4100, 32768):         # one-shot up to the default limit
            plain(rig, xa, 0, count, calls=3)
        plain(rig, xa, 0, 32772)                                 # the first two-shot count
        for nvec in sorted({1, max(1, W - 1), W, W + 1, 513 * W + 1}):
            for offset in (4, 600000):
                for max_wg in (1, 0):
                    plain(rig, xb, offset, 4 * nvec, max_wg=max_wg)
        fused(rig, "twoshot", xa, 0, XG_FC_N)                    # the fp32 step's fc bucket
        fused(rig, "oneshot", xa, OFF_CONV, XG_CONV_N, calls=3)  # ... and its conv bucket
        fused(rig, "twoshot", xb, OFF_CONV + 64, 4 * (2 * W + 1), calls=3)    # ragged, ada_base != 0 (conv1.weight)
        plain(rig, xa, 0, 32768, max_wg=1, calls=3)              # the one-shot grid floor (4 float4 a lane): 8 workgroups
        for max_wg in (0, 8, 1):                                 # wt off and on: the same channel, the same shape
            fused(rig, "fc", xa, max_wg=max_wg, calls=3 if max_wg == 0 else 1, against_separate=True, wt_pair=True)
        for B in (2, 86) + ((341,) if W == 1 else ()):           # 341: the real chain with c1red, world 1 only
            slabs = ConvSlabs(rig, B, real=B == 341)
            conv(rig, xa, slabs)                                 # whole [0, 309), planned grid
            conv(rig, xa, slabs, max_wg=39)                      # ... on 39 workgroups: 8 virtual blocks each
            conv(rig, xa, slabs, 0, R.RED_W2_PARTS)              # the engine's two parts, in its order,
            conv(rig, xa, slabs, R.RED_W2_PARTS, R.RED_ALL_PARTS)     # each on a channel of its own
    except Stop:
        pass
    except Exception as e:  # noqa: BLE001 - reported, nothing more is launched
        rig.records.append(dict(case="case list", ok=False, msg=f"{type(e).__name__}: {e}", stats={}, seconds=0.0))
    torch.cuda.synchronize()
    return rig.records


def worker(rank, world, port, args, q):
    """A spawned rank (tools/xgmi_check.py spawn_world): the set-up of that tool, then the case list."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import torch.distributed as dist
    import xgmi_check
    dev = xgmi_check.init_rank(rank, world, port, True)
    try:
        q.put((rank, True, run_cases(world, rank, dev)))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        q.put((rank, False, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()
