#!/usr/bin/env python3
"""Cost of one Auto-PGD iteration on the GPU: the native loop of ``ops/apgd.py`` against an L2 PGD iteration of
``ops/attack.py`` (the same six launches: the chain, ``input_grad``, one row kernel) and against the loop a user would
compose without the kernel, and ``apgd_step`` alone.

One process, one seeded net, synthetic test images, true labels.  Per batch of B images and per norm, each arm between
two device events on the current stream (a warm-up first, then ROUNDS alternated samples; the table gives the median
and the min-max spread), in us per iteration:
  native      ``fused_auto_pgd(..., steps=ITERS)`` divided by ITERS + 1 (its rounds)
  l2 pgd      ``fused_adversarial(..., steps=ITERS + 1, norm="l2")`` divided by ITERS + 1
  host loop   ITERS + 1 rounds of ``Predictor.input_gradient`` on the iterate plus ``apgd_step_reference`` (torch ops)
  step alone  ``apgd_step`` (a middle launch that closes a window) back to back on fixed operands, us per launch

    python tools/apgd_bench.py [--out profiles/apgd/apgd_bench.txt]

``--loss ce,cw,dlr`` prints another table instead: per batch the native L-inf loop under each of the named losses
(``fused_auto_pgd(loss=...)``, alternated in the same process; the launch count is the same, ``head_margin`` stands in
``head_train``'s place), and the head alone: ``head_train`` (no dropout, loss scale 1) against ``head_margin`` of each
kind, back to back on the partials of one forward, us per launch.

    python tools/apgd_bench.py --loss ce,cw,dlr [--out profiles/apgd/apgd_bench_loss.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist  # noqa: E402
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO, Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.ops import functional as Fk  # noqa: E402
from pytorch_mnist_ddp_amd.ops.apgd import fused_auto_pgd  # noqa: E402
from pytorch_mnist_ddp_amd.ops.attack import fused_adversarial  # noqa: E402


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fmt(v):
    return f"{statistics.median(v):9.1f} [{min(v):8.1f}-{max(v):8.1f}]"


def host_loop(pr, x0, y, eps, steps, norm):
    """Auto-PGD composed from ``input_gradient`` calls and ``apgd_step_reference``."""
    B = x0.shape[0]
    window = dict(Fk.apgd_checkpoints(steps))
    state = (x0.clone(), None, None, None, None, None)
    for j in range(steps + 1):
        g, lp = pr.input_gradient(state[0].view(B, 1, 28, 28), y)
        loss_rows = F.nll_loss(lp, y, reduction='none')
        state = Fk.apgd_step_reference(g.view(B, 784), loss_rows, x0, *state, 1, eps, PIXEL_LO, PIXEL_HI, norm=norm,
                                       first=j == 0, last=j == steps, window=window.get(j, 0))
    return state[2]


def loss_table(a, net, dev, batches, images, targets):
    """The ``--loss`` table (module docstring)."""
    from pytorch_mnist_ddp_amd.ops.fused_net import _step_state, fused_state
    losses = [v for v in a.loss.split(",") if v]
    for v in losses:
        if v not in ("ce", "cw", "dlr"):
            raise SystemExit(f"apgd_bench: --loss takes ce, cw, dlr, got {v!r}")
    kinds = [v for v in losses if v != "ce"] + (["dlr_t"] if "dlr" in losses else [])
    rounds = a.iters + 1
    eps = 0.1 / MNIST_STD
    st = fused_state(net)
    st.sync()
    ms = st.ms
    nodrop = _step_state(st, False, dev, 1)          # step 0, STEP_FLAG_NO_DROPOUT: the chains' own state
    head = " ".join(f"{'apgd ' + v:>29}" for v in losses) + " " + " ".join(
        f"{h:>29}" for h in ["head_train"] + ["head_margin " + k for k in kinds])
    lines = [f"apgd_bench --loss: L-inf, {a.iters} updates ({rounds} rounds) a sample, {a.rounds} samples; us per "
             f"iteration (apgd) and per launch (head alone), median [min-max]", f"{'B':>5} {head}"]
    for B in batches:
        y = targets[:B]
        x0 = _PIXEL_LUT.to(dev)[images[:B].long()]
        buf = Fk.StepBuffers.allocate(B, dev)
        lab = y.to(torch.int32).contiguous()
        tgt = ((lab + 1) % 10).contiguous()
        Fk.trunk_fwd(ms, None, None, buf, True, state=nodrop, xin=x0)
        Fk.fc1_fwd(ms, buf)
        arms = {"apgd " + v: (lambda v=v: fused_auto_pgd(net, x0, y, eps, a.iters, PIXEL_LO, PIXEL_HI, loss=v))
                for v in losses}
        reps = {k: max(1, 64 // B) for k in arms}
        per = {k: rounds for k in arms}
        arms["head_train"] = lambda: Fk.head_train(ms, lab, None, buf, state=nodrop, inv_batch=1.0)
        for k in kinds:
            arms["head_margin " + k] = lambda k=k: Fk.head_margin(ms, lab, buf, k, tgt if k == "dlr_t" else None)
        for k in arms:
            reps.setdefault(k, 200)
            per.setdefault(k, 1)
        for f in arms.values():
            timed(f, 1)
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, f in arms.items():
                res[k].append(timed(f, reps[k]) / per[k])
        lines.append(f"{B:>5} " + " ".join(f"{fmt(res[k]):>29}" for k in arms))
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,1000")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loss", default=None, metavar="L1,L2,...",
                    help="the loss table instead: the native L-inf loop under each of these losses (ce, cw, dlr) and "
                         "head_margin alone against head_train")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("apgd_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    pr = Predictor(net)
    batches = [int(v) for v in a.batches.split(",")]
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=max(batches), verbose=False)
    images = test.device_images(dev).reshape(-1, 784).contiguous()
    targets = test.targets.long().to(dev)
    rounds = a.iters + 1
    if a.loss:
        text = "\n".join(loss_table(a, net, dev, batches, images, targets))
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return 0
    lines = [f"apgd_bench: {a.iters} updates ({rounds} rounds) a sample, {a.rounds} samples; us per iteration, median "
             f"[min-max]",
             f"{'B':>5} {'norm':>5} {'native':>29} {'l2 pgd':>29} {'host loop':>29} {'ratio':>6} {'apgd_step alone':>29}"]
    for B in batches:
        y = targets[:B]
        x0 = _PIXEL_LUT.to(dev)[images[:B].long()]
        for norm, eps in (("linf", 0.1 / MNIST_STD), ("l2", 1.5 / MNIST_STD)):
            # fixed operands of the step alone: a middle launch, random gradients, every image inside its ball
            dx = torch.randn(B, 784, device=dev)
            loss = torch.rand(B, device=dev) + 1.0
            x, x_old, x_best = (x0.clone() for _ in range(3))
            g_best = torch.randn(B, 784, device=dev)
            fs = torch.tensor([eps, 1.0, 1.0, 1.0], device=dev).repeat(B, 1).contiguous()
            ist = torch.tensor([3, 0, 5, 0], dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
            arms = {"native": lambda: fused_auto_pgd(net, x0, y, eps, a.iters, PIXEL_LO, PIXEL_HI, norm=norm),
                    "pgd": lambda: fused_adversarial(net, x0, y, 1.5 / MNIST_STD, rounds, 0.3 / MNIST_STD, PIXEL_LO,
                                                     PIXEL_HI, norm="l2"),
                    "host": lambda: host_loop(pr, x0, y, eps, a.iters, norm),
                    "step": lambda: Fk.apgd_step(dx, loss, x0, x, x_old, x_best, g_best, fs, ist, 1, eps, PIXEL_LO,
                                                 PIXEL_HI, norm=norm, window=4)}
            reps = {"native": max(1, 64 // B), "pgd": max(1, 64 // B), "host": 1, "step": 200}
            per = {"native": rounds, "pgd": rounds, "host": rounds, "step": 1}
            for f in arms.values():
                timed(f, 1)
            res = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, f in arms.items():
                    res[k].append(timed(f, reps[k]) / per[k])
            ratio = statistics.median(res["host"]) / statistics.median(res["native"])
            lines.append(f"{B:>5} {norm:>5} {fmt(res['native']):>29} {fmt(res['pgd']):>29} {fmt(res['host']):>29} "
                         f"{ratio:>6.2f} {fmt(res['step']):>29}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
