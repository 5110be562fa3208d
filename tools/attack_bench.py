#!/usr/bin/env python3
"""Cost of one PGD iteration (L-inf or L2, on the normalised image) on the GPU, per batch size.

One process, the same seeded net and rows for every arm.  An arm is one eager call that runs STEPS
iterations between two device events (Python, autograd and launch costs included: what a caller waits
for), divided by STEPS.
  (a) the native loop: ``ops.attack.fused_adversarial`` (per iteration trunk_fwd -> fc1_fwd -> head_train
      -> fc_bwd role B -> input_grad in its step form, in place; ``--norm l2``: input_grad in its plain
      form -> pgd_l2_step, in place)
  (b) the loop a user composes from the public API: ``Predictor.input_gradient`` per iteration, then
      sign / add / min / max / clamp (``--norm l2``: the two norms, the scalings and the clamp) in torch ops
  (c) stock torch autograd over ``Net.forward_reference`` (fp32) on the GPU with the same torch ops

The arms alternate for ROUNDS rounds after a warm-up of each; the table gives the median and the min-max
spread of the rounds.  With ``--norm l2`` a last column gives ``pgd_l2_step`` alone: one captured
graph of KERNEL_LAUNCHES launches in place on the same buffers, replayed between two device events and
divided by their number (the launch boundary included, no host cost; the kernel's own duration is the
profiler's, see docs/PERF_NOTES.md).

    python tools/attack_bench.py [--out profiles/attack/attack_bench.txt]
    python tools/attack_bench.py --norm l2 [--out profiles/attack/attack_bench_l2.txt]
"""
import argparse
import copy
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8  # noqa: E402
from pytorch_mnist_ddp_amd.data.synthetic import generate  # noqa: E402
from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO, Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.ops import functional as Fk  # noqa: E402
from pytorch_mnist_ddp_amd.ops.attack import fused_adversarial  # noqa: E402

KERNEL_LAUNCHES = 200


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def fmt(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f}-{max(v):8.2f}]"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 200, 1000])
    ap.add_argument("--steps", type=int, default=20, help="PGD iterations per sample")
    ap.add_argument("--rounds", type=int, default=7, help="alternated samples per arm")
    ap.add_argument("--norm", choices=("linf", "l2"), default="linf", help="the attack's norm (default: linf)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("attack_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev).train()
    ref = copy.deepcopy(net).eval()                         # arm (c): the same function, no dropout
    pr = Predictor(net)
    l2 = a.norm == "l2"
    eps, alpha = (2.0 / MNIST_STD, 0.25 / MNIST_STD) if l2 else (0.1 / MNIST_STD, 0.01 / MNIST_STD)
    lo, hi = PIXEL_LO, PIXEL_HI
    stream = torch.cuda.current_stream()
    lines = [f"# {torch.cuda.get_device_name(0)}; us per {'L2' if l2 else 'L-inf'} PGD iteration: median [min-max] "
             f"of {a.rounds} alternated samples of {a.steps} eager iterations (host cost included)",
             f"{'B':>6} {'(a) native loop':>30} {'(b) input_gradient + torch':>30} {'(c) torch fp32 autograd':>30} "
             f"{'(a)/(b)':>8} {'(a)/(c)':>8}" + (f" {'pgd_l2_step alone':>30}" if l2 else "")]
    for B in a.batches:
        imgs, labels = generate(B, seed=5)
        x0 = normalize_u8(imgs).reshape(B, 784).to(dev)
        y = labels.long().to(dev)

        def step(x, g):
            if l2:
                return Fk.pgd_l2_step_reference(g, x, x0, eps, alpha, lo, hi)
            t = x + alpha * g.sign()
            return torch.min(torch.max(t, x0 - eps), x0 + eps).clamp(lo, hi)

        def native():
            return fused_adversarial(net, x0, y, eps, a.steps, alpha, lo, hi, norm=a.norm)

        def composed():
            x = x0
            for _ in range(a.steps):
                g, _ = pr.input_gradient(x.view(B, 1, 28, 28), y)
                x = step(x, g.view(B, 784))
            return x

        def stock():
            x = x0
            for _ in range(a.steps):
                xg = x.clone().requires_grad_()
                lp = ref.forward_reference(xg.view(B, 1, 28, 28))
                g, = torch.autograd.grad(F.nll_loss(lp, y, reduction='sum'), xg)
                x = step(x, g)
            return x

        arms = {"a": native, "b": composed, "c": stock}
        t = {k: [] for k in arms}
        for run in arms.values():
            run()                                           # warm-up of each arm
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, run in arms.items():
                t[k].append(timed(run, stream) / a.steps)
        ma, mb, mc = (statistics.median(t[k]) for k in "abc")
        lines.append(f"{B:>6} {fmt(t['a']):>30} {fmt(t['b']):>30} {fmt(t['c']):>30} {ma / mb:>8.2f} {ma / mc:>8.2f}")
        if l2:                                              # the new kernel alone, on a real gradient
            g, _ = pr.input_gradient(x0.view(B, 1, 28, 28), y)
            g, xk = g.reshape(B, 784).contiguous(), x0.clone()
            torch.cuda.synchronize()
            side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):                   # one captured chain: no host cost between the launches
                Fk.pgd_l2_step(g, xk, x0, eps, alpha, lo, hi, out=xk)
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(KERNEL_LAUNCHES):
                        Fk.pgd_l2_step(g, xk, x0, eps, alpha, lo, hi, out=xk)
                graph.replay()
                side.synchronize()
                tk = [timed(graph.replay, side) / KERNEL_LAUNCHES for _ in range(a.rounds)]
            lines[-1] += f" {fmt(tk):>30}"
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
