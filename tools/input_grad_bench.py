#!/usr/bin/env python3
"""Cost of the input gradient (``x.grad``) on the GPU, per batch size.

Two tables, one process, the same seeded net and rows for every arm.

``kernels``: the launches alone.  An arm is one captured graph of ITERS passes back to back on one
stream (the host's launch cost is outside the measurement, every kernel boundary inside it); a sample is
one replay between two device events, divided by ITERS.
  (a) trunk_fwd -> fc1_fwd -> head_train -> fc_bwd -> conv_bwd      (``Fk.train_step(update=False)``)
  (b) the same followed by input_grad
(b) - (a) is what the new launch adds to a pass.

``module``: what a caller of ``F.nll_loss(net(x), y).backward()`` waits for.  An arm is ITERS eager passes
between two device events (Python, autograd and launch costs included), divided by ITERS.
  (a) fused ``Net`` (bf16 kernels), x without a gradient
  (b) fused ``Net``, ``x.requires_grad_()``: x.grad from input_grad.hip
  (c) ``Net.forward_reference`` (stock torch fp32 ops) with ``x.requires_grad_()``, the only way to an
      input gradient on the GPU without the kernel

The arms alternate for ROUNDS rounds after a warm-up of each; the tables give the median and the min-max
spread of the rounds.

    python tools/input_grad_bench.py [--out profiles/input_grad/input_grad_bench.txt]
"""
import argparse
import copy
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8  # noqa: E402
from pytorch_mnist_ddp_amd.data.synthetic import generate  # noqa: E402
from pytorch_mnist_ddp_amd.engine.state import ModelState  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.ops import functional as Fk  # noqa: E402


def capture(fn, iters, stream):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        fn()
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(iters):
                fn()
    return graph


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rounds_of(arms, rounds, iters, stream):
    t = {k: [] for k in arms}
    with torch.cuda.stream(stream):
        for run in arms.values():
            run()                                           # warm-up of each arm
        stream.synchronize()
        for _ in range(rounds):
            for k, run in arms.items():
                t[k].append(timed(run, stream) / iters)
    return t


def fmt(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f}-{max(v):8.2f}]"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 200, 1000])
    ap.add_argument("--iters", type=int, default=100, help="passes per captured graph (kernels table)")
    ap.add_argument("--eager-iters", type=int, default=30, help="eager passes per sample (module table)")
    ap.add_argument("--rounds", type=int, default=7, help="alternated samples per arm")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("input_grad_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net()
    ref = copy.deepcopy(net).to(dev).train()
    ref.dropout1.p = ref.dropout2.p = 0.0                   # the same function in the three module arms
    fused = copy.deepcopy(ref)
    ms = ModelState(net, dev)
    stream = torch.cuda.Stream()
    head = f"# {torch.cuda.get_device_name(0)}; us per pass: median [min-max] of {a.rounds} alternated samples"
    k_lines = [head + f"; kernels: {a.iters} passes per graph replay",
               f"{'B':>6} {'grid':>6} {'(a) step kernels':>30} {'(b) + input_grad':>30} {'(b)-(a)':>8}"]
    m_lines = [f"# module: {a.eager_iters} eager passes per sample (host cost included)",
               f"{'B':>6} {'(a) fused, no x.grad':>30} {'(b) fused, x.grad':>30} {'(c) torch fp32, x.grad':>30} "
               f"{'(b)-(a)':>8} {'(b)/(c)':>8}"]
    for B in a.batches:
        imgs, labels = generate(B, seed=5)
        u8 = imgs.reshape(B, 784).contiguous().to(dev)
        lab = labels.to(torch.int32).to(dev)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        buf = Fk.StepBuffers.allocate(B, dev)
        dx = torch.empty(B, 784, dtype=torch.float32, device=dev)

        def step():
            Fk.train_step(ms, u8, lab, idx, buf, update=False)

        def step_dx():
            Fk.train_step(ms, u8, lab, idx, buf, update=False)
            Fk.input_grad(ms, buf, dx)

        graphs = {"a": capture(step, a.iters, stream), "b": capture(step_dx, a.iters, stream)}
        t = rounds_of({k: g.replay for k, g in graphs.items()}, a.rounds, a.iters, stream)
        plan = ms.C.input_grad_plan(B, torch.cuda.get_device_properties(0).multi_processor_count)
        k_lines.append(f"{B:>6} {plan['grid']:>6} {fmt(t['a']):>30} {fmt(t['b']):>30} "
                       f"{statistics.median(t['b']) - statistics.median(t['a']):>8.2f}")
        print(k_lines[-1], flush=True)

        x, y = normalize_u8(imgs).to(dev), labels.long().to(dev)

        def module_arm(model, want_dx):
            def run():
                for _ in range(a.eager_iters):
                    xi = x.detach().requires_grad_(want_dx)
                    model.zero_grad(set_to_none=True)
                    out = model(xi) if model is fused else model.forward_reference(xi)
                    F.nll_loss(out, y).backward()
            return run

        t = rounds_of({"a": module_arm(fused, False), "b": module_arm(fused, True), "c": module_arm(ref, True)},
                      a.rounds, a.eager_iters, stream)
        ma, mb, mc = (statistics.median(t[k]) for k in "abc")
        m_lines.append(f"{B:>6} {fmt(t['a']):>30} {fmt(t['b']):>30} {fmt(t['c']):>30} {mb - ma:>8.2f} {mb / mc:>8.2f}")
        print(m_lines[-1], flush=True)
    text = "\n".join(k_lines) + "\n\n" + "\n".join(m_lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
