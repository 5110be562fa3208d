#!/usr/bin/env python3
"""Cost of one adversarial training step (L-inf PGD-AT, K attack iterations + the training step) on the GPU.

One process, B images a step, the same seeded net and synthetic rows for every arm.  Arms, each timed between
two device events on the stream it runs on and divided by its step count:
  plain      the SERIAL engine step without the attack (``FusedTrainer(overlap=False)``): STEPS steps as captured
             chunks replayed - the step this change leaves as it was, on the same box
  engine K   the engine's adversarial step (``FusedTrainer(adversarial=dict(eps, steps=K))``): adv_init, K x five
             attack launches, the training step on the attacked batch, all inside the replayed graph
  composed K what a user composes from the public API: ``Predictor.adversarial(x, y, eps, steps=K)`` on the live
             net, then the module-path step (``net(x_adv)``, ``F.nll_loss``, ``backward()``, the fused
             ``Adadelta.step()``): autograd, allocations and Python per step (host cost included: what a caller
             waits for); COMPOSED_STEPS steps a sample
The arms alternate for ROUNDS rounds after a warm-up of each; the table gives the median and the min-max spread.

    python tools/adv_train_bench.py [--out profiles/adv_train/adv_train_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import load_mnist  # noqa: E402
from pytorch_mnist_ddp_amd.engine.state import ModelState  # noqa: E402
from pytorch_mnist_ddp_amd.engine.trainer import FusedTrainer  # noqa: E402
from pytorch_mnist_ddp_amd.inference import Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.optim import Adadelta  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 7], help="attack iterations per step")
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=100, help="engine steps per sample (chunks of --graph-steps)")
    ap.add_argument("--graph-steps", type=int, default=50)
    ap.add_argument("--composed-steps", type=int, default=20, help="composed-loop steps per sample")
    ap.add_argument("--rounds", type=int, default=7, help="alternated samples per arm")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("adv_train_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.batch * a.steps
    train = load_mnist(synthetic_data=True, train=True, synthetic_size=n, verbose=False)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    arms = {}

    def engine_arm(name, adversarial):
        torch.manual_seed(1)
        ms = ModelState(Net(), dev, lr=1.0)
        t = FusedTrainer(ms, train, None, B, 1000, num_samples=n, seed=1, graph_steps=a.graph_steps, overlap=False,
                         adversarial=adversarial)
        t.precapture(a.steps)

        def run():
            t.start_stream(idx, gather=True)                # (upload + row gather: before the first event)
            return timed(lambda: t.run_steps(a.steps), t.compute) / a.steps
        arms[name] = run
        return t

    keep = [engine_arm("plain", None)]
    for k in a.ks:
        keep.append(engine_arm(f"engine K={k}", {"eps": a.eps, "steps": k}))

    torch.manual_seed(1)
    net = Net().to(dev).train()
    opt = Adadelta(net.parameters(), lr=1.0)
    pr = Predictor(net)
    u8 = train.device_images(dev)
    labels = train.targets.to(dev)
    for k in a.ks:
        def loop(k=k):
            for s in range(a.composed_steps):
                rows = idx[s * B:(s + 1) * B].to(dev)
                y = labels[rows]
                x_adv, _ = pr.adversarial(u8[rows], y, eps=a.eps, steps=k)
                opt.zero_grad()
                F.nll_loss(net(x_adv), y).backward()
                opt.step()
        arms[f"composed K={k}"] = lambda loop=loop: timed(loop, torch.cuda.current_stream()) / a.composed_steps

    t = {name: [] for name in arms}
    for run in arms.values():                               # warm-up of each arm
        run()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, run in arms.items():
            t[name].append(run())
            torch.cuda.synchronize()
    plain = statistics.median(t["plain"])
    lines = [f"# {torch.cuda.get_device_name(0)}; B = {B}, eps = {a.eps}; us per training step: median [min-max] of "
             f"{a.rounds} alternated samples ({a.steps} engine steps as {a.graph_steps}-step graph replays; "
             f"{a.composed_steps} composed-loop steps, host cost included)",
             f"{'arm':>16} {'us / step':>30} {'x plain':>8} {'x engine':>9}"]
    for name in arms:
        m = statistics.median(t[name])
        rel = ""
        if name.startswith("composed"):
            rel = f"{m / statistics.median(t['engine' + name[len('composed'):]]):9.2f}"
        lines.append(f"{name:>16} {fmt(t[name]):>30} {m / plain:8.2f} {rel:>9}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
