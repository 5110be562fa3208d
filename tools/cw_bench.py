#!/usr/bin/env python3
"""Cost of one Carlini-Wagner L2 iteration on the GPU: the native loop of ``ops/cw.py`` beside an L2 Auto-PGD
iteration (``ops/apgd.py``: the same gradient chain, the same six launches a round), and ``cw_step`` alone.

Each batch size runs in a child process of its own, under its own time limit: one seeded net, synthetic test images,
true labels.  Each arm between two device events on the current stream (a warm-up first, then ROUNDS alternated
samples; the table gives the median and the min-max spread), in us per round of six launches:
  cw          ``fused_carlini_wagner(..., search_steps=1, steps=ITERS)`` divided by its ITERS + 1 rounds
  apgd l2     ``fused_auto_pgd(..., steps=ITERS, norm="l2")`` divided by its ITERS + 1 rounds
  step alone  ``cw_step`` (a plain Adam launch) back to back on fixed operands, us per launch

    python tools/cw_bench.py [--out profiles/cw/cw_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEAD = f"{'B':>5} {'cw':>34} {'apgd l2':>34} {'cw / apgd':>9} {'cw_step alone':>34}"


def timed(run, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fmt(v):
    return f"{statistics.median(v):10.1f} [{min(v):9.1f}-{max(v):9.1f}]"


def child(B: int, iters: int, rounds: int) -> int:
    import torch

    from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops.apgd import fused_auto_pgd
    from pytorch_mnist_ddp_amd.ops.cw import fused_carlini_wagner
    if not torch.cuda.is_available():
        print("cw_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=B, verbose=False)
    x0 = _PIXEL_LUT.to(dev)[test.device_images(dev).reshape(-1, 784)[:B].long()].contiguous()
    y = test.targets[:B].long().to(dev)
    # fixed operands of the step alone: a margin below kappa = 0 (the hinge is active), random gradient rows
    dx, loss = 0.05 * torch.randn(B, 784, device=dev), -torch.rand(B, device=dev) - 0.5
    w, m1, v, x, x_best = (torch.zeros(B, 784, device=dev) for _ in range(5))
    x.copy_(x0)
    fstate, istate = torch.zeros(B, 4, device=dev), torch.zeros(B, 4, dtype=torch.int32, device=dev)
    step = lambda first=False: Fk.cw_step(dx, loss, x0, w, m1, v, x, x_best, fstate, istate, 1, 0.0, 0.05, 1.0, 4, 0,   # noqa: E731
                                          PIXEL_LO, PIXEL_HI, first=first)
    step(first=True)
    arms = {"cw": lambda: fused_carlini_wagner(net, x0, y, 1, iters, 0.05, 1.0, 0.0, 1, PIXEL_LO, PIXEL_HI),
            "apgd": lambda: fused_auto_pgd(net, x0, y, 1.5 / MNIST_STD, iters, PIXEL_LO, PIXEL_HI, norm="l2"),
            "step": step}
    reps = {"cw": max(1, 64 // B), "apgd": max(1, 64 // B), "step": 200}
    per = {"cw": iters + 1, "apgd": iters + 1, "step": 1}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per[k])
    ratio = statistics.median(res["cw"]) / statistics.median(res["apgd"])
    print(f"{B:>5} {fmt(res['cw']):>34} {fmt(res['apgd']):>34} {ratio:>9.2f} {fmt(res['step']):>34}")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,1000")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a batch size's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.iters, a.rounds)
    lines = [f"cw_bench: {a.iters} updates a sample, {a.rounds} rounds; us per round of six launches, median [min-max]; "
             "measured once", HEAD]
    for B in (int(q) for q in a.batches.split(",")):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), "--iters", str(a.iters),
                            "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:                                # a failed child ends the run: nothing more is started
            print("\n".join(lines), r.stdout, r.stderr[-2000:], sep="\n", file=sys.stderr)
            return r.returncode or 1
        lines.append(r.stdout.rstrip("\n").splitlines()[-1])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
