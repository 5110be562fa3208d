#!/usr/bin/env python3
"""Cost of one FAB iteration on the GPU: the native loop of ``ops/fab.py`` in both norms beside a DeepFool iteration
of ``ops/deepfool.py`` at the same batch size (the same six launches, another step kernel), and ``fab_step`` alone.

One seeded net, synthetic test images, true labels.  Each batch size runs in a child process of its own under a time
limit (a hang at one size costs that row only).  In the child, each arm between two device events on the current
stream (a warm-up first, then ROUNDS samples with the arms alternated; the table gives the median and the min-max
spread), in us per iteration:
  fab linf / l2   ``fused_fab(..., steps=ITERS)`` divided by ITERS + 1 rounds (``deepfool_init`` included)
  deepfool        ``fused_minimum_norm(..., steps=ITERS, check_every=0)`` divided by ITERS
  step linf / l2  ``fab_step`` back to back on fixed operands that make every image take a forward step, us per launch

    python tools/fab_bench.py [--out profiles/fab/fab_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("fab linf", "fab l2", "deepfool", "step linf", "step l2")


def timed(run, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def child(B: int, iters: int, rounds: int) -> int:
    import torch
    from pytorch_mnist_ddp_amd.data.datasets import load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops.deepfool import fused_minimum_norm
    from pytorch_mnist_ddp_amd.ops.fab import fused_fab
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=B, verbose=False)
    u8 = test.device_images(dev).reshape(-1, 784).contiguous()[:B]
    y = test.targets.long().to(dev)[:B]
    x0 = _PIXEL_LUT.to(dev)[u8.long()]
    # fixed operands of the step alone: random gradient rows, y the smallest loss; the iterate is put back by the
    # launch itself (a forward step every time: the losses never change)
    dx = torch.randn(10 * B, 784, device=dev)
    loss = torch.rand(10 * B, device=dev) + 1.0
    loss.view(B, 10)[torch.arange(B, device=dev), y] = 0.5
    rows, x, x0s, x_best, status, its, _ = Fk.deepfool_init(x0)
    nb = torch.full((B,), float("inf"), device=dev)
    y32 = y.to(torch.int32)
    par = (0.1, 1.05, 0.9, PIXEL_LO, PIXEL_HI)
    step = lambda norm: Fk.fab_step(dx, loss, y32, x0s, x, x_best, nb, rows, status, its, *par, norm)   # noqa: E731
    arms = {"fab linf": lambda: fused_fab(net, u8, y, "linf", iters, *par),
            "fab l2": lambda: fused_fab(net, u8, y, "l2", iters, *par),
            "deepfool": lambda: fused_minimum_norm(net, u8, y, iters, 0.02, PIXEL_LO, PIXEL_HI, check_every=0),
            "step linf": lambda: step("linf"), "step l2": lambda: step("l2")}
    reps = {k: 200 if k.startswith("step") else max(1, 64 // B) for k in arms}
    per = {"fab linf": iters + 1, "fab l2": iters + 1, "deepfool": iters, "step linf": 1, "step l2": 1}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per[k])
    print("ROW " + f"{B:>5} " + " ".join(f"{statistics.median(res[k]):9.1f} [{min(res[k]):8.1f}-{max(res[k]):8.1f}]"
                                         for k in ARMS), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,800")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a batch size may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.iters, a.rounds)
    lines = [f"fab_bench: {a.iters} iterations a sample, {a.rounds} rounds; us per iteration, median [min-max]",
             f"{'B':>5} " + " ".join(f"{k:>29}" for k in ARMS)]
    for B in (int(v) for v in a.batches.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--iters", str(a.iters), "--rounds",
               str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{B:>5} no result: over the limit of {a.limit} s")
            break                                            # nothing more is started on a GPU that may be hung
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append(f"{B:>5} no result: exit status {r.returncode}")
            break
        lines.append(rows[0])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
