#!/usr/bin/env python3
"""Cost of one L2 DeepFool iteration on the GPU: the native loop of ``ops/deepfool.py`` against the loop a user would
compose without it, and ``deepfool_step`` alone.

One process, one seeded net, synthetic test images, true labels.  Per batch of B images, each arm between two device
events on the current stream (a warm-up first, then ROUNDS alternated samples; the table gives the median and the
min-max spread), in us per iteration:
  native      ``fused_minimum_norm(..., steps=ITERS, check_every=0)`` divided by ITERS (``deepfool_init`` included)
  host loop   ITERS iterations of: ten ``Predictor.input_gradient`` calls (one per class label) on the B iterates, the
              nine norms, the argmin, the step and the clamp in torch ops on a [B, 10, 784] temporary - no freezing
  step alone  ``deepfool_step`` back to back on fixed operands (10 B gradient rows), us per launch

    python tools/deepfool_bench.py [--out profiles/deepfool/deepfool_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import load_mnist  # noqa: E402
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO, Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.ops import functional as Fk  # noqa: E402
from pytorch_mnist_ddp_amd.ops.deepfool import fused_minimum_norm  # noqa: E402


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fmt(v):
    return f"{statistics.median(v):10.1f} [{min(v):9.1f}-{max(v):9.1f}]"


def host_loop(pr, x0, y, iters, overshoot):
    """DeepFool composed from ``input_gradient`` calls and torch ops (every image steps every iteration)."""
    B = x0.shape[0]
    ar = torch.arange(B, device=x0.device)
    x, r_tot = x0.clone(), torch.zeros_like(x0)
    for _ in range(iters):
        g = torch.empty(B, 10, 784, device=x0.device)
        for c in range(10):
            gc, lp = pr.input_gradient(x.view(B, 1, 28, 28), torch.full((B,), c, device=x0.device))
            g[:, c] = gc.view(B, 784)
        f = lp - lp[ar, y][:, None]
        w = g[ar, y][:, None, :] - g
        n2 = w.square().sum(dim=2)
        ratio = (f.abs() + Fk.DF_SLACK) / n2.sqrt()
        ratio[ar, y] = float("inf")
        l = ratio.argmin(dim=1)
        r_tot = r_tot + ((f.abs()[ar, l] + Fk.DF_SLACK) / n2[ar, l])[:, None] * w[ar, l]
        x = (x0 + (1.0 + overshoot) * r_tot).clamp(PIXEL_LO, PIXEL_HI)
    return x


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,800")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("deepfool_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    pr = Predictor(net)
    batches = [int(v) for v in a.batches.split(",")]
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=max(batches), verbose=False)
    images = test.device_images(dev).reshape(-1, 784).contiguous()
    targets = test.targets.long().to(dev)
    lines = [f"deepfool_bench: {a.iters} iterations a sample, {a.rounds} rounds; us per iteration, median [min-max]",
             f"{'B':>5} {'native':>34} {'host loop':>34} {'ratio':>7} {'deepfool_step alone':>34}"]
    for B in batches:
        u8, y = images[:B], targets[:B]
        x0 = _PIXEL_LUT.to(dev)[u8.long()]
        # fixed operands of the step alone: random gradient rows, y the smallest loss (every image steps every launch)
        dx = torch.randn(10 * B, 784, device=dev)
        loss = torch.rand(10 * B, device=dev) + 1.0
        loss.view(B, 10)[torch.arange(B, device=dev), y] = 0.5
        rows, x, x0s, r_tot, status, iters, norm = Fk.deepfool_init(x0)
        y32 = y.to(torch.int32)
        arms = {"native": lambda: fused_minimum_norm(net, u8, y, a.iters, 0.02, PIXEL_LO, PIXEL_HI, check_every=0),
                "host": lambda: host_loop(pr, x0, y, a.iters, 0.02),
                "step": lambda: Fk.deepfool_step(dx, loss, y32, x0s, r_tot, x, rows, status, iters, norm, 0.02,
                                                 PIXEL_LO, PIXEL_HI)}
        reps = {"native": max(1, 64 // B), "host": 1, "step": 200}
        per = {"native": a.iters, "host": a.iters, "step": 1}
        for f in arms.values():
            timed(f, 1)
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, f in arms.items():
                res[k].append(timed(f, reps[k]) / per[k])
        ratio = statistics.median(res["host"]) / statistics.median(res["native"])
        lines.append(f"{B:>5} {fmt(res['native']):>34} {fmt(res['host']):>34} {ratio:>7.2f} {fmt(res['step']):>34}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
