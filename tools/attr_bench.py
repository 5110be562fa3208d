#!/usr/bin/env python3
"""Cost of integrated gradients and SmoothGrad on the GPU: ``Predictor.attribute`` (the native loop of
``ops/attribute.py``) against the host loop a user would write without it.

One process, one seeded net, synthetic test images, true labels.  Per (B images, n gradient rows per image) and method,
each arm between two device events on the current stream (a warm-up first, then ROUNDS alternated samples; the table
gives the median and the min-max spread), in us per image:
  native      ``Predictor.attribute(x, labels, method, steps=n)``
  host loop   n calls of ``Predictor.input_gradient`` on the B rows of one sample index (the path point or the noised
              copy made with torch ops), summed with torch adds, then scaled (and multiplied by x - b): two autograd
              ``Function``s and their allocations per call

    python tools/attr_bench.py [--out profiles/attr/attr_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist  # noqa: E402
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_LO, Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402


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


def host_loop(pr, x0, labels, method, n, sigma_n, gen):
    """The attribution from ``input_gradient`` calls: one call per sample index over the B images."""
    B = x0.shape[0]
    acc = torch.zeros_like(x0)
    d = x0 - PIXEL_LO
    for s in range(n):
        if method == "integrated_gradients":
            rows = PIXEL_LO + ((s + 0.5) / n) * d
        else:
            rows = x0 + sigma_n * torch.randn(B, 784, device=x0.device, generator=gen)
        g, _ = pr.input_gradient(rows.view(B, 1, 28, 28), labels)
        acc += g.view(B, 784)
    acc *= -1.0 / n
    return acc * d if method == "integrated_gradients" else acc


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", type=str, default="1x32,64x32,200x32,8x1024", help="B x n, comma separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("attr_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    pr = Predictor(net)
    cases = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=max(b for b, _ in cases), verbose=False)
    images = test.device_images(dev).reshape(-1, 784).contiguous()
    targets = test.targets.long().to(dev)
    sigma_n = a.sigma / MNIST_STD
    gen = torch.Generator(device=dev).manual_seed(3)
    lines = [f"attr_bench: sigma {a.sigma}, {a.rounds} rounds; us per image, median [min-max]",
             f"{'B':>5} {'n':>5} {'method':<21} {'native':>34} {'host loop':>34} {'ratio':>7}"]
    for B, n in cases:
        u8, y = images[:B], targets[:B]
        x0 = _PIXEL_LUT.to(dev)[u8.long()]
        reps = max(1, 2048 // (B * n))                       # enough work a sample
        for method in ("integrated_gradients", "smoothgrad"):
            arms = {"native": lambda: pr.attribute(u8, y, method, steps=n, sigma=a.sigma, seed=3),
                    "host": lambda: host_loop(pr, x0, y, method, n, sigma_n, gen)}
            for f in arms.values():
                timed(f, 1)
            res = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, f in arms.items():
                    res[k].append(timed(f, reps) / B)
            ratio = statistics.median(res["host"]) / statistics.median(res["native"])
            lines.append(f"{B:>5} {n:>5} {method:<21} {fmt(res['native']):>34} {fmt(res['host']):>34} {ratio:>7.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
