#!/usr/bin/env python3
"""Cost of randomized smoothing on the GPU: the two kernels of ``csrc/kernels/smooth.hip`` alone, and certification
end to end.

One process, one seeded net, synthetic test images.  Measured, each between two device events on the current
stream (a warm-up first, then ROUNDS alternated samples; the table gives the median and the min-max spread):
  smooth_noise / smooth_vote   us per launch at 1, 256 and 8192 rows (M images x n = rows / M samples), REPS
                               launches back to back per sample
  forward                      the three eval launches (trunk_fwd(xin), fc1_fwd, head_eval) on the same rows: what the
                               noise launch sits next to in the native loop
  certify native               ``Predictor.certify(n0 = 100, n = 1000)`` on IMAGES images: images per second, host
                               time included (the bound is host code)
  certify composed             the same algorithm composed from torch ops on the same GPU, batched as the native loop
                               is (whole images, up to 8192 rows a chunk): a repeat of the images over ``[m * n, 784]``,
                               ``torch.randn`` + mul + add, ``Predictor.log_probs`` (the same three kernels), ``argmax``
                               and one ``bincount`` over (image, class) per chunk
  certify per-image            that composition one image at a time (chunks of at most 1000 rows, a ``bincount`` and
                               a host round trip per image and chunk): what the simplest user loop costs

    python tools/smooth_bench.py [--out profiles/smooth/smooth_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist  # noqa: E402
from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor  # noqa: E402
from pytorch_mnist_ddp_amd.models.net import Net  # noqa: E402
from pytorch_mnist_ddp_amd.ops import functional as Fk  # noqa: E402
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state  # noqa: E402
from pytorch_mnist_ddp_amd.ops.smooth import certify_from_counts  # noqa: E402


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fmt(v):
    return f"{statistics.median(v):10.2f} [{min(v):9.2f}-{max(v):9.2f}]"


def batched_composed_certify(pr, images_u8, sigma, n0, n, alpha, chunk_rows=8192):
    """Randomized smoothing from torch ops and the Predictor's forward, chunked as the native loop chunks: whole
    images, ``chunk_rows // samples`` of them a chunk; same procedure, torch's generator."""
    dev = pr.device
    sigma_n = sigma / MNIST_STD
    x0 = _PIXEL_LUT.to(dev)[images_u8.reshape(-1, 784).long()]
    B = x0.shape[0]
    both = []
    for total in (n0, n):
        per = max(1, chunk_rows // total)
        counts = torch.zeros(B, 10, dtype=torch.int64, device=dev)
        for i0 in range(0, B, per):
            m = min(per, B - i0)
            rows = x0[i0:i0 + m].repeat_interleave(total, dim=0)
            rows = rows.add(torch.randn(m * total, 784, device=dev).mul(sigma_n))
            pred = pr.log_probs(rows.view(m * total, 1, 28, 28)).argmax(dim=1)
            image = torch.arange(m, device=dev).repeat_interleave(total)
            counts[i0:i0 + m] += torch.bincount(image * 10 + pred, minlength=m * 10).view(m, 10)
        both.append(counts.cpu().tolist())
    return [certify_from_counts(both[0][j], both[1][j], sigma, alpha) for j in range(B)]


def composed_certify(pr, images_u8, sigma, n0, n, alpha, chunk_rows=8000):
    """The same composition one image at a time; same procedure, torch's generator."""
    dev = pr.device
    sigma_n = sigma / MNIST_STD
    lut = _PIXEL_LUT.to(dev)
    out = []
    for j in range(images_u8.shape[0]):
        x0 = lut[images_u8[j].reshape(784).long()]
        both = []
        for total in (n0, n):
            counts = torch.zeros(10, dtype=torch.int64, device=dev)
            for s0 in range(0, total, chunk_rows):
                ns = min(chunk_rows, total - s0)
                z = torch.randn(ns, 784, device=dev)
                rows = x0.repeat(ns, 1).add(z.mul(sigma_n))
                counts += torch.bincount(pr.log_probs(rows.view(ns, 1, 28, 28)).argmax(dim=1), minlength=10)
            both.append(counts.cpu().tolist())
        out.append(certify_from_counts(both[0], both[1], sigma, alpha))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 256, 8192])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--images", type=int, default=64, help="images per certify sample")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("smooth_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    pr = Predictor(net)
    ms = fused_state(net).ms
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=max(a.images, 8), verbose=False)
    images = test.device_images(dev).reshape(-1, 784).contiguous()
    sigma_n = a.sigma / MNIST_STD
    lines = [f"smooth_bench: sigma {a.sigma}, {a.reps} launches a sample, {a.rounds} rounds; us, median [min-max]",
             f"{'rows':>6} {'smooth_noise u8':>34} {'smooth_vote':>34} {'forward (3 launches)':>34}"]
    for rows in a.rows:
        M = 1 if rows < 8 else 8
        n = rows // M
        src = images[:M]
        x = torch.empty(M * n, 784, dtype=torch.float32, device=dev)
        buf = Fk.StepBuffers.allocate(M * n, dev)
        counts = torch.zeros(M, 10, dtype=torch.int32, device=dev)

        def noise():
            Fk.smooth_noise(src, sigma_n, n, 5, out=x)

        def vote():
            Fk.smooth_vote(buf.logp, M, n, counts=counts)

        def forward():
            Fk.trunk_fwd(ms, None, None, buf, False, xin=x)
            Fk.fc1_fwd(ms, buf)
            Fk.head_eval(ms, None, None, buf)

        arms = {"noise": noise, "vote": vote, "forward": forward}
        for f in arms.values():
            timed(f, 5)
        res = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, f in arms.items():
                res[k].append(timed(f, a.reps))
        lines.append(f"{M * n:>6} {fmt(res['noise']):>34} {fmt(res['vote']):>34} {fmt(res['forward']):>34}")
    # certification end to end
    batch = images[:a.images]

    def native():
        return pr.certify(batch, a.sigma, n0=100, n=1000, alpha=0.001, seed=3)

    def composed():
        return batched_composed_certify(pr, batch, a.sigma, 100, 1000, 0.001)

    def per_image():
        return composed_certify(pr, batch, a.sigma, 100, 1000, 0.001)

    arms = (("native", native), ("composed", composed), ("per-image", per_image))
    rates = {name: [] for name, _ in arms}
    for name, f in arms:
        f()
    for _ in range(max(3, a.rounds // 2)):
        for name, f in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            rates[name].append(a.images / (time.perf_counter() - t0))
    lines.append(f"certify (n0 = 100, n = 1000, {a.images} images): images per second, median [min-max]")
    for name in rates:
        lines.append(f"  {name:<9} {fmt(rates[name])}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
