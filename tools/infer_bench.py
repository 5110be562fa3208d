#!/usr/bin/env python3
"""Fused single-launch inference forward against the three-launch eval path, per batch size.

For each B both arms run the same seeded net on the same uint8 rows, in one process.  An arm is one
captured graph of ITERS forwards back to back on one stream (so the host's launch cost is outside the
measurement and every kernel boundary of the arm is inside it); a sample is one replay of that graph
between two device events, divided by ITERS.  The arms alternate (fused, three-launch, fused, ...) for
ROUNDS rounds after a warm-up replay of each; the table gives the median and the min-max spread of the
rounds.  "fused wins" only when its slowest round beats the three-launch arm's fastest one.

    python tools/infer_bench.py [--out profiles/infer/infer_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 64, 200, 1000])
    ap.add_argument("--iters", type=int, default=200, help="forwards per captured graph")
    ap.add_argument("--rounds", type=int, default=9, help="alternated replays per arm")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("infer_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    ms = ModelState(Net(), dev)
    stream = torch.cuda.Stream()
    lines = [f"# {torch.cuda.get_device_name(0)}; {a.iters} forwards per graph replay, {a.rounds} alternated rounds; "
             f"us per forward: median [min-max]",
             f"{'B':>6} {'ipw':>4} {'grid':>9} {'fused':>22} {'three-launch':>22} {'ratio':>6}  verdict"]
    for B in a.batches:
        imgs, labels = generate(B, seed=5)
        u8 = imgs.reshape(B, 784).contiguous().to(dev)
        lab = labels.to(torch.int32).to(dev)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        ibuf = Fk.InferBuffers.allocate(B, dev)
        sbuf = Fk.StepBuffers.allocate(B, dev)
        arms = {"fused": capture(lambda: Fk.infer_forward(ms, ibuf, B, u8=u8, labels=lab), a.iters, stream),
                "three": capture(lambda: Fk.eval_forward(ms, u8, lab, idx, sbuf), a.iters, stream)}
        torch.cuda.synchronize()
        if not torch.equal(ibuf.pred[:B].long(), sbuf.logp.argmax(1)):
            d = (ibuf.logp[:B] - sbuf.logp).abs().max().item()
            print(f"# B={B}: argmax differs on some row (max |dlogp| {d:.4f}; untrained net, near-ties)")
        t = {k: [] for k in arms}
        with torch.cuda.stream(stream):
            for g in arms.values():
                g.replay()                                  # warm-up replay of each arm
            stream.synchronize()
            for _ in range(a.rounds):
                for k, g in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    g.replay()
                    e1.record(stream)
                    e1.synchronize()
                    t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        f, th = t["fused"], t["three"]
        verdict = "fused wins" if max(f) < min(th) else "three-launch wins" if max(th) < min(f) else "within spread"
        plan = ms.C.infer_plan(B)
        fmt = lambda v: f"{statistics.median(v):8.2f} [{min(v):6.2f}-{max(v):6.2f}]"   # noqa: E731
        lines.append(f"{B:>6} {plan['images_per_wg']:>4} {'%dx%d' % plan['grid']:>9} {fmt(f):>22} {fmt(th):>22} "
                     f"{statistics.median(f) / statistics.median(th):>6.2f}  {verdict}")
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
