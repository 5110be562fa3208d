#!/usr/bin/env python3
"""Cost of one Square Attack query on the GPU: the native loop of ``ops/square.py`` (the eval chain plus one
``square_step``, four launches) against the loop a user would compose without the kernel, and ``square_step`` alone.

One seeded net, synthetic test images, true labels, eps 0.3, ``check_every`` = 0 (no host sync: every query is made).
Per batch of B images each arm is timed between two device events on the current stream (a warm-up first, then ROUNDS
alternated samples; the table gives the median and the min-max spread), in us per query:
  native      ``fused_square_attack(..., queries=QUERIES, check_every=0)`` divided by QUERIES
  host loop   QUERIES rounds of ``Predictor.log_probs`` on the candidates plus ``square_step_reference`` (torch ops
              on the GPU; its Philox words are drawn on the host)
  step alone  ``square_step`` (a middle launch, no image frozen) back to back on fixed operands, us per launch

Each batch size runs in a child process of its own under a time limit; after a child that fails no other is started.

    python tools/square_bench.py [--out profiles/square/square_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return f"{statistics.median(v):9.1f} [{min(v):8.1f}-{max(v):8.1f}]"


def host_loop(pr, x0, y, eps, queries, seed):
    """The Square Attack composed from ``log_probs`` calls and ``square_step_reference``."""
    from pytorch_mnist_ddp_amd.inference import PIXEL_HI, PIXEL_LO
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    B = x0.shape[0]
    sides = Fk.square_sides(0.8, queries)
    x_cand = Fk.square_init_reference(x0, eps, PIXEL_LO, PIXEL_HI, seed)
    x_best = state = None
    for j in range(queries):
        last = j == queries - 1
        lp = pr.log_probs(x_cand.view(B, 1, 28, 28))
        x_best, x_cand, state = Fk.square_step_reference(lp, y, x0, x_best, x_cand, state, eps, PIXEL_LO, PIXEL_HI, seed,
                                                         j + 1, 1 if last else sides[j], first=j == 0, last=last)
    return x_best


def one(B: int, queries: int, rounds: int) -> str:
    import torch

    from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO, Predictor
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops.square import fused_square_attack
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    pr = Predictor(net)
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=B, verbose=False)
    x0 = _PIXEL_LUT.to(dev)[test.device_images(dev).reshape(-1, 784)[:B].long()].contiguous()
    y = test.targets.long().to(dev)[:B]
    eps = 0.3 / MNIST_STD
    # fixed operands of the step alone: a middle launch, every image live and far from broken
    logits = torch.randn(B, 10, device=dev)
    logits[torch.arange(B, device=dev), y] += 10.0          # (the label leads: a margin > 0, equal from launch to launch)
    logp = torch.log_softmax(logits, dim=1)
    y32 = y.to(torch.int32)
    x_best = Fk.square_init(x0, eps, PIXEL_LO, PIXEL_HI, 1)
    x_cand = Fk.square_init(x0, eps, PIXEL_LO, PIXEL_HI, 2)
    state = torch.tensor([0x42C80000, 3, 0, 0], dtype=torch.int32, device=dev).repeat(B, 1).contiguous()   # 100.0f
    fixed = state.clone()

    def step():
        Fk.square_step(logp, y32, x0, x_best, x_cand, fixed, eps, PIXEL_LO, PIXEL_HI, 0, 7, 9)

    arms = {"native": lambda: fused_square_attack(net, x0, y, eps, queries, PIXEL_LO, PIXEL_HI, check_every=0),
            "host": lambda: host_loop(pr, x0, y, eps, queries, 0),
            "step": step}
    reps = {"native": max(1, 64 // B), "host": 1, "step": 200}
    per = {"native": queries, "host": queries, "step": 1}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per[k])
    ratio = statistics.median(res["host"]) / statistics.median(res["native"])
    return f"{B:>5} {fmt(res['native']):>29} {fmt(res['host']):>29} {ratio:>6.2f} {fmt(res['step']):>29}"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,1000")
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a batch size may take")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one is not None:
        print(one(a.one, a.queries, a.rounds))
        return 0
    lines = [f"square_bench: {a.queries} queries a sample, {a.rounds} samples; us per query, median [min-max]",
             f"{'B':>5} {'native':>29} {'host loop':>29} {'ratio':>6} {'square_step alone':>29}"]
    status = 0
    for B in (int(v) for v in a.batches.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), "--queries", str(a.queries),
                                "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"{B:>5} timed out after {a.step_timeout:g} s; nothing more was started")
            status = 3
            break
        if r.returncode != 0:
            lines.append(f"{B:>5} failed with status {r.returncode}; nothing more was started")
            sys.stderr.write(r.stderr[-2000:])
            status = 3
            break
        lines.append(r.stdout.rstrip("\n").splitlines()[-1])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
