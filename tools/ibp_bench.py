#!/usr/bin/env python3
"""Cost of one interval-bound-propagation round on the GPU: the native round of ``ops/ibp.py`` (three launches) beside
``ibp_reference`` in torch fp32 ops on the same device, and each of the three kernels alone.

Each batch size runs in a child process of its own, under its own time limit: one seeded net, synthetic test images,
true labels, eps = 0.002.  Each arm between two device events on the current stream (a warm-up first, then ROUNDS
alternated samples; the table gives the median and the min-max spread), in us:
  round       ``fused_ibp_radius(..., search_steps=ITERS - 1)`` divided by its ITERS rounds
  torch       ``ibp_reference`` on the GPU, one call
  trunk / fc1 / head   the kernel back to back on fixed operands, us per launch

    python tools/ibp_bench.py [--out profiles/ibp/ibp_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLS = ("round", "torch", "trunk", "fc1", "head")
HEAD = f"{'B':>5} " + " ".join(f"{c:>30}" for c in COLS) + f" {'round / torch':>13}"


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


def child(B: int, iters: int, rounds: int) -> int:
    import torch

    from pytorch_mnist_ddp_amd.data.datasets import load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
    from pytorch_mnist_ddp_amd.ops.ibp import fused_ibp_radius
    if not torch.cuda.is_available():
        print("ibp_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    param = fused_state(net).ms.param
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=B, verbose=False)
    x0 = _PIXEL_LUT.to(dev)[test.device_images(dev).reshape(-1, 784)[:B].long()].contiguous()
    y = test.targets[:B].long().to(dev)
    y32 = y.to(torch.int32)
    eps = torch.full((B,), 0.002, device=dev)
    rec = torch.zeros(B, 4, device=dev)
    rec[:, 0] = eps
    pl, pu = Fk.ibp_trunk(param, x0, rec)
    part = Fk.ibp_fc1(param, pl, pu)
    lb = Fk.ibp_head(param, part, y32, rec)
    arms = {"round": lambda: fused_ibp_radius(net, x0, y, 0.004, iters - 1),
            "torch": lambda: Fk.ibp_reference(net, x0, y, eps),
            "trunk": lambda: Fk.ibp_trunk(param, x0, rec, pl, pu),
            "fc1": lambda: Fk.ibp_fc1(param, pl, pu, part),
            "head": lambda: Fk.ibp_head(param, part, y32, rec, lb)}
    reps = {"round": 2, "torch": 2, "trunk": 50, "fc1": 50, "head": 50}
    per = {"round": iters}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per.get(k, 1))
    ratio = statistics.median(res["round"]) / statistics.median(res["torch"])
    print(f"{B:>5} " + " ".join(f"{fmt(res[c]):>30}" for c in COLS) + f" {ratio:>13.2f}")
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
    lines = [f"ibp_bench: {a.iters} rounds a sample, {a.rounds} samples; us per round (three launches) / per call / per "
             "launch, median [min-max]; measured once", HEAD]
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
