#!/usr/bin/env python3
"""Cost of one CROWN-IBP round on the GPU: the native round of ``ops/crown.py`` (six launches) beside an IBP round
(``ops/ibp.py``), beside ``crown_ibp_reference`` in torch fp32 ops on the same device, and each kernel alone.

As ``tools/ibp_bench.py``: each batch size in a child process of its own under its own time limit, one seeded net,
synthetic test images, true labels, eps = 0.002; each arm between two device events (a warm-up first, then ROUNDS
alternated samples; median and min-max), in us:
  round / ibp   ``fused_crown_ibp_radius`` / ``fused_ibp_radius`` (..., search_steps=ITERS - 1) divided by ITERS
  torch         ``crown_ibp_reference`` on the GPU, one call
  relax / fc1 / lambda / fc / bwd / head   the kernel back to back on fixed operands, us per launch

    python tools/crown_bench.py [--out profiles/crown/crown_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ibp_bench import fmt, timed  # noqa: E402

COLS = ("round", "ibp", "torch", "relax", "fc1", "lambda", "fc", "bwd", "head")
HEAD = f"{'B':>5} " + " ".join(f"{c:>30}" for c in COLS) + f" {'round / ibp':>11} {'round / torch':>13}"


def child(B: int, iters: int, rounds: int) -> int:
    import torch

    from pytorch_mnist_ddp_amd.data.datasets import load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops.crown import fused_crown_ibp_radius
    from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
    from pytorch_mnist_ddp_amd.ops.ibp import fused_ibp_radius
    if not torch.cuda.is_available():
        print("crown_bench: no GPU", file=sys.stderr)
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
    pl, pu, rx = Fk.crown_relax(param, x0, rec)
    part = Fk.ibp_fc1(param, pl, pu)
    lam, fcb = Fk.crown_lambda(param, part, y32)
    v, vb = Fk.crown_fc(param, rx, lam)
    sp = Fk.crown_bwd(param, x0, rec, rx, v, y32)
    lb = Fk.crown_head(fcb, vb, sp, y32, rec)
    arms = {"round": lambda: fused_crown_ibp_radius(net, x0, y, 0.004, iters - 1, rows_per_launch=B),
            "ibp": lambda: fused_ibp_radius(net, x0, y, 0.004, iters - 1),
            "torch": lambda: Fk.crown_ibp_reference(net, x0, y, eps),
            "relax": lambda: Fk.crown_relax(param, x0, rec, pl, pu, rx),
            "fc1": lambda: Fk.ibp_fc1(param, pl, pu, part),
            "lambda": lambda: Fk.crown_lambda(param, part, y32, lam, fcb),
            "fc": lambda: Fk.crown_fc(param, rx, lam, v, vb),
            "bwd": lambda: Fk.crown_bwd(param, x0, rec, rx, v, y32, sp),
            "head": lambda: Fk.crown_head(fcb, vb, sp, y32, rec, lb)}
    reps = dict({k: 20 for k in arms}, round=2, ibp=2, torch=1)
    per = {"round": iters, "ibp": iters}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per.get(k, 1))
    med = {k: statistics.median(q) for k, q in res.items()}
    print(f"{B:>5} " + " ".join(f"{fmt(res[c]):>30}" for c in COLS) +
          f" {med['round'] / med['ibp']:>11.2f} {med['round'] / med['torch']:>13.3f}")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=str, default="1,64,200,1000")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a batch size's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.iters, a.rounds)
    lines = [f"crown_bench: {a.iters} rounds a sample, {a.rounds} samples; us per round (six launches; ibp: three) / per "
             "call / per launch, median [min-max]; measured once", HEAD]
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
