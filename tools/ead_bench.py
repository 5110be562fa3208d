#!/usr/bin/env python3
"""Cost of one EAD (elastic-net) iteration on the GPU: the native loop of ``ops/ead.py`` beside a Carlini-Wagner
iteration (``ops/cw.py``) in the same process, the alternative launch layout that was weighed against it, and
``ead_step`` alone.

Each batch size runs in a child process of its own, under its own time limit: one seeded net, synthetic test images,
true labels.  Each arm between two device events on the current stream (a warm-up first, then ROUNDS alternated
samples; the table gives the median and the min-max spread), in us per round:
  ead         ``fused_elastic_net(..., search_steps=1, steps=ITERS)`` divided by its ITERS + 1 rounds: six launches, the
              gradient chain over 2 B rows (the slack points, then the shrunk points), ``input_grad`` over B
  split       the layout not taken, launches only: the gradient chain and ``input_grad`` over the B slack rows, the
              three-launch eval chain over the B shrunk rows, then ``ead_step`` (on the margins of the last ``ead``
              arm: the cost of nine launches, not a result)
  cw          ``fused_carlini_wagner(..., search_steps=1, steps=ITERS)`` divided by its ITERS + 1 rounds
  step alone  ``ead_step`` (a plain launch, rule en) back to back on fixed operands, us per launch

    python tools/ead_bench.py [--out profiles/ead/ead_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEAD = (f"{'B':>5} {'ead (6 launches, 2B rows)':>34} {'split (9 launches)':>34} {'cw':>34} {'ead / cw':>8} "
        f"{'ead_step alone':>34}")


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

    from pytorch_mnist_ddp_amd.data.datasets import load_mnist
    from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, PIXEL_HI, PIXEL_LO
    from pytorch_mnist_ddp_amd.models.net import Net
    from pytorch_mnist_ddp_amd.ops import functional as Fk
    from pytorch_mnist_ddp_amd.ops import native
    from pytorch_mnist_ddp_amd.ops.chain import EvalChain, GradChain
    from pytorch_mnist_ddp_amd.ops.cw import fused_carlini_wagner
    from pytorch_mnist_ddp_amd.ops.ead import fused_elastic_net
    from pytorch_mnist_ddp_amd.ops.fused_net import fused_state
    if not torch.cuda.is_available():
        print("ead_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    net = Net().to(dev)
    test = load_mnist(synthetic_data=True, train=False, synthetic_size=B, verbose=False)
    x0 = _PIXEL_LUT.to(dev)[test.device_images(dev).reshape(-1, 784)[:B].long()].contiguous()
    y = test.targets[:B].long().to(dev)
    lab = y.to(torch.int32)
    # fixed operands of the step alone: margins below kappa = 0 (the hinge is active, no success), random gradient rows
    dx, loss = 0.05 * torch.randn(B, 784, device=dev), -torch.rand(2 * B, device=dev) - 0.5
    ys, xs, x_best = x0.clone(), x0.clone(), torch.zeros(B, 784, device=dev)
    fstate, istate = torch.zeros(B, 4, device=dev), torch.zeros(B, 4, dtype=torch.int32, device=dev)
    step = lambda first=False, rows=loss: Fk.ead_step(dx, rows, x0, ys, xs, x_best, fstate, istate, 1, 0.0, 0.01, 1.0,   # noqa: E731
                                                      0.01, 4, 100, 0, PIXEL_LO, PIXEL_HI, "en", first=first)
    step(first=True)
    st = fused_state(net)
    st.sync()
    gchain, ebuf = GradChain(st, B, "cw"), Fk.EvalBuffers.allocate(B, dev)
    echain, p = EvalChain(st.ms, ebuf), native.ptr

    def split():
        for _ in range(iters + 1):
            gchain.run(p(ys), p(lab), B)
            gchain.input_grad(p(dx), B)
            echain.run(B, xin=p(xs), labels=p(lab))
            step()

    arms = {"ead": lambda: fused_elastic_net(net, x0, y, 1, iters, 0.01, 1.0, 0.01, 0.0, "en", 1, PIXEL_LO, PIXEL_HI),
            "split": split,
            "cw": lambda: fused_carlini_wagner(net, x0, y, 1, iters, 0.05, 1.0, 0.0, 1, PIXEL_LO, PIXEL_HI),
            "step": step}
    reps = {"ead": max(1, 64 // B), "split": max(1, 64 // B), "cw": max(1, 64 // B), "step": 200}
    per = {"ead": iters + 1, "split": iters + 1, "cw": iters + 1, "step": 1}
    for f in arms.values():
        timed(f, 1)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, reps[k]) / per[k])
    gchain.release()
    ratio = statistics.median(res["ead"]) / statistics.median(res["cw"])
    print(f"{B:>5} {fmt(res['ead']):>34} {fmt(res['split']):>34} {fmt(res['cw']):>34} {ratio:>8.2f} "
          f"{fmt(res['step']):>34}")
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
    lines = [f"ead_bench: {a.iters} updates a sample, {a.rounds} rounds; us per round, median [min-max]; measured once",
             HEAD]
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
