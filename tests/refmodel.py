"""fp32 torch reference oracle for the numerics tests (never used by the product path).

``reference_step`` runs the reference forward/backward (mnist_ddp.py:49-72) with stock torch
ops in fp32 on the CPU, optionally with given dropout masks, and returns loss, log-probs and
per-parameter gradients.

The second half is the stage-wise forward oracle: one float64 function per forward kernel stage on the
operands that kernel reads, the comparators (``assert_rounded_bf16``, ``assert_within``,
``assert_decisions``) and the per-kernel checks built from them, shared by
tests/test_forward_oracle_cpu.py and tests/test_gpu_forward_stages.py.  The last part is the same for the
backward kernels (tests/test_backward_oracle_cpu.py, tests/test_gpu_backward_stages.py).
The fp32 step's kernels (csrc/kernels/f32_net.hip) have their own stage oracle at the end of the file
(tests/test_fp32_oracle_cpu.py, tests/test_gpu_fp32_stages.py).
"""
from __future__ import annotations

import copy
import functools

import torch
import torch.nn.functional as F

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8


def reference_forward(net, x, mask1=None, mask2=None, train=True):
    x = F.relu(net.conv1(x))
    x = F.relu(net.conv2(x))
    x = F.max_pool2d(x, 2)
    if train and mask1 is not None:
        x = x * mask1.view_as(x) * (1.0 / 0.75)
    x = torch.flatten(x, 1)
    x = F.relu(net.fc1(x))
    if train and mask2 is not None:
        x = x * mask2.view_as(x) * 2.0
    x = net.fc2(x)
    return F.log_softmax(x, dim=1)


def reference_step(net, images_u8, labels, mask1=None, mask2=None, dtype=torch.float32):
    net = copy.deepcopy(net).cpu().to(dtype)
    net.zero_grad(set_to_none=True)
    x = normalize_u8(images_u8).to(dtype)
    mask1 = mask1.to(dtype) if mask1 is not None else None
    mask2 = mask2.to(dtype) if mask2 is not None else None
    out = reference_forward(net, x, mask1, mask2)
    loss = F.nll_loss(out, labels.long())
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    return loss.detach(), out.detach(), grads


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------- Philox-4x32-10 (numpy-free)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        hi0, lo0 = (p0 >> 32) & MASK, p0 & MASK
        hi1, lo1 = (p1 >> 32) & MASK, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def dropout_keep(seed: int, offset: int, elem: int, thr8: int) -> bool:
    """Kernel dropout rule: one Philox block per 16 elements, one byte per element, keep <=> byte < thr8."""
    blk = elem >> 4
    w = philox4x32((blk & MASK, blk >> 32, offset & MASK, offset >> 32), (seed & MASK, seed >> 32))
    k = elem & 15
    return ((w[k >> 2] >> (8 * (k & 3))) & 0xFF) < thr8


# ---------------------------------------------------------------- bf16-emulating reference
def emulated_bf16_step(net, images_u8, labels, mask1=None, mask2=None):
    """Manual fwd/bwd in float64 that rounds to bf16 exactly where the fused kernels do.

    Differences against the kernels are then only accumulation order (~1e-5 relative), so this
    oracle catches indexing/layout bugs that a bf16-vs-fp32 tolerance could hide.
    """
    import torch.nn.grad as G

    def q(t):
        return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)

    d = {n: p.detach().cpu().double() for n, p in net.named_parameters()}
    B = images_u8.shape[0]
    x = normalize_u8(images_u8).double()
    z0 = F.conv2d(x, d["conv1.weight"], d["conv1.bias"])
    a1 = q(F.relu(z0))
    w2q = q(d["conv2.weight"])
    y2 = F.conv2d(a1, w2q, d["conv2.bias"])
    pooled, arg = F.max_pool2d(F.relu(y2), 2, return_indices=True)
    drop1 = mask1.double().view_as(pooled) * (1.0 / 0.75) if mask1 is not None else torch.ones_like(pooled)
    p = q(pooled * drop1).flatten(1)
    w1q = q(d["fc1.weight"])
    z1 = p @ w1q.t() + d["fc1.bias"]
    drop2 = mask2.double().view_as(z1) * 2.0 if mask2 is not None else torch.ones_like(z1)
    h = F.relu(z1) * drop2
    logits = h @ d["fc2.weight"].t() + d["fc2.bias"]
    lp = F.log_softmax(logits, 1)
    y = labels.long()
    loss = -lp.gather(1, y.view(-1, 1)).mean()
    dl = (lp.exp() - F.one_hot(y, 10).double()) / B
    dh = dl @ d["fc2.weight"]
    dz1 = dh * drop2 * (z1 > 0)
    dz1q, hq, dlq = q(dz1), q(h), q(dl)
    grads = {"fc2.weight": dlq.t() @ hq, "fc2.bias": dlq.sum(0),
             "fc1.weight": dz1q.t() @ p, "fc1.bias": dz1q.sum(0)}
    dp = dz1q @ w1q
    g = q(dp * drop1.flatten(1) * (pooled.flatten(1) > 0)).view_as(pooled)
    dy = F.max_unpool2d(g, arg, 2, output_size=y2.shape[-2:])
    grads["conv2.weight"] = G.conv2d_weight(a1, w2q.shape, dy)
    grads["conv2.bias"] = dy.sum((0, 2, 3))
    da1 = G.conv2d_input(a1.shape, w2q, dy) * (z0 > 0)
    # conv1 weight/bias gradient: bf16 MFMA operands (input image and masked da1), fp32 accumulation
    grads["conv1.weight"] = G.conv2d_weight(q(x), d["conv1.weight"].shape, q(da1))
    grads["conv1.bias"] = q(da1).sum((0, 2, 3))
    return loss, lp, grads


def keep_mask(seed: int, offset: int, n: int, thr8: int) -> torch.Tensor:
    """Kernel dropout rule for elements [0, n): one Philox block per 16 elements, byte k of it."""
    out = torch.empty(n, dtype=torch.float32)
    for blk in range((n + 15) // 16):
        w = philox4x32((blk & 0xFFFFFFFF, blk >> 32, offset & 0xFFFFFFFF, offset >> 32),
                       (seed & 0xFFFFFFFF, seed >> 32))
        for k in range(min(16, n - 16 * blk)):
            out[16 * blk + k] = float(((w[k >> 2] >> (8 * (k & 3))) & 0xFF) < thr8)
    return out


def _mulhilo(a: int, b: torch.Tensor):
    """(hi, lo) 32-bit words of the constant a times the 32-bit values in the int64 tensor b."""
    t, u = a * (b & 0xFFFF), a * (b >> 16)
    lo = t + ((u & 0xFFFF) << 16)
    return (u >> 16) + (lo >> 32), lo & MASK


def keep_mask_at(seed: int, offset: int, elems: torch.Tensor, thr8: int, blocks: torch.Tensor | None = None):
    """``keep_mask`` for the given global element indices (int64 tensor, any shape), vectorised.
    ``blocks`` overrides the Philox counter block (default ``elems >> 4``) - the CPU test's mutations."""
    elems = elems.long()
    blk = elems >> 4 if blocks is None else blocks.long()
    c0, c1 = blk & MASK, blk >> 32
    c2, c3 = torch.full_like(blk, offset & MASK), torch.full_like(blk, (offset >> 32) & MASK)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        hi0, lo0 = _mulhilo(M0, c0)
        hi1, lo1 = _mulhilo(M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    w = torch.stack([c0, c1, c2, c3], -1)
    k = elems & 15
    byte = (w.gather(-1, (k >> 2).unsqueeze(-1)).squeeze(-1) >> (8 * (k & 3))) & 0xFF
    return (byte < thr8).float()


@functools.lru_cache(maxsize=None)
def trained_net():
    """The seed-1 ``Net`` after the 32 seeded CPU Adadelta steps of tests/test_gpu_infer.py: an untrained
    net's rows are almost all near-ties of three classes, so an argmax check on it checks nothing."""
    from pytorch_mnist_ddp_amd.data.synthetic import generate
    from pytorch_mnist_ddp_amd.models.net import Net
    torch.manual_seed(1)
    net = Net()
    imgs, labels = generate(1024, seed=11)
    x, y = normalize_u8(imgs), labels.long()
    opt = torch.optim.Adadelta(net.parameters(), lr=1.0)
    net.train()
    with torch.enable_grad():
        for step in range(32):
            i = (step * 64) % 1024
            opt.zero_grad()
            F.nll_loss(net.forward_reference(x[i:i + 64]), y[i:i + 64]).backward()
            opt.step()
    return net.eval()


# ---------------------------------------------------------------- stage-wise forward oracle
# One function per forward kernel stage, on the operands that stage's kernel reads.  dtype = float64
# is the oracle; dtype = float32 is "torch's fp32 CPU op on the same operands", which sets each
# stage's accumulation slack (stage_eps) and builds the CPU test's stand-in for the kernels.
F64, F32 = torch.float64, torch.float32
INV_KEEP1_F32 = float(torch.tensor(1.0, dtype=F32) / torch.tensor(0.75, dtype=F32))   # the kernel's 1.0f / KEEP1
EPS_MARGIN = 8.0            # kernel and torch both accumulate in fp32, in different orders over the same K
HEAD_ULPS = 16.0            # head outputs: a chain of about ten rounded fp32 operations incl. expf / logf
CAP = 1e-3                  # largest share of a decision tensor that may sit below the margin
CHECK_ROWS = (0, 1, 15, 16, 31, 32, 63, 64, 255, 256, 511, 512)


def check_rows(B: int) -> list[int]:
    """Rows the oracle is applied to: all up to B = 64, a fixed subset around the tile edges beyond."""
    if B <= 64:
        return list(range(B))
    return sorted({r for r in CHECK_ROWS + (B - 2, B - 1) if 0 <= r < B})


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(F32).to(torch.bfloat16)


def stage_conv1(x_norm, w, b, dtype=F64):
    """relu(conv1) [R,32,26,26] before rounding, from the normalised fp32 input rows [R,784]."""
    return F.relu(F.conv2d(x_norm.reshape(-1, 1, 28, 28).to(dtype), w.to(dtype), b.to(dtype)))


def pool_windows(y):
    """[R,64,24,24] -> [R,9216,4]: the 2x2 windows in window order 2*dy + dx, flatten order c*144 + y*12 + x."""
    R = y.shape[0]
    return y.view(R, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(R, 9216, 4)


def first_strict_max(x):
    """(max, index) over the last axis with explicit > comparisons in order 0, 1, ...: first maximum wins."""
    best, code = x[..., 0].clone(), torch.zeros(x.shape[:-1], dtype=torch.long)
    for k in range(1, x.shape[-1]):
        m = x[..., k] > best
        best = torch.where(m, x[..., k], best)
        code = torch.where(m, torch.full_like(code, k), code)
    return best, code


def stage_conv2_pool(a1_bf16, w2_bf16, b2, keep1=None, dtype=F64):
    """conv2 on bf16 operands (a1 NCHW [R,32,26,26], w2 [64,32,3,3]) + fp32 bias, ReLU, 2x2 max-pool,
    dropout-1.  All results [R,9216(,4)] in torch flatten order: ``windows`` (the four pre-ReLU values),
    ``pooled`` (max of their ReLUs), ``code`` (2*dy + dx of the first strict maximum), ``gap`` (between the
    two largest window values), ``p`` (pooled x keep x float32(1/0.75) with a keep mask, else unscaled)."""
    win = pool_windows(F.conv2d(a1_bf16.to(dtype), w2_bf16.to(dtype), b2.to(dtype)))
    pooled, code = first_strict_max(F.relu(win))
    top = win.topk(2, -1).values
    p = pooled if keep1 is None else pooled * keep1.reshape(pooled.shape).to(dtype) * INV_KEEP1_F32
    return dict(windows=win, pooled=pooled, code=code, gap=top[..., 0] - top[..., 1], p=p)


def stage_fc1_partials(p_bf16, w1_bf16, ksplit, dtype=F64):
    """[ksplit, R, 128]: chunk s = flat features [s*9216/ksplit, (s+1)*9216/ksplit) of p [R,9216] . w1 [128,9216]^T."""
    R, kc = p_bf16.shape[0], 9216 // ksplit
    a = p_bf16.to(dtype).view(R, ksplit, kc).permute(1, 0, 2)
    b = w1_bf16.to(dtype).view(128, ksplit, kc).permute(1, 2, 0)
    return torch.bmm(a, b)


def stage_head(z1part, b_fc1, w_fc2, b_fc2, labels=None, keep2=None, inv_batch=1.0, dtype=F64):
    """The head on the fc1 partials [ksplit,R,128]: z1 = bias + sum over chunks (in chunk order), h, logits,
    log-probs and, with labels, the per-row NLL, dl = (softmax - onehot) * inv_batch and dz1 = dh * keep2 * 2 *
    (z1 > 0) (keep2 None: dropout off, no factor 2)."""
    s = torch.zeros_like(z1part[0], dtype=dtype)
    for c in range(z1part.shape[0]):
        s = s + z1part[c].to(dtype)
    z1 = b_fc1.to(dtype) + s
    drop = torch.ones_like(z1) if keep2 is None else keep2.reshape(z1.shape).to(dtype) * 2.0
    h = F.relu(z1) * drop
    logits = h @ w_fc2.to(dtype).t() + b_fc2.to(dtype)
    logp = F.log_softmax(logits, 1)
    out = dict(z1=z1, h=h, logits=logits, logp=logp)
    if labels is not None:
        y = labels.long().view(-1, 1)
        out["nll"] = -logp.gather(1, y).squeeze(1)
        out["dl"] = (logp.exp() - F.one_hot(y.squeeze(1), 10).to(dtype)) * inv_batch
        out["dz1"] = (out["dl"] @ w_fc2.to(dtype)) * drop * (z1 > 0)
    return out


def stage_eps(ref32, ref64, head=False) -> float:
    """A stage's accumulation slack: EPS_MARGIN x max |torch fp32 CPU op - float64 oracle| on the same
    operands; for head tensors not below HEAD_ULPS fp32 ulps of the reference's largest magnitude."""
    eps = EPS_MARGIN * float((ref32.to(F64) - ref64).abs().max())
    if head:
        _, e = torch.frexp(ref64.abs().max())
        eps = max(eps, HEAD_ULPS * 2.0 ** (int(e) - 24))
    return eps


def halfulp_bf16(x64):
    """Half a bf16 ulp at x: 2^(e-9) with frexp(|x|) = (m in [0.5, 1), e); 0 at 0."""
    _, e = torch.frexp(x64.abs())
    return torch.where(x64 == 0, torch.zeros_like(x64), torch.ldexp(torch.ones_like(x64), e - 9))


def assert_rounded_bf16(out_bf16, ref64, eps, what="") -> float:
    """Every element: |out - ref| <= halfulp(ref) + eps - either bf16 neighbour only where ref is within eps
    of their midpoint; truncation, a one-ulp slip, a NaN or anything larger fails.  No element is excluded.
    Returns the largest |out - ref| - halfulp(ref) (<= eps; negative: no element needed the slack)."""
    assert out_bf16.dtype == torch.bfloat16 and out_bf16.shape == ref64.shape, (what, out_bf16.dtype, out_bf16.shape)
    over = (out_bf16.to(F64) - ref64).abs() - halfulp_bf16(ref64)
    bad = ~(over <= eps)                      # NaN compares false: an unwritten sentinel fails
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements off the bf16 rounding of the "
                           f"oracle by more than eps = {eps:.3g}; worst excess {float(over[bad].nan_to_num(1e30).max()):.3g}")
    return float(over.max())


def assert_within(out, ref64, eps, what="") -> float:
    """Every element within eps absolute of the oracle (fp32 outputs); returns the largest deviation."""
    assert out.shape == ref64.shape, (what, out.shape, ref64.shape)
    dev = (out.to(F64) - ref64).abs()
    bad = ~(dev <= eps)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements further than eps = {eps:.3g} "
                           f"from the oracle; worst {float(dev[bad].nan_to_num(1e30).max()):.3g}")
    return float(dev.max())


def assert_decisions(got, ref, margin64, tau, cap=CAP, what="") -> float:
    """Discrete outputs: got == ref wherever the oracle's margin is >= tau; the share of elements below tau
    must itself be <= cap (it fails otherwise: the exclusion cannot hide a failure).  Returns that share."""
    assert got.shape == ref.shape == margin64.shape, (what, got.shape, ref.shape, margin64.shape)
    firm = margin64 >= tau
    share = 1.0 - float(firm.double().mean())
    assert share <= cap, f"{what}: {share:.3g} of the elements have a margin below tau = {tau:.3g} (cap {cap:.3g})"
    bad = firm & (got != ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} decisions differ at a margin >= tau = {tau:.3g}"
    return share


# ---- the per-kernel checks: the GPU test calls them on the kernels' outputs (copied back), the CPU test
# on a stand-in built from torch fp32 ops and on its mutations.  Each returns {name: (deviation, eps)}.
def check_trunk(x_norm, w1c, b1c, w2_bf16, b2, p, a1, pm=None, keep1=None, check_a1=True, name="trunk"):
    """trunk_fwd on rows x_norm [R,784]: a1 bf16 NHWC [R,26,26,32], p bf16 [R,9216] and, in the train form, the
    flags pm = pmask_flat [R,9216]; keep1 [R,9216] 0/1 is the oracle's dropout-1 mask (None: dropout off).
    The eval form stores no a1: it is checked on the a1 that a train-form launch stored for the same images
    (check_a1=False: that launch's own check covers it).  Rounding the oracle's conv1 instead and excluding
    the windows that hold an a1 element within eps of a bf16 midpoint excludes 98 % of them (measured, B = 7
    and 257: a window reads 512 a1 elements), so that form of the check decides nothing."""
    stats = {}
    c1 = stage_conv1(x_norm, w1c, b1c)
    eps1 = stage_eps(stage_conv1(x_norm, w1c, b1c, F32), c1)
    a1n = a1.permute(0, 3, 1, 2)
    if check_a1:
        stats["a1"] = (assert_rounded_bf16(a1n, c1, eps1, f"{name} a1"), eps1)
    ref = stage_conv2_pool(a1n, w2_bf16, b2, keep1)
    eps2 = stage_eps(stage_conv2_pool(a1n, w2_bf16, b2, keep1, F32)["windows"], ref["windows"])
    eps_p = eps2 * (INV_KEEP1_F32 if keep1 is not None else 1.0)
    if pm is not None:
        pm = pm.long()
        assert (pm >> 4 == 0).all(), f"{name}: pmask bits above bit 3"
        want = torch.ones_like(pm) if keep1 is None else keep1.reshape(pm.shape).long()
        assert torch.equal((pm >> 2) & 1, want), f"{name}: keep bits differ from Philox"
    stats["p"] = (assert_rounded_bf16(p, ref["p"], eps_p, f"{name} p"), eps_p)
    if keep1 is not None:
        assert (p[keep1.reshape(p.shape) == 0].to(F32) == 0).all(), f"{name}: p is not 0 where dropout-1 drops"
    if pm is not None:
        tau = eps2
        top = ref["windows"].amax(-1)
        inf = torch.full_like(top, float("inf"))
        # all four <= -tau: code 0 and bit 3 clear for certain; else the code holds while both the gap to
        # the runner-up and the distance of the maximum from 0 (below it every ReLU is 0: code 0) are >= tau
        m_code = torch.where(top <= -tau, inf, torch.minimum(ref["gap"], top.abs()))
        stats["argmax_excluded"] = (assert_decisions(pm & 3, ref["code"], m_code, tau, CAP, f"{name} argmax code"), CAP)
        stats["pos_excluded"] = (assert_decisions((pm >> 3) & 1, (ref["pooled"] > 0).long(), top.abs(), tau, CAP,
                                                  f"{name} pooled > 0 bit"), CAP)
    return stats


def check_fc1(p, w1_bf16, z1part, ksplit, name="fc1"):
    """fc1_fwd: z1part f32 [ksplit,R,128] from p bf16 [R,9216]."""
    ref = stage_fc1_partials(p, w1_bf16, ksplit)
    eps = stage_eps(stage_fc1_partials(p, w1_bf16, ksplit, F32), ref)
    return {"z1part": (assert_within(z1part, ref, eps, f"{name} z1part"), eps)}


def _head_refs(z1part, hp, labels, keep2, inv_batch):
    args = (z1part, hp["fc1.bias"], hp["fc2.weight"], hp["fc2.bias"], labels, keep2, inv_batch)
    return stage_head(*args), stage_head(*args, dtype=F32)


def check_head_train(z1part, hp, labels, keep2, inv_batch, loss_rows, h_bf, dz1, dl_bf, name="head_train"):
    """head_train rows: z1part [ksplit,R,128], hp the fp32 head parameters by name, labels [R]; outputs
    loss_rows f32 [R], h_bf / dz1 bf16 [R,128], dl_bf bf16 [R,16].  Each tensor's eps comes from that tensor's
    own fp32-vs-float64 deviation, so it carries the dropout factor 2 and inv_batch by itself."""
    r64, r32 = _head_refs(z1part, hp, labels, keep2, inv_batch)
    e = {k: stage_eps(r32[k], r64[k], head=True) for k in ("z1", "h", "nll", "dl", "dz1")}
    stats = {"loss_rows": (assert_within(loss_rows, r64["nll"], e["nll"], f"{name} loss_rows"), e["nll"]),
             "h_bf": (assert_rounded_bf16(h_bf, r64["h"], e["h"], f"{name} h_bf"), e["h"]),
             "dz1": (assert_rounded_bf16(dz1, r64["dz1"], e["dz1"], f"{name} dz1"), e["dz1"]),
             "dl_bf": (assert_rounded_bf16(dl_bf[:, :10], r64["dl"], e["dl"], f"{name} dl_bf"), e["dl"])}
    assert (dl_bf[:, 10:].to(F32) == 0).all(), f"{name}: dl_bf columns 10..15 are not 0"
    live = torch.ones_like(r64["z1"], dtype=torch.bool) if keep2 is None else keep2.reshape(r64["z1"].shape) > 0
    assert (dz1[~live].to(F32) == 0).all() and (h_bf[~live].to(F32) == 0).all(), f"{name}: not 0 where dropout-2 drops"
    # zero pattern of dz1 among the kept units: 0 <=> z1 <= 0, decided wherever |z1| >= tau
    stats["dz1_zero_excluded"] = (assert_decisions((dz1.to(F32) == 0)[live], (r64["z1"] <= 0)[live],
                                                   r64["z1"].abs()[live], e["z1"], CAP, f"{name} dz1 zero pattern"), CAP)
    return stats


def check_head_padding(B, dz1, h_bf, dl_bf, sentinel_bits, name="head_train"):
    """Whole buffers [round_up(B,64), .]: rows [B, round_up(B,32)) exactly 0, rows above keep the sentinel."""
    Bp = (B + 31) // 32 * 32
    for t, nm in ((dz1, "dz1"), (h_bf, "h_bf"), (dl_bf, "dl_bf")):
        bits = t.view(torch.int16)
        assert (bits[B:Bp] == 0).all(), f"{name}: {nm} padding rows [{B}, {Bp}) are not 0"
        assert (bits[Bp:] == sentinel_bits).all(), f"{name}: {nm} rows from {Bp} were written"


def check_head_logp(z1part, hp, logp, keep2=None, labels=None, loss_rows=None, correct=None, name="head_eval"):
    """head_eval / head_fwd rows: logp f32 [R,10] (+ loss_rows f32 [R], correct i32 [R] with labels)."""
    r64, r32 = _head_refs(z1part, hp, labels, keep2, 1.0)
    eps = stage_eps(r32["logp"], r64["logp"], head=True)
    stats = {"logp": (assert_within(logp, r64["logp"], eps, f"{name} logp"), eps)}
    top = r64["logp"].topk(2, 1).values
    margin = top[:, 0] - top[:, 1]
    _, am = first_strict_max(r64["logp"])
    stats["argmax_excluded"] = (assert_decisions(first_strict_max(logp.to(F64))[1], am, margin, eps, CAP,
                                                 f"{name} argmax"), CAP)
    if labels is not None:
        e_nll = stage_eps(r32["nll"], r64["nll"], head=True)
        stats["loss_rows"] = (assert_within(loss_rows, r64["nll"], e_nll, f"{name} loss_rows"), e_nll)
        assert_decisions(correct.long(), (am == labels.long()).long(), margin, eps, CAP, f"{name} correct")
    return stats



# ---- the inputs of the stage-wise forward tests (tests/test_forward_oracle_cpu.py, test_gpu_forward_stages.py)
FWD_STEP, FWD_SEED, FWD_RNG_BASE = 3, 0x1234ABCD5678, 2 ** 33 + 1000   # both counter / key words non-trivial
TRUNK_B, FC1_B, HEAD_B, EVAL_B = (1, 7, 33, 257, 1025), (1, 7, 33, 511, 512, 513, 1025), (1, 7, 33, 511, 512, 513), (7, 513)


def fc1_ksplit(B: int) -> int:
    return 4 if B >= 512 else 32


@functools.lru_cache(maxsize=None)
def forward_case(B: int, data_seed: int = 5):
    """A dataset of 4B + 5 synthetic rows and a random permutation over it; with idx_stride = B, row b of
    step s reads idx[s*B + b].  Returns (images u8 [N,28,28], labels i64 [N], idx i64 [N])."""
    from pytorch_mnist_ddp_amd.data.synthetic import generate
    imgs, labels = generate(4 * B + 5, seed=data_seed)
    idx = torch.randperm(4 * B + 5, generator=torch.Generator().manual_seed(100 + B))
    return imgs, labels, idx


def keep_rows(offset: int, rows, width: int, thr8: int) -> torch.Tensor:
    """The keep mask [len(rows), width] of batch rows ``rows`` (global element index row*width + i)."""
    elems = torch.as_tensor(rows).long().view(-1, 1) * width + torch.arange(width)
    return keep_mask_at(FWD_SEED, offset, elems, thr8)


# ---------------------------------------------------------------- stage-wise backward oracle
# One function per backward kernel stage on the operands that kernel reads (csrc/include/kernels.h
# FcBwdArgs / ConvBwdArgs), dtype = F32 the torch-fp32 twin that sets stage_eps; layout helpers for the
# compact dy records, the conv2 partial slabs and the conv1 partial rows; the per-kernel checks, shared by
# tests/test_backward_oracle_cpu.py and tests/test_gpu_backward_stages.py.
FC_SPLIT_ROWS = 1024                          # kernels.h FC_BWD_SPLIT_ROWS
FC_NAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
CONV_NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")
FCB_PART = {"fc1.weight": (0, (128, 9216)), "fc1.bias": (128 * 9216, (128,)),
            "fc2.weight": (128 * 9216 + 128, (10, 128)), "fc2.bias": (128 * 9216 + 128 + 1280, (10,)),
            "loss": (128 * 9216 + 128 + 1280 + 10, ())}        # kernels.h FCB_PART_*
C1_PRE_SLABS = 256


def fc_splits(B: int) -> int:
    return (B + FC_SPLIT_ROWS - 1) // FC_SPLIT_ROWS


def conv_wgrad_groups(B: int) -> int:
    return min(256, (24 * B + 7) // 8)


def stage_fc_wgrads(dz1_bf16, p_bf16, h_bf16, dl_bf16, grad_scale=1.0, loss_rows=None, dtype=F64):
    """fc_bwd roles A and C (+ fc_grad_reduce) on rows [0, B) of dz1 / h [.,128], p [.,9216], dl [.,16]
    (B = len(loss_rows) if given, else p's rows): the four fc gradients x grad_scale, ``loss`` = mean of
    loss_rows, and ``parts``: per split s the unscaled sums over rows [1024 s, 1024 (s + 1)) and the split's
    loss sum - the FCB_PART_* partials when B > 1024; the gradients are the parts added in split order."""
    B = p_bf16.shape[0] if loss_rows is None else loss_rows.shape[0]
    parts = []
    for s in range(fc_splits(B)):
        r = slice(FC_SPLIT_ROWS * s, min(B, FC_SPLIT_ROWS * (s + 1)))
        z, d = dz1_bf16[r].to(dtype), dl_bf16[r, :10].to(dtype)
        part = {"fc1.weight": z.t() @ p_bf16[r].to(dtype), "fc1.bias": z.sum(0),
                "fc2.weight": d.t() @ h_bf16[r].to(dtype), "fc2.bias": d.sum(0)}
        if loss_rows is not None:
            part["loss"] = loss_rows[r].to(dtype).sum()
        parts.append(part)
    out = {"parts": parts}
    sc = torch.tensor(grad_scale, dtype=F32).to(dtype)
    for k in parts[0]:
        t = parts[0][k]
        for q in parts[1:]:
            t = t + q[k]
        out[k] = t * sc if k != "loss" else t / torch.tensor(float(B), dtype=dtype)
    return out


def stage_fc_dgrad(dz1_bf16, w1_bf16, pmask, no_dropout=False, dtype=F64):
    """fc_bwd role B on rows dz1 [R,128], w1 [128,9216], pmask flags [R,9216] (torch flatten order):
    ``g`` = the 64 x 144 pooled gradients per image before rounding, 0 unless (pm & 12) == 12 and scaled by
    float32(1/0.75) unless no_dropout; ``code`` = pm & 3 (copied into the records); ``live``."""
    pm = pmask.long()
    live = (pm & 12) == 12
    g = dz1_bf16.to(dtype) @ w1_bf16.to(dtype)
    if not no_dropout:
        g = g * torch.tensor(INV_KEEP1_F32, dtype=dtype)
    return dict(g=torch.where(live, g, torch.zeros_like(g)), code=pm & 3, live=live)


def route_planes(code):
    """[..., 64] codes 0..3 -> [..., 16] uint8 bit planes (the inverse of functional.route_codes)."""
    c = code.long().reshape(*code.shape[:-1], 8, 8)
    w = 1 << torch.arange(8)
    pl = torch.stack([((c & 1) * w).sum(-1), ((c >> 1) * w).sum(-1)], -1)
    return pl.reshape(*code.shape[:-1], 16).to(torch.uint8)


def dyc_pack(g_bf16, code):
    """[R,9216] bf16 gradients + codes (flatten order c*144 + pos) -> the u8 records [R, 144*144]."""
    n = g_bf16.shape[0]
    gb = g_bf16.view(n, 64, 144).permute(0, 2, 1).contiguous().view(torch.uint8)        # [R,144,128]
    pl = route_planes(code.view(n, 64, 144).permute(0, 2, 1))
    return torch.cat([gb, pl], -1).reshape(n, 144 * 144)


def dyc_unpack(rec):
    """The inverse: (g bf16 [R,9216], code i64 [R,9216]) in flatten order."""
    from pytorch_mnist_ddp_amd.ops.functional import route_codes
    n = rec.shape[0]
    rec = rec.view(n, 144, 144)
    g = rec[..., :128].contiguous().view(torch.bfloat16)
    return g.permute(0, 2, 1).reshape(n, 9216), route_codes(rec[..., 128:]).permute(0, 2, 1).reshape(n, 9216)


def dense_dy(g_bf16, code):
    """[R,64,24,24] bf16: dy[., c, 2 py + i, 2 px + j] = g where code == 2 i + j, else 0."""
    n = g_bf16.shape[0]
    g4, c4 = g_bf16.view(n, 64, 12, 12), code.view(n, 64, 12, 12)
    d = torch.zeros(n, 64, 12, 2, 12, 2, dtype=torch.bfloat16)
    for q in range(4):
        d[:, :, :, q >> 1, :, q & 1] = torch.where(c4 == q, g4, torch.zeros_like(g4))
    return d.view(n, 64, 24, 24)


def stage_conv2_wgrad(a1_bf16, dy_bf16, G=None, taps_transposed=False, drop_last_row_of=None, dtype=F64):
    """conv2_wgrad (either form) on a1 NCHW [B,32,26,26] and dense dy [B,64,24,24]: the per-group partials
    ``w`` [G,64,32,3,3] and ``b`` [G,64] - group g owns the rows [g 24B / G, (g + 1) 24B / G) of the batch's 24B dy
    rows (conv_bwd.hip r0 / r1 of both wgrad kernels) - and their sums ``conv2.weight`` / ``conv2.bias``.
    The two keyword mutations are the CPU test's."""
    B = dy_bf16.shape[0]
    G = conv_wgrad_groups(B) if G is None else G
    rows = 24 * B
    w, b = torch.zeros(G, 64, 288, dtype=dtype), torch.zeros(G, 64, dtype=dtype)
    for g in range(G):
        r0, r1 = g * rows // G, (g + 1) * rows // G
        if drop_last_row_of == g:
            r1 -= 1
        if r1 <= r0:
            continue
        b0, b1 = r0 // 24, (r1 - 1) // 24 + 1
        cols = F.unfold(a1_bf16[b0:b1].to(dtype), 3).permute(0, 2, 1).reshape(-1, 288)        # [px, ci*9 + tap]
        d = dy_bf16[b0:b1].to(dtype).permute(0, 2, 3, 1).reshape(-1, 64)
        px = slice((r0 - 24 * b0) * 24, (r1 - 24 * b0) * 24)
        w[g], b[g] = d[px].t() @ cols[px], d[px].sum(0)
    w = w.view(G, 64, 32, 3, 3)
    if taps_transposed:
        w = w.transpose(3, 4).contiguous()
    return {"w": w, "b": b, "conv2.weight": w.sum(0), "conv2.bias": b.sum(0)}


@functools.lru_cache(maxsize=None)
def _w2part_index():
    """Flat conv2.weight index co*288 + ci*9 + tap of slab element e < 18432 (conv_grad_reduce.h)."""
    e = torch.arange(18432)
    tile, ln, r = e >> 8, (e >> 2) & 63, e & 3
    mt, nt = tile // 18, tile % 18
    return (16 * mt + 4 * (ln >> 4) + r) * 288 + (16 * (nt & 1) + (ln & 15)) * 9 + (nt >> 1)


def w2part_unpack(slabs):
    """[G,18496] slabs -> (w [G,64,32,3,3], b [G,64])."""
    G = slabs.shape[0]
    w = torch.empty(G, 18432, dtype=slabs.dtype)
    w[:, _w2part_index()] = slabs[:, :18432]
    return w.view(G, 64, 32, 3, 3), slabs[:, 18432:18496]


def w2part_pack(w, b):
    return torch.cat([w.reshape(w.shape[0], 18432)[:, _w2part_index()], b], 1).contiguous()


def strip_rows(s: int):
    """conv1-output rows of dgrad strip s: 7, 7, 7, 5."""
    return 7 * s, min(26, 7 * s + 7)


def _c1_strip_sums(xcols, d):
    """[B,9,676] input taps, [B,32,676] per-pixel values -> [4B,320] rows (image, strip) x (ci*10 + tap | 9)."""
    B = d.shape[0]
    out = torch.zeros(B, 4, 32, 10, dtype=d.dtype)
    for s in range(4):
        y0, y1 = strip_rows(s)
        px = slice(26 * y0, 26 * y1)
        out[:, s, :, :9] = torch.einsum("bcp,btp->bct", d[:, :, px], xcols[:, :, px])
        out[:, s, :, 9] = d[:, :, px].sum(-1)
    return out.view(4 * B, 320)


def stage_conv2_dgrad_conv1(dy_bf16, w2_bf16, x_norm, a1_bf16, relu_geq=False, dtype=F64):
    """conv2_dgrad on dense dy [B,64,24,24], w2 [64,32,3,3], the normalised fp32 input rows [B,784] and the stored
    a1 NCHW [B,32,26,26]: ``da1`` = the transposed convolution before masking and rounding, ``mask`` = the conv1
    ReLU decision, and ``c1part`` [4B,320]: per (image, strip of 7 conv1 rows) the conv1 weight (ci*10 + tap) and
    bias (ci*10 + 9) partial from bf16-rounded masked da1 and bf16-rounded x, as the kernel's second MFMA takes
    them.  The kernel masks with the stored bf16 a1 > 0 (conv_bwd.hip dgrad_mask_load: no conv1 recompute), an
    operand it reads - so the decision is exact and needs no margin."""
    B = dy_bf16.shape[0]
    da1 = F.conv_transpose2d(dy_bf16.to(dtype), w2_bf16.to(dtype))
    mask = a1_bf16.to(F32) >= 0 if relu_geq else a1_bf16.to(F32) > 0
    dq = bf16_round(da1 * mask).to(dtype).view(B, 32, 676)
    xcols = F.unfold(bf16_round(x_norm).to(dtype).view(B, 1, 28, 28), 3)
    return dict(da1=da1, mask=mask, c1part=_c1_strip_sums(xcols, dq))


def c1red_rows(nslab: int) -> int:
    return (nslab + C1_PRE_SLABS - 1) // C1_PRE_SLABS


def stage_c1_prereduce(c1part, dtype=F64):
    """c1_prereduce: [256,320], row j = sum of the partial rows [j R, min(4B, (j + 1) R)), R = ceil(4B / 256)."""
    n, R_ = c1part.shape[0], c1red_rows(c1part.shape[0])
    pad = torch.zeros(C1_PRE_SLABS * R_ - n, 320, dtype=dtype)
    return torch.cat([c1part.to(dtype), pad]).view(C1_PRE_SLABS, R_, 320).sum(1)


def stage_conv_reduce(w2w, w2b, c1part, grad_scale=1.0, dtype=F64):
    """conv_grad_reduce on the partials (w2w [G,64,32,3,3], w2b [G,64], c1part or c1red rows [.,320]): the four
    conv gradients x grad_scale."""
    sc = torch.tensor(grad_scale, dtype=F32).to(dtype)
    c1 = c1part.to(dtype).view(-1, 32, 10).sum(0)
    return {"conv2.weight": w2w.to(dtype).sum(0) * sc, "conv2.bias": w2b.to(dtype).sum(0) * sc,
            "conv1.weight": c1[:, :9].reshape(32, 1, 3, 3) * sc, "conv1.bias": c1[:, 9] * sc}


# ---- the per-kernel checks of the backward stages; each returns {name: (deviation, eps)}
def check_fc_wgrads(dz1, p, h_bf, dl_bf, grad_scale, grads, loss_rows=None, loss=None, parts=None, names=FC_NAMES,
                    name="fc_bwd"):
    """grads: {name: fp32 tensor} of the parameters in ``names``; loss: loss_log[step]; parts: per split a dict
    as stage_fc_wgrads's (B > 1024).  dz1 / h_bf / dl_bf / p may carry padding rows: only rows < B are the oracle's
    (B = len(loss_rows) if given, else p's rows)."""
    args = (dz1, p, h_bf, dl_bf, grad_scale, loss_rows)
    r64, r32 = stage_fc_wgrads(*args), stage_fc_wgrads(*args, dtype=F32)
    stats = {}
    for k in names:
        eps = stage_eps(r32[k], r64[k])
        stats[k] = (assert_within(grads[k], r64[k], eps, f"{name} {k}"), eps)
    if loss is not None:
        eps = stage_eps(r32["loss"], r64["loss"], head=True)
        stats["loss"] = (assert_within(loss.reshape(()), r64["loss"], eps, f"{name} loss_log"), eps)
    if parts is not None:
        assert len(parts) == len(r64["parts"]), f"{name}: {len(parts)} splits"
        for s, (got, w64, w32) in enumerate(zip(parts, r64["parts"], r32["parts"])):
            for k in got:
                eps = stage_eps(w32[k], w64[k], head=k == "loss")
                dev = assert_within(got[k], w64[k], eps, f"{name} part {s} {k}")
                old = stats.get(f"part {k}", (0.0, 0.0))
                stats[f"part {k}"] = (max(old[0], dev), max(old[1], eps)) if dev / max(eps, 1e-300) >= \
                    old[0] / max(old[1], 1e-300) else old
    return stats


def check_fc_dgrad(dz1_rows, w1_bf16, pm_rows, no_dropout, rec_rows, name="fc_bwd dyc"):
    """Role B's records of the given rows: all 64 x 144 gradients against the bf16 rounding of the oracle, exactly
    0 where the flags are not 12, the code planes bit for bit pm & 3."""
    r64 = stage_fc_dgrad(dz1_rows, w1_bf16, pm_rows, no_dropout)
    eps = stage_eps(stage_fc_dgrad(dz1_rows, w1_bf16, pm_rows, no_dropout, F32)["g"], r64["g"])
    g, code = dyc_unpack(rec_rows)
    stats = {"dyc g": (assert_rounded_bf16(g, r64["g"], eps, f"{name} g"), eps)}
    assert (g.view(torch.int16)[~r64["live"]] & 0x7FFF == 0).all(), f"{name}: g is not 0 where the flags are not 12"
    assert torch.equal(code, r64["code"]), f"{name}: code planes differ from pmask & 3"
    return stats


def check_conv2_wgrad(a1_nchw, dy, slabs, name="conv2_wgrad"):
    """slabs f32 [G,18496]: every group's weight and bias partial, element by element."""
    G = slabs.shape[0]
    r64, r32 = stage_conv2_wgrad(a1_nchw, dy, G), stage_conv2_wgrad(a1_nchw, dy, G, dtype=F32)
    w, b = w2part_unpack(slabs)
    ew, eb = stage_eps(r32["w"], r64["w"]), stage_eps(r32["b"], r64["b"])
    return {"w2part w": (assert_within(w, r64["w"], ew, f"{name} w2part weight"), ew),
            "w2part b": (assert_within(b, r64["b"], eb, f"{name} w2part bias"), eb)}


def check_conv2_dgrad(dy, w2_bf16, x_norm, a1_nchw, c1part, name="conv2_dgrad"):
    """c1part f32 [4B,320] element by element.  A partial depends on the bf16 roundings of da1, which the oracle
    can only decide up to the accumulation error of da1, so its eps is stage_eps over the whole chain dy -> partial
    with both dtypes rounding da1 to bf16: the fp32 twin's midpoint flips are in the measured deviation.  On the
    MI355X this alone held at every size (docs/COVERAGE.md 2.4: the kernel's deviations are 1e-9 to 2e-7, below
    the chain eps throughout), so no explicit midpoint bound and no exclusion is needed."""
    args = (dy, w2_bf16, x_norm, a1_nchw)
    r64, r32 = stage_conv2_dgrad_conv1(*args), stage_conv2_dgrad_conv1(*args, dtype=F32)
    eps = stage_eps(r32["c1part"], r64["c1part"])
    return {"c1part": (assert_within(c1part, r64["c1part"], eps, f"{name} c1part"), eps)}


def check_c1red(c1part, c1red, name="c1_prereduce"):
    r64 = stage_c1_prereduce(c1part)
    eps = stage_eps(stage_c1_prereduce(c1part, F32), r64)
    return {"c1red": (assert_within(c1red, r64, eps, f"{name} c1red"), eps)}


def check_conv_reduce(slabs, c1rows, grad_scale, grads, name="conv_grad_reduce"):
    """grads {name: fp32} of the four conv parameters from slabs [G,18496] and the conv1 rows the reduce read
    (c1part [4B,320], or c1red [256,320])."""
    w, b = w2part_unpack(slabs)
    r64, r32 = stage_conv_reduce(w, b, c1rows, grad_scale), stage_conv_reduce(w, b, c1rows, grad_scale, F32)
    stats = {}
    for k in CONV_NAMES:
        eps = stage_eps(r32[k], r64[k])
        stats[k] = (assert_within(grads[k], r64[k], eps, f"{name} {k}"), eps)
    return stats


# ---- input_grad (csrc/kernels/input_grad.hip): the oracle, its comparator and the mutations that
# tests/test_input_grad_oracle_cpu.py proves the comparator on
IG_SENT_BITS = 0x7FC00000                     # what torch.full(.., nan) holds: the sentinel of dx and its guard row
IG_MUTATIONS = ("da1_bf16", "relu_geq", "denormal_off", "halo_zero_1", "halo_zero_2", "halo_zero_3", "row25_dropped",
                "pad_leak", "planes_swapped", "odd_by_even", "conv2_taps_transposed", "conv1_taps_transposed",
                "prev_image_mask", "pixel_27_27_zeroed", "corner_scaled", "guard_row_written")


def ig_ring() -> torch.Tensor:
    """bool [28,28]: rows and columns 0, 1, 26, 27 - the 208 pixels that fewer than nine conv1 taps reach."""
    m = torch.zeros(28, 28, dtype=torch.bool)
    m[[0, 1, 26, 27], :] = True
    m[:, [0, 1, 26, 27]] = True
    return m


def ig_support(py: int, px: int) -> torch.Tensor:
    """bool [28,28]: the dx pixels that the one pooled record (py, px) can reach - its 2 x 2 window of dy, widened by
    two rows and columns by each of the two 3 x 3 transposed convolutions."""
    m = torch.zeros(28, 28, dtype=torch.bool)
    m[2 * py:2 * py + 6, 2 * px:2 * px + 6] = True
    return m


def stage_input_grad(dy_bf16, w2_bf16, a1_bf16, w1c, dtype=F64, mut=None):
    """input_grad on dense dy [B,64,24,24], the bf16 conv2 weight [64,32,3,3], the stored a1 NCHW [B,32,26,26] and the
    fp32 conv1 weight [32,1,3,3]: dx [B,1,28,28] = conv_transpose2d(conv_transpose2d(dy, w2) * (a1 > 0), w1c).
    da1 stays in ``dtype`` throughout (the kernel does not round it to bf16: its contract); the mask is the stored
    a1, an operand, so the decision is exact and needs no margin.  ``mut``: one of IG_MUTATIONS that acts on the
    dense operands (the CPU test's; ``planes_swapped`` / ``odd_by_even`` act on the records and
    ``guard_row_written`` on the buffer, in that test's stand-in)."""
    B = dy_bf16.shape[0]
    dy, w2, w1 = dy_bf16.to(dtype), w2_bf16.to(dtype), w1c.to(dtype).reshape(32, 1, 3, 3)
    if mut == "conv2_taps_transposed":
        w2 = w2.transpose(2, 3)
    if mut == "conv1_taps_transposed":
        w1 = w1.transpose(2, 3)
    if mut == "pad_leak":                     # a dy tile without its zero columns: column -1 of row y + 1 is (y, 23)
        pad = F.pad(dy, (2, 2))
        pad[:, :, 1:, 1] = dy[:, :, :-1, 23]
        da1 = F.conv_transpose2d(pad, w2)[..., 2:28]
    else:
        da1 = F.conv_transpose2d(dy, w2)
    a1 = a1_bf16.to(F32)
    mask = a1 >= 0 if mut == "relu_geq" else a1 >= 2.0 ** -126 if mut == "denormal_off" else a1 > 0
    if mut == "prev_image_mask":
        mask = torch.roll(mask, 1, 0)
    da1 = da1 * mask
    if mut == "da1_bf16":
        da1 = bf16_round(da1).to(dtype)
    if mut == "row25_dropped":
        da1[:, :, 25] = 0
    dx = F.conv_transpose2d(da1, w1)
    if mut in ("halo_zero_1", "halo_zero_2", "halo_zero_3"):       # strip s computes its 7 rows without da1 row 7 s - 2
        y0 = 7 * int(mut[-1])
        cut = da1.clone()
        cut[:, :, y0 - 2] = 0
        dx[:, :, y0:y0 + 7] = F.conv_transpose2d(cut, w1)[:, :, y0:y0 + 7]
    if mut == "pixel_27_27_zeroed":
        dx[B - 1, 0, 27, 27] = 0
    if mut == "corner_scaled":
        dx[B - 1, 0, 0, 0] *= 1.5
    return dx


def check_input_grad(dy, w2_bf16, a1_nchw, w1c, dx, guard=None, name="input_grad"):
    """dx f32 [B,784] (or [B,1,28,28]) element by element, under the eps rule (f32_eps: 8 x max |torch fp32 on the
    CPU - float64| on the same operands, not below 4 fp32 ulps of the largest reference value) taken over three
    sets, each asserted: the whole launch; each image alone (images are independent in this kernel, and the hand case
    gives them gradient scales of 1e-6 .. 1e2: one eps over the launch would be the largest image's); the border ring
    alone.  ``guard``: the row after dx as it is after the launch - it must still hold the NaN sentinel's bits.
    The per-image entry of the result is the image whose deviation / eps is largest."""
    args = (dy, w2_bf16, a1_nchw, w1c)
    r64, r32 = stage_input_grad(*args), stage_input_grad(*args, dtype=F32)
    B = r64.shape[0]
    dx = dx.reshape(B, 1, 28, 28)
    stats = {}
    eps, _ = f32_eps(r32, r64)
    stats["dx"] = (assert_within(dx, r64, eps, f"{name} dx"), eps)
    worst = (0.0, 0.0)
    for b in range(B):
        e, _ = f32_eps(r32[b], r64[b])
        dev = assert_within(dx[b], r64[b], e, f"{name} dx image {b}")
        if dev / max(e, 1e-300) >= worst[0] / max(worst[1], 1e-300):
            worst = (dev, e)
    stats["dx image"] = worst
    ring = ig_ring()
    e, _ = f32_eps(r32[..., ring], r64[..., ring])
    stats["dx ring"] = (assert_within(dx[..., ring], r64[..., ring], e, f"{name} dx ring"), e)
    if guard is not None:
        assert (f32_bits(guard) == IG_SENT_BITS).all(), f"{name}: the guard row after dx was written"
    return stats


# ---- hand-made operands of the backward tests (shared by the CPU and the GPU test)
BWD_STEP = 3
FC_REAL_B, FC_HAND_B = (1, 5, 31, 32, 33, 127, 128), (1024, 1025, 2047, 2048, 2049)
CONV_B = (1, 2, 5, 85, 86, 128, 129, 341, 342)


def fcb_mr(B: int) -> int:
    return 8 if B >= 2048 else 2 if B >= 128 else 1


def dyc_check_rows(B: int) -> list[int]:
    """check_rows(B) and, beyond B = 64, the first and last row of every role-B workgroup's tile set."""
    rows = set(check_rows(B))
    if B > 64:
        n = 16 * fcb_mr(B)
        for r0 in range(0, B, n):
            rows |= {r0, min(B, r0 + n) - 1}
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def fc_hand_case(B: int):
    """Random bf16 operands of fc_bwd at realistic scales: dz1 / h_bf [Bp64,128], dl_bf [Bp64,16] with rows >= B
    and dl columns >= 10 zero (head_train's contract), p [Bp64,9216] with rows >= B NaN (they must be masked),
    loss_rows [B], and flags pm [B,9216] with all 16 low-nibble patterns in the 16 rows of every tile at
    every feature."""
    g = torch.Generator().manual_seed(7000 + B)
    Bp = (B + 63) // 64 * 64
    rn = lambda *s: torch.randn(*s, generator=g)
    keep = lambda *s: (torch.rand(*s, generator=g) < 0.5).float()
    dz1, h, dl = torch.zeros(Bp, 128), torch.zeros(Bp, 128), torch.zeros(Bp, 16)
    dz1[:B] = rn(B, 128) * keep(B, 128) * (0.05 / B)
    h[:B] = rn(B, 128).relu() * 2.0
    dl[:B, :10] = rn(B, 10) * (0.3 / B)
    p = torch.full((Bp, 9216), float("nan"))
    p[:B] = rn(B, 9216).relu() * INV_KEEP1_F32
    pm = ((torch.arange(B).view(-1, 1) + 5 * torch.arange(9216).view(1, -1) + (torch.arange(9216) >> 6)) & 15)
    return dict(dz1=bf16_round(dz1), h_bf=bf16_round(h), dl_bf=bf16_round(dl), p=bf16_round(p),
                pm=pm.to(torch.uint8), loss_rows=rn(B).abs() + 0.5)


def pmask_device(pm_flat):
    """[B,9216] flags in torch flatten order -> the device layout [B][36][64][4] (inverse of pmask_flat)."""
    B = pm_flat.shape[0]
    return pm_flat.view(B, 64, 36, 4).permute(0, 2, 1, 3).reshape(B, 9216).contiguous()


@functools.lru_cache(maxsize=None)
def conv_hand_case(B: int):
    """Dense records (every gradient non-zero, every code in every 8-channel chunk), a1 NHWC bf16 about half
    zeros, and the normalised input rows of forward_case(B)'s first B images."""
    g = torch.Generator().manual_seed(9000 + B)
    gr = bf16_round(torch.randn(B, 9216, generator=g) * (2e-3 / B))
    c = torch.arange(64).view(1, 64, 1)
    code = ((c + (c >> 3) + torch.arange(144).view(1, 1, 144) + torch.arange(B).view(B, 1, 1)) & 3).reshape(B, 9216)
    a1 = bf16_round(torch.randn(B, 26, 26, 32, generator=g).relu())
    imgs = forward_case(B)[0][:B]
    return dict(g=gr, code=code, a1=a1, imgs=imgs, x=normalize_u8(imgs).reshape(B, 784))


# a1 edge values (bf16 bits), cycled over the 32 channels at each of IG_EDGE_AT in every image: -0.0 and +0.0 (mask
# off), the smallest positive normal and two positive denormals (mask on: the kernel compares as int16 > 0), the
# largest finite value (mask on; only the sign and zero-ness of a1 reach dx)
IG_EDGE_BITS = (0x8000, 0x0000, 0x0080, 0x0001, 0x0040, 0x7F7F)
# (row, column) of a1: an interior pixel, the four corners, both sides of the strip boundaries 6 | 7, 13 | 14, 20 | 21
# (and the halo rows 5, 12, 19 above them), and the last row 25
IG_EDGE_AT = ((12, 9), (0, 0), (0, 25), (25, 0), (25, 25), (5, 3), (6, 3), (7, 3), (12, 17), (13, 17), (14, 17),
              (19, 24), (20, 24), (21, 24), (25, 13))
IG_ZERO_IMAGE, IG_CORNER_IMAGE, IG_ORIGIN_IMAGE = 1, 2, 3      # the special images (B >= 5 only)


@functools.lru_cache(maxsize=None)
def input_grad_hand_case(B: int):
    """conv_hand_case(B)'s dense records and a1 with, in addition: per-image gradient scales 1e2 .. 1e-6
    (torch.logspace over the batch, the pgd_l2_step test's span, falling: the last image is the one a norm over the
    launch sees least; image b's gradients are about 2e-3 x its scale); the
    a1 edge values IG_EDGE_BITS at IG_EDGE_AT in every image; and, from B = 5 (a smaller batch has no room for them
    beside an ordinary first and last image), image 1 all zero (every record byte 0), image 2 with the pooled corner
    record (11, 11) alone and image 3 with record (0, 0) alone, whose dx is zero outside ig_support.  Returns g bf16
    [B,9216], code [B,9216], a1 bf16 NHWC [B,26,26,32], scale [B]."""
    h = conv_hand_case(B)
    scale = torch.logspace(2, -6, B)
    g = bf16_round(h["g"].float() * (B * scale.view(B, 1)))
    code = h["code"].clone()
    a1 = h["a1"].clone()
    edge = torch.tensor(IG_EDGE_BITS * 6, dtype=torch.int32)[:32].to(torch.int16).view(torch.bfloat16)
    for k, (y, x) in enumerate(IG_EDGE_AT):
        a1[:, y, x, :] = torch.roll(edge, k)
    if B >= 5:
        g3, c3 = g.view(B, 64, 144), code.view(B, 64, 144)
        g3[IG_ZERO_IMAGE], c3[IG_ZERO_IMAGE] = 0, 0
        for b, pos in ((IG_CORNER_IMAGE, 143), (IG_ORIGIN_IMAGE, 0)):
            keep = torch.zeros(144, dtype=torch.bool)
            keep[pos] = True
            g3[b, :, ~keep], c3[b, :, ~keep] = 0, 0
    return dict(g=g, code=code, a1=a1, scale=scale)


# ---------------------------------------------------------------- optimizer-stage oracle
# One Adadelta update on the operands the kernels read (csrc/include/device_utils.h Ada::step), the bf16 shadow
# layouts, a model of the flat parameter layout, and the comparators shared by tests/test_optimizer_oracle_cpu.py
# and tests/test_gpu_optimizer_stages.py.
import numpy as np

ADA_OFFS = {"fc1.weight": 0, "fc1.bias": 1179648, "fc2.weight": 1179776, "fc2.bias": 1181056,
            "conv1.weight": 1181120, "conv1.bias": 1181440, "conv2.weight": 1181504, "conv2.bias": 1199936}
ADA_NUMEL = {"fc1.weight": 128 * 9216, "fc1.bias": 128, "fc2.weight": 1280, "fc2.bias": 10,
             "conv1.weight": 288, "conv1.bias": 32, "conv2.weight": 18432, "conv2.bias": 64}
PARAM_TOTAL, OFF_CONV = 1200000, 1181120          # mnist_common.h PARAM_TOTAL, OFF_CONV1_W (the bucket split)
ADA_ALL, ADA_FC, ADA_CONV = 0, 1, 2
ADA_RANGE = {ADA_ALL: (0, PARAM_TOTAL), ADA_FC: (0, OFF_CONV), ADA_CONV: (OFF_CONV, PARAM_TOTAL)}
ADA_STATE = ("param", "square_avg", "acc_delta")
ADA_SHADOWS = ("w1", "w1t", "w2f", "w2d")
ADA_SHADOW_OWNER = {"w1": ADA_FC, "w1t": ADA_FC, "w2f": ADA_CONV, "w2d": ADA_CONV}
ADA_RHO, ADA_EPS = 0.9, 1e-6
ADA_CONFIGS = ((1.0, 0.0), (0.7, 0.0), (0.7, 0.01))           # (lr, weight_decay)
ADA_LR_GAMMA = 0.7                                            # the lr rewritten on the device before step 3
RED_W2_PARTS, RED_ALL_PARTS = 289, 309
# what the tests put into param / square_avg / acc_delta where a launch must not write.  Finite on purpose: the
# kernels read-modify-write, and an update of a NaN is the same NaN (the CPU proof's fc_touches_conv1 mutation
# passes a NaN sentinel unseen)
ADA_SENTINEL = 4.0 / 3.0


def ada_padding() -> torch.Tensor:
    """Flat indices that belong to no parameter (after fc2.bias, conv1.weight and conv1.bias)."""
    used = torch.zeros(PARAM_TOTAL, dtype=torch.bool)
    for k, o in ADA_OFFS.items():
        used[o:o + ADA_NUMEL[k]] = True
    return (~used).nonzero().squeeze(1)


def _f32(v) -> np.float32:
    return np.float32(v)


def stage_adadelta(p, g, sq, acc, lr, rho, eps, wd, dtype=F64):
    """One Adadelta update in torch's documented order on fp32 operands; returns (param, square_avg, acc_delta).
    dtype = F64: the oracle, with the scalars first rounded to fp32 (the kernel receives them as float; its
    1 - rho is float32(1) - float32(rho)).  dtype = F32: every operation individually rounded in numpy float32,
    no fusion, denormals kept - the emulation of Ada::step."""
    lr, rho, eps, wd = _f32(lr), _f32(rho), _f32(eps), _f32(wd)
    c = _f32(1) - rho
    if dtype == F64:
        lr, rho, eps, wd, c = float(lr), float(rho), float(eps), float(wd), float(c)
        p, g, sq, acc = p.to(F64), g.to(F64), sq.to(F64), acc.to(F64)
        if wd != 0:
            g = g + wd * p
        sq = sq * rho + c * g * g
        d = (acc + eps).sqrt() / (sq + eps).sqrt() * g
        return p - lr * d, sq, acc * rho + c * d * d
    assert dtype == F32
    p, g, sq, acc = (t.detach().contiguous().numpy().astype(np.float32, copy=True) for t in (p, g, sq, acc))
    with np.errstate(all="ignore"):
        if wd != 0:
            g = g + wd * p
        sq = sq * rho + (c * g) * g
        sd = np.sqrt(sq + eps)
        d = np.sqrt(acc + eps)
        d = (d / sd) * g
        acc = acc * rho + (c * d) * d
        p = p + (-lr) * d
    assert p.dtype == sq.dtype == acc.dtype == np.float32
    return torch.from_numpy(p), torch.from_numpy(sq), torch.from_numpy(acc)


def torch_adadelta(p, g, sq, acc, lr, rho, eps, wd, foreach=None):
    """One step of torch.optim.Adadelta on the CPU, loaded with the same fp32 state."""
    par = torch.nn.Parameter(p.detach().clone())
    opt = torch.optim.Adadelta([par], lr=float(_f32(lr)), rho=rho, eps=eps, weight_decay=wd, foreach=foreach)
    opt.state[par] = {"step": torch.tensor(0.0), "square_avg": sq.detach().clone(), "acc_delta": acc.detach().clone()}
    par.grad = g.detach().clone()
    opt.step()
    st = opt.state[par]
    return par.detach(), st["square_avg"], st["acc_delta"]


def _shadow_layouts(fc1, c2):
    """fc1.weight [128,9216] and conv2.weight [64,32,3,3] (any dtype) in the four shadow layouts."""
    return {"w1": fc1.contiguous(), "w1t": fc1.t().contiguous(),
            "w2f": c2.permute(0, 2, 3, 1).reshape(64, 9, 32).contiguous(),      # [co][tap][ci]
            "w2d": c2.permute(2, 3, 1, 0).reshape(9, 32, 64).contiguous()}      # [tap][ci][co]


def stage_shadows(param):
    """The expected bf16 shadows (round to nearest even, NaN kept) of a flat fp32 parameter vector."""
    fc1 = param[:128 * 9216].view(128, 9216)
    o = ADA_OFFS["conv2.weight"]
    return {k: bf16_round(v) for k, v in _shadow_layouts(fc1, param[o:o + 18432].view(64, 32, 3, 3)).items()}


@functools.lru_cache(maxsize=None)
def shadow_sources():
    """Per shadow, the flat parameter index that each of its elements is a copy of."""
    e = torch.arange(PARAM_TOTAL)
    o = ADA_OFFS["conv2.weight"]
    return {k: v.reshape(-1) for k, v in
            _shadow_layouts(e[:128 * 9216].view(128, 9216), e[o:o + 18432].view(64, 32, 3, 3)).items()}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_shadow(got, want, what=""):
    """Bit for bit the expected bf16 value; where that is NaN, any NaN."""
    assert got.dtype == want.dtype == torch.bfloat16 and got.numel() == want.numel(), (what, got.dtype, got.shape)
    got, want = got.reshape(-1), want.reshape(-1)
    nan = torch.isnan(want)
    bad = torch.where(nan, ~torch.isnan(got), bits(got) != bits(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} shadow elements differ; first at {int(bad.nonzero()[0])}"


def ada_eps(ref64, *fp32_results):
    """Per tensor EPS_MARGIN x the largest |fp32 CPU - float64| over the given fp32 CPU results."""
    return [EPS_MARGIN * max(float((r[i].to(F64) - ref64[i]).abs().max()) for r in fp32_results) for i in range(3)]


def own_mask(lo=0, hi=0, idx=None) -> torch.Tensor:
    """Bool mask over the flat layout: the range [lo, hi) and / or the flat indices ``idx``."""
    m = torch.zeros(PARAM_TOTAL, dtype=torch.bool)
    m[lo:hi] = True
    if idx is not None:
        m[torch.as_tensor(idx, dtype=torch.long)] = True
    return m


def check_adadelta_update(before, after, own, lr, wd, rho=ADA_RHO, eps=ADA_EPS, grad=None, name="adadelta"):
    """One update of the flat elements in the bool mask ``own``: ``before`` / ``after`` hold the flat fp32 ``param``,
    ``square_avg``, ``acc_delta`` (CPU); the gradient is ``grad`` (default ``before['grad']``).  Each tensor is held to
    the float64 oracle within its measured eps; a zero gradient (without weight decay) leaves ``param`` bit-unchanged
    and makes ``square_avg`` and ``acc_delta`` exactly rho x themselves.  Returns {tensor: (deviation, eps)} and, under
    ``mismatch <tensor>``, the number of elements whose bits differ from the fp32 emulation."""
    g = (before["grad"] if grad is None else grad)[own]
    ops = (before["param"][own], g, before["square_avg"][own], before["acc_delta"][own])
    assert all(torch.isfinite(t).all() for t in ops), f"{name}: non-finite operands"
    r64 = stage_adadelta(*ops, lr, rho, eps, wd)
    emu = stage_adadelta(*ops, lr, rho, eps, wd, dtype=F32)
    e = ada_eps(r64, emu, torch_adadelta(*ops, lr, rho, eps, wd))
    stats = {}
    for i, k in enumerate(ADA_STATE):
        got = after[k][own]
        stats[k] = (assert_within(got, r64[i], e[i], f"{name} {k}"), e[i])
        stats[f"mismatch {k}"] = (float((bits(got) != bits(emu[i])).sum()), 0.0)
    if wd == 0:
        z = g == 0
        assert torch.equal(bits(after["param"][own])[z], bits(ops[0])[z]), f"{name}: param moved at a zero gradient"
        for k, old in (("square_avg", ops[2]), ("acc_delta", ops[3])):
            want = torch.from_numpy(old.numpy() * _f32(rho))
            assert torch.equal(bits(after[k][own])[z], bits(want)[z]), f"{name}: {k} is not rho x itself at a zero gradient"
    return stats


def check_ownership(before, after, own, shadows_owned, grad_own=None, name="adadelta"):
    """Outside the mask ``own``, ``param``, ``square_avg`` and ``acc_delta`` keep their bits (the caller's sentinels);
    ``grad`` keeps its bits outside ``grad_own`` (default: everywhere); the shadows named in ``shadows_owned`` are
    exactly stage_shadows of the launch's own ``param`` and the others keep their bits."""
    for k in ADA_STATE:
        assert torch.equal(bits(after[k])[~own], bits(before[k])[~own]), f"{name}: {k} was written outside its region"
    keep = torch.ones(PARAM_TOTAL, dtype=torch.bool) if grad_own is None else ~grad_own
    assert torch.equal(bits(after["grad"])[keep], bits(before["grad"])[keep]), f"{name}: grad was written"
    want = stage_shadows(after["param"])
    for k in ADA_SHADOWS:
        if k in shadows_owned:
            assert_shadow(after[k], want[k], f"{name} {k}")
        else:
            assert same_bits(after[k].reshape(-1), before[k].reshape(-1)), f"{name}: shadow {k} was written"


def check_isolation(clean, dirty, poisoned, emu_at, name="adadelta"):
    """``dirty`` = the launch of ``clean`` with a non-finite gradient at the flat indices ``poisoned``: exactly those
    elements of the three tensors take the emulation's non-finite values ``emu_at`` (param is NaN), exactly their
    shadow positions become NaN, every other element keeps the clean run's bits."""
    idx = torch.as_tensor(poisoned, dtype=torch.long)
    hit = torch.zeros(PARAM_TOTAL, dtype=torch.bool)
    hit[idx] = True
    for i, k in enumerate(ADA_STATE):
        got, want = dirty[k][idx], emu_at[i]
        assert not torch.isfinite(want).any(), f"{name}: the emulation stays finite in {k}"
        ok = torch.where(torch.isnan(want), torch.isnan(got), got == want)
        assert ok.all(), f"{name}: {k} at the poisoned elements {idx[~ok].tolist()} is {got[~ok].tolist()}"
        assert torch.equal(bits(dirty[k])[~hit], bits(clean[k])[~hit]), f"{name}: {k} changed next to a poisoned element"
    assert torch.isnan(dirty["param"][idx]).all(), f"{name}: param survived a non-finite gradient"
    for k, src in shadow_sources().items():
        h = hit[src]
        got = dirty[k].reshape(-1)
        assert torch.isnan(got[h]).all(), f"{name}: shadow {k} is finite at a poisoned element"
        assert torch.equal(bits(got)[~h], bits(clean[k].reshape(-1))[~h]), f"{name}: shadow {k} changed elsewhere"


def conv_sink_elements(lo=0, hi=RED_ALL_PARTS) -> torch.Tensor:
    """Flat parameter indices that reduce parts [lo, hi) own (conv_grad_reduce.h): the conv2 parts conv2.weight
    and conv2.bias, the conv1 parts conv1.weight and conv1.bias."""
    out = []
    if lo < RED_W2_PARTS:
        assert lo == 0 and hi >= RED_W2_PARTS, "the tests split the parts at the conv2 / conv1 boundary only"
        out += [torch.arange(ADA_OFFS[k], ADA_OFFS[k] + ADA_NUMEL[k]) for k in ("conv2.weight", "conv2.bias")]
    if hi > RED_W2_PARTS:
        assert hi == RED_ALL_PARTS and lo <= RED_W2_PARTS
        out += [torch.arange(ADA_OFFS[k], ADA_OFFS[k] + ADA_NUMEL[k]) for k in ("conv1.weight", "conv1.bias")]
    return torch.cat(out).sort().values


# ---- the inputs of the optimizer-stage tests
# square_avg = acc_delta = 0, a first step: in fc1.weight, across fc1.weight | fc1.bias, in fc2.weight, across
# conv1.weight | padding | conv1.bias, in conv2.weight - and at every padding element
ADA_ZERO_STATE = ((5000, 9000), (1179000, 1179700), (1180000, 1180400), (1181300, 1181460), (1185000, 1186000))
ADA_ZERO_GRAD = ((100000, 101000), (1181000, 1181300), (1190000, 1190100))
# the isolation test's elements: fc1 tile corners, first / last of every other tensor, the first padding element
ADA_POISON = tuple(sorted(
    [o * 9216 + i for o, i in ((0, 0), (63, 31), (64, 32), (127, 9215))] +
    [ADA_OFFS[k] + j for k in ("fc1.bias", "fc2.weight", "fc2.bias", "conv1.weight", "conv1.bias", "conv2.weight",
                               "conv2.bias") for j in (0, ADA_NUMEL[k] - 1)] +
    [ADA_OFFS["fc2.bias"] + ADA_NUMEL["fc2.bias"]]))


def _log_uniform(n, lo, hi, gen):
    return torch.pow(10.0, lo + (hi - lo) * torch.rand(n, generator=gen, dtype=F64)).to(F32)


@functools.lru_cache(maxsize=None)
def ada_case():
    """The seeded flat state: ``param`` a seed-1 Net (padding 0), ``square_avg`` / ``acc_delta`` 1e-12 .. 1e2 with
    the ADA_ZERO_STATE blocks exactly 0, and three gradients of both signs with magnitudes 1e-24 .. 1e3 (so that
    g x g is normal, denormal or 0), exactly 0 in the ADA_ZERO_GRAD blocks and of magnitude 0.1 .. 10 at the padding
    elements (whose state is 0: a skipped padding element is off by about 1e-3)."""
    from pytorch_mnist_ddp_amd.models.net import Net
    torch.manual_seed(1)
    net = Net()
    gen = torch.Generator().manual_seed(4242)
    param = torch.zeros(PARAM_TOTAL)
    for k, v in net.named_parameters():
        param[ADA_OFFS[k]:ADA_OFFS[k] + v.numel()] = v.detach().reshape(-1)
    sq, acc = _log_uniform(PARAM_TOTAL, -12, 2, gen), _log_uniform(PARAM_TOTAL, -12, 2, gen)
    pad, grads = ada_padding(), []
    for a, b in ADA_ZERO_STATE:
        sq[a:b], acc[a:b] = 0.0, 0.0
    sq[pad], acc[pad] = 0.0, 0.0
    for _ in range(3):
        g = _log_uniform(PARAM_TOTAL, -24, 3, gen) * (torch.randint(0, 2, (PARAM_TOTAL,), generator=gen) * 2 - 1)
        for a, b in ADA_ZERO_GRAD:
            g[a:b] = 0.0
        g[pad] = _log_uniform(len(pad), -1, 1, gen) * (torch.randint(0, 2, (len(pad),), generator=gen) * 2 - 1)
        grads.append(g)
    return dict(param=param, square_avg=sq, acc_delta=acc, grads=tuple(grads))


def shadow_specials() -> torch.Tensor:
    """fp32 values whose bf16 rounding is a corner: ties to even both ways, +-0, denormals, the largest finite fp32
    (rounds to inf), +-inf, NaN."""
    b = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties: down to even 0x3F80, up to even 0x3F82
         0x3F808001, 0x3F817FFF,                              # just above / below a tie
         0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF,   # +-0, denormals
         0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000]
    return torch.from_numpy(np.array(b, dtype=np.uint32).view(np.float32).copy())


# their bf16 bits (the last is any NaN)
SHADOW_SPECIAL_BITS = (0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F81, 0, 0x8000, 0, 0x8000, 0, 2, 0x80,
                       0x7F80, 0xFF80, 0x7F80, 0xFF80, None)
# where the refresh test places them: fc1.weight (o, i) at the corners of the 64 x 32 update tiles, and the first
# elements of conv2.weight (flat offsets from the tensor's start)
SHADOW_SPECIAL_AT = {"fc1.weight": [o * 9216 + i for o in (0, 63, 64, 127) for i in (0, 31, 32, 4607, 9215)][:18],
                     "conv2.weight": [0, 1, 8, 9, 287, 288, 289, 4000, 4001, 9215, 9216, 12345, 18000, 18142, 18143,
                                      18144, 18430, 18431]}


# ---------------------------------------------------------------- fp32-path stage oracle
# One function per kernel of csrc/kernels/f32_net.hip on the operands that kernel reads, in the kernel's own
# layouts (csrc/include/kernels.h F32Step), no bf16 rounding anywhere.  dtype = F64 is the oracle, dtype = F32 the
# torch-fp32 twin that sets each stage's eps and is the CPU proof's stand-in for the kernels; ``mut`` names the
# single mutations of tests/test_fp32_oracle_cpu.py.  ``f32_run_stage`` is the per-launch protocol (sentinel,
# launch, ownership, oracle, repeat) shared by that test and tests/test_gpu_fp32_stages.py.
import dataclasses

F32_ULPS = 4.0               # floor of an fp32 output's eps, in ulps of the largest reference magnitude (head: HEAD_ULPS)
F32_SENT_F, F32_SENT_I, F32_SENT_B = 0x7FC0F32A, -0x55555556, 0xAA      # sentinel bits: f32 (a NaN), i32, u8
F32_LOG_N, F32_OUT_ROW = 8, 1     # loss_log entries; loss_rows / correct are used from this row on (an offset pointer)
F32_FWD = {"prep": 1, "conv1": 2, "conv2": 4, "pool": 8, "fc1": 16, "head": 32}
F32_BWD = {"fc_small": 0, "fc1w": 1, "fc1x": 2, "conv2w": 3, "conv2x_conv1w": 4, "conv_reduce": 5}
F32_TRUNK_B, F32_HAND_B = (1, 3, 33, 65), (257, 1025)
PARAM_SHAPES = {"fc1.weight": (128, 9216), "fc1.bias": (128,), "fc2.weight": (10, 128), "fc2.bias": (10,),
                "conv1.weight": (32, 1, 3, 3), "conv1.bias": (32,), "conv2.weight": (64, 32, 3, 3), "conv2.bias": (64,)}


@dataclasses.dataclass
class F32Cfg:
    """What a launch takes besides its buffers: the StepState fields (``state`` False: a null pointer, the eval
    form), the input form (rows through ``idx`` or pre-gathered) and the loss scale."""
    B: int
    step: int = FWD_STEP
    seed: int = FWD_SEED
    rng_base: int = FWD_RNG_BASE
    flags: int = 0
    world: int = 1
    use_idx: bool = True
    train: bool = True

    @property
    def stride(self):
        return self.B if self.train else 0

    @property
    def inv_batch(self):
        return float(torch.tensor(1.0 / (self.B * self.world), dtype=F32)) if self.train else 0.0

    @property
    def dropout(self):
        return self.train and not (self.flags & 1)

    def rows(self, idx):
        """Dataset rows of the batch: row b of the step is step * stride + b, through idx when it is given."""
        r = (self.step if self.train else 0) * self.stride + torch.arange(self.B)
        return idx.long()[r] if self.use_idx else r


def f32_splits(B: int) -> dict:
    """f32_net.hip's host split rules: fc1 split-K, conv2 weight-gradient chunk / slabs, conv1 slabs."""
    K = B * 576
    kc = (-(-K // 128) + 15) // 16 * 16
    return dict(fc1=36 if B <= 1024 else 9, conv2w_kc=kc, conv2w=-(-K // kc), conv1w=1024)


def f32_flat_params(net) -> torch.Tensor:
    flat = torch.zeros(PARAM_TOTAL, dtype=F32)
    for n, p in net.named_parameters():
        flat[ADA_OFFS[n]:ADA_OFFS[n] + ADA_NUMEL[n]] = p.detach().reshape(-1).float()
    return flat


def f32_params(flat) -> dict:
    return {k: flat[o:o + ADA_NUMEL[k]].view(PARAM_SHAPES[k]) for k, o in ADA_OFFS.items()}


def f32o_prep(param, train=True, mut=None):
    """Pure permutations of conv2.weight [co][ci][tap] and fc1.weight [o][c*144 + pos]."""
    d = f32_params(param)
    w2 = d["conv2.weight"].reshape(64, 32, 9)
    w2b = d["conv2.weight"].transpose(2, 3).reshape(64, 32, 9) if mut == "w2bwd_taps_transposed" else w2
    out = {"w2fwd": w2.permute(2, 1, 0).contiguous(), "w2bwd": w2b.permute(2, 0, 1).contiguous()}
    if train:
        w1 = d["fc1.weight"]
        out["w1p"] = w1.view(128, 144, 64).contiguous() if mut == "w1p_swapped" else \
            w1.view(128, 64, 144).permute(0, 2, 1).contiguous()
    return out


def f32o_conv1(x_norm, param, dtype=F64):
    """a1 NHWC [B,26,26,32] = relu(conv1) of the normalised rows [B,784]."""
    d = f32_params(param)
    return stage_conv1(x_norm, d["conv1.weight"], d["conv1.bias"], dtype).permute(0, 2, 3, 1).contiguous()


def f32o_conv2(a1, w2fwd, param, dtype=F64):
    """y2 NHWC [B,24,24,64] from a1 NHWC and w2fwd [tap][ci][co]."""
    w = w2fwd.view(3, 3, 32, 64).permute(3, 2, 0, 1)
    y = F.conv2d(a1.permute(0, 3, 1, 2).to(dtype), w.to(dtype), f32_params(param)["conv2.bias"].to(dtype))
    return y.permute(0, 2, 3, 1).contiguous()


def f32o_pool(y2, cfg, dtype=F64, mut=None):
    """f32_pool: ``p`` [B,9216] torch flatten order, ``pm`` u8 [B,144,64] (None in the eval form), and the window
    values ``win`` [B,9216,4].  Dropout-1 draws Philox at rng_base + 2 step, block (b*9216 + flat) >> 4; under
    STEP_FLAG_NO_DROPOUT nothing is drawn: every unit is kept and p is unscaled."""
    B = y2.shape[0]
    win = pool_windows(y2.permute(0, 3, 1, 2).contiguous().to(dtype))
    r = F.relu(win)
    if mut == "last_max_wins":
        pooled, code = r[..., 0].clone(), torch.zeros(r.shape[:-1], dtype=torch.long)
        for k in range(1, 4):
            m = r[..., k] >= pooled
            pooled, code = torch.where(m, r[..., k], pooled), torch.where(m, torch.full_like(code, k), code)
    else:
        pooled, code = first_strict_max(r)
    keep = torch.ones(B, 9216, dtype=dtype)
    if cfg.dropout:
        elems = torch.arange(B).view(-1, 1) * 9216 + torch.arange(9216)
        off = cfg.rng_base + 2 * cfg.step + (1 if mut == "philox_offset" else 0)
        keep = keep_mask_at(cfg.seed, off, elems, 192).to(dtype)
    p = pooled * keep * torch.tensor(INV_KEEP1_F32 if cfg.dropout else 1.0, dtype=dtype)
    pm = None
    if cfg.train:
        pos = pooled >= 0 if mut == "pooled_geq" else pooled > 0
        flat = code | (keep.long() << 2) | (pos.long() << 3)
        pm = flat.view(B, 64, 144).permute(0, 2, 1).contiguous().to(torch.uint8)
    return dict(p=p, pm=pm, win=win, keep=keep)


def f32o_head(z1part, param, labels, cfg, dtype=F64, mut=None):
    """f32_head on z1part [S,B,128]: stage_head with dropout-2 at rng_base + 2 step + 1 and the launch's inv_batch;
    ``dl`` [B,16] (columns 10..15 zero), ``correct`` (eval)."""
    d = f32_params(param)
    B = z1part.shape[1]
    keep2 = None
    if cfg.dropout:
        keep2 = keep_mask_at(cfg.seed, cfg.rng_base + 2 * cfg.step + 1, torch.arange(B).view(-1, 1) * 128 + torch.arange(128), 128)
    inv = float(torch.tensor(1.0 / B, dtype=F32)) if mut == "inv_batch_no_world" else cfg.inv_batch
    zp = z1part[:12] if mut == "head_12_partials" else z1part
    out = stage_head(zp, d["fc1.bias"], d["fc2.weight"], d["fc2.bias"], labels, keep2, inv if cfg.train else 1.0, dtype)
    w2 = d["fc2.weight"].to(dtype)
    if mut == "dl_no_label":
        out["dl"] = out["logp"].exp() * inv
        out["dz1"] = (out["dl"] @ w2) * (1.0 if keep2 is None else keep2.to(dtype) * 2.0) * (out["z1"] > 0)
    if mut == "drop2_scale_missing" and keep2 is not None:
        out["dz1"] = (out["dl"] @ w2) * keep2.to(dtype) * (out["z1"] > 0)
    out["dl"] = torch.cat([out["dl"], torch.zeros(B, 6, dtype=dtype)], 1)
    out["keep2"] = keep2
    top = out["logp"].topk(2, 1).values
    out["gap"] = top[:, 0] - top[:, 1]
    out["correct"] = (first_strict_max(out["logp"])[1] == labels.long()).to(torch.int32)
    return out


def f32o_fc_small(h, dl, dz1, loss_rows, dtype=F64, mut=None):
    B = h.shape[0]
    d = dl[:, :10].to(dtype)
    n = (B + 3) // 4 * 4 if mut == "loss_padded_B" else B
    return {"fc2.weight": d.t() @ h.to(dtype), "fc2.bias": d.sum(0), "fc1.bias": dz1.to(dtype).sum(0),
            "loss": loss_rows.to(dtype).sum() / torch.tensor(float(n), dtype=dtype)}


def f32o_fc1w(dz1, p, dtype=F64):
    return dz1.to(dtype).t() @ p.to(dtype)


def f32o_fc1x(dz1, w1p, pm, cfg, dtype=F64, mut=None):
    """fc1 input gradient through dropout-1 and the un-pooling: dense NHWC ``dy2`` [R,24,24,64] and ``routed``,
    the elements that may be non-zero (the window position pm & 3 of the units with pm & 12 == 12)."""
    R_ = dz1.shape[0]
    dp = dz1.to(dtype) @ w1p.reshape(128, 9216).to(dtype)                       # [R, pos*64 + c]
    scale = INV_KEEP1_F32 if cfg.dropout and mut != "drop1_scale_missing" else 1.0
    pmv = pm.reshape(R_, 12, 12, 64).long()
    live, code = (pmv & 12) == 12, pmv & 3
    if mut == "wrong_quadrant":
        code = code ^ 1
    g = torch.where(live, dp.view(R_, 12, 12, 64) * torch.tensor(scale, dtype=dtype), torch.zeros((), dtype=dtype))
    dy = torch.zeros(R_, 12, 2, 12, 2, 64, dtype=dtype)
    routed = torch.zeros(R_, 12, 2, 12, 2, 64, dtype=torch.bool)
    for q in range(4):
        dy[:, :, q >> 1, :, q & 1, :] = torch.where(code == q, g, torch.zeros((), dtype=dtype))
        routed[:, :, q >> 1, :, q & 1, :] = (pmv & 3 == q) & live
    return dict(dy2=dy.view(R_, 24, 24, 64), routed=routed.view(R_, 24, 24, 64))


def f32o_conv2w(dy2, a1, dtype=F64, mut=None):
    """conv2 weight + bias partial slabs [splits,64,289]: slab z sums the output pixels [z kc, min(K, (z+1) kc)) of
    the batch's K = 576 B; column n = tap*32 + ci, column 288 the bias."""
    B = dy2.shape[0]
    sp = f32_splits(B)
    kc, S, K = sp["conv2w_kc"], sp["conv2w"], B * 576
    cols = F.unfold(a1.permute(0, 3, 1, 2).to(dtype), 3).view(B, 32, 9, 576).permute(0, 3, 2, 1).reshape(K, 288)
    d = dy2.reshape(K, 64).to(dtype)
    part = torch.zeros(S, 64, 289, dtype=dtype)
    for z in range(S):
        r = slice(z * kc, min(K, (z + 1) * kc))
        part[z, :, :288] = d[r].t() @ cols[r]
        part[z, :, 288] = part[z, :, 287] if mut == "bias_wrong_n" else d[r].sum(0)
    return part


def f32o_conv2x(dy2, w2bwd, a1, dtype=F64, mut=None):
    """conv2 input gradient (w2bwd [tap][co][ci]) times the stored a1 > 0: dx1 NHWC [B,26,26,32] and the mask."""
    w = w2bwd.view(3, 3, 64, 32).permute(2, 3, 0, 1)
    da1 = F.conv_transpose2d(dy2.permute(0, 3, 1, 2).to(dtype), w.to(dtype)).permute(0, 2, 3, 1)
    mask = a1 >= 0 if mut == "relu_geq" else a1 > 0
    return dict(dx1=torch.where(mask, da1, torch.zeros((), dtype=dtype)).contiguous(), mask=mask)


def f32o_conv1w(dx1, x_norm, dtype=F64, mut=None):
    """conv1 weight + bias partial slabs [1024,32,10]: slab g sums the pixels [P g / G, P (g+1) / G) of P = 676 B."""
    B, G = dx1.shape[0], 1024
    P_ = 676 * B
    xc = F.unfold(x_norm.reshape(B, 1, 28, 28).to(dtype), 3).permute(0, 2, 1).reshape(P_, 9)
    d = dx1.reshape(P_, 32).to(dtype)
    vals = torch.cat([d.unsqueeze(2) * xc.unsqueeze(1), d.unsqueeze(2)], 2)           # [P,32,10]
    bounds = torch.arange(G + 1) * P_ // G
    seg = torch.searchsorted(bounds[1:].contiguous(), torch.arange(P_), right=True)
    out = torch.zeros(G, 32, 10, dtype=dtype).index_add_(0, seg, vals)
    if mut == "c1w_range_off_by_one":           # a slab that ends inside an image's first row takes one pixel more
        for g in range(G - 1):
            lo, hi = int(bounds[g]), int(bounds[g + 1])
            if hi > lo and lo // 676 != hi // 676 and hi < P_:
                out[g] += vals[hi]
    return out


def f32o_conv_reduce(c2part, c1part, dtype=F64, mut=None, stale=None):
    """The slabs' sums in torch layouts.  c2part [s2,64,289], c1part [1024,32,10]; ``stale``: the slab after them."""
    c2 = c2part.to(dtype)
    if mut == "last_slab_dropped":
        c2 = c2[:-1]
    if mut == "stale_slab":
        c2 = torch.cat([c2, stale.to(dtype).unsqueeze(0)])
    s, c1 = c2.sum(0), c1part.to(dtype).sum(0)
    return {"conv2.weight": s[:, :288].reshape(64, 9, 32).permute(0, 2, 1).reshape(64, 32, 3, 3).contiguous(),
            "conv2.bias": s[:, 288].contiguous(), "conv1.weight": c1[:, :9].reshape(32, 1, 3, 3).contiguous(),
            "conv1.bias": c1[:, 9].contiguous()}


def f32_eps(r32, r64, head=False):
    """(eps, measured): measured = 8 x max |torch fp32 - float64|; eps = that, not below 4 (head tensors 16) fp32
    ulps of the reference's largest magnitude - except that a measured 0 stays 0: exact agreement."""
    raw = EPS_MARGIN * float((r32.to(F64) - r64).abs().max())
    if raw == 0.0:
        return 0.0, 0.0
    _, e = torch.frexp(r64.abs().max())
    return max(raw, (HEAD_ULPS if head else F32_ULPS) * 2.0 ** (int(e) - 24)), raw


def _held(stats, key, out, r32, r64, head=False, what=""):
    eps, raw = f32_eps(r32, r64, head)
    dev = assert_within(out, r64, eps, f"{what} {key}")
    stats[key] = (dev, eps, raw)


def f32_bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == F32 else t


def f32_sentinel(t):
    if t.dtype == F32:
        t.view(torch.int32).fill_(F32_SENT_F)
    elif t.dtype == torch.uint8:
        t.fill_(F32_SENT_B)
    else:
        t.fill_(F32_SENT_I)


def f32_owned(stage, cfg) -> list:
    """[(buffer, index)]: what a launch of ``stage`` at cfg may write - everything else keeps its bits."""
    B, sp, o = cfg.B, f32_splits(cfg.B), F32_OUT_ROW
    rows = slice(0, B)
    g = lambda k: ("grad", slice(ADA_OFFS[k], ADA_OFFS[k] + ADA_NUMEL[k]))
    return {
        "prep": [("w2fwd", slice(0, 9)), ("w2bwd", slice(0, 9))] + ([("w1p", slice(0, 128))] if cfg.train else []),
        "conv1": [("a1", rows)], "conv2": [("y2", rows)],
        "pool": [("p", rows)] + ([("pm", rows)] if cfg.train else []),
        "fc1": [("z1part", slice(0, sp["fc1"] * B))],
        "head": [("loss_rows", slice(o, o + B))] + ([("h", rows), ("dz1", rows), ("dl", rows)] if cfg.train
                                                    else [("correct", slice(o, o + B))]),
        "fc_small": [g("fc2.weight"), g("fc2.bias"), g("fc1.bias"), ("loss_log", slice(cfg.step, cfg.step + 1))],
        "fc1w": [g("fc1.weight")], "fc1x": [("y2", rows)], "conv2w": [("c2part", slice(0, sp["conv2w"]))],
        "conv2x_conv1w": [("dx1", rows), ("c1part", slice(0, 1024))],
        "conv_reduce": [g(k) for k in CONV_NAMES],
    }[stage]


def f32_x_rows(t, cfg):
    """The normalised rows [B,784] of the launch's batch, and its labels."""
    src = cfg.rows(t["idx"])
    return normalize_u8(t["data_u8"][src]).reshape(cfg.B, 784), t["labels"][src].long()


def f32_check(stage, before, after, cfg):
    """One launch of ``stage``: ``before`` / ``after`` are all buffers (with their guard rows) copied back around
    it.  Everything the stage does not own keeps its bits; everything it owns is compared with the oracle on the
    operands in ``before``.  Returns {tensor: (deviation, eps, measured eps)} / {decision: (share below margin, cap)}."""
    B, sp, o, what = cfg.B, f32_splits(cfg.B), F32_OUT_ROW, f"f32 {stage} B={cfg.B}"
    own = f32_owned(stage, cfg)
    for name in after:
        a, b = f32_bits(after[name]).clone(), f32_bits(before[name]).clone()
        for n, ix in own:
            if n == name:
                a[ix], b[ix] = 0, 0
        assert torch.equal(a, b), f"{what}: {name} was written outside what the stage owns ({int((a != b).sum())} elements)"
    t, s = before, {}
    if stage == "prep":
        for k, v in f32o_prep(t["param"], cfg.train).items():
            assert torch.equal(f32_bits(after[k][:v.shape[0]]), f32_bits(v)), f"{what}: {k} is not the permutation"
    elif stage == "conv1":
        x, _ = f32_x_rows(t, cfg)
        _held(s, "a1", after["a1"][:B], f32o_conv1(x, t["param"], F32), f32o_conv1(x, t["param"]), what=what)
    elif stage == "conv2":
        args = (t["a1"][:B], t["w2fwd"][:9], t["param"])
        _held(s, "y2", after["y2"][:B], f32o_conv2(*args, F32), f32o_conv2(*args), what=what)
    elif stage == "pool":
        r64, r32 = f32o_pool(t["y2"][:B], cfg), f32o_pool(t["y2"][:B], cfg, F32)
        _held(s, "p", after["p"][:B], r32["p"], r64["p"], what=what)
        assert (f32_bits(after["p"][:B])[r64["keep"] == 0] == 0).all(), f"{what}: p is not +0 where dropout-1 drops"
        if cfg.train:
            pm, ref = after["pm"][:B].long(), r64["pm"].long()
            assert (pm >> 4 == 0).all(), f"{what}: pm bits above bit 3"
            assert torch.equal((pm >> 2) & 1, (ref >> 2) & 1), f"{what}: keep bits differ from Philox"
            # y2 is an operand: the fp32 twin's pooled values equal float64's, tau is 0 and every decision is held
            tau = EPS_MARGIN * float((r32["win"].to(F64) - r64["win"]).abs().max())
            top = r64["win"].topk(2, -1).values
            best = top[..., 0].view(B, 64, 144).permute(0, 2, 1)
            gap = (top[..., 0] - top[..., 1]).view(B, 64, 144).permute(0, 2, 1)
            inf = torch.full_like(best, float("inf"))
            m_code = torch.where(best <= -tau, inf, torch.minimum(gap, best.abs())) if tau > 0 else inf
            s["argmax below margin"] = (assert_decisions(pm & 3, ref & 3, m_code, tau, CAP, f"{what} argmax code"), CAP)
            s["pooled>0 below margin"] = (assert_decisions((pm >> 3) & 1, (ref >> 3) & 1, best.abs() if tau > 0 else inf,
                                                           tau, CAP, f"{what} pooled > 0 bit"), CAP)
    elif stage == "fc1":
        S = sp["fc1"]
        w1 = f32_params(t["param"])["fc1.weight"]
        got = after["z1part"][:S * B].view(S, B, 128)
        _held(s, "z1part", got, stage_fc1_partials(t["p"][:B], w1, S, F32), stage_fc1_partials(t["p"][:B], w1, S), what=what)
    elif stage == "head":
        _, y = f32_x_rows(t, cfg) if "data_u8" in t else (None, t["labels"][cfg.rows(t["idx"])].long())
        z = t["z1part"][:sp["fc1"] * B].view(sp["fc1"], B, 128)
        r64, r32 = f32o_head(z, t["param"], y, cfg), f32o_head(z, t["param"], y, cfg, F32)
        _held(s, "loss_rows", after["loss_rows"][o:o + B], r32["nll"], r64["nll"], True, what)
        if cfg.train:
            for k in ("h", "dz1", "dl"):
                _held(s, k, after[k][:B], r32[k], r64[k], True, what)
            assert (f32_bits(after["dl"][:B, 10:]) == 0).all(), f"{what}: dl columns 10..15 are not +0"
            live = torch.ones(B, 128, dtype=torch.bool) if r64["keep2"] is None else r64["keep2"] > 0
            assert (after["dz1"][:B][~live] == 0).all() and (after["h"][:B][~live] == 0).all(), \
                f"{what}: not 0 where dropout-2 drops"
            ez = f32_eps(r32["z1"], r64["z1"], True)[0]
            s["dz1 zero below margin"] = (assert_decisions((after["dz1"][:B] == 0)[live], (r64["z1"] <= 0)[live],
                                                           r64["z1"].abs()[live], ez, CAP, f"{what} dz1 zero pattern"), CAP)
        else:
            el = f32_eps(r32["logp"], r64["logp"], True)[0]
            s["correct below margin"] = (assert_decisions(after["correct"][o:o + B], r64["correct"], r64["gap"], el, CAP,
                                                          f"{what} correct"), CAP)
    elif stage == "fc_small":
        args = (t["h"][:B], t["dl"][:B], t["dz1"][:B], t["loss_rows"][o:o + B])
        r64, r32 = f32o_fc_small(*args), f32o_fc_small(*args, F32)
        gv = f32_params(after["grad"])
        for k in ("fc2.weight", "fc2.bias", "fc1.bias"):
            _held(s, k, gv[k], r32[k], r64[k], what=what)
        _held(s, "loss_log", after["loss_log"][cfg.step], r32["loss"], r64["loss"], True, what)
    elif stage == "fc1w":
        args = (t["dz1"][:B], t["p"][:B])
        _held(s, "fc1.weight", f32_params(after["grad"])["fc1.weight"], f32o_fc1w(*args, F32), f32o_fc1w(*args), what=what)
    elif stage == "fc1x":
        rows = torch.tensor(check_rows(B))
        args = (t["dz1"][rows], t["w1p"][:128], t["pm"][rows], cfg)
        r64, r32 = f32o_fc1x(*args), f32o_fc1x(*args, F32)
        got = after["y2"][rows]
        _held(s, "dy2", got, r32["dy2"], r64["dy2"], what=what)
        assert (f32_bits(got)[~r64["routed"]] == 0).all(), f"{what}: dy2 is not +0 off the routed quadrant"
    elif stage == "conv2w":
        args = (t["y2"][:B], t["a1"][:B])
        _held(s, "c2part", after["c2part"][:sp["conv2w"]], f32o_conv2w(*args, F32), f32o_conv2w(*args), what=what)
    elif stage == "conv2x_conv1w":
        args = (t["y2"][:B], t["w2bwd"][:9], t["a1"][:B])
        r64, r32 = f32o_conv2x(*args), f32o_conv2x(*args, F32)
        _held(s, "dx1", after["dx1"][:B], r32["dx1"], r64["dx1"], what=what)
        assert (f32_bits(after["dx1"][:B])[~r64["mask"]] == 0).all(), f"{what}: dx1 is not +0 where the stored a1 is 0"
        x, _ = f32_x_rows(t, cfg)
        _held(s, "c1part", after["c1part"][:1024], f32o_conv1w(after["dx1"][:B], x, F32), f32o_conv1w(after["dx1"][:B], x),
              what=what)
    elif stage == "conv_reduce":
        args = (t["c2part"][:sp["conv2w"]], t["c1part"][:1024])
        r64, r32 = f32o_conv_reduce(*args), f32o_conv_reduce(*args, F32)
        gv = f32_params(after["grad"])
        for k in CONV_NAMES:
            _held(s, k, gv[k], r32[k], r64[k], what=what)
    else:
        raise KeyError(stage)
    return s


def f32_twin(stage, t, cfg, mut=None):
    """What a launch of ``stage`` leaves, from torch fp32 CPU ops (the oracle functions at dtype F32), written into
    the buffers ``t`` in place: the CPU proof's stand-in for the kernels, and with ``mut`` one subtly wrong kernel."""
    B, sp, o = cfg.B, f32_splits(cfg.B), F32_OUT_ROW
    f = lambda v: v.to(F32)
    if stage == "prep":
        for k, v in f32o_prep(t["param"], cfg.train, mut).items():
            t[k][:v.shape[0]] = v
    elif stage == "conv1":
        t["a1"][:B] = f32o_conv1(f32_x_rows(t, cfg)[0], t["param"], F32)
    elif stage == "conv2":
        t["y2"][:B] = f32o_conv2(t["a1"][:B], t["w2fwd"][:9], t["param"], F32)
    elif stage == "pool":
        r = f32o_pool(t["y2"][:B], cfg, F32, mut)
        t["p"][:B] = r["p"]
        if cfg.train:
            t["pm"][:B] = r["pm"]
    elif stage == "fc1":
        t["z1part"][:sp["fc1"] * B] = stage_fc1_partials(t["p"][:B], f32_params(t["param"])["fc1.weight"], sp["fc1"], F32).view(-1, 128)
    elif stage == "head":
        y = t["labels"][cfg.rows(t["idx"])].long()
        r = f32o_head(t["z1part"][:sp["fc1"] * B].view(sp["fc1"], B, 128), t["param"], y, cfg, F32, mut)
        t["loss_rows"][o:o + B] = r["nll"]
        if cfg.train:
            t["h"][:B], t["dz1"][:B], t["dl"][:B] = f(r["h"]), f(r["dz1"]), f(r["dl"])
        else:
            t["correct"][o:o + B] = r["correct"]
    elif stage == "fc_small":
        r = f32o_fc_small(t["h"][:B], t["dl"][:B], t["dz1"][:B], t["loss_rows"][o:o + B], F32, mut)
        gv = f32_params(t["grad"])
        for k in ("fc2.weight", "fc2.bias", "fc1.bias"):
            gv[k].copy_(r[k])
        t["loss_log"][cfg.step] = r["loss"]
    elif stage == "fc1w":
        f32_params(t["grad"])["fc1.weight"].copy_(f32o_fc1w(t["dz1"][:B], t["p"][:B], F32))
    elif stage == "fc1x":
        t["y2"][:B] = f32o_fc1x(t["dz1"][:B], t["w1p"][:128], t["pm"][:B], cfg, F32, mut)["dy2"]
    elif stage == "conv2w":
        t["c2part"][:sp["conv2w"]] = f32o_conv2w(t["y2"][:B], t["a1"][:B], F32, mut)
    elif stage == "conv2x_conv1w":
        t["dx1"][:B] = f32o_conv2x(t["y2"][:B], t["w2bwd"][:9], t["a1"][:B], F32, mut)["dx1"]
        t["c1part"][:1024] = f32o_conv1w(t["dx1"][:B], f32_x_rows(t, cfg)[0], F32, mut)
    elif stage == "conv_reduce":
        r = f32o_conv_reduce(t["c2part"][:sp["conv2w"]], t["c1part"][:1024], F32, mut, stale=t["c2part"][sp["conv2w"]])
        gv = f32_params(t["grad"])
        for k in CONV_NAMES:
            gv[k].copy_(r[k])
    else:
        raise KeyError(stage)
    if mut == "guard_row_written":
        for n, ix in f32_owned(stage, cfg):
            if n not in ("grad", "loss_log"):
                t[n][ix.stop] = 0


class F32Machine:
    """The buffers of one batch size by F32Step field name (CPU tensors here; the GPU test keeps them on the
    device) and ``launch(stage)``.  This base class launches the torch-fp32 twin."""

    def __init__(self, cfg, tensors, mut=None, mut_stage=None):
        self.cfg, self.t, self.mut, self.mut_stage = cfg, tensors, mut, mut_stage

    def launch(self, stage):
        f32_twin(stage, self.t, self.cfg, self.mut if stage == (self.mut_stage or stage) else None)

    def snapshot(self, names=None):
        return {k: v.detach().cpu().clone() for k, v in self.t.items() if v is not None and (names is None or k in names)}

    def sentinel(self, names):
        for k in names:
            f32_sentinel(self.t[k])


def f32_run_stage(m, stage, repeat=True):
    """The per-launch protocol: sentinel over every buffer the stage writes into, one launch, f32_check on the
    buffers copied back around it, and (``repeat``) a second launch over fresh sentinels that gives the same bits."""
    names = sorted({n for n, _ in f32_owned(stage, m.cfg)})
    m.sentinel(names)
    before = m.snapshot()
    m.launch(stage)
    after = m.snapshot()
    stats = f32_check(stage, before, after, m.cfg)
    if repeat:
        m.sentinel(names)
        m.launch(stage)
        again = m.snapshot(names)
        for k in names:
            assert torch.equal(f32_bits(again[k]), f32_bits(after[k])), f"f32 {stage} B={m.cfg.B}: {k} differs on a second launch"
    return stats


def f32_dataset(B, hand=False):
    """(images u8 [N,784], labels i32 [N], idx i32 [N]) with N = 4B + 5: forward_case(B), or for the hand-made
    cases (no trunk) blank images with random labels."""
    if not hand:
        imgs, labels, idx = forward_case(B)
        return imgs.reshape(-1, 784).contiguous(), labels.to(torch.int32), idx.to(torch.int32)
    g = torch.Generator().manual_seed(300 + B)
    N = 4 * B + 5
    return (torch.zeros(N, 784, dtype=torch.uint8), torch.randint(0, 10, (N,), generator=g).to(torch.int32),
            torch.randperm(N, generator=g).to(torch.int32))


def f32_state(cfg) -> torch.Tensor:
    """The 24-byte StepState as int64[3]: step | flags << 32, seed, rng_base."""
    return torch.tensor([cfg.step | (cfg.flags << 32), cfg.seed, cfg.rng_base], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def f32_hand_case(B: int):
    """Random fp32 operands of the fc kernels at realistic scales, in the spirit of fc_hand_case: p [B,9216], and
    pm [B,144,64] with all 16 flag patterns at every feature over 16 consecutive rows."""
    g = torch.Generator().manual_seed(7100 + B)
    p = torch.randn(B, 9216, generator=g).relu() * INV_KEEP1_F32
    pm = ((torch.arange(B).view(-1, 1) + 5 * torch.arange(9216).view(1, -1) + (torch.arange(9216) >> 6)) & 15)
    return dict(p=p, pm=pm.to(torch.uint8).view(B, 144, 64))


F32_TRUNK_STAGES = ("prep", "conv1", "conv2", "pool", "fc1", "head", "fc_small", "fc1w", "fc1x", "conv2w",
                    "conv2x_conv1w", "conv_reduce")
F32_HAND_STAGES = ("prep", "fc1", "head", "fc_small", "fc1w", "fc1x")
F32_EVAL_STAGES = F32_TRUNK_STAGES[:6]


@functools.lru_cache(maxsize=None)
def _f32_trained_flat():
    return f32_flat_params(trained_net())


def f32_make(cfg, hand=False, device="cpu"):
    """(F32Buffers, {F32Step field: tensor}) on ``device``: the workspace plus dataset, index vector, labels, state,
    parameters (trained_net), gradient and loss log - every buffer a launch writes filled with the sentinel."""
    from pytorch_mnist_ddp_amd.ops.functional import F32Buffers
    buf = F32Buffers.allocate(cfg.B, device, trunk=not hand)
    data, labels, idx = f32_dataset(cfg.B, hand)
    t = buf.tensors()
    for v in t.values():
        f32_sentinel(v)
    grad, log = torch.zeros(PARAM_TOTAL, dtype=F32, device=device), torch.zeros(F32_LOG_N, dtype=F32, device=device)
    f32_sentinel(grad), f32_sentinel(log)
    t.update(data_u8=data.to(device), labels=labels.to(device), idx=idx.to(device), state=f32_state(cfg).to(device),
             param=_f32_trained_flat().clone().to(device), grad=grad, loss_log=log)
    return buf, t


def f32_load_hand(t, B, which):
    """Hand-made operands into the buffers: "fwd" = p and pm (before fc1), "bwd" = h, dl, dz1, loss_rows (after
    the head: what fc_small / fc1w / fc1x read)."""
    h = f32_hand_case(B)
    if which == "fwd":
        t["p"][:B], t["pm"][:B] = h["p"].to(t["p"].device), h["pm"].to(t["pm"].device)
        return
    g = torch.Generator().manual_seed(7200 + B)
    rn = lambda *s: torch.randn(*s, generator=g)
    dl = torch.zeros(B, 16)
    dl[:, :10] = rn(B, 10) * (0.3 / B)
    dz1 = rn(B, 128) * (torch.rand(B, 128, generator=g) < 0.5).float() * (0.05 / B)
    for k, v in (("h", rn(B, 128).relu() * 2.0), ("dl", dl), ("dz1", dz1)):
        t[k][:B] = v.to(t[k].device)
    t["loss_rows"][F32_OUT_ROW:F32_OUT_ROW + B] = (rn(B).abs() + 0.5).to(t["loss_rows"].device)


def f32_run_chain(m, stages, hand=False, report=None, repeat=True):
    """Every stage of ``stages`` in order through f32_run_stage, each on what the stages before it left."""
    out = {}
    for st in stages:
        if hand and st == "fc1":
            f32_load_hand(m.t, m.cfg.B, "fwd")
        if hand and st == "fc_small":
            f32_load_hand(m.t, m.cfg.B, "bwd")
        out[st] = f32_run_stage(m, st, repeat)
        if report:
            report(st, m.cfg.B, out[st])
    return out


# ---------------------------------------------------------------- xGMI collective kernels
# numpy stand-ins of the four kernels of csrc/kernels/xgmi_allreduce.hip that walk the kernels' own index sets
# (shards, workgroup strides, fc units, virtual reduce blocks and LDS slots) over W ranks' buffers, the launchers'
# grid arithmetic, and the comparators shared by tests/test_xgmi_oracle_cpu.py and tests/test_gpu_xgmi_stages.py.
# The optimizer state is that of ONE observed rank (it is rank-local); the buffers a peer reads are all W ranks'.
XG_MAX_WG, XG_UNITS, XG_TILES, XG_TAIL_F4, XG_VB_MAX = 512, 577, 576, 368, 8
XG_FC_N, XG_CONV_N = OFF_CONV, PARAM_TOTAL - OFF_CONV
XG_SENTINEL = -7.25                                   # finite: what the tests put where a launch must not write
XG_MUTATIONS = ("rank_order_reversed", "peer_skipped", "peer_twice", "own_shard_not_updated", "own_shard_twice",
                "ragged_last_dropped", "stale_slot", "shadows_from_old_param", "w1t_untransposed", "tail_368_written",
                "ada_base_off", "conv1_part_touches_conv2", "wd_before_sum")


def _cdiv(a, b):
    return -(-a // b)


def xg_grid(kind, W, nvec=0, fuse=False, planned=XG_MAX_WG, max_wg=0, lo=0, hi=RED_ALL_PARTS):
    """The launchers' grids (clamp_grid): min(natural, cap) raised to the kernel's floor; cap = the planned grid,
    shrunk by a positive max_wg."""
    cap = planned if max_wg <= 0 else min(planned, max_wg)

    def clamp(nat, low):
        return max(1, min(XG_MAX_WG, max(low, min(nat, cap))))
    if kind == "twoshot":
        return clamp(min(XG_MAX_WG, max(1, _cdiv(_cdiv(nvec, W), 128 if fuse else 512))), 1)
    if kind == "oneshot":
        return clamp(_cdiv(nvec, 256), _cdiv(nvec, 1024))
    if kind == "fc":
        return clamp(min(_cdiv(XG_UNITS, W), XG_MAX_WG), 1)
    assert kind == "conv"
    return clamp(hi - lo, _cdiv(hi - lo, XG_VB_MAX))


def xg_fc_lo(p, W):
    return p * XG_UNITS // W


def xg_fc_f4(u, h, tail=XG_TAIL_F4):
    """fcu_f4 for all 256 lanes: the bucket float4 index of a lane's h-th float4 of unit u, -1 past the tail."""
    tid = np.arange(256)
    if u < XG_TILES:
        ot, it = divmod(u, 288)
        return ((64 * ot + (tid >> 2)) * 9216 + 32 * it + (tid & 3) * 8) // 4 + h
    q = tid + 256 * h
    return np.where(q < tail, ADA_OFFS["fc1.bias"] // 4 + q, -1)


def xg_fc_own_f4(r, W):
    """Bucket float4 indices of the units of shard r (what xgmi_fc_fused_kernel stores into rank r's out)."""
    qs = [xg_fc_f4(u, h) for u in range(xg_fc_lo(r, W), xg_fc_lo(r + 1, W)) for h in (0, 1)]
    q = np.concatenate(qs) if qs else np.zeros(0, np.int64)
    return np.unique(q[q >= 0])


@functools.lru_cache(maxsize=None)
def xg_conv_sink(bid):
    """conv_sink_index of reduce block bid: (lane * 4 + nv, flat element) of every value the block sinks."""
    slots, els = [], []
    for lane in range(16 if bid < RED_W2_PARTS else 4):
        for r in range(4):
            if bid < RED_W2_PARTS:
                e = 4 * (bid * 16 + lane)
                if e < 18432:
                    ln, tile = (e >> 2) & 63, e >> 8
                    mt, nt = divmod(tile, 18)
                    el = ADA_OFFS["conv2.weight"] + (16 * mt + 4 * (ln >> 4) + r) * 288 + (16 * (nt & 1) + (ln & 15)) * 9 + (nt >> 1)
                elif e < 18432 + 64:
                    el = ADA_OFFS["conv2.bias"] + (e - 18432) + r
                else:
                    continue
            else:
                ci, kk = divmod(4 * ((bid - RED_W2_PARTS) * 4 + lane) + r, 10)
                el = ADA_OFFS["conv1.weight"] + ci * 9 + kk if kk < 9 else ADA_OFFS["conv1.bias"] + ci
            slots.append(lane * 4 + r)
            els.append(el)
    return np.array(slots), np.array(els)


def _np_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


class XgWorld:
    """W ranks' in / out / staging buffers of one communicator channel and rank r's optimizer state.  The visit
    counters n_* take one increment per call and index: within one call the kernels' index sets are disjoint."""

    def __init__(self, W, r, ins, state=None, lr=1.0, wd=0.0, slot_floats=32768, arith=True):
        self.W, self.r, self.lr, self.wd, self.arith = W, r, lr, wd, arith
        self.inp = None
        if ins is not None:
            self.set_inputs(ins)
        n = len(self.inp[0]) if arith else PARAM_TOTAL
        self.out = [np.full(n, XG_SENTINEL, np.float32) for _ in range(W)] if arith else None
        self.stage = [np.full((2, slot_floats), XG_SENTINEL, np.float32) for _ in range(W)] if arith else None
        self.calls, self.step = 0, 0
        self.n_out = np.zeros(n, np.int32)              # stores into rank r's out, per float
        self.n_upd = np.zeros(PARAM_TOTAL, np.int32)    # Adadelta steps, per flat element
        self.n_shadow = {k: np.zeros(v.numel(), np.int32) for k, v in shadow_sources().items()}
        if state is not None:
            self.st = {k: state[k].numpy().copy() for k in ADA_STATE}
            self.sh = {k: state[k].reshape(-1).view(torch.int16).numpy().copy() for k in ADA_SHADOWS}

    def set_inputs(self, ins):
        self.inp = [t.numpy().astype(np.float32, copy=True) for t in ins]

    def snap(self, grad):
        d = {k: torch.from_numpy(self.st[k].copy()) for k in ADA_STATE}
        d.update({k: torch.from_numpy(self.sh[k].copy()).view(torch.bfloat16) for k in ADA_SHADOWS})
        d["grad"] = grad
        return d

    # ---- buffer access with the descriptor's bounds: loads past the bucket give 0, stores past it are dropped
    def _ld(self, buf, off, nvec, j):
        v = np.zeros((len(j), 4), np.float32)
        ok = (j >= 0) & (j < nvec)
        v[ok] = buf[off:off + 4 * nvec].reshape(nvec, 4)[j[ok]]
        return v

    def _st(self, buf, off, nvec, j, v, count=False):
        ok = (j >= 0) & (j < nvec)
        buf[off:off + 4 * nvec].reshape(nvec, 4)[j[ok]] = v[ok]
        if count:
            self.n_out[(off + 4 * j[ok][:, None] + np.arange(4)).reshape(-1)] += 1

    def _sum(self, vals, E, mut):
        """Rank-order fp32 sum of the W ranks' values at flat elements E, one rounding per add."""
        order = list(range(self.W))
        if mut == "rank_order_reversed":
            order.reverse()
        if mut == "peer_skipped" and self.W > 1:
            order.pop()
        if mut == "peer_twice" and self.W > 1:
            order.append(order[-1])
        if mut == "wd_before_sum":
            vals = [v + _f32(self.wd) * self.st["param"][E] for v in vals]
        with np.errstate(all="ignore"):
            s = vals[order[0]].astype(np.float32, copy=True)
            for p in order[1:]:
                s = s + vals[p]
        return s

    def _upd(self, E, g, mut):
        """Ada::step on flat elements E (any shape) with gradients g; returns (new, old) param values."""
        shape = E.shape
        E = E.reshape(-1) + (4 if mut == "ada_base_off" else 0)
        self.n_upd[E] += 1
        if not self.arith:
            return None, None
        st, t = self.st, torch.from_numpy
        old = st["param"][E]
        P, S, A = stage_adadelta(t(old), t(np.ascontiguousarray(g.reshape(-1))), t(st["square_avg"][E]), t(st["acc_delta"][E]),
                                 self.lr, ADA_RHO, ADA_EPS, 0.0 if mut == "wd_before_sum" else self.wd, dtype=F32)
        st["param"][E], st["square_avg"][E], st["acc_delta"][E] = P.numpy(), S.numpy(), A.numpy()
        return P.numpy().reshape(shape), old.reshape(shape)

    def _conv2_shadow(self, E, P, old, mut):
        E = E.reshape(-1) + (4 if mut == "ada_base_off" else 0)
        rel = E - ADA_OFFS["conv2.weight"]
        m = (rel >= 0) & (rel < 18432)
        co, rem = np.divmod(rel[m], 288)
        ci, t = np.divmod(rem, 9)
        self.n_shadow["w2f"][(co * 9 + t) * 32 + ci] += 1
        self.n_shadow["w2d"][(t * 32 + ci) * 64 + co] += 1
        if self.arith:
            h = _np_bf16((old if mut == "shadows_from_old_param" else P).reshape(-1)[m])
            self.sh["w2f"][(co * 9 + t) * 32 + ci] = h
            self.sh["w2d"][(t * 32 + ci) * 64 + co] = h

    def _elems(self, base, j):
        return base + 4 * j[:, None] + np.arange(4)

    # ---- xgmi_allreduce_kernel<W>: shard q = float4s [q S4, (q + 1) S4), workgroup stride G * 256
    def twoshot(self, offset, count, G, fuse=False, mut=None):
        W, r, nvec = self.W, self.r, count // 4
        S4, step, k0 = _cdiv(nvec, W), G * 256, np.arange(G * 256)
        self.calls += 1
        for q in range(W if self.arith else 0):                       # phase 1 of every rank: its shard of the sum
            for m in range(_cdiv(S4, step)):                          # i and i2 = i + step: together k0 + m step
                i = q * S4 + k0 + m * step
                i = i[i < (q + 1) * S4]
                s = self._sum([self._ld(self.inp[p], offset, nvec, i) for p in range(W)], self._elems(offset, np.minimum(i, nvec - 1)), mut)
                self._st(self.out[q], offset, nvec, i, s, count=q == r)
                if fuse and mut == "own_shard_twice" and q == r:
                    self._upd(self._elems(offset, i[i < nvec]), s[i < nvec], mut)
        if not self.arith:
            for m in range(_cdiv(S4, step)):
                i = r * S4 + k0 + m * step
                i = i[(i < (r + 1) * S4) & (i < nvec)]
                self.n_out[self._elems(offset, i).reshape(-1)] += 1
        for m in range(_cdiv(S4, step)):                              # phase 2 of rank r: the same index set per WG
            k = k0 + m * step
            k = k[k < S4]
            for p in range(W):
                j = p * S4 + k
                if fuse:
                    j = j[j < (nvec - 1 if mut == "ragged_last_dropped" else nvec)]
                if p != r:
                    if self.arith:
                        self._st(self.out[r], offset, nvec, j, self._ld(self.out[p], offset, nvec, j), count=True)
                    else:
                        self.n_out[self._elems(offset, j[j < nvec]).reshape(-1)] += 1
                if fuse and not (mut == "own_shard_not_updated" and p == r):
                    E = self._elems(offset, j)
                    P, old = self._upd(E, self._ld(self.out[p], offset, nvec, j) if self.arith else None, mut)
                    self._conv2_shadow(E, P, old, mut)

    # ---- xgmi_oneshot_kernel<W>: workgroup b owns float4s b 256 + tid + m G 256, m < 4
    def oneshot(self, offset, count, G, fuse=False, mut=None):
        W, r, nvec = self.W, self.r, count // 4
        step, k0 = G * 256, np.arange(G * 256)
        self.calls += 1
        slot = self.calls & 1
        rslot = (self.calls - 1) & 1 if mut == "stale_slot" else slot
        ks = [k0 + m * step for m in range(4)]
        ks = [k[k < nvec] for k in ks]
        if self.arith:
            for p in range(W):
                for k in ks:
                    self._st(self.stage[p][slot], 0, nvec, k, self._ld(self.inp[p], offset, nvec, k))
        for k in ks:
            E = self._elems(offset, k)
            s = None
            if self.arith:
                s = self._sum([self._ld(self.inp[p], offset, nvec, k) if p == r else self._ld(self.stage[p][rslot], 0, nvec, k)
                               for p in range(W)], E, mut)
            if fuse:
                P, old = self._upd(E, s, mut)
                self._conv2_shadow(E, P, old, mut)
            elif self.arith:
                self._st(self.out[r], offset, nvec, k, s, count=True)
            else:
                self.n_out[E.reshape(-1)] += 1

    # ---- xgmi_fc_fused_kernel<W>: shard p = units [p 577 / W, (p + 1) 577 / W), workgroup b owns lo_p + b + m G
    def _fc_unit(self, u, src, mut):
        """Unit u's reduced gradients from the W buffers ``src`` (one buffer: a gathered sum) and its lanes' elements."""
        nvec = XG_FC_N // 4
        q = np.stack([xg_fc_f4(u, h, XG_TAIL_F4 + (1 if mut == "tail_368_written" else 0)) for h in (0, 1)], 1)   # [256, 2]
        live = q >= 0
        E = 4 * q[:, :, None] + np.arange(4)                          # [256, 2, 4]
        g = None
        if self.arith:
            vals = [self._ld(b, 0, nvec, np.where(live, q, nvec).reshape(-1)).reshape(256, 2, 4) for b in src]
            g = self._sum(vals, np.where(live[:, :, None], E, 0), mut) if len(src) > 1 or src[0] is self.inp[0] else vals[0]
        return q, live, E, g

    def _fc_update(self, u, live, E, g, mut):
        P, old = self._upd(E[live], g[live] if self.arith else None, mut)
        if u >= XG_TILES:
            return
        ot, it = divmod(u, 288)
        rows, cols = 64 * ot + np.arange(64), 32 * it + np.arange(32)
        self.n_shadow["w1"][(rows[:, None] * 9216 + cols).reshape(-1)] += 1
        self.n_shadow["w1t"][(cols[:, None] * 128 + rows).reshape(-1)] += 1
        if not self.arith:
            return
        v8 = np.zeros((256, 2, 4), np.float32)
        v8[live] = old if mut == "shadows_from_old_param" else P
        tile = _np_bf16(v8.reshape(64, 32))                           # lane tid: row tid >> 2, columns (tid & 3) 8 ..+7
        self.sh["w1"].reshape(128, 9216)[np.ix_(rows, cols)] = tile
        ts = tile.reshape(32, 64) if mut == "w1t_untransposed" else tile.T     # the LDS transpose
        self.sh["w1t"].reshape(9216, 128)[np.ix_(cols, rows)] = ts

    def fc_fused(self, G, mut=None):
        W, r, nvec = self.W, self.r, XG_FC_N // 4
        self.calls += 1
        for q in range(W):                                            # phase 1 of every rank (the peers' phase-2 source)
            if q != r and not self.arith:
                continue
            for b in range(G):
                for u in range(xg_fc_lo(q, W) + b, xg_fc_lo(q + 1, W), G):
                    f4, live, E, g = self._fc_unit(u, self.inp if self.arith else None, mut)
                    if self.arith:
                        self._st(self.out[q], 0, nvec, f4[live], g[live], count=q == r)
                    elif q == r:
                        self.n_out[E[live].reshape(-1)] += 1
                    if q == r:
                        self._fc_update(u, live, E, g, mut)
        if W == 1:
            return
        M = _cdiv(_cdiv(XG_UNITS, W), G)
        for b in range(G):
            for j in range((W - 1) * M):                              # items: peer pp' = j mod (W - 1), m = j / (W - 1)
                pp, m = j % (W - 1), j // (W - 1)
                p = pp + (1 if pp >= r else 0)
                u = xg_fc_lo(p, W) + b + m * G
                if u >= xg_fc_lo(p + 1, W):
                    continue
                _, live, E, g = self._fc_unit(u, [self.out[p]] if self.arith else None, mut)
                self._fc_update(u, live, E, g, mut)

    # ---- xgmi_conv_reduce_fused_kernel<W>: virtual block lo + b + k G, LDS slot k 64 + lane 4 + nv
    def conv_fused(self, reds, G, lo=0, hi=RED_ALL_PARTS, mut=None):
        """reds[p]: rank p's conv_grad_reduce result, indexed by flat element - OFF_CONV."""
        W, r = self.W, self.r
        self.calls += 1
        slot = self.calls & 1
        rslot = (self.calls - 1) & 1 if mut == "stale_slot" else slot
        blocks = []
        for b in range(G):
            nvb = _cdiv(hi - lo - b, G)
            assert 0 <= nvb <= XG_VB_MAX, "more virtual blocks than LDS slots"
            idx = np.full(XG_VB_MAX * 64, -1)
            for k in range(nvb):
                sl, el = xg_conv_sink(lo + b + k * G)
                idx[k * 64 + sl] = el - OFF_CONV
            if mut == "conv1_part_touches_conv2" and lo >= RED_W2_PARTS and b == 0:
                idx[XG_VB_MAX * 64 - 1] = ADA_OFFS["conv2.weight"] + 7 - OFF_CONV
            I = idx[idx >= 0]
            blocks.append(I)
            for p in range(W if self.arith else 0):
                self.stage[p][slot][I] = reds[p][I]
        for I in blocks:
            g = None
            if self.arith:
                g = self._sum([reds[p][I] if p == r else self.stage[p][rslot][I] for p in range(W)], OFF_CONV + I, mut)
            P, old = self._upd(OFF_CONV + I, g, mut)
            self._conv2_shadow(OFF_CONV + I, P, old, mut)


# ---- the straight references and the comparators of the collective tests
def xg_ordered_sum(vals):
    """fp32 sum of the ranks' tensors in rank order, one rounding per add (what every kernel must give, bitwise)."""
    with np.errstate(all="ignore"):
        s = vals[0].numpy().astype(np.float32, copy=True)
        for v in vals[1:]:
            s = s + v.numpy()
    return torch.from_numpy(s)


def xg_same(a, b):
    """Per element: the same bits, or both NaN (the payload of a NaN made by inf - inf is the hardware's)."""
    return (bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))


def xg_check_reduce(got, vals, name="allreduce"):
    """A reduced range: bit for bit the rank-ordered fp32 sum, and within eps of the float64 sum where that is
    finite (eps = EPS_MARGIN x the ordered fp32 sum's own deviation).  Returns {"sum": (deviation, eps)}."""
    want = xg_ordered_sum(vals)
    bad = ~xg_same(got, want)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} sums differ from the rank-ordered fp32 sum; first at {int(bad.nonzero()[0])}"
    r64 = torch.stack([v.to(F64) for v in vals]).sum(0)
    fin = torch.isfinite(r64) & torch.isfinite(want)
    if not fin.any():
        return {"sum": (0.0, 0.0)}
    eps = stage_eps(want[fin], r64[fin])
    return {"sum": (assert_within(got[fin], r64[fin], eps, f"{name} sum"), eps)}


def xg_check_update(before, after, own, g32, g64, lr, wd, name="xgmi update"):
    """One fused update of the flat elements in ``own`` from the reduced gradients (g32: the rank-ordered fp32 sum,
    g64: the float64 sum, both flat): each state tensor within eps = EPS_MARGIN x max |fp32 emulation on g32 -
    float64 oracle on g64| where the oracle is finite, and bit for bit the emulation everywhere - which also holds a
    NaN / inf gradient to exactly its elements.  Returns {tensor: (deviation, eps), "mismatch <tensor>": (count, 0)}."""
    ops = [before[k][own] for k in ADA_STATE]
    assert all(torch.isfinite(t).all() for t in ops), f"{name}: non-finite state"
    r64 = stage_adadelta(ops[0], g64[own], ops[1], ops[2], lr, ADA_RHO, ADA_EPS, wd)
    emu = stage_adadelta(ops[0], g32[own], ops[1], ops[2], lr, ADA_RHO, ADA_EPS, wd, dtype=F32)
    stats = {}
    for i, k in enumerate(ADA_STATE):
        got = after[k][own]
        fin = torch.isfinite(r64[i]) & torch.isfinite(emu[i])
        eps = EPS_MARGIN * float((emu[i][fin].to(F64) - r64[i][fin]).abs().max()) if fin.any() else 0.0
        stats[k] = (assert_within(got[fin], r64[i][fin], eps, f"{name} {k}"), eps)
        n = int((~xg_same(got, emu[i])).sum())
        stats[f"mismatch {k}"] = (float(n), 0.0)
        assert n == 0, f"{name}: {n} elements of {k} differ from the fp32 emulation on the rank-ordered sum"
    return stats


def xg_bucket(seed, case, q, W, n, edges=(), poison=None, poison_at=()):
    """Rank q's input values for a bucket of n floats: randn at scales 1e-6 .. 1e3, and at every position of
    ``edges`` (and the first and last element) a 24-element block of +-1e8 / 1 triples whose fp32 sum depends on the
    order (placement rotated per element), denormals and +-0.  ``poison`` (NaN or inf) goes to ``poison_at`` on
    rank W - 1 only.  Every rank can build every rank's bucket."""
    g = torch.Generator().manual_seed(1000003 * seed + 1009 * case + q)
    v = torch.randn(n, generator=g) * _log_uniform(n, -6, 3, g)
    tri = (1e8, 1.0, -1e8)
    for e in sorted({0, max(0, n - 24), *[min(max(0, x - 12), max(0, n - 24)) for x in edges]}):
        for i in range(min(24, n - e)):
            role = (q + i) % max(W, 3)
            kind = i // 8
            if kind == 0:
                v[e + i] = tri[role] if role < 3 else v[e + i]
            elif kind == 1:
                v[e + i] = (1 - 2 * ((q + i) & 1)) * 1e-40 * (q + 1)
            else:
                v[e + i] = -0.0 if (q + i) % 3 == 0 else 0.0
    if poison is not None and q == W - 1:
        v[torch.as_tensor(list(poison_at), dtype=torch.long)] = poison
    return v
