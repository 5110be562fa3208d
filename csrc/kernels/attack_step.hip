// L2 projected-gradient step on the normalised image (L2 PGD, ascent or descent), fp32 [B][784].
//
// The L-inf step is an epilogue of input_grad (IgProjectedStep): it works element by element.  The L2
// step needs two norms per image - of the gradient and of the displacement from the clean image - and
// an image's gradient is written by four workgroups of input_grad, so this is a launch of its own that
// reads the dx input_grad stored in its plain form.  One workgroup per image, per image b:
//
//   n = sqrt(sum dx^2)                 t = x + (alpha / max(n, TINY)) * dx
//   d = t - x0;  m = sqrt(sum d^2)     d *= min(1, eps / max(m, TINY))
//   x_next = min(max(x0 + d, lo), hi)
//
// alpha < 0 is the descent (targeted) step.  A zero gradient gives n = 0, a step of alpha / TINY times
// zero, t = x.  The two max and the min and the clamps are written as comparisons that are false for a
// NaN, so a NaN anywhere in an image's dx makes n, hence every element of that image's x_next, a NaN (as
// torch.clamp does, and as the L-inf step form documents); no other image reads it.
// THE BALL: the caller gives x0 in [lo, hi], so the last clamp moves x0 + d towards x0 or not at all: it
// only shrinks |d_i|, and x_next stays inside the eps ball (up to the roundings of m, the scale and the
// sum x0 + d) as well as inside the box.
//
// SUMS: a fixed tree.  Thread t < 196 owns the float4 t of the image: (v0^2 + v1^2) + (v2^2 + v3^2); threads
// 196 .. 255 add zeros; then the xor butterfly over the wave's 64 lanes (wave_sum), then the four wave
// sums through LDS as (w0 + w1) + (w2 + w3).  Every operation is rounded on its own (contraction off), no
// atomics, nothing depends on the grid, the stream or the launch count: the same operands give the same
// bits.  x_next may alias x: a thread loads its x, x0 and dx elements before it stores, and it is the only
// one that touches them.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

__global__ __launch_bounds__(ROW_THREADS) void pgd_l2_step_kernel(PgdL2StepArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[2][ROW_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t v4 = (int64_t)blockIdx.x * ROW_VECS + (own ? tid : 0);   // (idle threads: a valid address)
  RW_ENTRY();
  float4 g = reinterpret_cast<const float4*>(a.dx)[v4];
  const float4 x = reinterpret_cast<const float4*>(a.x)[v4];
  const float4 c = reinterpret_cast<const float4*>(a.x0)[v4];
  if (!own) g = float4{0.0f, 0.0f, 0.0f, 0.0f};

  const float n = sqrtf(row_block_sum(row_sq4(g), part[0], wave, lane));
  const float r = a.alpha / (n < PGD_L2_TINY ? PGD_L2_TINY : n);
  float4 d;
  d.x = (x.x + r * g.x) - c.x;
  d.y = (x.y + r * g.y) - c.y;
  d.z = (x.z + r * g.z) - c.z;
  d.w = (x.w + r * g.w) - c.w;
  if (!own) d = float4{0.0f, 0.0f, 0.0f, 0.0f};

  const float m = sqrtf(row_block_sum(row_sq4(d), part[1], wave, lane));
  float sc = a.eps / (m < PGD_L2_TINY ? PGD_L2_TINY : m);
  sc = sc > 1.0f ? 1.0f : sc;
  if (own) {
    float4 o;
    o.x = clamp_nan_passes(c.x + d.x * sc, a.lo, a.hi);
    o.y = clamp_nan_passes(c.y + d.y * sc, a.lo, a.hi);
    o.z = clamp_nan_passes(c.z + d.z * sc, a.lo, a.hi);
    o.w = clamp_nan_passes(c.w + d.w * sc, a.lo, a.hi);
    reinterpret_cast<float4*>(a.x_next)[v4] = o;
  }
}

void launch_pgd_l2_step(const PgdL2StepArgs& a, int B, hipStream_t s) {
  if (B < 1 || B > INPUT_GRAD_MAX_B) throw std::runtime_error("pgd_l2_step: batch size out of range");
  if (!a.dx || !a.x || !a.x0 || !a.x_next) throw std::runtime_error("pgd_l2_step: null argument");
  if (misaligned(15, a.dx, a.x, a.x0, a.x_next))
    throw std::runtime_error("pgd_l2_step: the four arrays must be 16-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("pgd_l2_step: eps must be >= 0");
  hipLaunchKernelGGL(pgd_l2_step_kernel, dim3(B), dim3(ROW_THREADS), 0, s, a);
}

void preload_attack_step() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&pgd_l2_step_kernel));
}

}  // namespace mnist
