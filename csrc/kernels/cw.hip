// Carlini & Wagner's L2 attack (S&P 2017) on the normalised image, fp32 [M][784]: the whole per-image update of one
// iteration in one launch - the success test and the best point, the Adam step on the tanh-space variable, and the
// bisection of the trade-off constant c at the end of a search step.  It minimises |delta|^2 + c * hinge(margin) in
// w, with x = lo + (hi - lo) (tanh(w) + 1) / 2, so the pixel box holds by construction.
//
// One workgroup of ROW_THREADS per image, thread t < 196 owns the float4 t of each of the image's rows.  After the
// gradient chain with the CW margin at the iterate rows x: m = loss_rows[i] = max_{j != y} z_j - z_y (head_margin),
// g = dx[i] (input_grad's plain output), L = sign * m (sign = -1: targeted, labels are the classes to reach).
// D = sum (x - x0)^2 on the fixed tree, from the stored rows x: the exact bits the chain saw.
//
//   first:        c = c_init; c_lo = 0; c_hi = CW_C_INF; d_best = +inf; succ = found_search = iters = 0
//                 w = w0; m1 = v = 0; x_best = x0       (reads no state; the caller has set x = x0 exactly)
//   evaluate:     ok = (L > 0) and (L >= kappa)                          -- a NaN margin is never a success
//                 if ok: succ = 1;  if D < d_best: d_best = D; x_best = x; found_search = search + 1
//   last:         store the records and stop (w, m1, v, x keep their values)
//   search_end:   succ:  c_hi = min(c_hi, c); if c_hi < CW_C_BIG: c = (c_lo + c_hi) * 0.5
//                 else:  c_lo = max(c_lo, c); c = c_hi < CW_C_BIG ? (c_lo + c_hi) * 0.5 : c * 10
//                 succ = 0; w = w0; m1 = v = 0; x = x0 exactly           -- Carlini's re-initialised modifier
//   otherwise:    th = tanhf(w); act = (L < kappa) ? 1 : 0
//                 gx = (2 dist_scale) (x - x0) - (sign c act) g
//                 gw = gx * ((0.5 (hi - lo)) * (1 - th th))
//                 m1 = b1 m1 + (1 - b1) gw;  v = b2 v + ((1 - b2) gw) gw
//                 w  = w - (lr (m1 / bc1)) / (sqrtf(v / bc2) + adam_eps)
//                 x  = clamp_nan_passes(lo + (hi - lo) (0.5 (tanhf(w) + 1)), lo, hi);  iters += 1
//   w0 = atanhf((((x0 - lo) / (hi - lo)) * 2 - 1) * CW_SHRINK): recomputed from x0, never stored.
//
// Every search step starts from the clean image itself, so a clean image already outside `labels` is found at D = 0
// by the first launch.  bc1 = 1 - b1^t, bc2 = 1 - b2^t come from the host (float64, rounded once): the Adam step index
// t inside the current search is the same for every image.  dist_scale = MNIST_STD^2 puts the distance term in pixel
// units, so c weighs the same two quantities as in Carlini's code.
//
// DIFFERENCES from Carlini's code, all deliberate: there is no abort_early; every search step restarts from the
// clean image exactly (his modifier restarts at zero, the same point); success is read from the margin the gradient
// chain computed, not from a second forward; the targeted form shares the hinge through `sign`.
//
// Every decision is a comparison of input floats or of integers.  A NaN margin is never a success, and L < kappa is
// false for it too: the hinge is off and the step is the distance term's alone (times 0 * g: a NaN g still passes).
// A NaN in an image's gradient reaches that image's w and x only (its own elements), never another image's.
//
// SUMS: one, D, on pgd_l2_step's fixed tree with its own LDS words.  Every operation is rounded on its own
// (contraction off, no packed fp32), divisions and square roots are the correctly rounded ones, no atomics, nothing
// depends on the grid, the stream or the launch count: the same operands give the same bits.
//
// STATE: the per-image scalars are two 16-byte records (kernels.h); every thread loads them, thread 0 stores them.
// The __syncthreads between the loads and anything thread 0 stores keeps a wave that starts late from reading the
// new record.  Row elements are read and written by their owner only, and read before they are written.  The grid is
// exactly M workgroups: rows and records past M are untouched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   cw_step_kernel: VGPRs 40, SGPRs 64, LDS 16 B, scratch 0, occupancy 8 waves / SIMD
// There is no register array: the best point is one conditional store of the float4 just loaded.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
// w0 of the header: the tanh-space image of a clean pixel, pulled inside (-1, 1) by CW_SHRINK
__device__ __forceinline__ float cw_w0(float c, float lo, float span) {
#pragma clang fp contract(off)
  const float u = (c - lo) / span;
  return atanhf((u * 2.0f - 1.0f) * CW_SHRINK);
}
__device__ __forceinline__ float4 cw_w04(const float4& c, float lo, float span) {
  return float4{cw_w0(c.x, lo, span), cw_w0(c.y, lo, span), cw_w0(c.z, lo, span), cw_w0(c.w, lo, span)};
}

struct CwScalars {
  float k2, s, hs, b1, ob1, b2, ob2, lr, bc1, bc2, eps, lo, hi, span;
};

// one element's Adam step: w, m1, v in place, the new x returned
__device__ __forceinline__ float cw_adam(float& w, float& m1, float& v, float x, float c, float g, const CwScalars& k) {
#pragma clang fp contract(off)
  const float th = tanhf(w);
  const float gx = k.k2 * (x - c) - k.s * g;
  const float gw = gx * (k.hs * (1.0f - th * th));
  m1 = k.b1 * m1 + k.ob1 * gw;
  v = k.b2 * v + (k.ob2 * gw) * gw;
  w = w - (k.lr * (m1 / k.bc1)) / (sqrtf(v / k.bc2) + k.eps);
  return clamp_nan_passes(k.lo + k.span * (0.5f * (tanhf(w) + 1.0f)), k.lo, k.hi);
}
}  // namespace

__global__ __launch_bounds__(ROW_THREADS) void cw_step_kernel(CwStepArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[ROW_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + (own ? tid : 0);       // (idle threads: a valid address)
  RW_ENTRY();
  const float L = a.sign * a.loss_rows[i];
  const float4 c0 = reinterpret_cast<const float4*>(a.x0)[at];
  const float4 x = reinterpret_cast<const float4*>(a.x)[at];

  float c, c_lo, c_hi, d_best;
  int succ, found, iters, spare;
  if (a.first) {
    c = a.c_init; c_lo = 0.0f; c_hi = CW_C_INF; d_best = __builtin_inff();
    succ = found = iters = spare = 0;
  } else {
    const float4 f = reinterpret_cast<const float4*>(a.fstate)[i];
    const int4 n = reinterpret_cast<const int4*>(a.istate)[i];
    __syncthreads();                                       // every wave holds the old records before thread 0 stores
    c = f.x; c_lo = f.y; c_hi = f.z; d_best = f.w;
    succ = n.x; found = n.y; iters = n.z; spare = n.w;
  }

  // evaluate: the iterate the chain just saw
  float4 d{x.x - c0.x, x.y - c0.y, x.z - c0.z, x.w - c0.w};
  if (!own) d = float4{0.0f, 0.0f, 0.0f, 0.0f};
  const float D = row_block_sum(row_sq4(d), part, wave, lane);
  const bool ok = L > 0.0f && L >= a.kappa;
  const bool improved = ok && D < d_best;
  if (ok) succ = 1;
  if (improved) { d_best = D; found = a.search + 1; }
  if (own) {
    if (improved) reinterpret_cast<float4*>(a.x_best)[at] = x;
    else if (a.first) reinterpret_cast<float4*>(a.x_best)[at] = c0;
  }
  if (a.last) {
    if (tid == 0) {
      reinterpret_cast<float4*>(a.fstate)[i] = float4{c, c_lo, c_hi, d_best};
      reinterpret_cast<int4*>(a.istate)[i] = int4{succ, found, iters, spare};
    }
    return;
  }

  const float span = a.hi - a.lo;
  if (a.search_end) {                                      // bisect c, back to the clean image
    if (succ) {
      c_hi = c < c_hi ? c : c_hi;
      if (c_hi < CW_C_BIG) c = (c_lo + c_hi) * 0.5f;
    } else {
      c_lo = c > c_lo ? c : c_lo;
      c = c_hi < CW_C_BIG ? (c_lo + c_hi) * 0.5f : c * 10.0f;
    }
    if (own) {
      const float4 z{0.0f, 0.0f, 0.0f, 0.0f};
      reinterpret_cast<float4*>(a.w)[at] = cw_w04(c0, a.lo, span);
      reinterpret_cast<float4*>(a.m1)[at] = z;
      reinterpret_cast<float4*>(a.v)[at] = z;
      reinterpret_cast<float4*>(a.x)[at] = c0;
    }
    if (tid == 0) {
      reinterpret_cast<float4*>(a.fstate)[i] = float4{c, c_lo, c_hi, d_best};
      reinterpret_cast<int4*>(a.istate)[i] = int4{0, found, iters, spare};
    }
    return;
  }

  // the Adam step
  const float4 g = reinterpret_cast<const float4*>(a.dx)[at];
  float4 w, m1{0.0f, 0.0f, 0.0f, 0.0f}, v{0.0f, 0.0f, 0.0f, 0.0f};
  if (a.first) {
    w = cw_w04(c0, a.lo, span);
  } else {
    w = reinterpret_cast<const float4*>(a.w)[at];
    m1 = reinterpret_cast<const float4*>(a.m1)[at];
    v = reinterpret_cast<const float4*>(a.v)[at];
  }
  const float act = L < a.kappa ? 1.0f : 0.0f;
  CwScalars k;
  k.k2 = 2.0f * a.dist_scale;
  k.s = (a.sign * c) * act;
  k.hs = 0.5f * span;
  k.b1 = a.beta1; k.ob1 = 1.0f - a.beta1;
  k.b2 = a.beta2; k.ob2 = 1.0f - a.beta2;
  k.lr = a.lr; k.bc1 = a.bc1; k.bc2 = a.bc2; k.eps = a.adam_eps;
  k.lo = a.lo; k.hi = a.hi; k.span = span;
  float4 xn;
  xn.x = cw_adam(w.x, m1.x, v.x, x.x, c0.x, g.x, k);
  xn.y = cw_adam(w.y, m1.y, v.y, x.y, c0.y, g.y, k);
  xn.z = cw_adam(w.z, m1.z, v.z, x.z, c0.z, g.z, k);
  xn.w = cw_adam(w.w, m1.w, v.w, x.w, c0.w, g.w, k);
  if (own) {
    reinterpret_cast<float4*>(a.w)[at] = w;
    reinterpret_cast<float4*>(a.m1)[at] = m1;
    reinterpret_cast<float4*>(a.v)[at] = v;
    reinterpret_cast<float4*>(a.x)[at] = xn;
  }
  if (tid == 0) {
    reinterpret_cast<float4*>(a.fstate)[i] = float4{c, c_lo, c_hi, d_best};
    reinterpret_cast<int4*>(a.istate)[i] = int4{succ, found, iters + 1, spare};
  }
}

void launch_cw_step(const CwStepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("cw_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.x0 || !a.w || !a.m1 || !a.v || !a.x || !a.x_best || !a.fstate || !a.istate)
    throw std::runtime_error("cw_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.w, a.m1, a.v, a.x, a.x_best))
    throw std::runtime_error("cw_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.fstate, a.istate))
    throw std::runtime_error("cw_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.loss_rows)) throw std::runtime_error("cw_step: loss_rows must be 4-byte aligned");
  if (a.sign != 1.0f && a.sign != -1.0f) throw std::runtime_error("cw_step: sign must be +1 or -1");
  if (!(a.kappa >= 0.0f)) throw std::runtime_error("cw_step: kappa must be >= 0");
  if (!(a.lr > 0.0f)) throw std::runtime_error("cw_step: lr must be > 0");
  if (a.first && !(a.c_init > 0.0f)) throw std::runtime_error("cw_step: c_init must be > 0");
  if (!(a.beta1 >= 0.0f && a.beta1 < 1.0f && a.beta2 >= 0.0f && a.beta2 < 1.0f && a.adam_eps > 0.0f))
    throw std::runtime_error("cw_step: need beta1, beta2 in [0, 1) and adam_eps > 0");
  if (!(a.bc1 > 0.0f && a.bc1 <= 1.0f && a.bc2 > 0.0f && a.bc2 <= 1.0f))
    throw std::runtime_error("cw_step: the bias corrections must be in (0, 1]");
  if (!(a.dist_scale > 0.0f) || !(a.lo < a.hi)) throw std::runtime_error("cw_step: need dist_scale > 0 and lo < hi");
  if (a.search < 0) throw std::runtime_error("cw_step: the search index must be >= 0");
  if (a.first && a.last) throw std::runtime_error("cw_step: a launch is the first or the last, not both");
  hipLaunchKernelGGL(cw_step_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_cw() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&cw_step_kernel));
}

}  // namespace mnist
