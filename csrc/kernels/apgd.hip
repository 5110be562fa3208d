// Auto-PGD (Croce & Hein, ICML 2020: the gradient attack of AutoAttack) on the normalised image, fp32 [M][784]: the
// whole per-image update of one iteration in one launch - the momentum step, the step size that is halved at the
// scheduled checkpoints when progress stalls, and the restart from the best point found so far.
//
// One workgroup of ROW_THREADS per image, thread t < 196 owns the float4 t of each of the image's rows.  After the
// gradient chain at the iterate x: dx = d NLL / d x (input_grad's plain output), loss_rows = -log p_label
// (head_train).  With L = sign * loss_rows[i], g = sign * dx[i] (sign = -1: targeted, the labels' NLL is descended):
//
//   first:   eta = 2 eps; loss_best = loss_prev = loss_check = L; x_best = x; g_best = dx; n_up = 0; reduced = 1;
//            iters = 0; restarted = 0; a = 1; (src, gs) = (x, g)            -- reads no state, writes all of it
//   else:    if L > loss_prev: n_up += 1;   loss_prev = L
//            if L > loss_best: loss_best = L; x_best = x; g_best = dx
//            last: stop here (eta, loss_check, reduced, iters, restarted, x and x_old keep their values)
//            (src, gs) = (x, g); a = 0.75; restarted = 0
//            window k > 0:  osc = 4 n_up <= 3 k (integers);  stall = reduced == 0 and loss_check >= loss_best
//                           r = osc or stall;  reduced = r;  loss_check = loss_best;  n_up = 0
//                           if r: eta = 0.5 eta; (src, gs) = (x_best, sign * g_best); restarted = 1
//                                 (the best point as it is now: this launch's own x and dx if it just improved)
//   update:  linf: z = C(B(src + eta * sgn(gs)))          sgn: torch.sign, a NaN stays a NaN (input_grad's step form)
//                  x_new = C(B((src + a * (z - src)) + (1 - a) * (src - x_old)))
//                  B(t) = min(max(t, x0 - eps), x0 + eps),  C = clamp_nan_passes(., lo, hi)
//            l2:   z = P(src + (eta / max(|gs|, PGD_L2_TINY)) * gs)
//                  x_new = P((src + a * (z - src)) + (1 - a) * (src - x_old))
//                  P(t) = C(x0 + d * min(1, eps / max(|d|, PGD_L2_TINY))),  d = t - x0
//            x_old = src;  x = x_new;  iters += 1      (first: the (1 - a) term is dropped, x_old is not read)
//
// This is the authors' algorithm (initial step 2 eps, rho = 0.75, momentum 0.75).  ONE DELIBERATE DIFFERENCE: the
// first comparison of the first window (L > loss_prev at iteration 1) is against the start point's loss.  The
// authors' code compares against a zero-initialised slot it reaches through a wrapped index (loss_steps[-1]).
//
// Every decision is a comparison of input floats or of integers: a NaN loss never becomes the best and never counts
// as an increase (every comparison with it is false).  A NaN in an image's gradient reaches that image's x only
// (linf: its own elements; l2: the norm, hence the whole row).  A zero gradient with l2 gives a step of eta / TINY
// times zero: z = P(src).
//
// SUMS (l2): pgd_l2_step's fixed tree, three times, each with its own LDS words.  Every operation is rounded on its
// own (contraction off), no atomics, nothing depends on the grid, the stream or the launch count: the same operands
// give the same bits.  `norm` is a template parameter: the linf form has no LDS and no sum.
//
// STATE: the per-image scalars are two 16-byte records (kernels.h); every thread loads them, thread 0 stores them.
// The __syncthreads between the loads and anything thread 0 stores keeps a wave that starts late from reading the
// new record.  Row elements are read and written by their owner only, and read before they are written, so x_old,
// x_best and g_best need no ordering.  The grid is exactly M workgroups: rows and records past M are untouched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   apgd_step_kernel<false> (linf): VGPRs 32, SGPRs 46, LDS  0 B, scratch 0, occupancy 8 waves / SIMD
//   apgd_step_kernel<true>  (l2):   VGPRs 42, SGPRs 48, LDS 48 B, scratch 0, occupancy 8 waves / SIMD
// The best point is picked by a register select between the float4 just loaded and the one read from x_best: there
// is no register array here, and the select did not spill.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
__device__ __forceinline__ float ap_sgn(float s) { return s > 0.0f ? 1.0f : s < 0.0f ? -1.0f : s == s ? 0.0f : s; }

// (src + a (z - src)) + b (src - x_old); the second term only with `mom`
__device__ __forceinline__ float ap_mix(float src, float z, float xo, float a, float b, bool mom) {
#pragma clang fp contract(off)
  float t = src + a * (z - src);
  if (mom) t = t + b * (src - xo);
  return t;
}
__device__ __forceinline__ float4 ap_mix4(const float4& s, const float4& z, const float4& o, float a, float b, bool mom) {
  return float4{ap_mix(s.x, z.x, o.x, a, b, mom), ap_mix(s.y, z.y, o.y, a, b, mom), ap_mix(s.z, z.z, o.z, a, b, mom),
                ap_mix(s.w, z.w, o.w, a, b, mom)};
}
__device__ __forceinline__ float ap_box(float t, float c, float eps, float lo, float hi) {
#pragma clang fp contract(off)
  const float el = c - eps, eh = c + eps;                  // rounded to fp32 first, as the torch formula does
  return clamp_nan_passes(clamp_nan_passes(t, el, eh), lo, hi);
}
__device__ __forceinline__ float4 ap_box4(const float4& t, const float4& c, float eps, float lo, float hi) {
  return float4{ap_box(t.x, c.x, eps, lo, hi), ap_box(t.y, c.y, eps, lo, hi), ap_box(t.z, c.z, eps, lo, hi),
                ap_box(t.w, c.w, eps, lo, hi)};
}
__device__ __forceinline__ float ap_step1(float s, float r, float g) {
#pragma clang fp contract(off)
  const float t = r * g;
  return s + t;
}
// P(t) of the header; `part`: this sum's own ROW_WAVES words
__device__ __forceinline__ float4 ap_project(const float4& t, const float4& c, float eps, float lo, float hi, bool own,
                                             float* part, int wave, int lane) {
#pragma clang fp contract(off)
  float4 d{t.x - c.x, t.y - c.y, t.z - c.z, t.w - c.w};
  if (!own) d = float4{0.0f, 0.0f, 0.0f, 0.0f};
  const float m = sqrtf(row_block_sum(row_sq4(d), part, wave, lane));
  float sc = eps / (m < PGD_L2_TINY ? PGD_L2_TINY : m);
  sc = sc > 1.0f ? 1.0f : sc;
  float4 o;
  o.x = clamp_nan_passes(c.x + d.x * sc, lo, hi);
  o.y = clamp_nan_passes(c.y + d.y * sc, lo, hi);
  o.z = clamp_nan_passes(c.z + d.z * sc, lo, hi);
  o.w = clamp_nan_passes(c.w + d.w * sc, lo, hi);
  return o;
}
}  // namespace

template <bool L2>
__global__ __launch_bounds__(ROW_THREADS) void apgd_step_kernel(ApgdStepArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[L2 ? 3 : 1][ROW_WAVES];            // (linf: not used, the compiler drops it)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + (own ? tid : 0);       // (idle threads: a valid address)
  RW_ENTRY();
  const float L = a.sign * a.loss_rows[i];
  const float4 dx = reinterpret_cast<const float4*>(a.dx)[at];
  const float4 x = reinterpret_cast<const float4*>(a.x)[at];
  const float4 c = reinterpret_cast<const float4*>(a.x0)[at];

  float eta, loss_best, loss_prev, loss_check;
  int n_up, reduced, iters, restarted = 0;
  bool improved;
  if (a.first) {
    eta = 2.0f * a.eps;
    loss_best = loss_prev = loss_check = L;
    n_up = 0; reduced = 1; iters = 0;
    improved = true;                                       // x_best = x, g_best = dx
  } else {
    const float4 f = reinterpret_cast<const float4*>(a.fstate)[i];
    const int4 n = reinterpret_cast<const int4*>(a.istate)[i];
    __syncthreads();                                       // every wave holds the old records before thread 0 stores
    eta = f.x; loss_best = f.y; loss_prev = f.z; loss_check = f.w;
    n_up = n.x; reduced = n.y; iters = n.z; restarted = n.w;
    if (L > loss_prev) n_up += 1;
    loss_prev = L;
    improved = L > loss_best;
    if (improved) loss_best = L;
  }
  if (improved && own) {
    reinterpret_cast<float4*>(a.x_best)[at] = x;
    reinterpret_cast<float4*>(a.g_best)[at] = dx;
  }
  if (a.last && !a.first) {
    if (tid == 0) {
      reinterpret_cast<float4*>(a.fstate)[i] = float4{eta, loss_best, loss_prev, loss_check};
      reinterpret_cast<int4*>(a.istate)[i] = int4{n_up, reduced, iters, restarted};
    }
    return;
  }

  bool restart = false;
  if (!a.first) {
    restarted = 0;
    if (a.window > 0) {
      const bool osc = 4 * n_up <= 3 * a.window;
      const bool stall = reduced == 0 && loss_check >= loss_best;
      restart = osc || stall;
      reduced = restart ? 1 : 0;
      loss_check = loss_best;
      n_up = 0;
      if (restart) { eta = 0.5f * eta; restarted = 1; }
    }
  }
  float4 src = x, gb = dx;
  if (restart && !improved) {                              // (workgroup-uniform: the best point of an earlier launch)
    src = reinterpret_cast<const float4*>(a.x_best)[at];
    gb = reinterpret_cast<const float4*>(a.g_best)[at];
  }
  const float4 gs{a.sign * gb.x, a.sign * gb.y, a.sign * gb.z, a.sign * gb.w};
  const bool mom = !a.first;
  const float am = mom ? 0.75f : 1.0f, bm = 1.0f - am;
  float4 xo = src;
  if (mom) xo = reinterpret_cast<const float4*>(a.x_old)[at];

  float4 xn;
  if constexpr (L2) {
    float4 gz = gs;
    if (!own) gz = float4{0.0f, 0.0f, 0.0f, 0.0f};
    const float n = sqrtf(row_block_sum(row_sq4(gz), part[0], wave, lane));
    const float r = eta / (n < PGD_L2_TINY ? PGD_L2_TINY : n);
    const float4 t{ap_step1(src.x, r, gs.x), ap_step1(src.y, r, gs.y), ap_step1(src.z, r, gs.z),
                   ap_step1(src.w, r, gs.w)};
    const float4 z = ap_project(t, c, a.eps, a.lo, a.hi, own, part[1], wave, lane);
    xn = ap_project(ap_mix4(src, z, xo, am, bm, mom), c, a.eps, a.lo, a.hi, own, part[2], wave, lane);
  } else {
    const float4 t{ap_step1(src.x, eta, ap_sgn(gs.x)), ap_step1(src.y, eta, ap_sgn(gs.y)),
                   ap_step1(src.z, eta, ap_sgn(gs.z)), ap_step1(src.w, eta, ap_sgn(gs.w))};
    const float4 z = ap_box4(t, c, a.eps, a.lo, a.hi);
    xn = ap_box4(ap_mix4(src, z, xo, am, bm, mom), c, a.eps, a.lo, a.hi);
  }
  if (own) {
    reinterpret_cast<float4*>(a.x_old)[at] = src;
    reinterpret_cast<float4*>(a.x)[at] = xn;
  }
  if (tid == 0) {
    reinterpret_cast<float4*>(a.fstate)[i] = float4{eta, loss_best, loss_prev, loss_check};
    reinterpret_cast<int4*>(a.istate)[i] = int4{n_up, reduced, iters + 1, restarted};
  }
}

void launch_apgd_step(const ApgdStepArgs& a, int M, bool l2, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("apgd_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.x0 || !a.x || !a.x_old || !a.x_best || !a.g_best || !a.fstate || !a.istate)
    throw std::runtime_error("apgd_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.x, a.x_old, a.x_best, a.g_best))
    throw std::runtime_error("apgd_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.fstate, a.istate))
    throw std::runtime_error("apgd_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.loss_rows)) throw std::runtime_error("apgd_step: loss_rows must be 4-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("apgd_step: eps must be >= 0");
  if (a.sign != 1.0f && a.sign != -1.0f) throw std::runtime_error("apgd_step: sign must be +1 or -1");
  if (a.window < 0) throw std::runtime_error("apgd_step: window must be >= 0");
  if (a.first && a.last) throw std::runtime_error("apgd_step: a launch is the first or the last, not both");
  if (l2)
    hipLaunchKernelGGL(apgd_step_kernel<true>, dim3(M), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(apgd_step_kernel<false>, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_apgd() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&apgd_step_kernel<true>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&apgd_step_kernel<false>));
}

}  // namespace mnist
