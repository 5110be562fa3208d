// EAD, the elastic-net attack of Chen, Sharma, Zhang, Yi & Hsieh (AAAI 2018), on the normalised image, fp32 [M][784]:
// the whole per-image update of one iteration in one launch - the success test and the best point at the shrunk point
// x, the ISTA step with FISTA momentum from the slack point y, and the bisection of the trade-off constant c at the
// end of a search step.  It minimises c * hinge(margin) + |delta|_2^2 + beta |delta|_1 in pixel units; the L1 term is
// never differentiated: it is the shrinkage-thresholding around the clean image.
//
// One workgroup of ROW_THREADS per image, thread t < 196 owns the float4 t of each of the image's rows.  The gradient
// chain ran over 2 M rows with the CW margin: rows [0, M) the slack points y, rows [M, 2 M) the shrunk points x, so
//   L_y = sign * loss_rows[i]       g = dx[i] (input_grad's plain output at the y row)
//   L_x = sign * loss_rows[M + i]   (sign = -1: targeted, labels are the classes to reach)
// D1 = sum |x - x0|, D2 = sum (x - x0)^2 on the fixed tree, from the stored row x: the exact bits the chain saw.
//   dist = RULE_L1 ? std D1 : dist_scale D2 + beta (std D1)               (pixel units; std = MNIST_STD)
//
//   first:        c = c_init; c_lo = 0; c_hi = CW_C_INF; d_best = +inf; succ = found_search = iters = 0
//                 x_best = x0                       (reads no state; the caller has set x = y = x0 exactly)
//   evaluate:     ok = (L_x > 0) and (L_x >= kappa)                      -- a NaN margin is never a success
//                 if ok: succ = 1;  if dist < d_best: d_best = dist; x_best = x; found_search = search + 1
//   last:         store the records and stop (x, y keep their values; no gradient is loaded)
//   search_end:   cw_step's bisection of c on succ; succ = 0; x = y = x0 exactly (no gradient is loaded)
//   otherwise:    act = (L_y < kappa) ? 1 : 0
//                 z  = y - (lr_k / dist_scale) ((2 dist_scale) (y - x0) - (sign c act) g)
//                 d  = z - x0
//                 x+ = d > beta_n ? min(z - beta_n, hi) : (d < -beta_n ? max(z + beta_n, lo) : x0)
//                 y+ = x+ + zeta_k (x+ - x);  iters += 1                 -- y is not clamped (as in the authors' code)
//
// lr_k = lr sqrt(1 - k / steps) and zeta_k = k / (k + 3) of the update index k inside the search step come from the
// host (float64, rounded once), beta_n = beta / MNIST_STD too.  The threshold is beta, not lr beta: the authors' code.
// dist_scale = MNIST_STD^2 turns the pixel-unit step lr_k into normalised units and weighs the L2 term as c sees it.
//
// Every decision is a comparison of input floats or of integers.  A NaN margin L_x is never a success; a NaN L_y
// gives act = 0: the hinge is off (times 0 * g: a NaN g still passes into z).  A NaN z compares false both ways, so
// that element of x+ is the clean pixel; nothing of it reaches another element or another image.
//
// SUMS: two, D1 and D2, on pgd_l2_step's fixed tree (row_ops.h: the thread's four, the xor butterfly, the four wave
// sums), each with its own LDS words, behind one barrier; RULE_L1 forms D1 only.  Every operation is rounded on its
// own (contraction off, no packed fp32), the division is the correctly rounded one, no atomics, nothing depends on the
// grid, the stream or the launch count: the same operands give the same bits.
//
// STATE: the per-image scalars are cw_step's two 16-byte records (kernels.h); every thread loads them, thread 0
// stores them.  The __syncthreads between the loads and anything thread 0 stores keeps a wave that starts late from
// reading the new record.  Row elements are read and written by their owner only, and read before they are written.
// The grid is exactly M workgroups: rows and records past M are untouched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   ead_step_kernel<EN>: VGPRs 31, SGPRs 64, LDS 32 B, scratch 0, occupancy 8 waves / SIMD
//   ead_step_kernel<L1>: VGPRs 31, SGPRs 62, LDS 16 B, scratch 0, occupancy 8 waves / SIMD
// There is no register array: the best point is one conditional store of the float4 just loaded.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
// a thread's share of a row's sum of magnitudes: (|v0| + |v1|) + (|v2| + |v3|)
__device__ __forceinline__ float row_abs4(const float4& v) {
#pragma clang fp contract(off)
  return (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
}

struct EadScalars {
  float k2, s, lrs, bn, nbn, zeta, lo, hi;
};

// one element's ISTA step from the slack point y: the new shrunk point in xn, the new slack point returned
__device__ __forceinline__ float ead_ista(float& xn, float y, float x, float c, float g, const EadScalars& k) {
#pragma clang fp contract(off)
  const float gx = k.k2 * (y - c) - k.s * g;
  const float z = y - k.lrs * gx;
  const float d = z - c;
  const float up = z - k.bn, dn = z + k.bn;
  xn = d > k.bn ? (up > k.hi ? k.hi : up) : (d < k.nbn ? (dn < k.lo ? k.lo : dn) : c);
  return xn + k.zeta * (xn - x);
}
}  // namespace

template <int RULE>
__global__ __launch_bounds__(ROW_THREADS) void ead_step_kernel(EadStepArgs a, int M) {
#pragma clang fp contract(off)
  __shared__ float part1[ROW_WAVES];
  __shared__ float part2[RULE == EAD_RULE_EN ? ROW_WAVES : 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + (own ? tid : 0);       // (idle threads: a valid address)
  RW_ENTRY();
  const float Lx = a.sign * a.loss_rows[M + i];
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

  // evaluate: the shrunk point the chain just saw.  Both sums go through LDS behind one barrier.
  float4 d{x.x - c0.x, x.y - c0.y, x.z - c0.z, x.w - c0.w};
  if (!own) d = float4{0.0f, 0.0f, 0.0f, 0.0f};
  const float w1 = wave_sum(row_abs4(d));
  float w2 = 0.0f;
  if constexpr (RULE == EAD_RULE_EN) w2 = wave_sum(row_sq4(d));
  if (lane == 0) {
    part1[wave] = w1;
    if constexpr (RULE == EAD_RULE_EN) part2[wave] = w2;
  }
  lds_barrier();
  const float l1p = a.std * row_waves_sum(part1);
  float dist = l1p;
  if constexpr (RULE == EAD_RULE_EN) dist = a.dist_scale * row_waves_sum(part2) + a.beta * l1p;
  const bool ok = Lx > 0.0f && Lx >= a.kappa;
  const bool improved = ok && dist < d_best;
  if (ok) succ = 1;
  if (improved) { d_best = dist; found = a.search + 1; }
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

  if (a.search_end) {                                      // bisect c, back to the clean image
    if (succ) {
      c_hi = c < c_hi ? c : c_hi;
      if (c_hi < CW_C_BIG) c = (c_lo + c_hi) * 0.5f;
    } else {
      c_lo = c > c_lo ? c : c_lo;
      c = c_hi < CW_C_BIG ? (c_lo + c_hi) * 0.5f : c * 10.0f;
    }
    if (own) {
      reinterpret_cast<float4*>(a.x)[at] = c0;
      reinterpret_cast<float4*>(a.y)[at] = c0;
    }
    if (tid == 0) {
      reinterpret_cast<float4*>(a.fstate)[i] = float4{c, c_lo, c_hi, d_best};
      reinterpret_cast<int4*>(a.istate)[i] = int4{0, found, iters, spare};
    }
    return;
  }

  // the ISTA step from the slack point, then the momentum
  const float Ly = a.sign * a.loss_rows[i];
  const float4 g = reinterpret_cast<const float4*>(a.dx)[at];
  const float4 y = reinterpret_cast<const float4*>(a.y)[at];
  const float act = Ly < a.kappa ? 1.0f : 0.0f;
  EadScalars k;
  k.k2 = 2.0f * a.dist_scale;
  k.s = (a.sign * c) * act;
  k.lrs = a.lr_k / a.dist_scale;
  k.bn = a.beta_n; k.nbn = -a.beta_n;
  k.zeta = a.zeta_k;
  k.lo = a.lo; k.hi = a.hi;
  float4 xn, yn;
  yn.x = ead_ista(xn.x, y.x, x.x, c0.x, g.x, k);
  yn.y = ead_ista(xn.y, y.y, x.y, c0.y, g.y, k);
  yn.z = ead_ista(xn.z, y.z, x.z, c0.z, g.z, k);
  yn.w = ead_ista(xn.w, y.w, x.w, c0.w, g.w, k);
  if (own) {
    reinterpret_cast<float4*>(a.x)[at] = xn;
    reinterpret_cast<float4*>(a.y)[at] = yn;
  }
  if (tid == 0) {
    reinterpret_cast<float4*>(a.fstate)[i] = float4{c, c_lo, c_hi, d_best};
    reinterpret_cast<int4*>(a.istate)[i] = int4{succ, found, iters + 1, spare};
  }
}

void launch_ead_step(const EadStepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B / 2) throw std::runtime_error("ead_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.x0 || !a.y || !a.x || !a.x_best || !a.fstate || !a.istate)
    throw std::runtime_error("ead_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.y, a.x, a.x_best))
    throw std::runtime_error("ead_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.fstate, a.istate))
    throw std::runtime_error("ead_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.loss_rows)) throw std::runtime_error("ead_step: loss_rows must be 4-byte aligned");
  if (a.sign != 1.0f && a.sign != -1.0f) throw std::runtime_error("ead_step: sign must be +1 or -1");
  if (!(a.kappa >= 0.0f)) throw std::runtime_error("ead_step: kappa must be >= 0");
  if (!(a.lr_k >= 0.0f) || !(a.zeta_k >= 0.0f && a.zeta_k < 1.0f))
    throw std::runtime_error("ead_step: need lr_k >= 0 and zeta_k in [0, 1)");
  if (a.first && !(a.c_init > 0.0f)) throw std::runtime_error("ead_step: c_init must be > 0");
  if (!(a.beta >= 0.0f && a.beta_n >= 0.0f)) throw std::runtime_error("ead_step: beta and beta_n must be >= 0");
  if (!(a.dist_scale > 0.0f) || !(a.std > 0.0f) || !(a.lo < a.hi))
    throw std::runtime_error("ead_step: need dist_scale > 0, std > 0 and lo < hi");
  if (a.search < 0) throw std::runtime_error("ead_step: the search index must be >= 0");
  if (a.first && a.last) throw std::runtime_error("ead_step: a launch is the first or the last, not both");
  if (a.rule == EAD_RULE_EN)
    hipLaunchKernelGGL(ead_step_kernel<EAD_RULE_EN>, dim3(M), dim3(ROW_THREADS), 0, s, a, M);
  else if (a.rule == EAD_RULE_L1)
    hipLaunchKernelGGL(ead_step_kernel<EAD_RULE_L1>, dim3(M), dim3(ROW_THREADS), 0, s, a, M);
  else
    throw std::runtime_error("ead_step: the decision rule must be EAD_RULE_EN or EAD_RULE_L1");
}

void preload_ead() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&ead_step_kernel<EAD_RULE_EN>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&ead_step_kernel<EAD_RULE_L1>));
}

}  // namespace mnist
