// Minimum-norm adversarial examples: the L2 DeepFool step (Moosavi-Dezfooli, Fawzi, Frossard 2016) on the
// normalised image, fp32.
//
// Image i of a chunk of M owns the ten rows 10 i + c, c = 0 .. 9, of the row buffer [10 M][784] (the xin of
// trunk_fwd; row c is labelled c) and of the gradient buffer dx (input_grad's plain output).  After the gradient
// chain, dx[10 i + c] = g_c = d NLL_c / d x and loss_rows[10 i + c] = -log p_c: every class gradient and every logit
// difference of the image.  One workgroup of 256 threads per image; thread t < 196 owns the float4 t of each row.
//
// deepfool_init: the ten rows and x[i] = x0_i (uint8 rows through normalize_u8_alu, bit for bit
// inference._PIXEL_LUT[u8], or fp32 rows), r_tot[i] = 0, status[i] = iters[i] = 0, norm[i] = 0; x0_out[i] = x0_i
// when given (required with uint8 rows: the step reads it).
//
// deepfool_step, with y = y[i] the class being left:
//   1. status[i] != 0: the workgroup stores nothing (frozen).
//   2. f_k = loss_y - loss_k (= log p_k - log p_y), k != y.
//   3. crossed: some loss_k < loss_y, or loss_k == loss_y with k < y (head_eval: the first maximum wins):
//      status[i] = DF_CROSSED, nothing else is stored.
//   4. w_k = g_y - g_k per element, n2_k = sum w_k^2: nine sums, one barrier (36 LDS words).
//   5. ratio_k = (|f_k| + DF_SLACK) / sqrt(n2_k).  A class with sqrt(n2_k) < PGD_L2_TINY or a NaN ratio is skipped;
//      l = the smallest ratio in ascending k under a strict <: the first of equal ratios wins.
//      No class left: if some ratio was a NaN (a NaN in g_y makes every one of them a NaN), l = the first such k,
//      and its NaN scale below fills the image's r_tot, x, rows and norm - the NaN is seen, not swallowed; no
//      other image reads it.  Otherwise status[i] = DF_STUCK, nothing else is stored.  (A NaN row beside a
//      selectable class is skipped and changes nothing.)  y outside [0, 10): DF_STUCK.
//   6. r_tot += ((|f_l| + DF_SLACK) / n2_l) * w_l
//   7. x_next = min(max(x0 + (1 + overshoot) * r_tot, lo), hi), the clamps comparisons that let a NaN pass
//   8. x[i] and the ten rows = x_next
//   9. norm[i] = sqrt(sum (x_next - x0)^2): a tenth sum after a second barrier
//  10. iters[i] += 1
//
// SUMS: pgd_l2_step's fixed tree.  Per thread (v0^2 + v1^2) + (v2^2 + v3^2), threads 196 .. 255 add zeros; the xor
// butterfly over the wave's 64 lanes (wave_sum); the four wave sums through LDS as (w0 + w1) + (w2 + w3).  Every
// operation is rounded on its own (contraction off), no atomics, nothing depends on the grid, the stream or the
// launch count: the same operands give the same bits.  Every early exit is taken by the whole workgroup (the
// decision is a function of status, y, loss_rows and the LDS sums, which every thread reads alike), so no thread
// waits at a barrier others have left.  A thread reads its r_tot element before it stores it and is the only one
// that touches it; dx, loss_rows, y and x0 are only read.  The grid is exactly M workgroups: nothing past M is
// touched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   deepfool_step_kernel:        VGPRs 38, SGPRs 62, LDS 160 B, scratch 0, occupancy 8 waves / SIMD
//   deepfool_init_kernel<true>:  VGPRs 30, SGPRs 23, LDS   0 B, scratch 0, occupancy 8
//   deepfool_init_kernel<false>: VGPRs 12, SGPRs 20, LDS   0 B, scratch 0, occupancy 8
// A first form held the ten gradient float4s and the ten losses in arrays and picked g_y and g_l by unrolled
// selects: the compiler turned the selects back into a dynamic index and the arrays into 208 B of scratch per lane
// (45 VGPRs).  So g_y, loss_y and the chosen row are read by address instead - the rows were read a moment before,
// these are cache hits - and every index into registers is a loop counter of an unrolled loop: no scratch.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
constexpr int DF_OTHERS = DF_CLASSES - 1;                // the classes k != y; class k owns the LDS words j = k - (k > y)

__device__ __forceinline__ float4 df_sub4(const float4& a, const float4& b) {
#pragma clang fp contract(off)
  return float4{a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
}
__device__ __forceinline__ float df_next(float c, float os1, float r, float lo, float hi) {
#pragma clang fp contract(off)
  const float t = os1 * r;
  return clamp_nan_passes(c + t, lo, hi);
}
__device__ __forceinline__ float df_acc(float r, float sc, float w) {
#pragma clang fp contract(off)
  const float t = sc * w;
  return r + t;
}
}  // namespace

template <bool U8>
__global__ __launch_bounds__(ROW_THREADS) void deepfool_init_kernel(DeepfoolInitArgs a) {
  RW_ENTRY();
  const int v = threadIdx.x;
  const int64_t i = blockIdx.x;
  if (v == 0) {
    a.status[i] = DF_RUNNING;
    a.iters[i] = 0;
    a.norm[i] = 0.0f;
  }
  if (v >= ROW_VECS) return;
  float4 c;                                              // (fp32 rows: read here, not through row_load - row_ops.h)
  if constexpr (U8) c = row_load_u8(a.x_u8, i, v);
  else c = reinterpret_cast<const float4*>(a.x_f32)[i * ROW_VECS + v];
  const int64_t at = i * ROW_VECS + v;
  reinterpret_cast<float4*>(a.x)[at] = c;
  if (a.x0_out) reinterpret_cast<float4*>(a.x0_out)[at] = c;
  reinterpret_cast<float4*>(a.r_tot)[at] = float4{0.0f, 0.0f, 0.0f, 0.0f};
  float4* row = reinterpret_cast<float4*>(a.rows) + i * (DF_CLASSES * ROW_VECS) + v;
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) row[k * ROW_VECS] = c;
}

__global__ __launch_bounds__(ROW_THREADS) void deepfool_step_kernel(DeepfoolStepArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[DF_OTHERS + 1][ROW_WAVES];        // the nine class sums (36 words), then the norm's
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  RW_ENTRY();
  if (a.status[i] != DF_RUNNING) return;                 // 1. frozen
  const int y = a.y[i];
  if (y < 0 || y >= DF_CLASSES) {
    if (tid == 0) a.status[i] = DF_STUCK;
    return;
  }
  const float* lrow = a.loss_rows + i * DF_CLASSES;
  const float ly = lrow[y];
  float loss[DF_CLASSES];
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) loss[k] = lrow[k];
  bool crossed = false;                                  // 3.
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) crossed = crossed || (k != y && (loss[k] < ly || (loss[k] == ly && k < y)));
  if (crossed) {
    if (tid == 0) a.status[i] = DF_CROSSED;
    return;
  }

  const int64_t at = i * ROW_VECS + (own ? tid : 0);      // (idle threads: a valid address)
  const float4* grow = reinterpret_cast<const float4*>(a.dx) + i * (DF_CLASSES * ROW_VECS) + (own ? tid : 0);
  const float4 gy = grow[y * ROW_VECS];                   // by address: every index into registers stays static
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) {                 // 4. class k != y owns the words j = k - (k > y)
    if (k == y) continue;
    const float4 w = df_sub4(gy, grow[k * ROW_VECS]);
    const float s = wave_sum(own ? row_sq4(w) : 0.0f);
    if (lane == 0) part[k - (k > y ? 1 : 0)][wave] = s;
  }
  lds_barrier();

  int l = -1, l_nan = -1;                                // 5. the chosen class; the first class with a NaN ratio
  float best = 0.0f, num_l = 0.0f, n2_l = 0.0f, num_nan = 0.0f, n2_nan = 0.0f;
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) {
    if (k == y) continue;
    const float f = ly - loss[k];
    const float n2 = row_waves_sum(part[k - (k > y ? 1 : 0)]);
    const float n = sqrtf(n2);
    const float num = fabsf(f) + DF_SLACK;
    const float ratio = num / n;
    if (ratio != ratio) {
      if (l_nan < 0) { l_nan = k; num_nan = num; n2_nan = n2; }
    } else if (!(n < PGD_L2_TINY) && (l < 0 || ratio < best)) {
      l = k; best = ratio; num_l = num; n2_l = n2;
    }
  }
  if (l < 0) {
    if (l_nan < 0) {
      if (tid == 0) a.status[i] = DF_STUCK;
      return;
    }
    l = l_nan; num_l = num_nan; n2_l = n2_nan;
  }
  const float4 w = df_sub4(gy, grow[l * ROW_VECS]);       // (the chosen row again: a cache hit, not a register array)
  const float sc = num_l / n2_l;                         // 6.
  float4 r = reinterpret_cast<const float4*>(a.r_tot)[at];
  const float4 c = reinterpret_cast<const float4*>(a.x0)[at];
  r.x = df_acc(r.x, sc, w.x);
  r.y = df_acc(r.y, sc, w.y);
  r.z = df_acc(r.z, sc, w.z);
  r.w = df_acc(r.w, sc, w.w);
  const float os1 = 1.0f + a.overshoot;                  // 7.
  float4 o;
  o.x = df_next(c.x, os1, r.x, a.lo, a.hi);
  o.y = df_next(c.y, os1, r.y, a.lo, a.hi);
  o.z = df_next(c.z, os1, r.z, a.lo, a.hi);
  o.w = df_next(c.w, os1, r.w, a.lo, a.hi);
  float4 d = df_sub4(o, c);
  if (own) {                                             // 8.
    reinterpret_cast<float4*>(a.r_tot)[at] = r;
    reinterpret_cast<float4*>(a.x)[at] = o;
    float4* row = reinterpret_cast<float4*>(a.rows) + i * (DF_CLASSES * ROW_VECS) + tid;
#pragma unroll
    for (int k = 0; k < DF_CLASSES; ++k) row[k * ROW_VECS] = o;
  } else {
    d = float4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const float m = wave_sum(row_sq4(d));                  // 9.
  if (lane == 0) part[DF_OTHERS][wave] = m;
  lds_barrier();
  if (tid == 0) {
    a.norm[i] = sqrtf(row_waves_sum(part[DF_OTHERS]));
    a.iters[i] = a.iters[i] + 1;                         // 10.
  }
}

void launch_deepfool_init(const DeepfoolInitArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > DF_MAX_M) throw std::runtime_error("deepfool_init: image count out of range");
  check_one_row_source("deepfool_init", a.x_u8, a.x_f32);
  if (!a.rows || !a.x || !a.r_tot || !a.status || !a.iters || !a.norm || (a.x_u8 && !a.x0_out))
    throw std::runtime_error("deepfool_init: null argument");
  if (misaligned(15, a.x_f32, a.rows, a.x, a.x0_out, a.r_tot))
    throw std::runtime_error("deepfool_init: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(3, a.x_u8, a.status, a.iters, a.norm))
    throw std::runtime_error("deepfool_init: the uint8 rows and the per-image vectors must be 4-byte aligned");
  if (a.x_u8)
    hipLaunchKernelGGL(deepfool_init_kernel<true>, dim3(M), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(deepfool_init_kernel<false>, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void launch_deepfool_step(const DeepfoolStepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > DF_MAX_M) throw std::runtime_error("deepfool_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.y || !a.x0 || !a.r_tot || !a.x || !a.rows || !a.status || !a.iters || !a.norm)
    throw std::runtime_error("deepfool_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.r_tot, a.x, a.rows))
    throw std::runtime_error("deepfool_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(3, a.loss_rows, a.y, a.status, a.iters, a.norm))
    throw std::runtime_error("deepfool_step: the per-image vectors must be 4-byte aligned");
  if (!(a.overshoot >= 0.0f)) throw std::runtime_error("deepfool_step: overshoot must be >= 0");
  hipLaunchKernelGGL(deepfool_step_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_deepfool() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&deepfool_step_kernel));
}

}  // namespace mnist
