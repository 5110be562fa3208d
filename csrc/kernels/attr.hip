// Attribution (integrated gradients, Sundararajan et al. 2017; SmoothGrad, Smilkov et al. 2017): the producer of
// the rows of the integration path and the per-image reduction of the gradient rows.
//
// attr_path: out[r][784] fp32, r = i * ns + s for image i < M and sample s < ns,
//
//   alpha = (float(sample_base + s) + 0.5f) / float(n_total)          the midpoint rule, IEEE division
//   out   = b_i + alpha * (x_i - b_i)
//
// x_i the normalised image: uint8 rows through normalize_u8_alu (bit for bit inference._PIXEL_LUT[u8]) or fp32
// [M][784] rows; b_i the baseline: fp32 [M][784] rows, or the scalar base_value when the pointer is null.  The
// subtract, the multiply and the add are each rounded on their own (contraction off): numpy's float32 arithmetic
// gives the same bits.  One thread owns one float4 of a row (196 per row, one workgroup of 256 threads per row; the
// 60 spare threads leave).  16-byte stores, no LDS, no atomics; the grid is exactly M * ns workgroups, so nothing
// past the last row is written, and a row depends on (x_i, b_i, sample_base + s, n_total) alone: the same bits
// under any chunking of the samples.
//
// attr_reduce: acc[i][e] (+)= sum over s < ns of dx[i * ns + s][e], the adds in ascending s, in fp32, starting from
// the stored acc[i][e] (accumulate) or from 0.  That serial order is the contract: the sum of an image's n rows is
// the same bits whether they arrive in one launch or in several accumulating ones, and equals a numpy loop of
// float32 adds.  finish stores, after the last add and instead of the running sum,
//
//   ATTR_FINISH_SCALE:  out = acc * scale                              (SmoothGrad: scale = -1 / n)
//   ATTR_FINISH_PATH:   out = (acc * scale) * (x_i - b_i)              (integrated gradients)
//
// x_i and b_i read as attr_path reads them, each multiply and the subtract rounded on its own.  out may alias acc
// (a thread reads its element of acc before it writes that element of out, and no other thread touches it).
// Parallel over (image, float4 column) only: item = i * 196 + v, one item per thread, workgroups of one wave, so
// one image alone is spread over four workgroups; the grid is ceil(M * 196 / 64) and items past M * 196 leave, so
// rows of acc / out past M are untouched.  A thread issues the loads of AR_AHEAD rows before the dependent adds
// (the rows of one column are 3136 B apart: AR_AHEAD independent 16-byte loads in flight per thread).  An element
// of the result depends on that element of the image's rows alone: a NaN reaches only its own element.  No LDS,
// no atomics, no cross-lane operation.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
constexpr int AR_THREADS = 64;
constexpr int AR_AHEAD = 8;                              // rows whose loads are in flight before the adds

// the float4 v of image i's baseline (the image itself: row_load)
__device__ __forceinline__ float4 at_base(const float* base, float base_value, int64_t i, int v) {
  if (base) return reinterpret_cast<const float4*>(base)[i * ROW_VECS + v];
  return make_float4(base_value, base_value, base_value, base_value);
}
__device__ __forceinline__ float at_point(float x, float b, float alpha) {
#pragma clang fp contract(off)
  const float d = x - b;
  const float m = alpha * d;
  return b + m;
}
__device__ __forceinline__ float at_finish(float acc, float scale, float x, float b, bool path) {
#pragma clang fp contract(off)
  const float t = acc * scale;
  if (!path) return t;
  const float d = x - b;
  return t * d;
}
}  // namespace

template <bool U8>
__global__ __launch_bounds__(ROW_THREADS) void attr_path_kernel(AttrPathArgs a) {
  RW_ENTRY();
  const int v = threadIdx.x;
  if (v >= ROW_VECS) return;
  const int64_t r = blockIdx.x;
  const int64_t i = (uint32_t)blockIdx.x / (uint32_t)a.ns;     // rows <= SMOOTH_MAX_ROWS: 32-bit division
  const int s = (int)(r - i * a.ns);
  float alpha;
  {
#pragma clang fp contract(off)
    alpha = ((float)(a.sample_base + s) + 0.5f) / (float)a.n_total;
  }
  const float4 x = row_load<U8>(a.x_u8, a.x_f32, i, v);
  const float4 b = at_base(a.base, a.base_value, i, v);
  float4 o;
  o.x = at_point(x.x, b.x, alpha);
  o.y = at_point(x.y, b.y, alpha);
  o.z = at_point(x.z, b.z, alpha);
  o.w = at_point(x.w, b.w, alpha);
  reinterpret_cast<float4*>(a.out)[r * ROW_VECS + v] = o;
}

// SRC 0: no image is read (finish none / scale); 1: uint8 rows; 2: fp32 rows (ATTR_FINISH_PATH)
template <int SRC>
__global__ __launch_bounds__(AR_THREADS) void attr_reduce_kernel(AttrReduceArgs a, int M) {
  RW_ENTRY();
  const int64_t item = (int64_t)blockIdx.x * AR_THREADS + threadIdx.x;
  if (item >= (int64_t)M * ROW_VECS) return;
  const int64_t i = (uint32_t)item / (uint32_t)ROW_VECS;        // items <= 196 * SMOOTH_MAX_ROWS < 2^32
  const int v = (int)(item - i * ROW_VECS);
  float4* accp = reinterpret_cast<float4*>(a.acc) + item;
  float4 t = a.accumulate ? *accp : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4* row = reinterpret_cast<const float4*>(a.dx) + i * a.ns * ROW_VECS + v;
  int s = 0;
  for (; s + AR_AHEAD <= a.ns; s += AR_AHEAD) {
    float4 g[AR_AHEAD];
#pragma unroll
    for (int k = 0; k < AR_AHEAD; ++k) g[k] = row[(int64_t)(s + k) * ROW_VECS];
#pragma unroll
    for (int k = 0; k < AR_AHEAD; ++k) { t.x += g[k].x; t.y += g[k].y; t.z += g[k].z; t.w += g[k].w; }
  }
  for (; s < a.ns; ++s) {
    const float4 g = row[(int64_t)s * ROW_VECS];
    t.x += g.x; t.y += g.y; t.z += g.z; t.w += g.w;
  }
  if (a.finish == ATTR_FINISH_NONE) {
    *accp = t;
    return;
  }
  float4 x = t, b = t;                                         // (unused by ATTR_FINISH_SCALE)
  if constexpr (SRC != 0) {
    x = row_load<SRC == 1>(a.x_u8, a.x_f32, i, v);
    b = at_base(a.base, a.base_value, i, v);
  }
  constexpr bool path = SRC != 0;
  float4 o;
  o.x = at_finish(t.x, a.scale, x.x, b.x, path);
  o.y = at_finish(t.y, a.scale, x.y, b.y, path);
  o.z = at_finish(t.z, a.scale, x.z, b.z, path);
  o.w = at_finish(t.w, a.scale, x.w, b.w, path);
  reinterpret_cast<float4*>(a.out)[item] = o;
}

void launch_attr_path(const AttrPathArgs& a, int M, hipStream_t s) {
  if (!a.out) throw std::runtime_error("attr_path: null argument");
  if (M < 1 || a.ns < 1 || (int64_t)M * a.ns > SMOOTH_MAX_ROWS) throw std::runtime_error("attr_path: M * ns out of range");
  check_row_source("attr_path", a.x_u8, a.x_f32, a.base);
  if (misaligned(15, a.out)) throw std::runtime_error("attr_path: out must be 16-byte aligned");
  if (a.n_total < 1 || a.n_total > ATTR_MAX_STEPS || a.sample_base < 0 || (int64_t)a.sample_base + a.ns > a.n_total)
    throw std::runtime_error("attr_path: need 0 <= sample_base, sample_base + ns <= n_total <= ATTR_MAX_STEPS");
  const unsigned rows = (unsigned)((int64_t)M * a.ns);
  if (a.x_u8)
    hipLaunchKernelGGL(attr_path_kernel<true>, dim3(rows), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(attr_path_kernel<false>, dim3(rows), dim3(ROW_THREADS), 0, s, a);
}

void launch_attr_reduce(const AttrReduceArgs& a, int M, hipStream_t s) {
  if (!a.dx || !a.acc) throw std::runtime_error("attr_reduce: null argument");
  if (M < 1 || a.ns < 1 || (int64_t)M * a.ns > SMOOTH_MAX_ROWS) throw std::runtime_error("attr_reduce: M * ns out of range");
  if (a.finish != ATTR_FINISH_NONE && a.finish != ATTR_FINISH_SCALE && a.finish != ATTR_FINISH_PATH)
    throw std::runtime_error("attr_reduce: unknown finish form");
  if (a.finish != ATTR_FINISH_NONE && !a.out) throw std::runtime_error("attr_reduce: null argument (finish needs out)");
  if (misaligned(15, a.dx, a.acc, a.out))
    throw std::runtime_error("attr_reduce: dx, acc and out must be 16-byte aligned");
  const unsigned grid = (unsigned)(((int64_t)M * ROW_VECS + AR_THREADS - 1) / AR_THREADS);
  if (a.finish == ATTR_FINISH_PATH) {
    check_row_source("attr_reduce", a.x_u8, a.x_f32, a.base);
    if (a.x_u8)
      hipLaunchKernelGGL(attr_reduce_kernel<1>, dim3(grid), dim3(AR_THREADS), 0, s, a, M);
    else
      hipLaunchKernelGGL(attr_reduce_kernel<2>, dim3(grid), dim3(AR_THREADS), 0, s, a, M);
  } else {
    hipLaunchKernelGGL(attr_reduce_kernel<0>, dim3(grid), dim3(AR_THREADS), 0, s, a, M);
  }
}

void preload_attr() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&attr_path_kernel<true>));
}

}  // namespace mnist
