// What the "elementwise on rows of 784" kernels share (adv_train, attack_step, smooth, attr, deepfool and the
// step epilogue of input_grad): the row geometry, the normalising uint8 row load, the clamp that lets a NaN pass
// and the fixed-tree sums.  Each is written once here because the files' promises rest on it: "bit for bit
// inference._PIXEL_LUT[u8]", "a NaN passes the clamp", "a fixed tree, the same bits on any launch".
// Every helper is force-inlined and keeps the per-operation rounding (contraction off) of the code it replaced.
#pragma once
#include "../include/device_utils.h"
#include "../include/kernels.h"

namespace mnist {

// one workgroup of ROW_THREADS per row, thread v < ROW_VECS owns the float4 v of the row (60 threads spare)
constexpr int ROW_THREADS = 256, ROW_WAVES = ROW_THREADS / 64;
constexpr int ROW_VECS = IMG * IMG / 4;                  // 196 float4 per row
static_assert(ROW_VECS * 4 == IMG * IMG && ROW_VECS <= ROW_THREADS && ROW_WAVES == 4, "one float4 per thread");

// the float4 v of uint8 row i, normalised: normalize_u8_alu, the in-register arithmetic of trunk_fwd, bit for bit
// the table entry (inference._PIXEL_LUT[u8]).  One aligned 32-bit load: rows are 784 B, the array 4-byte aligned.
__device__ __forceinline__ float4 row_load_u8(const uint8_t* rows, int64_t i, int v) {
  const uint32_t px = reinterpret_cast<const uint32_t*>(rows + i * (IMG * IMG))[v];
  float4 c;
  c.x = normalize_u8_alu(px & 0xffu);
  c.y = normalize_u8_alu((px >> 8) & 0xffu);
  c.z = normalize_u8_alu((px >> 16) & 0xffu);
  c.w = normalize_u8_alu(px >> 24);
  return c;
}

// the float4 v of image i: uint8 rows normalised, or fp32 [M][784] rows that are already normalised (attr.hip).
// smooth_noise and deepfool_init take only row_load_u8 and read their fp32 rows in the kernel body: there the row
// index is the workgroup's and the load shares its address with the store, which the compiler sees only when both
// stand in one function (through this helper the step form of smooth_noise and the fp32 deepfool_init compiled to
// other instructions).
template <bool U8>
__device__ __forceinline__ float4 row_load(const uint8_t* x_u8, const float* x_f32, int64_t i, int v) {
  if constexpr (U8) return row_load_u8(x_u8, i, v);
  else return reinterpret_cast<const float4*>(x_f32)[i * ROW_VECS + v];
}

// min(max(t, lo), hi) written as comparisons: both are false for a NaN, so a NaN t reaches the output (as
// torch.clamp does).  fminf / fmaxf return the other operand and would swallow it.
__device__ __forceinline__ float clamp_nan_passes(float t, float lo, float hi) {
  t = t < lo ? lo : t;
  return t > hi ? hi : t;
}

// a thread's share of a row's sum of squares: (v0^2 + v1^2) + (v2^2 + v3^2)
__device__ __forceinline__ float row_sq4(const float4& v) {
#pragma clang fp contract(off)
  return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
}

// the four wave sums of a workgroup, as (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float row_waves_sum(const float* part) {
#pragma clang fp contract(off)
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// sum over the workgroup: the xor butterfly over the wave's 64 lanes, then the four wave sums through LDS;
// `part` is this sum's own ROW_WAVES words (one barrier, no reuse)
__device__ __forceinline__ float row_block_sum(float v, float* part, int wave, int lane) {
#pragma clang fp contract(off)
  v = wave_sum(v);
  if (lane == 0) part[wave] = v;
  lds_barrier();
  return row_waves_sum(part);
}

}  // namespace mnist
