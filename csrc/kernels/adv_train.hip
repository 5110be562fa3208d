// adv_init: the first launch of an adversarial training step (Madry-style PGD-AT / FGSM-RS), ahead of the
// attack loop.  Per batch row b of the step it writes
//
//   x0[b][784]   fp32  the normalised image: normalize_u8_alu, the in-register arithmetic of trunk_fwd,
//                      bit for bit the table entry (inference._PIXEL_LUT[u8])
//   x[b][784]    fp32  the attack's iterate: x0 (random start off), or
//                      min(max(x0 + (2u - 1) * eps, lo), hi),  u = (w >> 8) * 2^-24
//                      with w one Philox-4x32-10 word per element; every operation rounded on its own
//                      (contraction off; 2u and 2u - 1 are exact: u has 24 bits)
//   labels[b]    int32 the row's label
//
// ROWS: as trunk_fwd / head_train resolve them from StepState.step: r = step * stride + b; with an index
// vector the image and the label are rows idx[r] of the HBM-resident set, without one (pre-gathered epoch
// rows) they are rows r.
//
// PHILOX COUNTER LAYOUT (a domain of its own): element e = 4 v + j of row b (v = its float4, 0 .. 195)
// uses word j of
//
//   philox4x32(c0 = b * 196 + v, c1 = ADV_PHILOX_DOMAIN, c2 = step, c3 = 0; key = seed lo, seed hi)
//
// Both dropout streams (device_utils.h dropout_block) use c1 = the high half of a 16-element block index,
// which is zero for every batch the engine can run (B * 9216 / 16 < 2^32), and c2, c3 = rng_base + 2 step
// (+ 1).  ADV_PHILOX_DOMAIN is non-zero, so under one seed no counter of this kernel is ever a dropout
// counter, whatever the step and the epoch's rng_base.  The key is the run's seed, the counter holds the
// step and the element: the draw depends on nothing else (not on rng_base, so not on the epoch).
//
// One thread owns one float4 of a row (196 per row, one workgroup of 256 threads per row; the 60 spare
// threads of a workgroup leave).  16-byte stores, no atomics, no LDS; the grid is exactly B workgroups, so
// nothing past row B - 1 is written, and a thread's values depend only on (seed, step, b, v): the same
// bits on any grid, stream and launch.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
__device__ __forceinline__ float ai_start(float x0, uint32_t w, float eps, float lo, float hi) {
#pragma clang fp contract(off)
  const float u = (float)(w >> 8) * 0x1p-24f;            // [0, 1), exact
  return clamp_nan_passes(x0 + (2.0f * u - 1.0f) * eps, lo, hi);
}
}  // namespace

template <bool IDX>
__global__ __launch_bounds__(ROW_THREADS) void adv_init_kernel(AdvInitArgs a) {
  RW_ENTRY();
  const int b = blockIdx.x, v = threadIdx.x;
  const int step = a.state->step;
  const uint64_t seed = a.state->seed;
  const int64_t row = (int64_t)step * a.idx_step_stride + b;
  int64_t src = row;
  if constexpr (IDX) src = a.idx[row];
  if (v == 0) a.labels_out[b] = a.labels[src];
  if (v >= ROW_VECS) return;
  const float4 c = row_load_u8(a.data_u8, src, v);
  float4 s = c;
  if (a.random_start) {
    const u32x4 w = philox4x32((uint32_t)b * ROW_VECS + v, ADV_PHILOX_DOMAIN, (uint32_t)step, 0u, (uint32_t)seed,
                               (uint32_t)(seed >> 32));
    s.x = ai_start(c.x, w[0], a.eps, a.lo, a.hi);
    s.y = ai_start(c.y, w[1], a.eps, a.lo, a.hi);
    s.z = ai_start(c.z, w[2], a.eps, a.lo, a.hi);
    s.w = ai_start(c.w, w[3], a.eps, a.lo, a.hi);
  }
  const int64_t v4 = (int64_t)b * ROW_VECS + v;
  reinterpret_cast<float4*>(a.x0)[v4] = c;
  reinterpret_cast<float4*>(a.x)[v4] = s;
}

void launch_adv_init(const AdvInitArgs& a, int B, hipStream_t s) {
  if (B < 1 || B > ADV_INIT_MAX_B) throw std::runtime_error("adv_init: batch size out of range");
  if (!a.data_u8 || !a.labels || !a.state || !a.x0 || !a.x || !a.labels_out)
    throw std::runtime_error("adv_init: null argument");
  if (misaligned(15, a.x0, a.x)) throw std::runtime_error("adv_init: x0 and x must be 16-byte aligned");
  if (misaligned(3, a.data_u8)) throw std::runtime_error("adv_init: the image rows must be 4-byte aligned");
  if (a.x0 == a.x) throw std::runtime_error("adv_init: x must not be x0");
  if (a.random_start && !(a.eps >= 0.0f && a.lo <= a.hi))
    throw std::runtime_error("adv_init: need eps >= 0 and lo <= hi");
  if (a.idx)
    hipLaunchKernelGGL(adv_init_kernel<true>, dim3(B), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(adv_init_kernel<false>, dim3(B), dim3(ROW_THREADS), 0, s, a);
}

void preload_adv_train() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&adv_init_kernel<true>));
}

}  // namespace mnist
