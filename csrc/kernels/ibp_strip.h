// The strip of ibp_trunk (ibp.hip has the design), as a template over its epilogue so that crown_relax (crown.hip) is
// a second instance of the same conv1 / conv2 code: RELAX = false is ibp_trunk, the same operations in the same
// order; RELAX = true also writes, per pooled unit, the CROWN relaxation record of the ReLU-and-pool pair.
#pragma once
#include "../include/device_utils.h"
#include "../include/kernels.h"

namespace mnist {

constexpr int IBP_P = 2;                           // pooled rows a strip
constexpr int IBP_STRIPS = HP / IBP_P;             // 6
constexpr int IBP_A1_ROWS = 2 * IBP_P + 2;         // 6 conv1 rows
constexpr int IBP_A1_PIX = IBP_A1_ROWS * H1;       // 156 conv1 pixels
constexpr int IBP_X_PIX = (IBP_A1_ROWS + 2) * IMG; // 224 input pixels
constexpr int IBP_MT = 2 * IBP_P * H2 / 16;        // 6 row tiles of 16 conv2 pixels (4 pool windows each)
constexpr int IBP_KS = NFLAT / IBP_SPLITS;         // 256 fc1 inputs a split
static_assert(IBP_STRIPS * IBP_P == HP && IBP_MT * 16 == 2 * IBP_P * H2 && IBP_KS * IBP_SPLITS == NFLAT &&
              IBP_KS % 16 == 0 && IBP_X_PIX <= 256, "ibp geometry");

__device__ __forceinline__ float relu_nan_passes(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float max_nan_passes(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float min_nan_passes(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The CROWN relaxation of y = relu(z), l <= z <= u: sL z <= y <= sU z + bU.  l >= 0: the identity; u <= 0: zero;
// else the chord above and, below, the line of slope 1 (u > -l) or 0 that encloses the smaller area.
struct ReluRelax { float sL, sU, bU; };
__device__ __forceinline__ ReluRelax relu_relax(float l, float u) {
#pragma clang fp contract(off)
  if (l >= 0.0f) return {1.0f, 1.0f, 0.0f};
  if (u <= 0.0f) return {0.0f, 0.0f, 0.0f};
  const float d = u - l;
  return {u > -l ? 1.0f : 0.0f, u / d, (-l * u) / d};
}

template <bool RELAX>
__device__ __forceinline__ void ibp_strip(const IbpArgs& a, float4* relax) {
  __shared__ float4 s_mu[C1 / 4][IBP_A1_PIX];      // post-ReLU conv1 bounds, centre: [ci / 4][pixel][ci % 4]
  __shared__ float4 s_r[C1 / 4][IBP_A1_PIX];       // ... radius
  __shared__ float s_xm[IBP_X_PIX], s_xr[IBP_X_PIX];
  __shared__ float s_w1[C1 * 9], s_b1[C1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int strip = blockIdx.x;
  const int64_t img = blockIdx.y;
  RW_ENTRY();

  // this wave's conv2 weight slice, in registers for the whole kernel
  float wreg[72];
  {
    const float* w2 = a.param + OFF_CONV2_W + (16 * wave + n) * (C1 * 9) + g * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int cib = 0; cib < 8; ++cib) wreg[tap * 8 + cib] = w2[cib * 36 + tap];
  }

  // the input box of the strip's 8 rows, clipped to the pixel range, as centre and radius
  {
#pragma clang fp contract(off)
    const float eps_n = a.rec[img * 4] / a.pix_std;
    if (tid < IBP_X_PIX) {
      const float x = a.x0[img * (IMG * IMG) + strip * (2 * IBP_P * IMG) + tid];
      float l = x - eps_n, u = x + eps_n;
      l = l < a.lo ? a.lo : l;
      u = u > a.hi ? a.hi : u;
      s_xm[tid] = (l + u) * 0.5f;
      s_xr[tid] = (u - l) * 0.5f;
    }
    for (int i = tid; i < C1 * 9; i += 256) s_w1[i] = a.param[OFF_CONV1_W + i];
    if (tid < C1) s_b1[tid] = a.param[OFF_CONV1_B + tid];
  }
  __syncthreads();

  // conv1 in interval form + ReLU -> (mu, r) planes: item = (channel block, pixel), one float4 store each
  for (int item = tid; item < (C1 / 4) * IBP_A1_PIX; item += 256) {
#pragma clang fp contract(off)
    const int cib = item / IBP_A1_PIX, pix = item - cib * IBP_A1_PIX;
    const int r0 = pix / H1, c0 = pix - r0 * H1;
    float xm[9], xr[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      xm[tap] = s_xm[(r0 + tap / 3) * IMG + c0 + tap % 3];
      xr[tap] = s_xr[(r0 + tap / 3) * IMG + c0 + tap % 3];
    }
    float mu[4], rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 4 * cib + j;
      float c = 0.0f, rad = 0.0f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float w = s_w1[co * 9 + tap];
        c = c + w * xm[tap];
        rad = rad + __builtin_fabsf(w) * xr[tap];
      }
      c = c + s_b1[co];
      const float l = relu_nan_passes(c - rad), u = relu_nan_passes(c + rad);
      mu[j] = (l + u) * 0.5f;
      rr[j] = (u - l) * 0.5f;
    }
    s_mu[cib][pix] = float4{mu[0], mu[1], mu[2], mu[3]};
    s_r[cib][pix] = float4{rr[0], rr[1], rr[2], rr[3]};
  }
  __syncthreads();

  // conv2: M = 96 pixels ordered by pool window, N = this wave's 16 channels, K = 288, both products per fragment
  const float* pm[IBP_MT];
  const float* pr[IBP_MT];
#pragma unroll
  for (int t = 0; t < IBP_MT; ++t) {
    const int win = 4 * t + (n >> 2), wy = win / HP, wx = win - wy * HP;
    const int pix = (2 * wy + ((n >> 1) & 1)) * H1 + 2 * wx + (n & 1);
    pm[t] = reinterpret_cast<const float*>(&s_mu[0][0]) + pix * 4 + g;
    pr[t] = reinterpret_cast<const float*>(&s_r[0][0]) + pix * 4 + g;
  }
  floatx4 accc[IBP_MT], accr[IBP_MT];
#pragma unroll
  for (int t = 0; t < IBP_MT; ++t) accc[t] = accr[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int cib = 0; cib < 8; ++cib) {
      const float w = wreg[tap * 8 + cib], wa = __builtin_fabsf(w);
      const int off = cib * (IBP_A1_PIX * 4) + ((tap / 3) * H1 + tap % 3) * 4;
#pragma unroll
      for (int t = 0; t < IBP_MT; ++t) {
        accc[t] = mfma4(pm[t][off], w, accc[t]);
        accr[t] = mfma4(pr[t][off], wa, accr[t]);
      }
    }

  // epilogue: a lane's four registers are the four pixels of pool window 4 t + g of channel 16 wave + n
  {
#pragma clang fp contract(off)
    const int co = 16 * wave + n;
    const float b = a.param[OFF_CONV2_B + co];
    const int64_t out = img * NFLAT + co * NPOOL + strip * (IBP_P * HP) + g;
#pragma unroll
    for (int t = 0; t < IBP_MT; ++t) {
      float lmax = 0.0f, umax = 0.0f;
      float ls = 0.0f, us = 0.0f, u2max = 0.0f;      // RELAX: the pre-activation bounds of pixel i*, the largest u2
      int is = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float c = accc[t][q] + b, rad = accr[t][q];
        const float l2 = c - rad, u2 = c + rad;
        const float l = relu_nan_passes(l2), u = relu_nan_passes(u2);
        lmax = q ? max_nan_passes(l, lmax) : l;
        umax = q ? max_nan_passes(u, umax) : u;
        if constexpr (RELAX) {
          if (q == 0 || l2 > ls) { ls = l2; us = u2; is = q; }
          u2max = q ? max_nan_passes(u2, u2max) : u2;
        }
      }
      a.pl[out + 4 * t] = lmax;
      a.pu[out + 4 * t] = umax;
      if constexpr (RELAX) {
        // dominant: no other pixel of the window can exceed pixel i*; then the window is relu(z_i*), else only its
        // lower side is (max >= relu(z_i*)) and the upper side is the constant U
        bool dom = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) dom = dom && (q == is || ls >= accc[t][q] + b + accr[t][q]);
        ReluRelax r = relu_relax(ls, us);
        if (!dom) { r.sU = 0.0f; r.bU = u2max; }
        if (u2max <= 0.0f) r = ReluRelax{0.0f, 0.0f, 0.0f};
        relax[out + 4 * t] = float4{r.sL, r.sU, r.bU, __int_as_float(is)};
      }
    }
  }
}

}  // namespace mnist
