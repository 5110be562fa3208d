// Interval bound propagation (IBP; Gowal et al. 2018, Mirman et al. 2018) of the fp32 Net over an L-inf box, in centre /
// radius form: for an affine layer mu = (l + u) / 2, r = (u - l) / 2, c = W mu + b, rad = |W| r, l' = c - rad,
// u' = c + rad; ReLU and the 2 x 2 max-pool are monotone and act on l and u separately.  Every product runs on
// v_mfma_f32_16x16x4_f32 (fp32 operands, exact products, a k-ordered chain) from the fp32 parameters: a bf16 operand
// carries a 2^-9 relative error, more than the margins that decide a certificate.  Rounding inside the bound is not
// propagated outward.  One round is three launches on one stream, no allocation, no atomics, no host sync:
//
// ibp_trunk  grid (6 strips, B), 256 threads.  Work item = (image, strip of 2 pooled rows = 4 conv2 rows = 6 conv1
//   rows = 8 input rows).
//   * The strip.  The two fp32 a1 planes of a whole image are 173 KB, more than the 160 KB of LDS, so an image is cut
//     along pooled rows.  A strip of P pooled rows stages 2P + 2 conv1 rows: the halo costs (2P + 2) / 2P in conv1
//     work and LDS (P = 1: 2.0, P = 2: 1.5, P = 3: 1.33).  P = 2 is 39.9 KB for both planes (three workgroups a
//     CU), M = 96 conv2 pixels = 6 MFMA row tiles a wave, whose 12 accumulators (centre and radius) are 48 VGPRs, and
//     6 workgroups an image, so a single image already spreads over 6 CUs.  P = 3 would save a ninth of the conv1
//     work for 72 accumulator VGPRs and 53 KB.
//   * The weights are not staged in LDS at all.  Wave w owns output channels 16 w .. 16 w + 15 for every pixel of the
//     strip, so its whole B operand is 288 x 16 floats = 72 VGPRs a lane: lane (n, g) loads conv2.weight[16 w + n]
//     [4 cib + g][tap] for the 8 channel blocks cib and 9 taps straight from the torch layout, once, before conv1
//     runs (the loads' latency hides under it).  Each fragment serves both products: W against mu, and |W| - the sign
//     bit cleared in the register - against r.  |W| is never stored and there is no second weight read.
//   * conv1 (one input channel, nine taps) is interval arithmetic on the VALU from the clipped input box, ReLU
//     applied, written as (mu, r) into the LDS planes [ci / 4][pixel][ci % 4]: a thread stores one float4, and the
//     A-operand read of lane (m, g) - pixel of row m, channel 4 cib + g - is one ds_read_b32 at a constant offset
//     from a per-row-tile base (16 pixels x 4 channels: 2 lanes a bank).
//   * M is ordered by pool window (row m = 4 window + position), so the four accumulator registers of a lane are
//     the four pixels of one window: bias, l = c - rad, u = c + rad, ReLU and the 2 x 2 max of l and of u happen in
//     registers, and pl / pu leave in torch flatten order, each element written once.
//   K order: step (tap, cib), k inside the step = g, i.e. ci = 4 cib + g - a fixed chain of 288 fma per output.
//
// ibp_fc1  grid (IBP_SPLITS = 36, ceil(B / 64)), 256 threads, no LDS.  z1c = W1 mu_p, z1r = |W1| r_p, K = 9216.
//   The weights are the A operand (wave w: outputs 32 w .. 32 w + 31), 16 images a column tile, up to 4 tiles a
//   workgroup, so each fc1.weight fragment (one float4 a lane along k: four MFMA steps) is loaded once and serves both
//   products of up to 64 images.  mu_p = (pl + pu) / 2 and r_p = (pu - pl) / 2 are formed in the image loads.
//   Split-K with a fixed number of splits (256 inputs each, whatever B is) into the slab part[z][b][2][128]: an
//   output is a chain over its image's own column in a fixed k order, so an image's bits depend on nothing but the
//   image - not on B, its position or the chunking.  36 splits keep 36 CUs reading the 4.7 MB of weights at B = 1 and
//   the slab at 36 KB an image.
//
// ibp_head  one wave per image, 4 images a workgroup.  Lane k owns hidden units k and k + 64: the partials are
//   summed in split order, + fc1 bias, l = c - rad, u = c + rad, ReLU; then for each class j != y, with C = w2[y] -
//   w2[j]: lb_j = sum_k (max(C_k, 0) l_k + min(C_k, 0) u_k) + (b_y - b_j), each operation rounded on its own, the sum
//   as (t_k + t_{k+64}) then the xor butterfly 32 .. 1; lb_y = +inf.  With `search` lane 0 bisects the record.
//
// A NaN passes every clamp, ReLU and max (they are comparisons, not fminf / fmaxf) and reaches its own image only:
// a work item never reads another image.  Rows and records past B are untouched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the README table; no
// kernel uses scratch.
#include "../runtime/host_logic.h"
#include "../include/device_utils.h"
#include "../include/kernels.h"
#include "ibp_strip.h"

#include <stdexcept>

namespace mnist {

// The strip's code is the template of ibp_strip.h, which crown.hip instantiates a second time with its own epilogue.
__global__ __launch_bounds__(256) void ibp_trunk_kernel(IbpArgs a) { ibp_strip<false>(a, nullptr); }

__global__ __launch_bounds__(256) void ibp_fc1_kernel(IbpArgs a, int B) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int z = blockIdx.x, i0 = blockIdx.y * 64;
  const int ntile = min(4, (B - i0 + 15) / 16);
  RW_ENTRY();
  const float* w = a.param + OFF_FC1_W + (int64_t)(32 * wave + n) * NFLAT + z * IBP_KS + 4 * g;
  const int64_t xoff = (int64_t)(i0 + n) * NFLAT + z * IBP_KS + 4 * g;
  floatx4 cc[2][4], cr[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) cc[i][j] = cr[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int it = 0; it < IBP_KS / 16; ++it) {
    float wv[2][4], wa[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(w + (int64_t)i * 16 * NFLAT + it * 16);
      wv[i][0] = v.x; wv[i][1] = v.y; wv[i][2] = v.z; wv[i][3] = v.w;
#pragma unroll
      for (int q = 0; q < 4; ++q) wa[i][q] = __builtin_fabsf(wv[i][q]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
      if (j >= ntile) continue;
      float4 l{0.f, 0.f, 0.f, 0.f}, u{0.f, 0.f, 0.f, 0.f};
      if (i0 + 16 * j + n < B) {
        l = *reinterpret_cast<const float4*>(a.pl + xoff + (int64_t)j * 16 * NFLAT + it * 16);
        u = *reinterpret_cast<const float4*>(a.pu + xoff + (int64_t)j * 16 * NFLAT + it * 16);
      }
      const float mu[4] = {(l.x + u.x) * 0.5f, (l.y + u.y) * 0.5f, (l.z + u.z) * 0.5f, (l.w + u.w) * 0.5f};
      const float rr[4] = {(u.x - l.x) * 0.5f, (u.y - l.y) * 0.5f, (u.z - l.z) * 0.5f, (u.w - l.w) * 0.5f};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          cc[i][j] = mfma4(wv[i][q], mu[q], cc[i][j]);
          cr[i][j] = mfma4(wa[i][q], rr[q], cr[i][j]);
        }
    }
  }
  // D: column = image n of the tile, rows 4 g .. 4 g + 3 = four consecutive outputs
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int im = i0 + 16 * j + n;
    if (j >= ntile || im >= B) continue;
    float* dst = a.part + ((int64_t)z * B + im) * (2 * NH) + 32 * wave + 4 * g;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<float4*>(dst + 16 * i) = float4{cc[i][j][0], cc[i][j][1], cc[i][j][2], cc[i][j][3]};
      *reinterpret_cast<float4*>(dst + NH + 16 * i) = float4{cr[i][j][0], cr[i][j][1], cr[i][j][2], cr[i][j][3]};
    }
  }
}

__global__ __launch_bounds__(256) void ibp_head_kernel(IbpArgs a, int B) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (img >= B) return;                                      // (no barrier below: a wave is on its own)
  RW_ENTRY();
  float lk[2], uk[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    float c = 0.0f, rad = 0.0f;
    for (int z = 0; z < IBP_SPLITS; ++z) {
      const float* p = a.part + ((int64_t)z * B + img) * (2 * NH) + k;
      c = c + p[0];
      rad = rad + p[NH];
    }
    c = c + a.param[OFF_FC1_B + k];
    lk[h] = relu_nan_passes(c - rad);
    uk[h] = relu_nan_passes(c + rad);
  }
  const int yl = a.labels[img];
  const int y = (unsigned)yl < (unsigned)NCLS ? yl : 0;
  const float* w2 = a.param + OFF_FC2_W;
  const float wy0 = w2[y * NH + lane], wy1 = w2[y * NH + lane + 64], by = a.param[OFF_FC2_B + y];
  float margin = __builtin_inff(), mine = 0.0f;
  for (int j = 0; j < NCLS; ++j) {
    float lbj = __builtin_inff();
    if (j != y) {
      const float c0 = wy0 - w2[j * NH + lane], c1 = wy1 - w2[j * NH + lane + 64];
      const float t0 = (c0 > 0.0f ? c0 : 0.0f) * lk[0] + (c0 < 0.0f ? c0 : 0.0f) * uk[0];
      const float t1 = (c1 > 0.0f ? c1 : 0.0f) * lk[1] + (c1 < 0.0f ? c1 : 0.0f) * uk[1];
      lbj = wave_sum(t0 + t1) + (by - a.param[OFF_FC2_B + j]);
    }
    margin = min_nan_passes(lbj, margin);
    if (lane == j) mine = lbj;
  }
  if (lane < NCLS) a.lb[(int64_t)img * NCLS + lane] = mine;
  if (a.search && lane == 0) {
    float4 r = reinterpret_cast<const float4*>(a.rec)[img];  // {eps, lo, hi, margin}
    if (margin > 0.0f) r.y = r.x; else r.z = r.x;
    r.x = r.y + 0.5f * (r.z - r.y);
    r.w = margin;
    reinterpret_cast<float4*>(a.rec)[img] = r;
  }
}

namespace {
void ibp_check_B(const char* who, int B) {
  if (B < 1 || B > IBP_MAX_B) throw std::runtime_error(std::string(who) + ": image count out of range");
}
}  // namespace

void launch_ibp_trunk(const IbpArgs& a, int B, hipStream_t s) {
  ibp_check_B("ibp_trunk", B);
  if (!a.param || !a.x0 || !a.rec || !a.pl || !a.pu) throw std::runtime_error("ibp_trunk: null argument");
  if (misaligned(15, a.param, a.x0, a.rec, a.pl, a.pu))
    throw std::runtime_error("ibp_trunk: the arrays must be 16-byte aligned");
  if (!(a.pix_std > 0.0f) || !(a.lo < a.hi)) throw std::runtime_error("ibp_trunk: need pix_std > 0 and lo < hi");
  hipLaunchKernelGGL(ibp_trunk_kernel, dim3(IBP_STRIPS, B), dim3(256), 0, s, a);
}

void launch_ibp_fc1(const IbpArgs& a, int B, hipStream_t s) {
  ibp_check_B("ibp_fc1", B);
  if (!a.param || !a.pl || !a.pu || !a.part) throw std::runtime_error("ibp_fc1: null argument");
  if (misaligned(15, a.param, a.pl, a.pu, a.part)) throw std::runtime_error("ibp_fc1: the arrays must be 16-byte aligned");
  hipLaunchKernelGGL(ibp_fc1_kernel, dim3(IBP_SPLITS, (B + 63) / 64), dim3(256), 0, s, a, B);
}

void launch_ibp_head(const IbpArgs& a, int B, hipStream_t s) {
  ibp_check_B("ibp_head", B);
  if (!a.param || !a.part || !a.labels || !a.lb || !a.rec) throw std::runtime_error("ibp_head: null argument");
  if (misaligned(15, a.param, a.part, a.rec)) throw std::runtime_error("ibp_head: the arrays must be 16-byte aligned");
  if (misaligned(3, a.labels, a.lb)) throw std::runtime_error("ibp_head: labels and lb must be 4-byte aligned");
  hipLaunchKernelGGL(ibp_head_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, B);
}

void preload_ibp() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&ibp_trunk_kernel));
}

}  // namespace mnist
