// CROWN-IBP (Zhang et al. 2018 / 2020) of the fp32 Net over an L-inf box: IBP's boxes (ibp.hip) bound every hidden
// pre-activation, and the last interval step is replaced by one backward pass of linear relaxations from the margin rows
// C_j = fc2.weight[y] - fc2.weight[j] down to the input box.  At a relaxed layer with incoming coefficients A the
// outgoing ones are A+ sL + A- sU and the bias gains sum A- bU; at an affine layer the bias gains A b and A <- A W; at
// the input lb_j = sum (A0+ xl + A0- xu) + bias.  The ReLU and the pool that follows it are one relaxation per pooled
// unit: only the window's pixel i* (first argmax of the lower bounds) ever receives a coefficient (ibp_strip.h).
// The statement is IBP's: the fp32 net in real arithmetic, rounding inside the bound not propagated outward.  Every
// product of the two large layers runs on v_mfma_f32_16x16x4_f32, every sum has a fixed order, an image's bits depend
// on the image alone, and no kernel uses atomics, scratch or the host.  One round, one stream:
//
// crown_relax   ibp_trunk's strip (ibp_strip.h) with a second epilogue: the window's four (l2, u2) are a lane's four
//   accumulator registers, so i*, U, `dominant` and the record (sL, sU, bU, i*) - 16 bytes a pooled unit - are formed
//   in registers next to pl / pu.
// ibp_fc1       unchanged, on pl / pu.
// crown_lambda  one wave an image (lane k: hidden units k, k + 64): the slab summed as ibp_head does, the fc1
//   relaxations, Lambda[j][k] = C+ sL + C- sU (rows y and 10 .. 15 zero), the bias so far (b_y - b_j + sum C- bU +
//   Lambda b_fc1) and lb_ibp, the same operations as ibp_head's.
// crown_fc      A_p = Lambda fc1.weight: rows = (image, 16 slots), K = 128, N = 9216.  grid (144, min(B, 16)), 256
//   threads.  Wave w of workgroup x owns the 16 columns 64 x + 16 w ..; its B operand - all 128 k of those columns - is
//   32 VGPRs a lane (lane (n, g), step s: fc1.weight[32 g + s][col + n]), loaded once, and the images of the
//   workgroup's share stream through it: the A operand of lane (j, g) is Lambda[image][j][32 g .. 32 g + 31], eight
//   float4 loads, so the K order is step s, then g inside the MFMA.  fc1.weight is read min(B, 16) times a launch, not
//   B times.  Epilogue: lane (n, g) holds slots 4 g .. 4 g + 3 of column n: the pool relaxation from the record, v
//   written, and the bias terms (A- bU + v conv2.bias) summed over the slice's 16 columns by the xor butterfly 8 .. 1.
// crown_bwd     grid (7 strips, B), 256 threads; the transposed trunk in gather form: a coefficient is complete
//   before its sign is taken.  Work item = (image, 4 input rows [r, r + 4)), which needs conv1 rows [r - 2, r + 4) (6 x
//   26 = 156 pixels, 10 MFMA row tiles) and conv2 rows [r - 4, r + 4).
//   * Registers.  Wave w owns input channels 16 (w & 1) .. and row tiles 5 (w >> 1) ..: its conv2.weight fragments for
//     all 64 x 9 k are 144 VGPRs a lane (lane (n, g), step (tap, cob): weight[4 cob + g][ci][tap]), loaded once for all
//     ten rows.  A lane's 20 accumulator elements are 20 fixed (channel, conv1 pixel) pairs, so their conv1
//     relaxations - recomputed from the box with ibp_trunk's arithmetic - are 60 more VGPRs and never touch LDS.
//   * LDS.  The dense coefficients of the strip's conv2 pixels, [co / 4][8 rows x 28 columns][co % 4] (two zero
//     columns each side, zero rows outside the image: 56 KB), rewritten per row j from v at each window's i*; the A
//     operand is one ds_read_b32 at a constant offset from a per-tile base.  The relaxed conv1 coefficients [ci][6 rows
//     x 30 columns] (22.5 KB) feed the transposed conv1 on the VALU: thread (pixel, half) sums 16 channels x 9 taps,
//     the halves meet by one shuffle, and the pixel is concretised against its own box.
//   * The input strips partition the pixels; a halo conv1 row is recomputed but its bias terms count only in the
//     strip whose input rows contain it (rows 24, 25: the last strip).  Output: (concretised sum, bias) per row j.
// crown_head    one wave an image: bias and partials summed in a fixed order (strips, then slices), max with lb_ibp,
//   lb_y = +inf; with `search` lane 0 bisects the record by ibp_head's rule.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the README table; no
// kernel uses scratch.
#include "../runtime/host_logic.h"
#include "../include/device_utils.h"
#include "../include/kernels.h"
#include "ibp_strip.h"

#include <stdexcept>

namespace mnist {

namespace {
constexpr int CB_H = 4;                            // input rows a strip
constexpr int CB_R1 = CB_H + 2, CB_R2 = CB_H + 4;  // conv1 / conv2 rows a strip touches
constexpr int CB_M = CB_R1 * H1;                   // 156 conv1 pixels
constexpr int CB_MT = (CB_M + 15) / 16;            // 10 row tiles
constexpr int CB_VW = H2 + 4, CB_VPIX = CB_R2 * CB_VW;   // padded conv2 plane of the strip: 8 x 28
constexpr int CB_AW = H1 + 4;                      // padded conv1 row: 30
constexpr int CB_XPIX = (CB_H + 4) * IMG;          // input rows [r - 2, r + 6)
constexpr int CB_UNITS = C2 * (CB_R2 / 2) * HP / 256;    // 12 pooled units a thread
static_assert(CROWN_STRIPS * CB_H == IMG && CB_MT == 10 && CB_UNITS * 256 == C2 * (CB_R2 / 2) * HP &&
              CROWN_SLICES * 16 == NFLAT && CB_H * IMG * 2 <= 256, "crown geometry");

__device__ __forceinline__ float relaxed(float a, float sL, float sU) {
#pragma clang fp contract(off)
  return a > 0.0f ? a * sL : a * sU;
}
__device__ __forceinline__ float relax_bias(float a, float bU) {
#pragma clang fp contract(off)
  return a < 0.0f ? a * bU : 0.0f;
}
}  // namespace

__global__ __launch_bounds__(256) void crown_relax_kernel(IbpArgs a, float4* relax) { ibp_strip<true>(a, relax); }

__global__ __launch_bounds__(256) void crown_lambda_kernel(CrownArgs a, int B) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (img >= B) return;                                      // (no barrier below: a wave is on its own)
  RW_ENTRY();
  float lk[2], uk[2], b1[2];
  ReluRelax rx[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    float c = 0.0f, rad = 0.0f;
    for (int z = 0; z < IBP_SPLITS; ++z) {
      const float* p = a.part + ((int64_t)z * B + img) * (2 * NH) + k;
      c = c + p[0];
      rad = rad + p[NH];
    }
    b1[h] = a.param[OFF_FC1_B + k];
    c = c + b1[h];
    rx[h] = relu_relax(c - rad, c + rad);
    lk[h] = relu_nan_passes(c - rad);
    uk[h] = relu_nan_passes(c + rad);
  }
  const int yl = a.labels[img];
  const int y = (unsigned)yl < (unsigned)NCLS ? yl : 0;
  const float* w2 = a.param + OFF_FC2_W;
  const float wy0 = w2[y * NH + lane], wy1 = w2[y * NH + lane + 64], by = a.param[OFF_FC2_B + y];
  float* lam = a.lam + (int64_t)img * (CROWN_SPEC * NH);
  float bias = 0.0f, ibp = 0.0f;
  for (int j = 0; j < CROWN_SPEC; ++j) {
    float l0 = 0.0f, l1 = 0.0f;
    if (j < NCLS && j != y) {
      const float c0 = wy0 - w2[j * NH + lane], c1 = wy1 - w2[j * NH + lane + 64];
      const float t0 = (c0 > 0.0f ? c0 : 0.0f) * lk[0] + (c0 < 0.0f ? c0 : 0.0f) * uk[0];
      const float t1 = (c1 > 0.0f ? c1 : 0.0f) * lk[1] + (c1 < 0.0f ? c1 : 0.0f) * uk[1];
      const float db = by - a.param[OFF_FC2_B + j];
      const float lbj = wave_sum(t0 + t1) + db;
      l0 = relaxed(c0, rx[0].sL, rx[0].sU);
      l1 = relaxed(c1, rx[1].sL, rx[1].sU);
      const float s0 = relax_bias(c0, rx[0].bU) + l0 * b1[0], s1 = relax_bias(c1, rx[1].bU) + l1 * b1[1];
      const float bj = wave_sum(s0 + s1) + db;
      if (lane == j) { bias = bj; ibp = lbj; }
    }
    lam[j * NH + lane] = l0;
    lam[j * NH + lane + 64] = l1;
  }
  if (lane == y) ibp = __builtin_inff();
  if (lane < CROWN_SPEC) {
    a.fcb[(int64_t)img * (2 * CROWN_SPEC) + lane] = bias;
    a.fcb[(int64_t)img * (2 * CROWN_SPEC) + CROWN_SPEC + lane] = ibp;
  }
}

__global__ __launch_bounds__(256) void crown_fc_kernel(CrownArgs a, int B) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x * 4 + wave, col = slice * 16 + n;
  RW_ENTRY();
  float wreg[32];
  {
    const float* w = a.param + OFF_FC1_W + (int64_t)(32 * g) * NFLAT + col;
#pragma unroll
    for (int s = 0; s < 32; ++s) wreg[s] = w[(int64_t)s * NFLAT];
  }
  const float b2 = a.param[OFF_CONV2_B + col / NPOOL];
  for (int img = blockIdx.y; img < B; img += gridDim.y) {
    const float4 rec = reinterpret_cast<const float4*>(a.relax)[(int64_t)img * NFLAT + col];
    const float4* lp = reinterpret_cast<const float4*>(a.lam + (int64_t)img * (CROWN_SPEC * NH) + n * NH + 32 * g);
    floatx4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      const float4 l = lp[s4];
      acc = mfma4(l.x, wreg[4 * s4], acc);
      acc = mfma4(l.y, wreg[4 * s4 + 1], acc);
      acc = mfma4(l.z, wreg[4 * s4 + 2], acc);
      acc = mfma4(l.w, wreg[4 * s4 + 3], acc);
    }
    // D: column n, slots 4 g .. 4 g + 3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma clang fp contract(off)
      const int j = 4 * g + q;
      const float vv = relaxed(acc[q], rec.x, rec.y);
      float tb = relax_bias(acc[q], rec.z) + vv * b2;
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) tb = tb + __shfl_xor(tb, o, 64);
      if (j < NCLS) {
        a.v[((int64_t)img * NCLS + j) * NFLAT + col] = vv;
        if (n == 0) a.vb[((int64_t)img * CROWN_SLICES + slice) * CROWN_SPEC + j] = tb;
      }
    }
  }
}

__global__ __launch_bounds__(256) void crown_bwd_kernel(CrownArgs a) {
  __shared__ float s_v[(C2 / 4) * CB_VPIX * 4];    // dense conv2 coefficients [co / 4][row][28][co % 4]
  __shared__ float s_a1[C1 * CB_R1 * CB_AW];       // relaxed conv1 coefficients [ci][row][30]
  __shared__ float s_xl[CB_XPIX], s_xu[CB_XPIX], s_xm[CB_XPIX], s_xr[CB_XPIX];
  __shared__ float s_w1[C1 * 9];
  __shared__ float s_red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int strip = blockIdx.x, r = strip * CB_H;
  const int64_t img = blockIdx.y;
  const int nt = wave & 1, mh = wave >> 1, ci = 16 * nt + n;
  RW_ENTRY();

  // this wave's conv2 weight slice: step (tap, cob), lane (n, g) -> weight[4 cob + g][ci][tap]
  float wreg[144];
  {
    const float* w2 = a.param + OFF_CONV2_W + g * (C1 * 9) + ci * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int cob = 0; cob < 16; ++cob) wreg[tap * 16 + cob] = w2[cob * (4 * C1 * 9) + tap];
  }

  // the box of input rows [r - 2, r + 6) (zero outside the image), the conv1 weights, zeroed coefficient planes
  {
#pragma clang fp contract(off)
    const float eps_n = a.rec[img * 4] / a.pix_std;
    if (tid < CB_XPIX) {
      const int row = r - 2 + tid / IMG;
      float l = 0.0f, u = 0.0f;
      if (row >= 0 && row < IMG) {
        const float x = a.x0[img * (IMG * IMG) + row * IMG + tid % IMG];
        l = x - eps_n;
        u = x + eps_n;
        l = l < a.lo ? a.lo : l;
        u = u > a.hi ? a.hi : u;
      }
      s_xl[tid] = l;
      s_xu[tid] = u;
      s_xm[tid] = (l + u) * 0.5f;
      s_xr[tid] = (u - l) * 0.5f;
    }
    for (int i = tid; i < C1 * 9; i += 256) s_w1[i] = a.param[OFF_CONV1_W + i];
    for (int i = tid; i < (C2 / 4) * CB_VPIX * 4; i += 256) s_v[i] = 0.0f;
    for (int i = tid; i < C1 * CB_R1 * CB_AW; i += 256) s_a1[i] = 0.0f;
  }
  __syncthreads();

  // the conv1 relaxations of this lane's 20 accumulator elements: tile 5 mh + tt, pixel 16 tile + 4 g + q
  float sU[5][4], bU[5][4];                      // (sL is 0 or 1: a bit)
  unsigned valid = 0, own = 0, sLbit = 0;
  const float b1 = a.param[OFF_CONV1_B + ci];
  {
#pragma clang fp contract(off)
    float w[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) w[tap] = s_w1[ci * 9 + tap];
#pragma unroll
    for (int tt = 0; tt < 5; ++tt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = 16 * (5 * mh + tt) + 4 * g + q, mv = m < CB_M ? m : CB_M - 1;
        const int rl = mv / H1, cc = mv - rl * H1, row = r - 2 + rl;
        float c = 0.0f, rad = 0.0f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int xi = (rl + tap / 3) * IMG + cc + tap % 3;
          c = c + w[tap] * s_xm[xi];
          rad = rad + __builtin_fabsf(w[tap]) * s_xr[xi];
        }
        c = c + b1;
        const ReluRelax rx = relu_relax(c - rad, c + rad);
        sU[tt][q] = rx.sU; bU[tt][q] = rx.bU;
        if (rx.sL != 0.0f) sLbit |= 1u << (4 * tt + q);
        const bool ok = m < CB_M && row >= 0 && row < H1;
        if (ok) valid |= 1u << (4 * tt + q);
        if (ok && row >= r) own |= 1u << (4 * tt + q);
      }
  }

  // A-operand bases: lane (n, g) reads conv1 pixel 16 tile + n of channel block cob at component g
  const float* pv[5];
#pragma unroll
  for (int tt = 0; tt < 5; ++tt) {
    const int m = 16 * (5 * mh + tt) + n, mv = m < CB_M ? m : CB_M - 1;
    const int rl = mv / H1, cc = mv - rl * H1;
    pv[tt] = s_v + ((rl + 2) * CB_VW + cc + 2) * 4 + g;
  }

  // this thread's 12 pooled units of the strip's 4 pooled rows
  uint64_t istar = 0;                              // 3 bits a unit: i*, or 4 outside the image
#pragma unroll
  for (int i = 0; i < CB_UNITS; ++i) {
    const int idx = tid + 256 * i, co = idx / (4 * HP), rem = idx - co * (4 * HP), lp = rem / HP, px = rem - lp * HP;
    const int py = r / 2 - 2 + lp;
    int is = 4;
    if (py >= 0 && py < HP)
      is = __float_as_int(a.relax[((int64_t)img * NFLAT + co * NPOOL + py * HP + px) * 4 + 3]) & 3;
    istar |= (uint64_t)is << (3 * i);
  }

  const int yl = a.labels[img];
  const int y = (unsigned)yl < (unsigned)NCLS ? yl : 0;
#pragma unroll 1
  for (int j = 0; j < NCLS; ++j) {
    float* out = a.sp + (((int64_t)img * CROWN_STRIPS + strip) * NCLS + j) * 2;
    if (j == y) {                                  // (uniform: the whole workgroup skips the row)
      if (tid < 2) out[tid] = 0.0f;
      continue;
    }
    // densify: each window's four pixels, v at i* and zero elsewhere
    const float* vj = a.v + ((int64_t)img * NCLS + j) * NFLAT;
#pragma unroll
    for (int i = 0; i < CB_UNITS; ++i) {
      const int idx = tid + 256 * i, co = idx / (4 * HP), rem = idx - co * (4 * HP), lp = rem / HP, px = rem - lp * HP;
      const int is = (int)(istar >> (3 * i)) & 7;
      if (is < 4) {
        const float val = vj[co * NPOOL + (r / 2 - 2 + lp) * HP + px];
        float* d = s_v + ((co >> 2) * CB_VPIX + 2 * lp * CB_VW + 2 * px + 2) * 4 + (co & 3);
#pragma unroll
        for (int q = 0; q < 4; ++q) d[((q >> 1) * CB_VW + (q & 1)) * 4] = q == is ? val : 0.0f;
      }
    }
    __syncthreads();

    // transposed conv2: A1[ci][R][C] = sum_{co, ky, kx} V[co][R - ky][C - kx] weight[co][ci][ky][kx]
    floatx4 acc[5];
#pragma unroll
    for (int tt = 0; tt < 5; ++tt) acc[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int cob = 0; cob < 16; ++cob) {
        const int off = cob * (CB_VPIX * 4) - ((tap / 3) * CB_VW + tap % 3) * 4;
#pragma unroll
        for (int tt = 0; tt < 5; ++tt) acc[tt] = mfma4(pv[tt][off], wreg[tap * 16 + cob], acc[tt]);
        if (cob % 4 == 3) asm volatile("" ::: "memory");   // at most 20 operand reads in flight: no spills
      }

    // the conv1 relaxation, in registers; bias terms of the rows this strip owns
    float bias = 0.0f;
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int tt = 0; tt < 5; ++tt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = 16 * (5 * mh + tt) + 4 * g + q, mv = m < CB_M ? m : CB_M - 1;
          const int rl = mv / H1, cc = mv - rl * H1, bit = 4 * tt + q;
          const float av = acc[tt][q];
          const float o = relaxed(av, ((sLbit >> bit) & 1) ? 1.0f : 0.0f, sU[tt][q]);
          if ((own >> bit) & 1) bias = bias + (relax_bias(av, bU[tt][q]) + o * b1);
          if (m < CB_M) s_a1[(ci * CB_R1 + rl) * CB_AW + cc + 2] = ((valid >> bit) & 1) ? o : 0.0f;
        }
    }
    __syncthreads();

    // transposed conv1 on the VALU and the concretisation over the strip's own 4 x 28 pixels
    float term = 0.0f;
    {
#pragma clang fp contract(off)
      const int pix = tid >> 1, half = tid & 1;
      float s = 0.0f;
      if (pix < CB_H * IMG) {
        const int yy = pix / IMG, xx = pix - yy * IMG;
        for (int c = 16 * half; c < 16 * half + 16; ++c)
#pragma unroll
          for (int tap = 0; tap < 9; ++tap)
            s = s + s_a1[(c * CB_R1 + yy + 2 - tap / 3) * CB_AW + xx + 2 - tap % 3] * s_w1[c * 9 + tap];
      }
      const float a0 = s + __shfl_xor(s, 1, 64);
      if (pix < CB_H * IMG && half == 0) {
        const int xi = 2 * IMG + pix;
        term = a0 > 0.0f ? a0 * s_xl[xi] : a0 * s_xu[xi];
      }
      term = wave_sum(term);
      bias = wave_sum(bias);
      if (lane == 0) { s_red[wave][0] = term; s_red[wave][1] = bias; }
    }
    __syncthreads();
    if (tid < 2) {
#pragma clang fp contract(off)
      out[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
  }
}

__global__ __launch_bounds__(256) void crown_head_kernel(CrownArgs a, int B) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (img >= B) return;
  RW_ENTRY();
  const int yl = a.labels[img];
  const int y = (unsigned)yl < (unsigned)NCLS ? yl : 0;
  const float* fcb = a.fcb + (int64_t)img * (2 * CROWN_SPEC);
  const float* vb = a.vb + (int64_t)img * CROWN_SLICES * CROWN_SPEC;
  const float* sp = a.sp + (int64_t)img * CROWN_STRIPS * NCLS * 2;
  float margin = __builtin_inff(), mine = 0.0f, minec = 0.0f;
  for (int j = 0; j < NCLS; ++j) {
    float lbj = __builtin_inff(), lbc = __builtin_inff();
    if (j != y) {
      float t = 0.0f;
      for (int i = 0; i < CROWN_SLICES / 64; ++i) t = t + vb[(lane + 64 * i) * CROWN_SPEC + j];
      t = wave_sum(t);
      float s = fcb[j];
      for (int z = 0; z < CROWN_STRIPS; ++z) s = (s + sp[(z * NCLS + j) * 2]) + sp[(z * NCLS + j) * 2 + 1];
      lbc = s + t;
      lbj = max_nan_passes(lbc, fcb[CROWN_SPEC + j]);
    }
    margin = min_nan_passes(lbj, margin);
    if (lane == j) { mine = lbj; minec = lbc; }
  }
  if (lane < NCLS) {
    a.lb[(int64_t)img * NCLS + lane] = mine;
    if (a.lbc) a.lbc[(int64_t)img * NCLS + lane] = minec;
  }
  if (a.search && lane == 0) {
    float4 r = reinterpret_cast<const float4*>(a.rec)[img];  // {eps, lo, hi, margin}
    if (margin > 0.0f) r.y = r.x; else r.z = r.x;
    r.x = r.y + 0.5f * (r.z - r.y);
    r.w = margin;
    reinterpret_cast<float4*>(a.rec)[img] = r;
  }
}

namespace {
void crown_check_B(const char* who, int B) {
  if (B < 1 || B > IBP_MAX_B) throw std::runtime_error(std::string(who) + ": image count out of range");
}
template <class... Ps>
void crown_check(const char* who, const Ps*... p) {
  if (((p == nullptr) || ...)) throw std::runtime_error(std::string(who) + ": null argument");
  if (misaligned(15, p...)) throw std::runtime_error(std::string(who) + ": the arrays must be 16-byte aligned");
}
void crown_check_labels(const char* who, const int32_t* labels) {
  if (!labels || misaligned(3, labels)) throw std::runtime_error(std::string(who) + ": labels must be 4-byte aligned");
}
void crown_check_box(const char* who, const CrownArgs& a) {
  if (!(a.pix_std > 0.0f) || !(a.lo < a.hi)) throw std::runtime_error(std::string(who) + ": need pix_std > 0 and lo < hi");
}
}  // namespace

void launch_crown_relax(const CrownArgs& a, int B, hipStream_t s) {
  crown_check_B("crown_relax", B);
  crown_check("crown_relax", a.param, a.x0, a.rec, a.pl, a.pu, a.relax);
  crown_check_box("crown_relax", a);
  IbpArgs i{};
  i.param = a.param; i.x0 = a.x0; i.rec = a.rec; i.pl = a.pl; i.pu = a.pu;
  i.pix_std = a.pix_std; i.lo = a.lo; i.hi = a.hi;
  hipLaunchKernelGGL(crown_relax_kernel, dim3(IBP_STRIPS, B), dim3(256), 0, s, i, reinterpret_cast<float4*>(a.relax));
}

void launch_crown_lambda(const CrownArgs& a, int B, hipStream_t s) {
  crown_check_B("crown_lambda", B);
  crown_check("crown_lambda", a.param, a.part, a.lam, a.fcb);
  crown_check_labels("crown_lambda", a.labels);
  hipLaunchKernelGGL(crown_lambda_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, B);
}

void launch_crown_fc(const CrownArgs& a, int B, hipStream_t s) {
  crown_check_B("crown_fc", B);
  crown_check("crown_fc", a.param, a.relax, a.lam, a.v, a.vb);
  hipLaunchKernelGGL(crown_fc_kernel, dim3(CROWN_SLICES / 4, B < 16 ? B : 16), dim3(256), 0, s, a, B);
}

void launch_crown_bwd(const CrownArgs& a, int B, hipStream_t s) {
  crown_check_B("crown_bwd", B);
  crown_check("crown_bwd", a.param, a.x0, a.rec, a.relax, a.v, a.sp);
  crown_check_labels("crown_bwd", a.labels);
  crown_check_box("crown_bwd", a);
  hipLaunchKernelGGL(crown_bwd_kernel, dim3(CROWN_STRIPS, B), dim3(256), 0, s, a);
}

void launch_crown_head(const CrownArgs& a, int B, hipStream_t s) {
  crown_check_B("crown_head", B);
  crown_check("crown_head", a.fcb, a.vb, a.sp, a.rec);
  crown_check_labels("crown_head", a.labels);
  if (!a.lb || misaligned(3, a.lb) || (a.lbc && misaligned(3, a.lbc)))
    throw std::runtime_error("crown_head: lb must be 4-byte aligned");
  hipLaunchKernelGGL(crown_head_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, B);
}

void preload_crown() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&crown_bwd_kernel));
}

}  // namespace mnist
