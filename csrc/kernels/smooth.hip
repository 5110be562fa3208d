// Randomized smoothing (Cohen, Rosenfeld, Kolter 2019): the generator of the Gaussian-noised rows and the vote.
//
// smooth_noise: out[r][784] fp32, r = i * n + s for image i < M and sample s < n,
//
//   out = x0_i + sigma * z
//
// x0_i the normalised image: uint8 rows through normalize_u8_alu (the in-register arithmetic of trunk_fwd,
// bit for bit inference._PIXEL_LUT[u8]) or fp32 [M][784] rows that are already normalised.  sigma is in
// normalised units.  There is no clamp: the smoothed classifier is defined on the unclamped Gaussian.
//
// PHILOX COUNTER LAYOUT (a domain of its own): the float4 v (0 .. 195) of sample s of image i uses the four
// words of
//
//   philox4x32(c0 = sample_base + s, c1 = SMOOTH_PHILOX_DOMAIN, c2 = id_base + i, c3 = v; key = seed lo, hi)
//
// Both dropout streams (device_utils.h dropout_block) use c1 = the high half of a 16-element block index,
// which is zero for every batch the engine can run; adv_init (adv_train.hip) uses c1 = ADV_PHILOX_DOMAIN.
// SMOOTH_PHILOX_DOMAIN is non-zero and differs from ADV_PHILOX_DOMAIN, so under one seed no counter of this
// kernel is ever a dropout or an adv_init counter, whatever the step, the epoch's rng_base, the image id and
// the sample index.  Within the domain (c0, c2, c3) = (sample, image, float4) names each draw once: the launcher
// keeps sample_base + n and id_base + M within 32 bits, so neither word wraps onto another draw.
//
// BOX-MULLER: the words (w0, w1) and (w2, w3) each feed one pair,
//
//   u1 = ((w >> 8) + 1) * 2^-24  in (0, 1]      u2 = (w' >> 8) * 2^-24  in [0, 1)
//   r = sqrtf(-2 logf(u1))      z = r cosf(2 pi u2),  r sinf(2 pi u2)
//
// elements 4v .. 4v + 3 = (cos, sin) of (w0, w1), then (cos, sin) of (w2, w3).  Both u are exact (24 bits);
// every other operation is rounded on its own (contraction off) and logf / sinf / cosf / sqrtf are the precise
// device functions, not the __-prefixed fast ones.
// TAILS: u1 >= 2^-24, so r <= sqrt(48 ln 2) = 5.768: no |z| beyond 5.77 sigma is ever drawn.  A true Gaussian
// has 2 Phi(-5.768) = 8.0e-9 of its mass out there (per element; the radius r itself loses exp(-r^2 / 2) =
// 2^-24 = 6.0e-8), far below what a vote of 10^5 samples resolves.
//
// STEP FORM (the engine's Gaussian-noise training step): the same body on the rows of a step, in place on the
// copy adv_init made: x[b] = x0[b] + sigma * z with counter (c0 = low 32 bits of rng_base + 2 step, DOMAIN,
// c2 = b, c3 = v) and key state->seed - the plain form fed sample_base = that c0, id_base = 0, n = 1.  rng_base
// moves with the epoch, so the draw differs between epochs.
//
// One thread owns one float4 of a row (196 per row, one workgroup of 256 threads per row; the 60 spare threads
// of a workgroup leave).  16-byte stores, no atomics, no LDS; the grid is exactly M * n workgroups, so nothing
// past the last row is written, and a thread's values depend only on (seed, image id, sample index, v, sigma,
// x0): the same bits on any grid, chunking, stream and launch.
//
// smooth_vote: counts[i][10] int32 from logp[M * n][10] fp32 (rows ordered as above).  One workgroup per image,
// its threads stride over the image's n rows; each row votes for its argmax, the first maximum wins a tie, a
// row holding a NaN votes for nothing.  A thread keeps its ten bins in registers, a wave sums them by shuffles,
// the four waves meet in LDS: integer adds only, so the order is irrelevant.  accumulate adds to the counts
// already there (the samples of one image may arrive in several launches); rows of counts past M are untouched.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
constexpr int SV_THREADS = 256, SV_WAVES = SV_THREADS / 64;

// one Box-Muller pair from two Philox words
__device__ __forceinline__ void sn_pair(uint32_t wa, uint32_t wb, float& zc, float& zs) {
#pragma clang fp contract(off)
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;   // (0, 1], exact
  const float u2 = (float)(wb >> 8) * 0x1p-24f;          // [0, 1), exact
  const float r = sqrtf(-2.0f * logf(u1));
  const float t = 6.28318530717958647692f * u2;
  zc = r * cosf(t);
  zs = r * sinf(t);
}
__device__ __forceinline__ float sn_add(float x0, float sigma, float z) {
#pragma clang fp contract(off)
  return x0 + sigma * z;
}
}  // namespace

// SRC 0: uint8 rows; 1: fp32 rows; 2: the step form (fp32 rows x0, counters from the StepState)
template <int SRC>
__global__ __launch_bounds__(ROW_THREADS) void smooth_noise_kernel(SmoothNoiseArgs a) {
  RW_ENTRY();
  const int v = threadIdx.x;
  if (v >= ROW_VECS) return;
  const int64_t r = blockIdx.x;
  int64_t i;
  uint32_t c0, c2;
  uint64_t seed;
  if constexpr (SRC == 2) {
    i = r;
    seed = a.state->seed;
    c0 = (uint32_t)(a.state->rng_base + 2ull * (uint64_t)(uint32_t)a.state->step);
    c2 = (uint32_t)r;
  } else {
    i = (uint32_t)blockIdx.x / (uint32_t)a.n;            // rows <= SMOOTH_MAX_ROWS: 32-bit division
    seed = a.seed;
    c0 = a.sample_base + (uint32_t)(r - i * a.n);
    c2 = a.id_base + (uint32_t)i;
  }
  float4 c;                                              // (fp32 rows: read here, not through row_load - row_ops.h)
  if constexpr (SRC == 0) c = row_load_u8(a.x_u8, i, v);
  else c = reinterpret_cast<const float4*>(a.x_f32)[i * ROW_VECS + v];
  const u32x4 w = philox4x32(c0, SMOOTH_PHILOX_DOMAIN, c2, (uint32_t)v, (uint32_t)seed, (uint32_t)(seed >> 32));
  float z0, z1, z2, z3;
  sn_pair(w[0], w[1], z0, z1);
  sn_pair(w[2], w[3], z2, z3);
  float4 o;
  o.x = sn_add(c.x, a.sigma, z0);
  o.y = sn_add(c.y, a.sigma, z1);
  o.z = sn_add(c.z, a.sigma, z2);
  o.w = sn_add(c.w, a.sigma, z3);
  reinterpret_cast<float4*>(a.out)[r * ROW_VECS + v] = o;
}

__global__ __launch_bounds__(SV_THREADS) void smooth_vote_kernel(SmoothVoteArgs a) {
  RW_ENTRY();
  __shared__ int wbins[SV_WAVES][NCLS];
  const int i = blockIdx.x, tid = threadIdx.x;
  int bins[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) bins[c] = 0;
  const float* rows = a.logp + (int64_t)i * a.n * NCLS;
  for (int s = tid; s < a.n; s += SV_THREADS) {
    const float* p = rows + (int64_t)s * NCLS;
    float best = p[0];
    int bi = 0;
    bool nan = best != best;
#pragma unroll
    for (int c = 1; c < NCLS; ++c) {
      const float x = p[c];
      nan |= x != x;
      if (x > best) { best = x; bi = c; }                // strict: the first maximum wins a tie
    }
#pragma unroll
    for (int c = 0; c < NCLS; ++c) bins[c] += (!nan && bi == c) ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    int t = bins[c];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((tid & 63) == 0) wbins[tid >> 6][c] = t;
  }
  __syncthreads();
  if (tid < NCLS) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < SV_WAVES; ++w) t += wbins[w][tid];
    int* out = a.counts + (int64_t)i * NCLS + tid;
    *out = a.accumulate ? *out + t : t;
  }
}

namespace {
void check_noise_common(const SmoothNoiseArgs& a, const void* src, int64_t rows) {
  if (!src || !a.out) throw std::runtime_error("smooth_noise: null argument");
  if (rows < 1 || rows > SMOOTH_MAX_ROWS) throw std::runtime_error("smooth_noise: M * n out of range");
  if (!(a.sigma >= 0.0f)) throw std::runtime_error("smooth_noise: need sigma >= 0");
  if (misaligned(15, a.out)) throw std::runtime_error("smooth_noise: out must be 16-byte aligned");
}
}  // namespace

void launch_smooth_noise(const SmoothNoiseArgs& a, int M, hipStream_t s) {
  check_one_row_source("smooth_noise", a.x_u8, a.x_f32);
  if (M < 1 || a.n < 1) throw std::runtime_error("smooth_noise: M * n out of range");
  const int64_t rows = (int64_t)M * a.n;
  check_noise_common(a, a.x_u8 ? static_cast<const void*>(a.x_u8) : a.x_f32, rows);
  check_row_source_aligned("smooth_noise", a.x_u8, a.x_f32);
  if ((uint64_t)a.sample_base + (uint64_t)a.n > (1ull << 32))
    throw std::runtime_error("smooth_noise: sample_base + n must not exceed 2^32");
  if ((uint64_t)a.id_base + (uint64_t)M > (1ull << 32))
    throw std::runtime_error("smooth_noise: id_base + M must not exceed 2^32");
  if (a.x_u8)
    hipLaunchKernelGGL(smooth_noise_kernel<0>, dim3((unsigned)rows), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(smooth_noise_kernel<1>, dim3((unsigned)rows), dim3(ROW_THREADS), 0, s, a);
}

void launch_smooth_noise_step(const StepState* state, const float* x0, float* x, float sigma, int B, hipStream_t s) {
  SmoothNoiseArgs a{nullptr, x0, x, state, sigma, 0, 0u, 0u, 1};
  if (!state) throw std::runtime_error("smooth_noise: null argument");
  check_noise_common(a, x0, B);
  check_row_source_aligned("smooth_noise", nullptr, x0);
  hipLaunchKernelGGL(smooth_noise_kernel<2>, dim3((unsigned)B), dim3(ROW_THREADS), 0, s, a);
}

void launch_smooth_vote(const SmoothVoteArgs& a, int M, hipStream_t s) {
  if (!a.logp || !a.counts) throw std::runtime_error("smooth_vote: null argument");
  if (M < 1 || a.n < 1 || (int64_t)M * a.n > SMOOTH_MAX_ROWS) throw std::runtime_error("smooth_vote: M * n out of range");
  if (misaligned(3, a.logp, a.counts)) throw std::runtime_error("smooth_vote: logp and counts must be 4-byte aligned");
  hipLaunchKernelGGL(smooth_vote_kernel, dim3(M), dim3(SV_THREADS), 0, s, a);
}

void preload_smooth() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&smooth_noise_kernel<0>));
}

}  // namespace mnist
