// fc1 forward (split-K MFMA GEMM), the fused head (bias+ReLU+dropout(0.5)+fc2+log_softmax+NLL and
// its backward), and the fused fc backward (dW_fc1, db_fc1, dW_fc2, db_fc2, dgrad to the conv trunk).
//
// Reference ops replaced: mnist_ddp.py:57-61 (fc1, relu, dropout2, fc2, log_softmax), :71 (nll_loss)
// and their autograd backward at :72.
#include "../include/device_utils.h"
#include "../include/kernels.h"
#include "../include/timeline.h"
#include "../runtime/host_logic.h"

#include <stdexcept>
#include <stdlib.h>

namespace mnist {

// ============================================================================================
// fc1 forward: z1part[s][b][o] = sum_{i in chunk s} p[b][i] * w1[o][i]
// M = B rows, N = 128, K = 9216 split FC1_KSPLIT (32) ways (288 = 9 k-steps each).
// WG = (16-row M-tile, K-chunk); its 4 waves split N (32 columns each), so every CU streams a
// distinct 18 KB slice of w1 (L2/MALL resident) and the grid is ceil(B/16) x 32 WGs.  All 27
// fragment loads of a wave are independent and issued before the MFMAs.
// ============================================================================================
// MR = 16-row M-tiles per workgroup: MR = 2 (default) halves the w1 fragment traffic per output
// (each wave's B fragments feed two M-tiles) at half the workgroups; bitwise the MR = 1 result.
// One fc1 workgroup (row tile x K-chunk) of the R x 32 grid, linear id `lin`.
template <int MR>
__device__ __forceinline__ void fc1_tile(const uint16_t* __restrict__ p, const uint16_t* __restrict__ w1,
                                        float* __restrict__ z1part, int B, int R, int xcd, int j, int wave) {
  constexpr int KC = NFLAT / FC1_KSPLIT;   // 288
  constexpr int KS = KC / 32;              // 9
  const int lane = threadIdx.x & 63;
  const int m = lane & 15, kg = lane >> 4;
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (linear id mod 8), so
  // give every XCD 4 whole K-chunks (all row tiles of each): a chunk's 74 KB w1 slice is then
  // fetched into ONE XCD's L2 instead of all eight (grid = R x 32, R*32 divisible by 8)
  static_assert(FC1_KSPLIT == 32, "4 K-chunks per XCD");
  const int chunk = 4 * xcd + j / R;
  const int tile = j - (j / R) * R;
  const uint16_t* pb = w1 + (int64_t)(32 * wave + m) * NFLAT + chunk * KC + 8 * kg;
  bf16x8 A[MR][KS], B0[KS], B1[KS];
  bool valid[MR];
#pragma unroll
  for (int t = 0; t < MR; ++t) {
    const int row = (tile * MR + t) * 16 + m;
    valid[t] = row < B;
    const uint16_t* pa = p + (int64_t)(valid[t] ? row : 0) * NFLAT + chunk * KC + 8 * kg;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) A[t][ks] = ld16(pa + ks * 32);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    B0[ks] = ld16(pb + ks * 32);
    B1[ks] = ld16(pb + 16 * NFLAT + ks * 32);
  }
  // z1^T tiles (w1 fragments as the A operand): lane (m, kg) ends with outputs o = 32 wave + 4 kg
  // + r (r = 0..3) of batch row m - 16 contiguous bytes of z1part, one 16-B store (write-through at
  // small batches: only the head reads them) instead of four scattered 4-B stores
#pragma unroll
  for (int t = 0; t < MR; ++t) {
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 a = valid[t] ? A[t][ks] : zero_frag();
      acc0 = mfma16x16x32(B0[ks], a, acc0);
      acc1 = mfma16x16x32(B1[ks], a, acc1);
    }
    const int b = (tile * MR + t) * 16 + m;
    if (b < B) {
      const int64_t e = ((int64_t)chunk * B + b) * NH + 32 * wave + 4 * kg;
      store16(B <= WT_MAX_B, z1part, e * 4, acc0);
      store16(B <= WT_MAX_B, z1part, (e + 16) * 4, acc1);
    }
  }
}

template <int MR>
__global__ __launch_bounds__(256) void fc1_fwd_kernel(const uint16_t* __restrict__ p,
                                                      const uint16_t* __restrict__ w1,
                                                      float* __restrict__ z1part, int B) {
  RW_ENTRY();
  TL_SCOPE(TL_FC1);
  const int lin = blockIdx.x + gridDim.x * blockIdx.y;
  fc1_tile<MR>(p, w1, z1part, B, gridDim.x, lin & 7, lin >> 3, threadIdx.x >> 6);
}

// Large batches: 64 rows x 128 columns per workgroup, K split 4 ways (2304 = 36 stages of 64),
// A [64][64] and B [128][64] bf16 stages double-buffered in LDS (128-B rows, chunk ^ (row>>1 & 7)
// swizzle: conflict-free ds_read_b128 fragment reads), next stage prefetched into VGPRs.  Each wave
// owns 32 rows x 64 columns (2 x 4 MFMA tiles): w1 is read from L2 once per 64 rows, not per 16.
namespace {
constexpr int F1B_ROWS = 64, F1B_KS = 64;
constexpr int F1B_KC = NFLAT / FC1_KSPLIT_BIG;            // 2304
constexpr int F1B_STAGES = F1B_KC / F1B_KS;               // 36
constexpr int F1B_ABYTES = F1B_ROWS * F1B_KS * 2;         // 8192
constexpr int F1B_BBYTES = NH * F1B_KS * 2;               // 16384
constexpr int F1B_STAGE = F1B_ABYTES + F1B_BBYTES;        // 24576
__device__ __forceinline__ int f1b_swz(int row) { return (row >> 1) & 7; }
}  // namespace

__global__ __launch_bounds__(256) void fc1_fwd_big_kernel(const uint16_t* __restrict__ p,
                                                          const uint16_t* __restrict__ w1,
                                                          float* __restrict__ z1part, int B) {
  RW_ENTRY();
  TL_SCOPE(TL_FC1);
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * F1B_STAGE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, kg = lane >> 4;
  const int r0 = blockIdx.x * F1B_ROWS, split = blockIdx.y;
  const int kbase = split * F1B_KC;
  const int wr = 32 * (wave & 1), wc = 64 * (wave >> 1);
  // staging map: A 512 chunks (2/thread), B 1024 chunks (4/thread); chunk = (row, 16-B column)
  uint4 ra0, ra1, rb0, rb1, rb2, rb3;
#define F1B_FETCH(st)                                                                             \
  {                                                                                               \
    const int k0 = kbase + (st) * F1B_KS;                                                         \
    const int ar0 = tid >> 3, ar1 = (tid + 256) >> 3, cc = tid & 7;                               \
    ra0 = (r0 + ar0 < B) ? *reinterpret_cast<const uint4*>(p + (int64_t)(r0 + ar0) * NFLAT + k0 + cc * 8) \
                         : uint4{0u, 0u, 0u, 0u};                                                 \
    ra1 = (r0 + ar1 < B) ? *reinterpret_cast<const uint4*>(p + (int64_t)(r0 + ar1) * NFLAT + k0 + cc * 8) \
                         : uint4{0u, 0u, 0u, 0u};                                                 \
    rb0 = *reinterpret_cast<const uint4*>(w1 + (int64_t)(tid >> 3) * NFLAT + k0 + cc * 8);          \
    rb1 = *reinterpret_cast<const uint4*>(w1 + (int64_t)((tid + 256) >> 3) * NFLAT + k0 + cc * 8);  \
    rb2 = *reinterpret_cast<const uint4*>(w1 + (int64_t)((tid + 512) >> 3) * NFLAT + k0 + cc * 8);  \
    rb3 = *reinterpret_cast<const uint4*>(w1 + (int64_t)((tid + 768) >> 3) * NFLAT + k0 + cc * 8);  \
  }
#define F1B_STORE(buf)                                                                            \
  {                                                                                               \
    uint4* as_ = reinterpret_cast<uint4*>(smem + (buf) * F1B_STAGE);                              \
    uint4* bs_ = reinterpret_cast<uint4*>(smem + (buf) * F1B_STAGE + F1B_ABYTES);                 \
    const int cc = tid & 7;                                                                       \
    int row = tid >> 3;                                                                           \
    as_[row * 8 + (cc ^ f1b_swz(row))] = ra0;                                                     \
    bs_[row * 8 + (cc ^ f1b_swz(row))] = rb0;                                                     \
    row += 32;                                                                                    \
    as_[row * 8 + (cc ^ f1b_swz(row))] = ra1;                                                     \
    bs_[row * 8 + (cc ^ f1b_swz(row))] = rb1;                                                     \
    row += 32;                                                                                    \
    bs_[row * 8 + (cc ^ f1b_swz(row))] = rb2;                                                     \
    row += 32;                                                                                    \
    bs_[row * 8 + (cc ^ f1b_swz(row))] = rb3;                                                     \
  }
  floatx4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  F1B_FETCH(0);
  F1B_STORE(0);
  __syncthreads();
  for (int st = 0; st < F1B_STAGES; ++st) {
    const int buf = st & 1;
    if (st + 1 < F1B_STAGES) F1B_FETCH(st + 1);               // in flight under this stage's MFMAs
    const uint16_t* as = reinterpret_cast<const uint16_t*>(smem + buf * F1B_STAGE);
    const uint16_t* bs = reinterpret_cast<const uint16_t*>(smem + buf * F1B_STAGE + F1B_ABYTES);
#pragma unroll
    for (int t = 0; t < F1B_KS / 32; ++t) {
      const int ch = 4 * t + kg;
      bf16x8 A[2], Bf[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wr + 16 * i + m;
        A[i] = ld16(as + row * F1B_KS + ((ch ^ f1b_swz(row)) << 3));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wc + 16 * j + m;
        Bf[j] = ld16(bs + row * F1B_KS + ((ch ^ f1b_swz(row)) << 3));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16x16x32(Bf[j], A[i], acc[i][j]);   // z1^T tiles
    }
    if (st + 1 < F1B_STAGES) F1B_STORE(buf ^ 1);
    __syncthreads();
  }
#undef F1B_FETCH
#undef F1B_STORE
  // transposed C fragment: lane (m, kg) holds outputs o = wc + 16 j + 4 kg + r (r = 0..3) of batch
  // row b = wr + 16 i + m - one 16-B store each (write-through up to WT_MAX_B: the head reads them)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int b = r0 + wr + 16 * i + m;
    if (b < B) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        store16(B <= WT_MAX_B, z1part, (((int64_t)split * B + b) * NH + wc + 16 * j + 4 * kg) * 4, acc[i][j]);
    }
  }
}

void launch_fc1_fwd(const uint16_t* p, const uint16_t* w1, float* z1part, int B, hipStream_t s) {
  if (fc1_ksplit(B) == FC1_KSPLIT_BIG) {
    hipLaunchKernelGGL(fc1_fwd_big_kernel, dim3((B + F1B_ROWS - 1) / F1B_ROWS, FC1_KSPLIT_BIG), dim3(256), 0, s,
                       p, w1, z1part, B);
    return;
  }
  // two 16-row tiles per workgroup (MR = 2; measured B = 200 75.6-77.0 -> 73.8-74.7 us/step against
  // MR = 1, B = 300 97.0-97.2 -> 95.6-96.3; MR = 4 was slower: docs/PERF_NOTES.md)
  hipLaunchKernelGGL(fc1_fwd_kernel<2>, dim3((B + 31) / 32, FC1_KSPLIT), dim3(256), 0, s, p, w1, z1part, B);
}

// ============================================================================================
// Head (one wave per batch row; lane owns hidden units o = lane and lane + 64)
// ============================================================================================
namespace {
struct HeadRow {
  float z[2], h[2];
  bool keep[2];
  float logit[NCLS];
};

__device__ __forceinline__ void head_forward_row(const HeadArgs& a, int B, int b, int lane, bool train,
                                                 bool no_dropout, uint64_t seed, uint64_t off, HeadRow& r) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = lane + 64 * j;
    float z = a.b_fc1[o];
    // torch adds the bias after the GEMM; the partial sums are accumulated in fixed chunk order
    float s = 0.f;
    if (fc1_ksplit(B) == FC1_KSPLIT) {
#pragma unroll
      for (int c = 0; c < FC1_KSPLIT; ++c) s += a.z1part[((int64_t)c * B + b) * NH + o];
    } else {
#pragma unroll
      for (int c = 0; c < FC1_KSPLIT_BIG; ++c) s += a.z1part[((int64_t)c * B + b) * NH + o];
    }
    z += s;
    r.z[j] = z;
    float h = fmaxf(z, 0.0f);
    bool keep = true;
    if (train) {
      if (!no_dropout) {
        const u32x4 w = dropout_block(seed, off, ((uint64_t)b * NH + o) >> 4);
        keep = dropout_byte(w, o & 15) < KEEP2_THR8;
      }
      h = keep ? (no_dropout ? h : h * (1.0f / KEEP2)) : 0.0f;
    }
    r.keep[j] = keep;
    r.h[j] = h;
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float v = r.h[0] * a.w_fc2[c * NH + lane] + r.h[1] * a.w_fc2[c * NH + lane + 64];
    r.logit[c] = wave_sum(v) + a.b_fc2[c];
  }
}

// torch log_softmax: (x - max) - log(sum(exp(x - max)))
__device__ __forceinline__ void log_softmax10(const float* x, float* lp) {
  float mx = x[0];
#pragma unroll
  for (int c = 1; c < NCLS; ++c) mx = fmaxf(mx, x[c]);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) se += expf(x[c] - mx);
  const float lse = logf(se);
#pragma unroll
  for (int c = 0; c < NCLS; ++c) lp[c] = (x[c] - mx) - lse;
}
}  // namespace

// Training head.  Every load of the row is issued up front - the KS split-K partial sums, fc1 bias,
// fc2 weights and bias, the label - with no load under a branch (IDX / KS are template parameters):
// a branch-guarded load ends in vmcnt(0), which used to finish the label + bias round trip before
// the partial-sum loads even went out.  Arithmetic (order and expression forms) is that of
// head_forward_row / the module head, so the results are bitwise unchanged.
// One wave = one batch row b.
template <int KS, bool IDX>
__device__ __forceinline__ void head_train_row(const HeadArgs& a, int B, int b, int lane) {
  if (b >= B) {  // padding rows of the bf16 operands consumed by the backward GEMMs
    a.dz1[(int64_t)b * NH + lane] = 0;
    a.dz1[(int64_t)b * NH + lane + 64] = 0;
    a.h_bf[(int64_t)b * NH + lane] = 0;
    a.h_bf[(int64_t)b * NH + lane + 64] = 0;
    if (lane < 16) a.dl_bf[(int64_t)b * 16 + lane] = 0;
    return;
  }
  const int step = a.state->step;
  const uint64_t seed = a.state->seed;
  const uint64_t off = a.state->rng_base + 2ull * (uint64_t)step + 1ull;
  const bool no_drop = (a.state->flags & STEP_FLAG_NO_DROPOUT) != 0;
  const int64_t lrow = (int64_t)step * a.idx_step_stride + b;     // !IDX: pre-gathered labels
  const int32_t* lab = a.labels ? a.labels : &g_zero_state.step;   // module API (dlogp): no labels
  int64_t li = lrow;
  if constexpr (IDX) li = a.idx[lrow];
  const int y_raw = lab[a.labels ? li : 0];
  float part[KS][2], bf1[2], w2v[NCLS][2];
#pragma unroll
  for (int c = 0; c < KS; ++c)
#pragma unroll
    for (int j = 0; j < 2; ++j) part[c][j] = a.z1part[((int64_t)c * B + b) * NH + lane + 64 * j];
#pragma unroll
  for (int j = 0; j < 2; ++j) bf1[j] = a.b_fc1[lane + 64 * j];
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
#pragma unroll
    for (int j = 0; j < 2; ++j) w2v[c][j] = a.w_fc2[c * NH + lane + 64 * j];
  HeadRow r;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = lane + 64 * j;
    float z = bf1[j];
    float s = 0.f;                                   // partial sums in fixed chunk order
#pragma unroll
    for (int c = 0; c < KS; ++c) s += part[c][j];
    z += s;
    r.z[j] = z;
    float h = fmaxf(z, 0.0f);
    bool keep = true;
    if (!no_drop) {
      const u32x4 w = dropout_block(seed, off, ((uint64_t)b * NH + o) >> 4);
      keep = dropout_byte(w, o & 15) < KEEP2_THR8;
    }
    h = keep ? (no_drop ? h : h * (1.0f / KEEP2)) : 0.0f;
    r.keep[j] = keep;
    r.h[j] = h;
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float v = r.h[0] * w2v[c][0] + r.h[1] * w2v[c][1];
    r.logit[c] = wave_sum(v) + a.b_fc2[c];
  }
  float lp[NCLS];
  log_softmax10(r.logit, lp);
  float dl[NCLS];
  if (a.dlogp) {
    // module API: generic log_softmax backward  dl = go - exp(lp) * sum(go)
    float go[NCLS], sg = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) { go[c] = a.dlogp[(int64_t)b * NCLS + c]; sg += go[c]; }
#pragma unroll
    for (int c = 0; c < NCLS; ++c) dl[c] = go[c] - expf(lp[c]) * sg;
  } else {
    const int y = y_raw;
    if (lane == 0) a.loss_rows[b] = -lp[y];
    // nll(mean) backward: go[c] = -[c==y]/B; log_softmax backward: go - exp(lp) * sum(go)
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      const float go = (c == y) ? -a.inv_batch : 0.0f;
      dl[c] = go - expf(lp[c]) * (-a.inv_batch);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = lane + 64 * j;
    float dh = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) dh = __builtin_fmaf(dl[c], w2v[c][j], dh);
    const float dz = (r.keep[j] && r.z[j] > 0.0f) ? (no_drop ? dh : dh * (1.0f / KEEP2)) : 0.0f;
    a.dz1[(int64_t)b * NH + o] = f2bf(dz);
    a.h_bf[(int64_t)b * NH + o] = f2bf(r.h[j]);
  }
  if (lane < 16) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) v = (lane == c) ? dl[c] : v;
    a.dl_bf[(int64_t)b * 16 + lane] = f2bf(v);
  }
}

template <int KS, bool IDX>
__global__ __launch_bounds__(256) void head_train_kernel(HeadArgs a, int B) {
  TL_SCOPE(TL_HEAD);
  RW_ENTRY();
  head_train_row<KS, IDX>(a, B, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void head_eval_kernel(HeadArgs a, int B) {
  RW_ENTRY();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  const int y = a.labels ? a.labels[a.idx ? a.idx[b] : b] : -1;   // issued before the partial sums
  HeadRow r;
  head_forward_row(a, B, b, lane, false, true, 0, 0, r);
  float lp[NCLS];
  log_softmax10(r.logit, lp);
  if (lane == 0) {
    int am = 0;
#pragma unroll
    for (int c = 1; c < NCLS; ++c) am = (lp[c] > lp[am]) ? c : am;
    if (a.loss_rows) a.loss_rows[b] = (y >= 0) ? -lp[y] : 0.0f;
    if (a.correct_out) a.correct_out[b] = (am == y) ? 1 : 0;
  }
  if (a.logp_out && lane < NCLS) {
    float v = lp[0];
#pragma unroll
    for (int c = 1; c < NCLS; ++c) v = (lane == c) ? lp[c] : v;
    a.logp_out[(int64_t)b * NCLS + lane] = v;
  }
}

// module API forward: log-probs (train: with dropout-2 drawn from StepState exactly as head_train does)
__global__ __launch_bounds__(256) void head_fwd_kernel(HeadArgs a, int B, int train) {
  RW_ENTRY();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  const bool no_drop = !train || (a.state->flags & STEP_FLAG_NO_DROPOUT) != 0;
  const uint64_t seed = a.state ? a.state->seed : 0;
  const uint64_t off = a.state ? a.state->rng_base + 2ull * (uint64_t)a.state->step + 1ull : 0;
  HeadRow r;
  head_forward_row(a, B, b, lane, train != 0, no_drop, seed, off, r);
  float lp[NCLS];
  log_softmax10(r.logit, lp);
  if (lane < NCLS) {
    float v = lp[0];
#pragma unroll
    for (int c = 1; c < NCLS; ++c) v = (lane == c) ? lp[c] : v;
    a.logp_out[(int64_t)b * NCLS + lane] = v;
  }
}

void launch_head_fwd(const HeadArgs& a, int B, bool train, hipStream_t s) {
  hipLaunchKernelGGL(head_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, B, train ? 1 : 0);
}

// One row (wave) per workgroup: the 224 one-wave workgroups spread the rows' partial-sum loads
// (16 KB each) over 224 CUs instead of 4 rows on each of 56 - the head is a per-row latency chain,
// and its load phase shortened: B = 200, 600 steps, same box interleaved 61.04-61.47 -> 60.37-60.89
// us/step over 5 rounds (profiles/r6/ab/head_rows/; round 2's 1 / 2 / 4 rows per workgroup read
// 82.9 / 82.1 / 82.2 on that step).  Same rows, same math: bitwise the same results.
void launch_head_train(const HeadArgs& a, int B, int Bp, hipStream_t s) {
  const dim3 g(Bp), t(64);   // (Bp is a multiple of 32)
  if (fc1_ksplit(B) == FC1_KSPLIT) {
    if (a.idx) hipLaunchKernelGGL((head_train_kernel<FC1_KSPLIT, true>), g, t, 0, s, a, B);
    else hipLaunchKernelGGL((head_train_kernel<FC1_KSPLIT, false>), g, t, 0, s, a, B);
  } else {
    if (a.idx) hipLaunchKernelGGL((head_train_kernel<FC1_KSPLIT_BIG, true>), g, t, 0, s, a, B);
    else hipLaunchKernelGGL((head_train_kernel<FC1_KSPLIT_BIG, false>), g, t, 0, s, a, B);
  }
}
void launch_head_eval(const HeadArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(head_eval_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, B);
}

// ============================================================================================
// Margin head: head_train's forward in inference semantics (no StepState, no dropout, labels given per
// row) with a margin loss on the logits in place of log_softmax + NLL: the CW margin, the DLR loss of
// Croce & Hein (2020) and its targeted form (kernels.h HeadMarginArgs has the formulas).  The losses are
// shift-invariant, so no log-softmax is taken.  Same structure as head_train_row: one wave = one batch
// row, every load of the row issued up front and none under a branch (KS and the loss kind are template
// parameters); z1, h and the logits in head_train's expression forms and chunk order, so they carry the
// bits head_train gives with dropout off.  The loss part is rounded operation by operation (contraction
// off).  The ten-element selections are selects over unrolled loops - no dynamically indexed array, so
// the logits and dl stay in registers.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), KS = 32 / KS = 4:
//   head_margin_kernel<KS, CW>:    VGPRs 75 / 44, SGPRs 46 / 46, LDS 0 B, scratch 0, occupancy 6 / 8 waves / SIMD
//   head_margin_kernel<KS, DLR>:   VGPRs 76 / 46, SGPRs 54 / 54, LDS 0 B, scratch 0, occupancy 6 / 8 waves / SIMD
//   head_margin_kernel<KS, DLR_T>: VGPRs 76 / 48, SGPRs 72 / 72, LDS 0 B, scratch 0, occupancy 6 / 8 waves / SIMD
// (head_train_kernel<32, false>: VGPRs 114, occupancy 4.)  mg_at starts its select chain at 0 and class 0, the form
// of the dl_bf column pick: started at z[0] and class 1 the compiler turned the chain into an indexed read of a
// ten-float array that it placed in LDS (2560 B a workgroup).
// ============================================================================================
namespace {
// class i as a bit of mg_first_max's `taken` (i outside [0, 10): no bit)
__device__ __forceinline__ unsigned mg_bit(int i) { return (unsigned)i < (unsigned)NCLS ? 1u << i : 0u; }
// z[i] by selects (i outside [0, 10): 0)
__device__ __forceinline__ float mg_at(const float (&z)[NCLS], int i) {
  float v = 0.0f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) v = (i == c) ? z[c] : v;
  return v;
}
// The first maximum of z over the classes whose bit in `taken` is clear: explicit > in ascending class
// order, the first of equals wins (a NaN never wins over an earlier class).  Returns the class, its
// logit in `best`.
__device__ __forceinline__ int mg_first_max(const float (&z)[NCLS], unsigned taken, float& best) {
  int idx = -1;
  best = 0.0f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const bool take = !((taken >> c) & 1u) && (idx < 0 || z[c] > best);
    best = take ? z[c] : best;
    idx = take ? c : idx;
  }
  return idx;
}
// dl[i] += v
__device__ __forceinline__ void mg_add(float (&dl)[NCLS], int i, float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < NCLS; ++c) dl[c] = (i == c) ? dl[c] + v : dl[c];
}

// loss L and d L * s / d z of one row from its logits (kernels.h HeadMarginArgs)
template <int KIND>
__device__ __forceinline__ float margin_loss(const float (&z)[NCLS], int y, int t, float s, float (&dl)[NCLS]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < NCLS; ++c) dl[c] = 0.0f;
  const float zy = mg_at(z, y);
  if constexpr (KIND == MARGIN_CW) {
    float zo;
    const int o = mg_first_max(z, mg_bit(y), zo);
    mg_add(dl, o, s);
    mg_add(dl, y, -s);
    return zo - zy;
  } else {
    float z1, z2, z3, z4;
    const int p1 = mg_first_max(z, 0u, z1);
    const int p2 = mg_first_max(z, mg_bit(p1), z2);
    const int p3 = mg_first_max(z, mg_bit(p1) | mg_bit(p2), z3);
    if constexpr (KIND == MARGIN_DLR) {
      float zo;
      const int o = mg_first_max(z, mg_bit(y), zo);
      const float d = (z1 - z3) + 1e-12f;
      const float L = (zo - zy) / d;
      const float g = s / d;
      mg_add(dl, o, g);
      mg_add(dl, y, -g);
      const float q = (s * L) / d;
      mg_add(dl, p1, -q);
      mg_add(dl, p3, q);
      return L;
    } else {
      const int p4 = mg_first_max(z, mg_bit(p1) | mg_bit(p2) | mg_bit(p3), z4);
      const float zt = mg_at(z, t);
      const float d = (z1 - 0.5f * (z3 + z4)) + 1e-12f;
      const float L = (zy - zt) / d;
      const float g = s / d;
      mg_add(dl, y, g);
      mg_add(dl, t, -g);
      const float q = (s * L) / d;
      const float hq = 0.5f * q;
      mg_add(dl, p1, -q);
      mg_add(dl, p3, hq);
      mg_add(dl, p4, hq);
      return L;
    }
  }
}
}  // namespace

template <int KS, int KIND>
__global__ __launch_bounds__(64) void head_margin_kernel(HeadMarginArgs a, int B) {
  RW_ENTRY();
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  if (b >= B) {  // padding rows of the bf16 operands consumed by the backward GEMMs
    a.dz1[(int64_t)b * NH + lane] = 0;
    a.dz1[(int64_t)b * NH + lane + 64] = 0;
    a.h_bf[(int64_t)b * NH + lane] = 0;
    a.h_bf[(int64_t)b * NH + lane + 64] = 0;
    if (lane < 16) a.dl_bf[(int64_t)b * 16 + lane] = 0;
    return;
  }
  const int y = a.labels[b];
  int t = 0;
  if constexpr (KIND == MARGIN_DLR_T) t = a.targets[b];
  float part[KS][2], bf1[2], w2v[NCLS][2], bf2[NCLS];
#pragma unroll
  for (int c = 0; c < KS; ++c)
#pragma unroll
    for (int j = 0; j < 2; ++j) part[c][j] = a.z1part[((int64_t)c * B + b) * NH + lane + 64 * j];
#pragma unroll
  for (int j = 0; j < 2; ++j) bf1[j] = a.b_fc1[lane + 64 * j];
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
#pragma unroll
    for (int j = 0; j < 2; ++j) w2v[c][j] = a.w_fc2[c * NH + lane + 64 * j];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) bf2[c] = a.b_fc2[c];
  float z1[2], h[2], logit[NCLS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float z = bf1[j];
    float s = 0.f;                                   // partial sums in fixed chunk order
#pragma unroll
    for (int c = 0; c < KS; ++c) s += part[c][j];
    z += s;
    z1[j] = z;
    h[j] = fmaxf(z, 0.0f);
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float v = h[0] * w2v[c][0] + h[1] * w2v[c][1];
    logit[c] = wave_sum(v) + bf2[c];
  }
  float dl[NCLS];
  const float L = margin_loss<KIND>(logit, y, t, a.scale, dl);
  if (lane == 0) a.loss_rows[b] = L;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = lane + 64 * j;
    float dh = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) dh = __builtin_fmaf(dl[c], w2v[c][j], dh);
    const float dz = (z1[j] > 0.0f) ? dh : 0.0f;
    a.dz1[(int64_t)b * NH + o] = f2bf(dz);
    a.h_bf[(int64_t)b * NH + o] = f2bf(h[j]);
  }
  if (lane < 16) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) v = (lane == c) ? dl[c] : v;
    a.dl_bf[(int64_t)b * 16 + lane] = f2bf(v);
  }
}

void launch_head_margin(const HeadMarginArgs& a, int B, int Bp, int kind, hipStream_t s) {
  if (kind != MARGIN_CW && kind != MARGIN_DLR && kind != MARGIN_DLR_T)
    throw std::runtime_error("head_margin: unknown loss code");
  if (!a.z1part || !a.b_fc1 || !a.w_fc2 || !a.b_fc2 || !a.labels || !a.loss_rows || !a.dz1 || !a.h_bf || !a.dl_bf)
    throw std::runtime_error("head_margin: null argument");
  if (kind == MARGIN_DLR_T && !a.targets)
    throw std::runtime_error("head_margin: null argument (the targeted DLR loss needs the targets)");
  if (B <= 0) throw std::runtime_error("head_margin: row count out of range");
  if (Bp % 32 != 0 || Bp < B) throw std::runtime_error("head_margin: Bp must be a multiple of 32 that is >= B");
  if (misaligned(3, a.z1part, a.b_fc1, a.w_fc2, a.b_fc2, a.loss_rows) || misaligned(3, a.labels, a.targets))
    throw std::runtime_error("head_margin: the fp32 and int32 arrays must be 4-byte aligned");
  if (misaligned(1, a.dz1, a.h_bf, a.dl_bf)) throw std::runtime_error("head_margin: the bf16 rows must be 2-byte aligned");
  const dim3 g(Bp), t(64);   // one row (wave) per workgroup, as head_train
#define HM_LAUNCH(KS)                                                                                       \
  switch (kind) {                                                                                           \
    case MARGIN_CW: hipLaunchKernelGGL((head_margin_kernel<KS, MARGIN_CW>), g, t, 0, s, a, B); break;       \
    case MARGIN_DLR: hipLaunchKernelGGL((head_margin_kernel<KS, MARGIN_DLR>), g, t, 0, s, a, B); break;     \
    default: hipLaunchKernelGGL((head_margin_kernel<KS, MARGIN_DLR_T>), g, t, 0, s, a, B); break;           \
  }
  if (fc1_ksplit(B) == FC1_KSPLIT) HM_LAUNCH(FC1_KSPLIT) else HM_LAUNCH(FC1_KSPLIT_BIG)
#undef HM_LAUNCH
}

// ============================================================================================
// fc backward, three workgroup roles in one launch:
//   A (145 WGs): dW_fc1[o][i] = sum_b dz1[b][o] p[b][i]  (M=128, N=64 per WG, K=B); WG 144 computes
//                db_fc1 = dz1^T * ones.  Both operands are k(=batch)-major in memory, so each
//                32-row k-slab is staged in LDS and read with ds_read_b64_tr_b16 (hardware transpose).
//   B (ceil(B/16)*36 WGs): dy = unpool((dz1 . w1) * dropout-1 / ReLU mask) as dense NHWC bf16 (M=B, N=9216, K=128)
//   C (1 WG): dW_fc2 = dl^T h, db_fc2 = dl^T 1 (MFMA, 4 waves split K, LDS reduce) + mean loss.
// ============================================================================================
namespace {
constexpr int ROLE_A_WGS = NFLAT / 64 + 1;   // 145
// k(=batch)-major LDS tiles read with ds_read_b64_tr_b16: one instruction touches rows
// {8g+q (+4)} x one 32-B column segment per row, so without a swizzle every row of a 256-B
// (128-B) row pitch lands on the same banks (8-way / 4-way).  XOR the 32-B segment index
// (16 bf16) with a row code that is distinct over those 8 rows (gfx950: 2 x 32-lane groups,
// bank = dword mod 64).  Writes (16-B chunks) apply the same map.
__device__ __forceinline__ int swz_row256(int row, int col) {   // 128 bf16 per row, 8 segments
  const int code = (row & 3) | (((row >> 3) & 1) << 2);
  return (((col >> 4) ^ code) << 4) | (col & 15);
}
__device__ __forceinline__ int swz_row128(int row, int col) {   // 64 bf16 per row, 4 segments x 2 halves
  const int code = ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
  return (((col >> 4) ^ code) << 4) | (col & 15);
}
constexpr int ROLE_B_SBLOCKS = NPOOL / 4;    // 36 blocks of 4 pooled positions (one third of a row)

// Adadelta step of one element whose gradient g is final (fc1 bias, fc2): grad buffer, param, state
__device__ __forceinline__ void ada_elem(const AdadeltaArgs& u, const Ada& ad, int64_t e, float g) {
  float p = u.param[e], sq = u.square_avg[e], ac = u.acc_delta[e];
  const_cast<float*>(u.grad)[e] = g;               // (the engine grad buffer, = FcBwdArgs::grad)
  ad.step(p, g, sq, ac);
  u.param[e] = p;
  u.square_avg[e] = sq;
  u.acc_delta[e] = ac;
}

// fused update epilogue of a role-A tile (grad_scale 1: the engine's head carries 1/B); acc[mt][nt]:
// lane (l & 15, g) of wave w holds columns i0 + 16 nt + 4 g + r of row o = 32 w + 16 mt + (l & 15)
__device__ __forceinline__ void fc_role_a_update(const AdadeltaArgs& u, const floatx4 (&acc)[2][4], bool ones, int i0,
                                                 unsigned char* smem) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4;
  const Ada ad{u.rho, u.eps, u.weight_decay, *u.lr};
  if (ones) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((lane & 15) == 0) ada_elem(u, ad, OFF_FC1_B + 32 * wave + 16 * mt + 4 * g + r, acc[mt][0][r]);
    return;
  }
  constexpr int TR = 72, TT = 136;                     // padded LDS rows: w1 tile [128 o][64 i], w1t [64 i][128 o]
  uint16_t* tr = reinterpret_cast<uint16_t*>(smem);
  uint16_t* tt = reinterpret_cast<uint16_t*>(smem + 128 * TR * 2);
  __syncthreads();                                     // every wave's last MFMA operand reads are done
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int ol = 32 * wave + 16 * mt + (lane & 15);
    float4 pp[4], sq[4], ac[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {                   // all loads of the half-tile first
      const int64_t e = OFF_FC1_W + (int64_t)ol * NFLAT + i0 + 16 * nt + 4 * g;
      pp[nt] = *reinterpret_cast<const float4*>(u.param + e);
      sq[nt] = *reinterpret_cast<const float4*>(u.square_avg + e);
      ac[nt] = *reinterpret_cast<const float4*>(u.acc_delta + e);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int il = 16 * nt + 4 * g;
      const int64_t e = OFF_FC1_W + (int64_t)ol * NFLAT + i0 + il;
      const floatx4 gv = acc[mt][nt];
      store16(u.wt, u.grad, e * 4, gv);
      ad.step(pp[nt].x, gv[0], sq[nt].x, ac[nt].x);
      ad.step(pp[nt].y, gv[1], sq[nt].y, ac[nt].y);
      ad.step(pp[nt].z, gv[2], sq[nt].z, ac[nt].z);
      ad.step(pp[nt].w, gv[3], sq[nt].w, ac[nt].w);
      store16(u.wt, u.param, e * 4, make_floatx4(pp[nt]));
      store16(u.wt, u.square_avg, e * 4, make_floatx4(sq[nt]));
      store16(u.wt, u.acc_delta, e * 4, make_floatx4(ac[nt]));
      const float v[4] = {pp[nt].x, pp[nt].y, pp[nt].z, pp[nt].w};
      *reinterpret_cast<uint2*>(tr + ol * TR + il) = uint2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
#pragma unroll
      for (int r = 0; r < 4; ++r) tt[(il + r) * TT + ol] = f2bf(v[r]);
    }
  }
  lds_barrier();
#pragma unroll
  for (int k = 0; k < 4; ++k) {                        // w1: 128 rows x 128 B, w1t: 64 rows x 256 B
    const int c = tid + 256 * k;
    const int o = c >> 3, ic = (c & 7) * 8;
    store16(u.wt, u.w1, ((int64_t)o * NFLAT + i0 + ic) * 2, *reinterpret_cast<const uint4*>(tr + o * TR + ic));
    const int il = c >> 4, oc = (c & 15) * 8;
    store16(u.wt, u.w1t, ((int64_t)(i0 + il) * NH + oc) * 2, *reinterpret_cast<const uint4*>(tt + il * TT + oc));
  }
}

// A: dW_fc1 tile [128 o][64 i] over K = batch.  Register-prefetch pipeline: the next 32-row k-slab is
// loaded into VGPRs while the current one feeds the MFMAs.  DB: double-buffered LDS (24 KB), one
// barrier per slab; !DB: one 12-KB buffer and a second barrier (fc_bwd_dw1_kernel, which must fit
// beside two conv2_dgrad workgroups' 140 KB of LDS).  The same MFMA order either way.
// UPD (single GPU, S == 1, fc_wgrad_update_kernel): the epilogue also applies the Adadelta step to the
// tile (gradient -> grad buffer, param / square_avg / acc_delta, bf16 shadows w1 and w1t staged through
// LDS for 16-B stores) - per element the same math as adadelta_kernel's fc1_tile, so the same bits.
template <bool DB = true, bool UPD = false>
__device__ __forceinline__ void fc_bwd_role_a(const FcBwdArgs& a, int B, int Bp, int ib, int sp, int S,
                                              unsigned char* smem, const AdadeltaArgs* up = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const bool ones = (ib == NFLAT / 64);
  const int i0 = ones ? 0 : ib * 64;
  floatx4 acc[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8 onesfrag;
  {
    const uint16_t one = ((lane & 15) == 0) ? 0x3F80 : 0;
    typedef __attribute__((ext_vector_type(8))) unsigned short us8;
    us8 v = {one, one, one, one, one, one, one, one};
    onesfrag = __builtin_bit_cast(bf16x8, v);
  }
  // this split's k(=batch) blocks of 32 rows
  const int kb0 = sp * (FC_BWD_SPLIT_ROWS / 32);
  const int kb1 = min(Bp / 32, kb0 + FC_BWD_SPLIT_ROWS / 32);
  const int prow = tid >> 3, pc8 = tid & 7;
  uint4 rz0, rz1, rp = {0u, 0u, 0u, 0u};
  auto fetch = [&](int kb) {
    rz0 = *reinterpret_cast<const uint4*>(a.dz1 + (int64_t)(kb * 32 + (tid >> 4)) * NH + (tid & 15) * 8);
    rz1 = *reinterpret_cast<const uint4*>(a.dz1 + (int64_t)(kb * 32 + 16 + (tid >> 4)) * NH + (tid & 15) * 8);
    const int b = kb * 32 + prow;
    rp = uint4{0u, 0u, 0u, 0u};
    if (!ones && b < B) rp = *reinterpret_cast<const uint4*>(a.p + (int64_t)b * NFLAT + i0 + pc8 * 8);
  };
  fetch(kb0);
  for (int kb = kb0; kb < kb1; ++kb) {
    const int buf = DB ? (kb & 1) : 0;
    uint16_t* dzs = reinterpret_cast<uint16_t*>(smem + buf * 12288);          // [32][128]
    uint16_t* ps = reinterpret_cast<uint16_t*>(smem + buf * 12288 + 8192);    // [32][64]
    {
      const int r0 = tid >> 4, r1 = 16 + (tid >> 4), c = (tid & 15) * 8;
      *reinterpret_cast<uint4*>(dzs + r0 * 128 + swz_row256(r0, c)) = rz0;
      *reinterpret_cast<uint4*>(dzs + r1 * 128 + swz_row256(r1, c)) = rz1;
      *reinterpret_cast<uint4*>(ps + prow * 64 + swz_row128(prow, pc8 * 8)) = rp;
    }
    if (kb + 1 < kb1) fetch(kb + 1);
    __syncthreads();
    const int rlo = 8 * g + q, rhi = rlo + 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int ob = 32 * wave + 16 * mt + 4 * pp;
      const bf16x8 A = tr_frag(dzs + rlo * 128 + swz_row256(rlo, ob), dzs + rhi * 128 + swz_row256(rhi, ob));
      if (ones) {
        acc[mt][0] = mfma16x16x32(A, onesfrag, acc[mt][0]);
      } else {
        // dW1^T tiles (p fragments as the A operand): lane (l & 15, g) ends with columns
        // i0 + 16 nt + 4 g + r (r = 0..3) of row o = 32 wave + 16 mt + (l & 15) - one 16-B store
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int nb = 16 * nt + 4 * pp;
          const bf16x8 Bf = tr_frag(ps + rlo * 64 + swz_row128(rlo, nb), ps + rhi * 64 + swz_row128(rhi, nb));
          acc[mt][nt] = mfma16x16x32(Bf, A, acc[mt][nt]);
        }
      }
    }
    if (!DB) __syncthreads();                          // the next slab rewrites the one buffer
  }
  // S == 1: final (scaled) gradient (write-through at small batches: read by the fc update only);
  // S > 1: unscaled partial in the same layout (fc_grad_reduce)
  float* dst = (S == 1) ? a.grad : a.part + (int64_t)sp * FCB_PART_STRIDE;
  const float sc = (S == 1) ? a.grad_scale : 1.0f;
  if constexpr (UPD) {
    fc_role_a_update(*up, acc, ones, i0, smem);
    return;
  }
  if (ones) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((lane & 15) == 0) dst[OFF_FC1_B + 32 * wave + 16 * mt + 4 * g + r] = acc[mt][0][r] * sc;
  } else {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int o = 32 * wave + 16 * mt + (lane & 15);
        const floatx4 v = {acc[mt][nt][0] * sc, acc[mt][nt][1] * sc, acc[mt][nt][2] * sc, acc[mt][nt][3] * sc};
        store16(S == 1 && B <= WT_MAX_B, dst, (OFF_FC1_W + (int64_t)o * NFLAT + i0 + 16 * nt + 4 * g) * 4, v);
      }
  }
}

// B: gradient into the conv trunk.  WG = 16 batch rows x 4 consecutive pooled positions x 64 channels
// (N = 256 columns of dz1 . w1).  The epilogue applies dropout-1 scale/keep and the ReLU (pooled > 0)
// and writes the *compact* un-pooled gradient: one DYC_REC (144-B) record per (image, pooled
// position) = 64 bf16 pooled gradients (DYC_ROUTE = 128 B) + the 2-bit argmax codes as two bit planes
// per 8-channel chunk (16 B; layout in kernels.h next to DYC_REC / DYC_ROUTE).  The conv backward
// kernels expand it into the dense NHWC tile while staging, so the 75 %-zero dense map never touches
// HBM.
template <bool CACHE_W>
__device__ __forceinline__ void fc_bwd_role_b(const FcBwdArgs& a, int B, int Bp, int rb, int MR,
                                              unsigned char* smem) {
  uint8_t* pms = smem;                                 // [16 b][64 c][4 j]
  unsigned char* recs = smem + 4096;                   // [16 b][4 j] records of DYC_REC bytes
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, kg = lane >> 4;
  const int bb = rb / ROLE_B_SBLOCKS, sb = rb - bb * ROLE_B_SBLOCKS;
  const int s0 = sb * 4;                               // 4 consecutive pooled positions (row-major 12x12)
  const StepState* st = a.state ? a.state : &g_zero_state;   // unconditional load (no vmcnt(0) join)
  const float dscale = (st->flags & STEP_FLAG_NO_DROPOUT) ? 1.0f : (1.0f / KEEP1);
  // large batches (CACHE_W): this wave's w1 slice (pooled position s0 + wave, 64 channels, K = 128)
  // stays in VGPRs for all MR row tiles of the workgroup; small batches (MR = 1) stream it, which
  // keeps the kernel at 3 workgroups per CU
  bf16x8 Bw[CACHE_W ? NH / 32 : 1][4];
  if (CACHE_W) {
#pragma unroll
    for (int ks = 0; ks < (CACHE_W ? NH / 32 : 1); ++ks)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        Bw[ks][nt] = ld16(a.w1t + (int64_t)((16 * nt + m) * NPOOL + s0 + wave) * NH + ks * 32 + 8 * kg);
  }
  // The next row tile's pmask words and dz1 fragments are loaded under this tile's MFMAs and
  // record epilogue (the tiles of a workgroup ran back to back, each paying a full HBM round trip
  // first: role B alone 98.5 us at B = 8192), and the tile barriers are LDS-only (lds_barrier) so
  // that prefetch stays in flight across them.
  // Every load of a tile is unconditional (clamped row, value masked after): loads under a branch
  // each end in vmcnt(0), which turned the tile's staging into dependent round trips.
  uint32_t pmv[4];
  bf16x8 Af[NH / 32];
  auto tile_loads = [&](int b0, uint32_t (&pm)[4], bf16x8 (&af)[NH / 32]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 256 * k, bl = idx >> 6, c = idx & 63;
      const int row = b0 + bl < B ? b0 + bl : B - 1;
      pm[k] = *reinterpret_cast<const uint32_t*>(a.pmask + (int64_t)row * NFLAT + ((s0 >> 2) * C2 + c) * 4);
    }
    const int arow_b = b0 + m < Bp ? b0 + m : Bp - 1;   // rows < Bp: zero padding rows
    const uint16_t* arow = a.dz1 + (int64_t)arow_b * NH + 8 * kg;
#pragma unroll
    for (int ks = 0; ks < NH / 32; ++ks) af[ks] = ld16(arow + ks * 32);
  };
  tile_loads(bb * MR * 16, pmv, Af);
  for (int t = 0; t < MR; ++t) {
    const int b0 = (bb * MR + t) * 16;
    if (b0 >= B) break;                                // workgroup-uniform
    bf16x8 Bs[CACHE_W ? 1 : NH / 32][4];
    if (!CACHE_W) {
#pragma unroll
      for (int ks = 0; ks < NH / 32; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          Bs[CACHE_W ? 0 : ks][nt] = ld16(a.w1t + (int64_t)((16 * nt + m) * NPOOL + s0 + wave) * NH + ks * 32 + 8 * kg);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 256 * k, bl = idx >> 6;
      reinterpret_cast<uint32_t*>(pms)[idx] = b0 + bl < B ? pmv[k] : 0u;
    }
    floatx4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NH / 32; ++ks) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 Bf = CACHE_W ? Bw[CACHE_W ? ks : 0][nt] : Bs[CACHE_W ? 0 : ks][nt];
        acc[nt] = mfma16x16x32(Af[ks], Bf, acc[nt]);
      }
    }
    const int nb0 = b0 + 16;
    if (t + 1 < MR && nb0 < B) tile_loads(nb0, pmv, Af);   // workgroup-uniform; in flight below
    lds_barrier();
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int bl = 4 * kg + r, c = 16 * nt + m;
        const int mk = pms[(bl * 64 + c) * 4 + wave];
        const float v = ((mk & 12) == 12) ? acc[nt][r] * dscale : 0.0f;   // kept by dropout, ReLU alive
        unsigned char* rec = recs + (bl * 4 + wave) * DYC_REC;
        reinterpret_cast<uint16_t*>(rec)[c] = f2bf(v);
        // argmax code bit planes: ballot bit 16 kg + m = channel 16 nt + m of row 4 kg + r, so the
        // 16-bit slice kg of each ballot is this row's planes of chunks 2 nt (low byte), 2 nt + 1
        const uint64_t p0 = __ballot(mk & 1), p1 = __ballot(mk & 2);
        if (m == 0) {
          const uint32_t w0 = (uint32_t)(p0 >> (16 * kg)), w1 = (uint32_t)(p1 >> (16 * kg));
          // bytes [plane 0, plane 1] of chunk 2 nt, then of chunk 2 nt + 1
          reinterpret_cast<uint32_t*>(rec + DYC_ROUTE)[nt] = __builtin_amdgcn_perm(w1, w0, 0x05010400u);
        }
      }
    lds_barrier();
    // 16 runs of 4 contiguous records (576 B) -> 36 x 16 B per image row
    constexpr int RUN16 = 4 * DYC_REC / 16;
    static_assert(RUN16 * 16 <= 3 * 256, "three 16-B chunks per thread");
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int cidx = tid + 256 * k, bl = cidx / RUN16, off = cidx - bl * RUN16;
      if (cidx < RUN16 * 16 && b0 + bl < B)   // write-through: the conv backward kernels read the records
        store16(B <= WT_MAX_B, a.dyc, ((int64_t)(b0 + bl) * NPOOL + s0) * DYC_REC + off * 16,
                   reinterpret_cast<const uint4*>(recs)[cidx]);
    }
    if (t + 1 < MR) lds_barrier();                     // pms / recs are rewritten by the next tile
  }
}

template <bool UPD = false>
__device__ __forceinline__ void fc_bwd_role_c(const FcBwdArgs& a, int B, int Bp, int sp, int S,
                                              unsigned char* smem, const AdadeltaArgs* up = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  uint16_t* hs = reinterpret_cast<uint16_t*>(smem + wave * 9216);          // [32][128]
  uint16_t* dls = reinterpret_cast<uint16_t*>(smem + wave * 9216 + 8192);  // [32][16]
  floatx4 acc[9];
#pragma unroll
  for (int nt = 0; nt < 9; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8 onesfrag;
  {
    const uint16_t one = ((lane & 15) == 0) ? 0x3F80 : 0;
    typedef __attribute__((ext_vector_type(8))) unsigned short us8;
    us8 v = {one, one, one, one, one, one, one, one};
    onesfrag = __builtin_bit_cast(bf16x8, v);
  }
  const int kb0 = sp * (FC_BWD_SPLIT_ROWS / 32);
  const int kb1 = min(Bp / 32, kb0 + FC_BWD_SPLIT_ROWS / 32);
  const int iters = (kb1 - kb0 + 3) / 4;
  for (int it = 0; it < iters; ++it) {
    const int kb = kb0 + it * 4 + wave;
    const bool active = kb < kb1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = lane + 64 * j, row = c >> 4, c16 = c & 15;
      uint4 v = {0u, 0u, 0u, 0u};
      if (active) v = *reinterpret_cast<const uint4*>(a.h_bf + (int64_t)(kb * 32 + row) * NH + c16 * 8);
      *reinterpret_cast<uint4*>(hs + row * 128 + swz_row256(row, c16 * 8)) = v;
    }
    {
      const int row = lane >> 1, c8 = lane & 1;
      uint4 v = {0u, 0u, 0u, 0u};
      if (active) v = *reinterpret_cast<const uint4*>(a.dl_bf + (int64_t)(kb * 32 + row) * 16 + c8 * 8);
      *reinterpret_cast<uint4*>(dls + row * 16 + c8 * 8) = v;
    }
    __syncthreads();
    const int rlo = 8 * g + q, rhi = rlo + 4;
    const bf16x8 A = tr_frag(dls + rlo * 16 + 4 * pp, dls + rhi * 16 + 4 * pp);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      const int nb = 16 * nt + 4 * pp;
      const bf16x8 Bf = tr_frag(hs + rlo * 128 + swz_row256(rlo, nb), hs + rhi * 128 + swz_row256(rhi, nb));
      acc[nt] = mfma16x16x32(A, Bf, acc[nt]);
    }
    acc[8] = mfma16x16x32(A, onesfrag, acc[8]);
    __syncthreads();
  }
  // cross-wave reduction through LDS: red[wave][nt][r][lane]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int nt = 0; nt < 9; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((wave * 9 + nt) * 4 + r) * 64 + lane] = acc[nt][r];
  __syncthreads();
  for (int e = tid; e < 9 * 4 * 64; e += 256) {
    const float s = red[e] + red[e + 2304] + red[e + 2 * 2304] + red[e + 3 * 2304];
    const int ln = e & 63, r = (e >> 6) & 3, nt = e >> 8;
    const int c = 4 * (ln >> 4) + r;        // row of the 16x16 output = class
    const int col = ln & 15;
    float* dst = (S == 1) ? a.grad : a.part + (int64_t)sp * FCB_PART_STRIDE;
    const float sc = (S == 1) ? a.grad_scale : 1.0f;
    const int64_t k = (c >= NCLS) ? -1 : (nt < 8) ? OFF_FC2_W + c * NH + 16 * nt + col : (col == 0) ? OFF_FC2_B + c : -1;
    if constexpr (UPD) {
      if (k >= 0) ada_elem(*up, Ada{up->rho, up->eps, up->weight_decay, *up->lr}, k, s * sc);
    } else {
      if (k >= 0) dst[k] = s * sc;
    }
  }
  if (wave == 0) {
    const int b_lo = sp * FC_BWD_SPLIT_ROWS, b_hi = min(B, b_lo + FC_BWD_SPLIT_ROWS);
    float s = 0.f;
    for (int b = b_lo + lane; b < b_hi; b += 64) s += a.loss_rows[b];
    s = wave_sum(s);
    if (lane == 0) {
      if (S == 1) {
        if (a.loss_log) a.loss_log[a.state->step] = s / (float)B;
      } else {
        a.part[(int64_t)sp * FCB_PART_STRIDE + FCB_PART_LOSS] = s;
      }
    }
  }
}
}  // namespace

__host__ __device__ inline int fc_bwd_role_b_wgs(int B) {
  const int rows16 = (B + 15) / 16, mr = fcb_mr(B);
  return ((rows16 + mr - 1) / mr) * ROLE_B_SBLOCKS;
}

// workgroups [C | A | B]; bid0 offsets a partial grid (launch_fc_bwd_role)
// roles: mask of FCB_ROLE_C / _A / _B; the grid covers the enabled roles' ranges in [C | A | B] order
// (the side schedules split the launch: weight gradients on the comm stream, role B on compute)
template <bool BIG>
__global__ __launch_bounds__(256, BIG ? 2 : 3) void fc_bwd_kernel(FcBwdArgs a, int B, int Bp, int bid0, int roles) {
  TL_SCOPE(TL_FC_BWD);
  __shared__ __attribute__((aligned(16))) unsigned char smem[4096 + 32768];
  if (a.signal_ctr && blockIdx.x == 0 && threadIdx.x == 0)
    (RW_SIGNAL(), __hip_atomic_fetch_add(a.signal_ctr, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT));
  RW_ENTRY();
  const int S = fc_bwd_splits(B);
  const int nA = S * ROLE_A_WGS;
  int bid = blockIdx.x + bid0;
  if (!(roles & FCB_ROLE_C)) bid += S;
  if (!(roles & FCB_ROLE_A) && bid >= S) bid += nA;
  // role C (long-running, one per split) first so it is dispatched before the short role-B tiles
  if (bid < S) {
    fc_bwd_role_c(a, B, Bp, bid, S, smem);
  } else if (bid < S + nA) {
    const int r = bid - S;
    fc_bwd_role_a(a, B, Bp, r % ROLE_A_WGS, r / ROLE_A_WGS, S, smem);
  } else {
    fc_bwd_role_b<BIG>(a, B, Bp, bid - S - nA, fcb_mr(B), smem);
  }
}

// Role A alone (large batches, side schedules): the fc1 weight gradient's split partials on the comm
// stream, beside conv2_wgrad / conv2_dgrad instead of on the compute chain.  It streams p once from
// HBM (151 MB at B = 8192) at ~11 % MFMA use, the complement of the conv kernels' LDS / MFMA-bound
// loops; 12 KB of LDS and <= 80 VGPRs (6 waves per SIMD) so that it fits beside both of them
// (dgrad: 2 x 70 KB LDS, 2 x 216 VGPRs per SIMD; wgrad: 89 KB, 2 x 208).  Bitwise the same partials.
__global__ __launch_bounds__(256, 6) void fc_bwd_dw1_kernel(FcBwdArgs a, int B, int Bp) {
  RW_ENTRY();
  __shared__ __attribute__((aligned(16))) unsigned char smem[12288];
  const int S = fc_bwd_splits(B);
  const int r = blockIdx.x;
  fc_bwd_role_a<false>(a, B, Bp, r % ROLE_A_WGS, r / ROLE_A_WGS, S, smem);
}

// Single-GPU OVERLAP chain, B <= 1024 (one split): the fc weight gradients (roles C + A, 146
// workgroups) with the fc Adadelta step fused into their epilogues, on the comm stream beside fc_bwd's
// role B and the conv backward - one launch instead of the gradient launch + adadelta_kernel(ADA_FC),
// no gradient round trip, each tile updated as soon as its gradient is final.  The completion hold
// (u.hold_*) is adadelta_kernel's: the conv2 update that follows on the stream starts after dgrad's start.
__global__ __launch_bounds__(256, 2) void fc_wgrad_update_kernel(FcBwdArgs a, AdadeltaArgs u, int B, int Bp) {
  TL_SCOPE(TL_ADA_FC);
  RW_ENTRY();
  __shared__ __attribute__((aligned(16))) unsigned char smem[4096 + 32768];
  if (blockIdx.x == 0) fc_bwd_role_c<true>(a, B, Bp, 0, 1, smem, &u);
  else fc_bwd_role_a<true, true>(a, B, Bp, blockIdx.x - 1, 0, 1, smem, &u);
  if (u.hold_a && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    spin_until_geq(u.hold_a, __hip_atomic_load(u.hold_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + u.hold_delta,
                   u.hold_err);
}

void launch_fc_wgrad_update(const FcBwdArgs& a, const AdadeltaArgs& u, int B, int Bp, hipStream_t s) {
  if (fc_bwd_splits(B) != 1 || a.grad_scale != 1.0f || u.grad != a.grad || u.state_inc || u.signal_start)
    throw std::runtime_error("fc_wgrad_update: one split, unit grad scale, the engine's grad buffer");
  hipLaunchKernelGGL(fc_wgrad_update_kernel, dim3(1 + ROLE_A_WGS), dim3(256), 0, s, a, u, B, Bp);
}

// S > 1: fixed-order sum of the split partials (fc1.w, fc1.b, fc2.w, fc2.b share the grad layout
// [0, OFF_FC2_B + 10)), scaled by grad_scale (1.0 from the engine: the head carries 1/(B*world)),
// plus the mean loss.
__global__ __launch_bounds__(256) void fc_grad_reduce_kernel(FcBwdArgs a, int B, int S) {
  TL_SCOPE(TL_FC_BWD);
  RW_ENTRY();
  constexpr int64_t N4 = (OFF_FC2_B + NCLS + 3) / 4;   // float4 columns (the tail pads into fc2.b's pad)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N4) {
    float4 t = reinterpret_cast<const float4*>(a.part)[i];
    for (int sp = 1; sp < S; ++sp) {
      const float4 u = reinterpret_cast<const float4*>(a.part + (int64_t)sp * FCB_PART_STRIDE)[i];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const float sc = a.grad_scale;
    const int64_t e = 4 * i;
    const float v[4] = {t.x * sc, t.y * sc, t.z * sc, t.w * sc};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e + k < OFF_FC2_B + NCLS) a.grad[e + k] = v[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.loss_log) {
    float s = 0.f;
    for (int sp = 0; sp < S; ++sp) s += a.part[(int64_t)sp * FCB_PART_STRIDE + FCB_PART_LOSS];
    a.loss_log[a.state->step] = s / (float)B;
  }
}



void launch_fc_grad_reduce(const FcBwdArgs& a, int B, hipStream_t s) {
  const int S = fc_bwd_splits(B);
  if (S <= 1) return;
  constexpr int64_t N4 = (OFF_FC2_B + NCLS + 3) / 4;
  hipLaunchKernelGGL(fc_grad_reduce_kernel, dim3((unsigned)((N4 + 255) / 256)), dim3(256), 0, s, a, B, S);
}

void launch_fc_bwd(const FcBwdArgs& a, int B, int Bp, hipStream_t s, bool reduce, int roles) {
  const int S = fc_bwd_splits(B);
  if (S > 1 && !a.part) throw std::runtime_error("fc_bwd: batch > 1024 needs the split-partial workspace");
  if (roles <= 0 || roles > FCB_ROLES_ALL) throw std::runtime_error("fc_bwd: bad role mask");
  if (roles != FCB_ROLES_ALL && S > 1 && reduce)
    throw std::runtime_error("fc_bwd: a partial launch leaves the split partials for a later reduce");
  const int grid = ((roles & FCB_ROLE_C) ? S : 0) + ((roles & FCB_ROLE_A) ? S * ROLE_A_WGS : 0) +
                   ((roles & FCB_ROLE_B) ? fc_bwd_role_b_wgs(B) : 0);
  if (fcb_mr(B) > 1) hipLaunchKernelGGL(fc_bwd_kernel<true>, dim3(grid), dim3(256), 0, s, a, B, Bp, 0, roles);
  else hipLaunchKernelGGL(fc_bwd_kernel<false>, dim3(grid), dim3(256), 0, s, a, B, Bp, 0, roles);
  if (reduce) launch_fc_grad_reduce(a, B, s);
}

void launch_fc_bwd_dw1(const FcBwdArgs& a, int B, int Bp, hipStream_t s) {
  const int S = fc_bwd_splits(B);
  if (S <= 1 || !a.part) throw std::runtime_error("fc_bwd_dw1: split partials only (batch > 1024)");
  hipLaunchKernelGGL(fc_bwd_dw1_kernel, dim3(S * ROLE_A_WGS), dim3(256), 0, s, a, B, Bp);
}

// profiling aid: one role of fc_bwd on its own (0 = C, 1 = A, 2 = B)
void launch_fc_bwd_role(const FcBwdArgs& a, int B, int Bp, int role, hipStream_t s) {
  const int S = fc_bwd_splits(B);
  const int nb = fc_bwd_role_b_wgs(B);
  const int grid = role == 0 ? S : role == 1 ? S * ROLE_A_WGS : nb;
  const int bid0 = role == 0 ? 0 : role == 1 ? S : S + S * ROLE_A_WGS;
  if (fcb_mr(B) > 1) hipLaunchKernelGGL(fc_bwd_kernel<true>, dim3(grid), dim3(256), 0, s, a, B, Bp, bid0, FCB_ROLES_ALL);
  else hipLaunchKernelGGL(fc_bwd_kernel<false>, dim3(grid), dim3(256), 0, s, a, B, Bp, bid0, FCB_ROLES_ALL);
}

TL_DEFINE_HOST(fc_head)

// load this translation unit's gfx950 code object now (startup prewarm thread) instead of at its
// first launch inside the timed run
void preload_fc_head() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&head_eval_kernel));
}

}  // namespace mnist
