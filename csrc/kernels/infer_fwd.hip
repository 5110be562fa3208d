// Single-launch inference forward: gather+normalise -> conv1+ReLU -> conv2 (MFMA) -> +bias -> ReLU ->
// maxpool 2x2 -> fc1 (split-K MFMA over the 12 pooled rows) -> [last arriver of the group:] +bias ->
// ReLU -> fc2 -> log_softmax -> argmax (+ NLL / hit).  Eval semantics: no dropout.
//
// The three-launch eval path (trunk_fwd<false> -> fc1_fwd -> head_eval) sends the pooled features
// (B x 9216 bf16) and a 32-way split-K partial set through HBM and pays two kernel boundaries; at
// small batch that is most of its time.  Here one workgroup = one BAND (pooled row: 2 conv2 output
// rows, 4 conv1 rows, 6 input rows) of a GROUP of up to 16 images:
//   * the group's input rows are fetched in one round trip and normalised with trunk_fwd's arithmetic;
//   * per image: conv1 on the VALU (trunk_fwd's fma chain) into a double-buffered bf16 NHWC LDS tile,
//     conv2 as 3 M-tiles (pool-window-major, 4 windows each) x 4 N-tiles of mfma16x16x32 - wave w owns
//     N-tile w and keeps its 9 weight fragments in registers for every image of the group - then
//     bias + ReLU + max-pool in registers; the 768 pooled bf16 features go to LDS [image][768];
//   * fc1: z1part[band][b][0..128) = feats[b][0..768) x w1[:, band's 768 columns]^T on MFMA with
//     M = the group's images (rows past the group's count are zero fragments), the w1 fragments
//     streamed from L2 double-buffered in registers; feature index k = 12 * channel + pooled x, so
//     every 4-run of k is 8 contiguous bytes of w1;
//   * hand-off: the partial stores are write-through and drained, then one lane takes a ticket
//     (agent-scope acq_rel add); the workgroup that draws INFER_BANDS - 1 acquires (every thread: the
//     other bands ran on other CUs, mostly behind other XCDs' L2s), sums the partials in band order
//     and finishes the group's rows, then writes the ticket back to 0.  No workgroup waits for
//     another one: there is no spin loop in this kernel, and residency does not matter.
// Partials are written, never accumulated; the sums are in fixed order, so the same (parameters,
// input, B) gives the same bits on every launch and under graph replay.  Rows >= B of every output
// and of the workspace are not touched.
#include "../include/device_utils.h"
#include "../include/kernels.h"

#include <stdexcept>

namespace mnist {

namespace {
constexpr int IF_THREADS = 256;
constexpr int IF_XROWS = 6, IF_XPIX = IF_XROWS * IMG;          // 168 input pixels per (image, band)
constexpr int IF_A1ROWS = 4, IF_A1PIX = IF_A1ROWS * H1;        // 104 conv1 pixels
constexpr int IF_K = C2 * HP;                                  // 768 features per band
constexpr int IF_FEAT_LD = IF_K + 8;                           // 388 words = 4 mod 32: conflict-free 16-B rows
constexpr int IF_XJ = (INFER_MAX_IPW * IF_XPIX + IF_THREADS - 1) / IF_THREADS;   // 11 pixels per thread
constexpr int IF_KSTEPS = IF_K / 32;                           // 24
constexpr int IF_KB = 6, IF_KBLOCKS = IF_KSTEPS / IF_KB;       // w1 fragments fetched 6 k-steps at a time
// LDS carve (bytes, 16-aligned)
constexpr int IF_XS_OFF = 0, IF_XS_BYTES = INFER_MAX_IPW * IF_XPIX * 4;          // 10752
constexpr int IF_W1S_OFF = IF_XS_OFF + IF_XS_BYTES, IF_W1S_BYTES = (C1 * 9 + C1) * 4;   // 1280
constexpr int IF_A1S_OFF = IF_W1S_OFF + IF_W1S_BYTES, IF_A1S_BYTES = IF_A1PIX * C1 * 2; // 6656 (x 2)
constexpr int IF_FEAT_OFF = IF_A1S_OFF + 2 * IF_A1S_BYTES, IF_FEAT_BYTES = INFER_MAX_IPW * IF_FEAT_LD * 2;
constexpr int IF_LDS = IF_FEAT_OFF + IF_FEAT_BYTES;            // 50176
static_assert(IF_W1S_OFF % 16 == 0 && IF_A1S_OFF % 16 == 0 && IF_A1S_BYTES % 16 == 0 && IF_FEAT_OFF % 16 == 0 &&
              (IF_FEAT_LD * 2) % 16 == 0, "LDS alignment");
static_assert(IF_KBLOCKS * IF_KB == IF_KSTEPS && INFER_BANDS * IF_K == NFLAT, "band split");

__device__ __forceinline__ int if_swz_a1(int col) { return col & 3; }
// feature k (= 12 * channel + pooled x) -> offset inside the band's columns of one w1 row
__device__ __forceinline__ int if_koff(int k) { return k + (NPOOL - HP) * (k / HP); }

__device__ __forceinline__ bf16x8 frag_from(uint2 lo, uint2 hi) {
  const u32x4 v = {lo.x, lo.y, hi.x, hi.y};
  return __builtin_bit_cast(bf16x8, v);
}

// every wave that stored handed-off bytes waits for its stores before the barrier in front of the
// ticket add (the stores are write-through: once drained they are past this XCD's L2)
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// torch log_softmax: (x - max) - log(sum(exp(x - max)))  (head_eval's expression forms)
__device__ __forceinline__ void if_log_softmax10(const float* x, float* lp) {
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

// input form (a template parameter, as TrunkX: phase 0 has no load under a branch)
enum InferX { IX_U8 = 0, IX_IDX = 1, IX_XIN = 2 };

template <int XM>
__global__ __launch_bounds__(IF_THREADS, 2) void infer_fwd_kernel(InferArgs a, int B, int ipw) {
  RW_ENTRY();
  __shared__ __attribute__((aligned(16))) unsigned char smem[IF_LDS];
  __shared__ int s_ticket;
  float* xs = reinterpret_cast<float*>(smem + IF_XS_OFF);
  float* w1s = reinterpret_cast<float*>(smem + IF_W1S_OFF);
  uint16_t* feats = reinterpret_cast<uint16_t*>(smem + IF_FEAT_OFF);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, kg = lane >> 4;
  const int band = blockIdx.x, g = blockIdx.y;
  const int b0 = g * ipw;
  const int nimg = min(ipw, B - b0);                 // 1..16 (the launcher's grid has no empty group)

  // ---- phase 0: every global load of the conv part up front, all unconditional: the group's input
  // rows (one pixel each, clamped past the group's end), conv1 weights + bias, this wave's conv2
  // weight fragments (N-tile = wave) and conv2 bias
  const int c = tid & 3;                             // conv1: fixed 8-channel chunk per thread
  {
    const int npx = nimg * IF_XPIX;
    float xv[IF_XJ];
#pragma unroll
    for (int j = 0; j < IF_XJ; ++j) {
      const int e = tid + IF_THREADS * j;
      const int ec = e < npx ? e : 0;
      const int slot = ec / IF_XPIX, px = ec - slot * IF_XPIX;
      const int b = b0 + slot;
      const int64_t off = (int64_t)band * 2 * IMG + px;
      if constexpr (XM == IX_XIN) {
        xv[j] = a.xin[(int64_t)b * (IMG * IMG) + off];
      } else {
        const int64_t row = (XM == IX_IDX) ? (int64_t)a.idx[b] : (int64_t)b;
        xv[j] = __builtin_bit_cast(float, (uint32_t)a.data_u8[row * (IMG * IMG) + off]);
      }
    }
    const float4 w1v = tid < 72 ? reinterpret_cast<const float4*>(a.w1c)[tid]
                                : reinterpret_cast<const float4*>(a.b1c)[tid < 80 ? tid - 72 : 0];
    if (tid < 80) {                                  // pair-interleaved: [chunk c][pair jp][tap t | bias][2]
      const float fv[4] = {w1v.x, w1v.y, w1v.z, w1v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f = 4 * tid + e;                   // w1c[ch][t] (f < 288) or b1c[ch]
        const int ch = f < C1 * 9 ? f / 9 : f - C1 * 9, t = f < C1 * 9 ? f - 9 * (f / 9) : 9;
        w1s[(((ch >> 3) * 4 + ((ch & 7) >> 1)) * 10 + t) * 2 + (ch & 1)] = fv[e];
      }
    }
#pragma unroll
    for (int j = 0; j < IF_XJ; ++j) {
      const int e = tid + IF_THREADS * j;
      if (e < npx) xs[e] = (XM == IX_XIN) ? xv[j] : normalize_u8_alu(__builtin_bit_cast(uint32_t, xv[j]));
    }
  }
  bf16x8 Bw[9];                                      // conv2 weights of channels 16 wave + m, 8 ci at kg
#pragma unroll
  for (int t = 0; t < 9; ++t) Bw[t] = ld16(a.w2f + ((16 * wave + m) * 9 + t) * C1 + 8 * kg);
  const float bias2 = a.b2c[16 * wave + m];
  __syncthreads();

  float2v wp[4][9], bp[4];                           // conv1 weights of this thread's 8 channels
  {
    const float2v* wl = reinterpret_cast<const float2v*>(w1s) + c * 40;
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
#pragma unroll
      for (int t = 0; t < 9; ++t) wp[jp][t] = wl[jp * 10 + t];
      bp[jp] = wl[jp * 10 + 9];
    }
  }
  int pix_base[3], col_base[3];                      // conv2 A fragments: pixel m of M-tile mt
#pragma unroll
  for (int mt = 0; mt < 3; ++mt) {
    const int pc = 4 * mt + (m >> 2), q = m & 3;     // pool window (= pooled x), position in it
    col_base[mt] = 2 * pc + (q & 1);
    pix_base[mt] = (q >> 1) * H1 + col_base[mt];
  }

  // ---- per image: conv1 -> a1 tile (buffer s & 1) | barrier | conv2 + pool -> feats[s].  The next
  // image's conv1 writes the other buffer, so one barrier per image is enough.
  for (int s = 0; s < nimg; ++s) {
    uint16_t* a1s = reinterpret_cast<uint16_t*>(smem + IF_A1S_OFF + (s & 1) * IF_A1S_BYTES);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pidx = (tid >> 2) + (IF_THREADS / 4) * i;
      if (pidx < IF_A1PIX) {
        const int r = pidx / H1, col = pidx - r * H1;
        const float* xp = xs + s * IF_XPIX + r * IMG + col;
        float xv[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) xv[t] = xp[(t / 3) * IMG + t % 3];
        float o[8];
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {             // trunk_fwd's chain: bias, then taps in row-major order
          float2v acc = bp[jp];
#pragma unroll
          for (int t = 0; t < 9; ++t) acc = __builtin_elementwise_fma(float2v{xv[t], xv[t]}, wp[jp][t], acc);
          o[2 * jp] = fmaxf(acc.x, 0.0f);
          o[2 * jp + 1] = fmaxf(acc.y, 0.0f);
        }
        uint4 v;
        v.x = pack2bf(o[0], o[1]); v.y = pack2bf(o[2], o[3]);
        v.z = pack2bf(o[4], o[5]); v.w = pack2bf(o[6], o[7]);
        *reinterpret_cast<uint4*>(a1s + pidx * C1 + ((c ^ if_swz_a1(col)) * 8)) = v;
      }
    }
    __syncthreads();
    floatx4 acc[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) acc[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int toff = (t / 3) * H1 + (t % 3);
#pragma unroll
      for (int mt = 0; mt < 3; ++mt) {
        const bf16x8 A = ld16(a1s + (pix_base[mt] + toff) * C1 + ((kg ^ if_swz_a1(col_base[mt] + t % 3)) * 8));
        acc[mt] = mfma16x16x32(A, Bw[t], acc[mt]);
      }
    }
    // lane (m, kg) of wave w holds the 2x2 window 4 mt + kg of channel 16 w + m
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
      float best = fmaxf(acc[mt][0] + bias2, 0.0f);
#pragma unroll
      for (int r = 1; r < 4; ++r) best = fmaxf(best, fmaxf(acc[mt][r] + bias2, 0.0f));
      feats[s * IF_FEAT_LD + (16 * wave + m) * HP + 4 * mt + kg] = f2bf(best);
    }
  }
  __syncthreads();

  // ---- fc1: z1^T tiles (w1 fragments as the A operand, as fc1_fwd): wave w owns outputs
  // 32 w .. 32 w + 31 (two 16-row tiles); lane (m, kg) ends with outputs o0 + 4 kg + r of image m.
  const uint16_t* wr0 = a.w1 + (int64_t)(32 * wave + m) * NFLAT + band * HP;
  const uint16_t* wr1 = wr0 + (int64_t)16 * NFLAT;
  uint2 cur[IF_KB][4], nxt[IF_KB][4];
#define IF_FETCH(dst, blk)                                                                   \
  _Pragma("unroll") for (int i = 0; i < IF_KB; ++i) {                                        \
    const int k0 = ((blk) * IF_KB + i) * 32 + 8 * kg;                                        \
    const int o0 = if_koff(k0), o1 = if_koff(k0 + 4);                                        \
    dst[i][0] = *reinterpret_cast<const uint2*>(wr0 + o0);                                   \
    dst[i][1] = *reinterpret_cast<const uint2*>(wr0 + o1);                                   \
    dst[i][2] = *reinterpret_cast<const uint2*>(wr1 + o0);                                   \
    dst[i][3] = *reinterpret_cast<const uint2*>(wr1 + o1);                                   \
  }
  IF_FETCH(cur, 0);
  floatx4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
  const bool valid = m < nimg;
  const uint16_t* frow = feats + (valid ? m : 0) * IF_FEAT_LD + 8 * kg;
#pragma unroll 1
  for (int blk = 0; blk < IF_KBLOCKS; ++blk) {
    const int nb = blk + 1 < IF_KBLOCKS ? blk + 1 : blk;   // (the last block re-fetches itself: no load under a branch)
    IF_FETCH(nxt, nb);
#pragma unroll
    for (int i = 0; i < IF_KB; ++i) {
      const bf16x8 f = valid ? ld16(frow + (blk * IF_KB + i) * 32) : zero_frag();
      z0 = mfma16x16x32(frag_from(cur[i][0], cur[i][1]), f, z0);
      z1 = mfma16x16x32(frag_from(cur[i][2], cur[i][3]), f, z1);
    }
#pragma unroll
    for (int i = 0; i < IF_KB; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) cur[i][j] = nxt[i][j];
  }
#undef IF_FETCH
  if (valid) {
    const int64_t e = ((int64_t)band * B + b0 + m) * NH + 32 * wave + 4 * kg;
    store_wt16(a.z1part, e * 4, z0);
    store_wt16(a.z1part, (e + 16) * 4, z1);
  }

  // ---- hand-off: drained write-through partials -> barrier -> one ticket per workgroup
  drain_stores();
  __syncthreads();
  if (tid == 0) {
    RW_SIGNAL();
    s_ticket = __hip_atomic_fetch_add(a.tickets + g, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_ticket != INFER_BANDS - 1) return;
  // last arriver of the group: every partial of it is published.  Every thread acquires before its
  // own loads of them.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // ---- head: one wave per row; lane owns hidden units lane and lane + 64
  for (int s = wave; s < nimg; s += IF_THREADS / 64) {
    const int b = b0 + s;
    int y = -1;
    if (a.labels) y = a.labels[(XM == IX_IDX) ? a.idx[b] : b];
    float part[INFER_BANDS][2];
#pragma unroll
    for (int k = 0; k < INFER_BANDS; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) part[k][j] = a.z1part[((int64_t)k * B + b) * NH + lane + 64 * j];
    float h[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float sum = 0.f;                               // fixed band order; torch adds the bias after the GEMM
#pragma unroll
      for (int k = 0; k < INFER_BANDS; ++k) sum += part[k][j];
      h[j] = fmaxf(a.b_fc1[lane + 64 * j] + sum, 0.0f);
    }
    float logit[NCLS], lp[NCLS];
#pragma unroll
    for (int k = 0; k < NCLS; ++k) {
      const float v = h[0] * a.w_fc2[k * NH + lane] + h[1] * a.w_fc2[k * NH + lane + 64];
      logit[k] = wave_sum(v) + a.b_fc2[k];
    }
    if_log_softmax10(logit, lp);
    if (lane == 0) {
      int am = 0;
#pragma unroll
      for (int k = 1; k < NCLS; ++k) am = (lp[k] > lp[am]) ? k : am;
      a.pred[b] = am;
      if (a.loss_rows) a.loss_rows[b] = (y >= 0 && y < NCLS) ? -lp[y] : 0.0f;
      if (a.correct) a.correct[b] = (am == y) ? 1 : 0;
    }
    if (lane < NCLS) {
      float v = lp[0];
#pragma unroll
      for (int k = 1; k < NCLS; ++k) v = (lane == k) ? lp[k] : v;
      a.logp[(int64_t)b * NCLS + lane] = v;
    }
  }
  // the ticket back to 0 for the next launch (all 12 adds of this launch are in: nobody adds again)
  if (tid == 0) __hip_atomic_store(a.tickets + g, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void launch_infer_fwd(const InferArgs& a, int B, hipStream_t s) {
  if (B < 1 || B > INFER_MAX_B) throw std::runtime_error("infer_fwd: batch size out of range");
  if (!a.xin && !a.data_u8) throw std::runtime_error("infer_fwd: no input");
  if ((a.loss_rows || a.correct) && !a.labels) throw std::runtime_error("infer_fwd: loss / correct need labels");
  const int ipw = infer_images_per_wg(B);
  const dim3 grid(INFER_BANDS, (B + ipw - 1) / ipw), block(IF_THREADS);
  if (a.xin) hipLaunchKernelGGL((infer_fwd_kernel<IX_XIN>), grid, block, 0, s, a, B, ipw);
  else if (a.idx) hipLaunchKernelGGL((infer_fwd_kernel<IX_IDX>), grid, block, 0, s, a, B, ipw);
  else hipLaunchKernelGGL((infer_fwd_kernel<IX_U8>), grid, block, 0, s, a, B, ipw);
}

}  // namespace mnist
