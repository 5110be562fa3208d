// Input gradient of the fused Net: dx = d loss / d (normalised input image), fp32 [B][784].
//
// Replaces, for the module API and the Predictor, the part of the autograd backward the training step
// never needs: convolution_backward's grad_input of conv1 (reference mnist_ddp.py:50-51).  Inputs are
// what conv_bwd reads - the compact dy records fc_bwd wrote, the stored bf16 conv1 activations, the
// bf16 conv2 weight in dgrad layout and the fp32 conv1 weight - and nothing here writes any of them.
//
// Item = (image, strip of IG_ROWS = 7 dx rows); 4 strips tile the 28 rows, so every dx element is
// written exactly once by a plain store and the caller does not pre-zero.  Per item:
//   stage 1  da1 rows Y0-2 .. Y0+6 (the strip's two-row halo is recomputed, not exchanged): the
//            transposed conv2 as an implicit GEMM on v_mfma_f32_16x16x32_bf16, M = 9 x 26 pixels (15
//            tiles of 16, 4 per wave), N = 32 ci, K = 9 taps x 64 co.  A = the dense dy tile (11 rows x
//            28 columns incl. the zero padding, NHWC, expanded from the records into LDS), B = w2d
//            (staged into LDS once per workgroup).  The conv1 ReLU mask is the stored bf16 a1 > 0.
//   stage 2  the transposed conv1 (32 -> 1, 3 x 3) on the fp32 VALU: the masked fp32 accumulators go
//            to an LDS tile [9][30][32 (+1 pad)] with zero columns on both sides, and one thread per
//            dx pixel sums its 288 products in a fixed order.
// da1 FORM: da1 stays fp32 from the MFMA accumulators to the last fma (it is NOT rounded to bf16).
// Rows of da1 outside the image (strip 0: -2, -1; strip 3: 26, 27) are stored as zeros.
// No atomics, no cross-workgroup traffic, no waits: any grid gives the same bits.
//
// EPILOGUE: what the thread that owns dx[b][Y][X] does with its sum s is a compile-time policy of the
// one kernel body (template parameter).  IgStoreGrad stores s (launch_input_grad; instruction for
// instruction the kernel as it was before the policy existed).  IgProjectedStep writes the next iterate of
// an L-inf signed-gradient ascent (FGSM / PGD) instead, and s itself only when asked:
//   t = x + alpha * sgn(s);  t = min(max(t, x0 - eps), x0 + eps);  x_next = min(max(t, lo), hi)
// (launch_input_grad_step).  Its x / x0 loads are issued before stage 2 and land under the 288 fmas.
#include "row_ops.h"

#include <stdexcept>

namespace mnist {

namespace {
constexpr int IG_THREADS = 256;
constexpr int IG_DA_ROWS = IG_ROWS + 2;                  // 9 da1 rows per item (2 halo rows on top)
constexpr int IG_DY_ROWS = IG_DA_ROWS + 2;               // 11 dy rows (2 more)
constexpr int IG_DY_COLS = H2 + 4;                       // 28: 2 zero columns on each side
constexpr int IG_DY_PIX = IG_DY_ROWS * IG_DY_COLS;       // 308 tile pixels of 64 co (128 B)
constexpr int IG_NPIX = IG_DA_ROWS * H1;                 // 234 da1 pixels per item
constexpr int IG_MT = 4;                                 // M-tiles per wave: 16 tiles cover 234 pixels
constexpr int IG_PROWS = 6;                              // pooled rows under the 11 dy rows
constexpr int IG_JOBS = IG_PROWS * HP * 8;               // 576 record chunks (16 B = 8 channels)
constexpr int IG_JV = (IG_JOBS + IG_THREADS - 1) / IG_THREADS;   // 3 per thread
constexpr int IG_DA_COLS = H1 + 4;                       // 30: da1 columns -2 .. 27
constexpr int IG_DA_LD = C1 + 1;                         // 33 words per pixel: stage 2 reads conflict-free
constexpr int IG_DYS_BYTES = IG_DY_PIX * C2 * 2;         // 39424
constexpr int IG_DAS_BYTES = IG_DA_ROWS * IG_DA_COLS * IG_DA_LD * 4;   // 35640, aliases the dy tile
constexpr int IG_W2DS_BYTES = 9 * C1 * C2 * 2;           // 36864
constexpr int IG_W1S_BYTES = C1 * 9 * 4;                 // 1152
constexpr int IG_LDS = IG_DYS_BYTES + IG_W2DS_BYTES + IG_W1S_BYTES;    // 77440: two per CU
static_assert(IG_DAS_BYTES <= IG_DYS_BYTES && 2 * IG_LDS <= 160 * 1024, "input_grad LDS carve");
static_assert(IG_NPIX <= 4 * IG_MT * 16 && IG_ROWS * IMG <= IG_THREADS, "tile / thread cover");
static_assert(IG_W2DS_BYTES % (16 * IG_THREADS) == 0, "w2d staging");

// element (bf16) offset of 16-B chunk `chunk` of 128-B row `row`; the XOR spreads the 16 rows of a
// fragment read over the banks (dy tile: row = tile pixel; w2d: row = tap * 32 + ci)
__device__ __forceinline__ int ig_off(int row, int chunk) { return row * C2 + ((chunk ^ (row & 7)) << 3); }

// keep channel pair (2k, 2k + 1) of a record chunk where its argmax code equals q: r16 bit j = code
// bit 0 of channel j, bit 8 + j = code bit 1 (kernels.h DYC_ROUTE)
__device__ __forceinline__ uint32_t ig_keep_pair(uint32_t g, uint32_t r16, int k, int q) {
  const uint32_t c0 = ((r16 >> (2 * k)) & 1u) | (((r16 >> (8 + 2 * k)) & 1u) << 1);
  const uint32_t c1 = ((r16 >> (2 * k + 1)) & 1u) | (((r16 >> (9 + 2 * k)) & 1u) << 1);
  return g & ((c0 == (uint32_t)q ? 0x0000FFFFu : 0u) | (c1 == (uint32_t)q ? 0xFFFF0000u : 0u));
}
}  // namespace

// ---- epilogue policies: `load(e)` is issued before stage 2 for dx element e = b * 784 + Y * 28 + X,
// `store(dx, e, s, v)` after its last fma, both by the one thread that owns e
struct IgStoreGrad {
  struct Loaded {};
  __device__ __forceinline__ Loaded load(int64_t) const { return {}; }
  __device__ __forceinline__ void store(float* dx, int64_t e, float s, Loaded) const { dx[e] = s; }
};

struct IgProjectedStep {
  const float* x;
  const float* x0;
  float* x_next;              // may alias x: element e is read and written by its owner only
  float alpha, eps, lo, hi;
  struct Loaded { float x, x0; };
  __device__ __forceinline__ Loaded load(int64_t e) const { return {x[e], x0[e]}; }
  __device__ __forceinline__ void store(float* dx, int64_t e, float s, Loaded v) const {
    if (dx) dx[e] = s;                                     // optional here
    // torch.sign, except that a NaN gradient stays a NaN (every comparison below is false for it, so it
    // passes both clamps): a broken gradient is not turned into "no step"
    const float sg = s > 0.0f ? 1.0f : s < 0.0f ? -1.0f : s == s ? 0.0f : s;
    const float t = v.x + alpha * sg;                           // alpha * sg is exact: contraction cannot change it
    const float el = v.x0 - eps, eh = v.x0 + eps;          // rounded to fp32 first, as the torch formula does
    x_next[e] = clamp_nan_passes(clamp_nan_passes(t, el, eh), lo, hi);
  }
};

template <class Epilogue>
__global__ __launch_bounds__(IG_THREADS, 2) void input_grad_kernel(InputGradArgs a, int B, Epilogue epi) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[IG_LDS];
  uint16_t* dys = reinterpret_cast<uint16_t*>(smem);
  float* das = reinterpret_cast<float*>(smem);             // aliases the dy tile (after the MFMA loop)
  uint16_t* w2ds = reinterpret_cast<uint16_t*>(smem + IG_DYS_BYTES);
  float* w1s = reinterpret_cast<float*>(smem + IG_DYS_BYTES + IG_W2DS_BYTES);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kg = lane >> 4;
  const int n = IG_STRIPS * B, G = gridDim.x;
  RW_ENTRY();

  // conv weights, once per workgroup
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.w2d);
    uint4 w[IG_W2DS_BYTES / 16 / IG_THREADS];
#pragma unroll
    for (int i = 0; i < IG_W2DS_BYTES / 16 / IG_THREADS; ++i) w[i] = src[tid + IG_THREADS * i];
#pragma unroll
    for (int i = 0; i < IG_W2DS_BYTES / 16 / IG_THREADS; ++i) {
      const int c = tid + IG_THREADS * i;
      *reinterpret_cast<uint4*>(w2ds + ig_off(c >> 3, c & 7)) = w[i];
    }
    for (int i = tid; i < C1 * 9; i += IG_THREADS) w1s[i] = a.w1c[i];
  }

  for (int it = blockIdx.x; it < n; it += G) {
    const int strip = it % IG_STRIPS, b = it / IG_STRIPS;
    const int Y0 = strip * IG_ROWS;                        // first dx row
    const int r0 = Y0 - 2;                                 // first da1 row of the tile (may be -2)
    const int d0 = r0 - 2;                                 // first dy row of the tile
    const int py0 = d0 >> 1;                               // arithmetic shift: floor

    // ---- dy tile: record chunks -> the (up to) 4 pixels of their 2x2 windows, zeros outside 24 x 24
    uint4 g[IG_JV];
    uint32_t rt[IG_JV];
#pragma unroll
    for (int k = 0; k < IG_JV; ++k) {
      const int jb = tid + IG_THREADS * k;
      const int j = jb < IG_JOBS ? jb : 0;
      const int c8 = j & 7, pc = (j >> 3) % HP, py = py0 + (j >> 3) / HP;
      const bool ok = py >= 0 && py < HP;
      const uint8_t* rec = a.dyc + (int64_t)b * DYC_BYTES_PER_IMAGE + ((ok ? py : 0) * HP + pc) * DYC_REC;
      g[k] = *reinterpret_cast<const uint4*>(rec + c8 * 16);
      rt[k] = *reinterpret_cast<const uint16_t*>(rec + DYC_ROUTE + c8 * 2);
      if (!ok) g[k] = uint4{0u, 0u, 0u, 0u};
    }
    // conv1 ReLU mask operand: the stored a1 of this wave's accumulator elements (tile i, pixel
    // 4 kg + r, channels m and m + 16), in flight under the staging and the MFMA loop; pixels past the
    // tile and rows outside the image load a clamped address and are zeroed by `live` below
    uint16_t mk[IG_MT][4][2];
#pragma unroll
    for (int i = 0; i < IG_MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = min(16 * (wave + 4 * i) + 4 * kg + r, IG_NPIX - 1);
        const int qy = q / H1, qx = q - qy * H1;
        const int ry = min(max(r0 + qy, 0), H1 - 1);
        const uint16_t* src = a.a1 + (((int64_t)b * H1 + ry) * H1 + qx) * C1 + m;
        mk[i][r][0] = src[0];
        mk[i][r][1] = src[16];
      }
#pragma unroll
    for (int k = 0; k < IG_JV; ++k) {
      const int jb = tid + IG_THREADS * k;
      if (jb < IG_JOBS) {
        const int c8 = jb & 7, pc = (jb >> 3) % HP, pr = (jb >> 3) / HP;
        const int ly0 = 2 * (py0 + pr) - d0;               // tile row of the window's top pixels
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ly = ly0 + (q >> 1);
          if (ly >= 0 && ly < IG_DY_ROWS) {
            const int row = ly * IG_DY_COLS + 2 * pc + (q & 1) + 2;
            uint4 e;
            e.x = ig_keep_pair(g[k].x, rt[k], 0, q);
            e.y = ig_keep_pair(g[k].y, rt[k], 1, q);
            e.z = ig_keep_pair(g[k].z, rt[k], 2, q);
            e.w = ig_keep_pair(g[k].w, rt[k], 3, q);
            *reinterpret_cast<uint4*>(dys + ig_off(row, c8)) = e;
          }
        }
      }
    }
    // padding columns 0, 1, 26, 27 of the 11 tile rows
    for (int j = tid; j < IG_DY_ROWS * 4 * 8; j += IG_THREADS) {
      const int c8 = j & 7, pcol = (j >> 3) & 3, ly = j >> 5;
      const int row = ly * IG_DY_COLS + (pcol < 2 ? pcol : pcol + H2);
      *reinterpret_cast<uint4*>(dys + ig_off(row, c8)) = uint4{0u, 0u, 0u, 0u};
    }
    lds_barrier();                                         // dy tile (and, first item, the weights) staged

    // ---- stage 1: da1[pixel][ci] = sum over tap (d, c), co of dy[y - d][x - c][co] * w2d[tap][ci][co]
    // da1 pixel (qy, qx) of the tile sits over dy tile pixel (qy + 2, qx + 2)
    int qbase[IG_MT];
#pragma unroll
    for (int i = 0; i < IG_MT; ++i) {
      const int q = min(16 * (wave + 4 * i) + m, IG_NPIX - 1);   // past the tile: a valid pixel, not stored
      const int qy = q / H1, qx = q - qy * H1;
      qbase[i] = (qy + 2) * IG_DY_COLS + qx + 2;
    }
    floatx4 acc[IG_MT][2];
#pragma unroll
    for (int i = 0; i < IG_MT; ++i) acc[i][0] = acc[i][1] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {                          // (rolled: the 72 fragment addresses of the
      const int d = t / 3, c = t - 3 * d;                  // unrolled form cost more registers than time)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf16x8 Bf[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) Bf[nt] = ld16(w2ds + ig_off(t * C1 + nt * 16 + m, kg + 4 * h));
#pragma unroll
        for (int i = 0; i < IG_MT; ++i) {
          const bf16x8 A = ld16(dys + ig_off(qbase[i] - d * IG_DY_COLS - c, kg + 4 * h));
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[i][nt] = mfma16x16x32(A, Bf[nt], acc[i][nt]);
        }
      }
    }
    lds_barrier();                                         // every wave is done reading the dy tile

    // ---- masked fp32 da1 -> LDS tile [9][30][33]: acc[i][nt][r] = pixel 16 tile + 4 kg + r, ci 16 nt + m
#pragma unroll
    for (int i = 0; i < IG_MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * (wave + 4 * i) + 4 * kg + r;
        if (q < IG_NPIX) {
          const int qy = q / H1, qx = q - qy * H1;
          const bool live = r0 + qy >= 0 && r0 + qy < H1;
          float* dst = das + (qy * IG_DA_COLS + qx + 2) * IG_DA_LD + m;
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)                   // bf16 a1 > 0 <=> as int16 > 0
            dst[16 * nt] = (live && (int16_t)mk[i][r][nt] > 0) ? acc[i][nt][r] : 0.0f;
        }
      }
    for (int j = tid; j < IG_DA_ROWS * 4 * C1; j += IG_THREADS) {   // zero columns -2, -1, 26, 27
      const int ci = j & 31, pcol = (j >> 5) & 3, row = j >> 7;
      das[(row * IG_DA_COLS + (pcol < 2 ? pcol : pcol + H1)) * IG_DA_LD + ci] = 0.0f;
    }
    lds_barrier();

    // ---- stage 2: dx[Y][X] = sum over ci, ky, kx of da1[Y - ky][X - kx][ci] * w1c[ci][3 ky + kx]
    if (tid < IG_ROWS * IMG) {
      const int yl = tid / IMG, X = tid - yl * IMG;
      const typename Epilogue::Loaded ev = epi.load((int64_t)b * (IMG * IMG) + (Y0 + yl) * IMG + X);
      const float* base = das + ((yl + 2) * IG_DA_COLS + X + 2) * IG_DA_LD;   // da1 (Y, X)
      // (four chains with 16-B weight reads measured slower, 28.2 against 26.4 us at B = 200: the
      // stage is bound by LDS bytes, not by instruction count or the fma chain)
      float s = 0.0f;
#pragma unroll 4
      for (int ci = 0; ci < C1; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
            s = __builtin_fmaf(base[-(ky * IG_DA_COLS + kx) * IG_DA_LD + ci], w1s[ci * 9 + ky * 3 + kx], s);
      epi.store(a.dx, (int64_t)b * (IMG * IMG) + (Y0 + yl) * IMG + X, s, ev);
    }
    lds_barrier();                                         // the next dy store must not overtake these reads
  }
}
static int input_grad_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  }
  return cus;
}

// the planned grid, or `grid` workgroups where that is fewer (0: the plan)
static int input_grad_grid(int B, int grid) {
  if (grid < 0) throw std::invalid_argument("input_grad: grid must not be negative");
  const InputGradPlan p = input_grad_plan(B, input_grad_cus());
  return grid > 0 && grid < p.grid ? grid : p.grid;
}

void launch_input_grad(const InputGradArgs& a, int B, hipStream_t s, int grid) {
  if (B < 1 || B > INPUT_GRAD_MAX_B) throw std::runtime_error("input_grad: batch size out of range");
  if (!a.dyc || !a.a1 || !a.w2d || !a.w1c || !a.dx) throw std::runtime_error("input_grad: null argument");
  const int G = input_grad_grid(B, grid);
  hipLaunchKernelGGL(input_grad_kernel<IgStoreGrad>, dim3(G), dim3(IG_THREADS), 0, s, a, B, IgStoreGrad{});
}

void launch_input_grad_step(const InputGradStepArgs& a, int B, hipStream_t s, int grid) {
  if (B < 1 || B > INPUT_GRAD_MAX_B) throw std::runtime_error("input_grad_step: batch size out of range");
  if (!a.g.dyc || !a.g.a1 || !a.g.w2d || !a.g.w1c || !a.x || !a.x0 || !a.x_next)
    throw std::runtime_error("input_grad_step: null argument");   // (g.dx is optional)
  const int G = input_grad_grid(B, grid);
  hipLaunchKernelGGL(input_grad_kernel<IgProjectedStep>, dim3(G), dim3(IG_THREADS), 0, s, a.g, B,
                     IgProjectedStep{a.x, a.x0, a.x_next, a.alpha, a.eps, a.lo, a.hi});
}

void preload_input_grad() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&input_grad_kernel<IgStoreGrad>));
}

void preload_input_grad_step() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&input_grad_kernel<IgProjectedStep>));
}

}  // namespace mnist
