// Square Attack (Andriushchenko, Croce, Flammarion, Hein, ECCV 2020: the score-based black-box attack of AutoAttack),
// L-inf, on the normalised image, fp32 [M][784]: the start point, and one query's whole per-image decision - read the
// margin of the candidate, accept or reject it, freeze an image that is broken, draw the next square and write the
// next candidate - in one launch.
//
// One workgroup of ROW_THREADS per image, thread v < 196 owns the float4 v of each of the image's rows: columns
// 4 (v % 7) .. + 3 of row v / 7.  Every candidate pixel is V+(p) = C(x0[p] + eps) or V-(p) = C(x0[p] - eps), C =
// clamp_nan_passes(., lo, hi): the offset is added to the clean image, never to a point already moved.
//
// MARGIN of a row lp of ten log-probabilities and the class y:  ly = lp[y],  mo = max over j != y of lp[j]
//   untargeted:  L = ly - mo        targeted (y the class to reach):  L = mo - ly        (one fp32 subtraction)
// L < 0: broken.  The maximum lets a NaN through (a NaN among the others makes mo a NaN, as torch.max does), so a
// NaN anywhere in the row, inf - inf, and a y outside [0, 10) (ly = NaN) give a NaN margin; every comparison with it
// is false: it is never accepted and never freezes an image.
//
// PHILOX COUNTER LAYOUT (a domain of its own, kernels.h SQUARE_PHILOX_DOMAIN): image i, query index q use
//
//   philox4x32(c0 = q, c1 = SQUARE_PHILOX_DOMAIN, c2 = id_base + i, c3 = k; key = seed lo, hi)
//
// a draw depends on (seed, image id, query index) alone, never on the batch, the chunking or the grid.  The launcher
// keeps q and id_base + M within 32 bits.
//
// square_init (q = 0, vertical stripes): column c of every row gets V+ when bit 0 of word c & 3 of the call with
// k = c >> 2 is set, else V-.  The owner of float4 v makes the one call k = v % 7; element e takes word e.
//
// square_step, round j, after the eval chain wrote logp of x_cand; the record is {margin_best, queries_used, done, -}:
//   first:          margin_best = L; x_best = x_cand; queries_used = 1                     -- reads no record
//   done on entry:  the workgroup stores nothing at all (frozen)
//   else:           queries_used += 1;  L < margin_best (strict): margin_best = L, x_best = x_cand
//   done = margin_best < 0
//   last:           x_cand is not written
//   else, done:     x_cand = x_best            (once: the image's later forwards are harmless)
//   else:           the proposal of query q = j + 1 with side s: one call k = 0;
//                   row0 = (w0 * (29 - s)) >> 32, col0 = (w1 * (29 - s)) >> 32 (64-bit products: 0 .. 28 - s),
//                   V+ when w2 & 1 else V-;  x_cand = x_best, the pixels of rows row0 .. row0 + s - 1 and columns
//                   col0 .. col0 + s - 1 replaced by that vertex of x0's box
// The paper resamples until the window changes the point; that loop is not built.
//
// Every operation is an integer operation, a select, one add and one clamp, each rounded on its own (contraction
// off): the same operands give the same bits on any grid, stream and launch.  No atomics, no LDS, 16-byte accesses.
//
// STATE: every thread loads the 40-byte logp row, the label and the 16-byte record; thread 0 stores the record.  The
// __syncthreads between the loads and that store keeps a wave that starts late from reading the new record (all the
// decisions are workgroup-uniform, so every thread reaches the barrier or none).  Row elements are read and written
// by their owner only, and read before they are written.  The grid is exactly M workgroups: rows and records past M
// are untouched.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   square_step_kernel: VGPRs 17, SGPRs 45, LDS 0 B, scratch 0, occupancy 8 waves / SIMD
//   square_init_kernel: VGPRs 14, SGPRs 20, LDS 0 B, scratch 0, occupancy 8 waves / SIMD
// The label picks lp[y] by ten unrolled selects on a loop counter, not by a dynamic index into registers: no scratch.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
// V+ / V- of one pixel
__device__ __forceinline__ float sq_vertex(float c, float eps, bool plus, float lo, float hi) {
#pragma clang fp contract(off)
  const float t = plus ? c + eps : c - eps;
  return clamp_nan_passes(t, lo, hi);
}

// the margin of the header; workgroup-uniform
__device__ __forceinline__ float sq_margin(const float* lp, int y, bool targeted) {
#pragma clang fp contract(off)
  float ly = __builtin_nanf("");
  float mo = 0.0f;
  bool any = false;
#pragma unroll
  for (int k = 0; k < NCLS; ++k) {
    const float v = lp[k];
    if (k == y) {
      ly = v;
    } else if (!any) {
      mo = v;
      any = true;
    } else {
      mo = (v > mo || v != v) ? v : mo;                    // (a NaN mo stays: both tests are false from then on)
    }
  }
  return targeted ? mo - ly : ly - mo;
}
}  // namespace

__global__ __launch_bounds__(ROW_THREADS) void square_init_kernel(SquareInitArgs a) {
  RW_ENTRY();
  const int v = threadIdx.x;
  if (v >= ROW_VECS) return;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + v;
  const float4 c = reinterpret_cast<const float4*>(a.x0)[at];
  const u32x4 w = philox4x32(0u, SQUARE_PHILOX_DOMAIN, a.id_base + (uint32_t)i, (uint32_t)(v % 7), (uint32_t)a.seed,
                             (uint32_t)(a.seed >> 32));
  float4 o;
  o.x = sq_vertex(c.x, a.eps, (w[0] & 1u) != 0u, a.lo, a.hi);
  o.y = sq_vertex(c.y, a.eps, (w[1] & 1u) != 0u, a.lo, a.hi);
  o.z = sq_vertex(c.z, a.eps, (w[2] & 1u) != 0u, a.lo, a.hi);
  o.w = sq_vertex(c.w, a.eps, (w[3] & 1u) != 0u, a.lo, a.hi);
  reinterpret_cast<float4*>(a.x_cand)[at] = o;
}

__global__ __launch_bounds__(ROW_THREADS) void square_step_kernel(SquareStepArgs a) {
  const int tid = threadIdx.x;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + (own ? tid : 0);       // (idle threads: a valid address)
  RW_ENTRY();
  const float L = sq_margin(a.logp + i * NCLS, a.y[i], a.targeted != 0);
  float margin_best;
  int used, spare = 0;
  bool accept;
  if (a.first) {
    margin_best = L;
    used = 1;
    accept = true;
  } else {
    const int4 rec = reinterpret_cast<const int4*>(a.state)[i];
    __syncthreads();                                       // every wave holds the old record before thread 0 stores
    if (rec.z != 0) return;                                // frozen: nothing is stored
    const float was = __int_as_float(rec.x);
    used = rec.y + 1;
    spare = rec.w;
    accept = L < was;
    margin_best = accept ? L : was;
  }
  const bool done = margin_best < 0.0f;
  float4 best = reinterpret_cast<const float4*>(a.x_cand)[at];
  if (accept) {
    if (own) reinterpret_cast<float4*>(a.x_best)[at] = best;
  } else {
    best = reinterpret_cast<const float4*>(a.x_best)[at];
  }
  if (!a.last) {
    float4 o = best;
    if (!done) {
      const float4 c = reinterpret_cast<const float4*>(a.x0)[at];
      const u32x4 w = philox4x32(a.q, SQUARE_PHILOX_DOMAIN, a.id_base + (uint32_t)i, 0u, (uint32_t)a.seed,
                                 (uint32_t)(a.seed >> 32));
      const uint32_t span = (uint32_t)(IMG + 1 - a.side);
      const int row0 = (int)(((uint64_t)w[0] * span) >> 32), col0 = (int)(((uint64_t)w[1] * span) >> 32);
      const bool plus = (w[2] & 1u) != 0u;
      const int r = tid / 7, cb = 4 * (tid - 7 * r);
      const bool in_rows = r >= row0 && r < row0 + a.side;
      const int c_lo = col0 - cb, c_hi = col0 + a.side - cb;     // element e is inside when c_lo <= e < c_hi
      if (in_rows && 0 >= c_lo && 0 < c_hi) o.x = sq_vertex(c.x, a.eps, plus, a.lo, a.hi);
      if (in_rows && 1 >= c_lo && 1 < c_hi) o.y = sq_vertex(c.y, a.eps, plus, a.lo, a.hi);
      if (in_rows && 2 >= c_lo && 2 < c_hi) o.z = sq_vertex(c.z, a.eps, plus, a.lo, a.hi);
      if (in_rows && 3 >= c_lo && 3 < c_hi) o.w = sq_vertex(c.w, a.eps, plus, a.lo, a.hi);
    }
    if (own) reinterpret_cast<float4*>(a.x_cand)[at] = o;
  }
  if (tid == 0)
    reinterpret_cast<int4*>(a.state)[i] = int4{__float_as_int(margin_best), used, done ? 1 : 0, spare};
}

void launch_square_init(const SquareInitArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("square_init: image count out of range");
  if (!a.x0 || !a.x_cand) throw std::runtime_error("square_init: null argument");
  if (misaligned(15, a.x0, a.x_cand)) throw std::runtime_error("square_init: the fp32 row arrays must be 16-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("square_init: eps must be >= 0");
  if ((uint64_t)a.id_base + (uint64_t)M > (1ull << 32))
    throw std::runtime_error("square_init: id_base + M must not exceed 2^32");
  hipLaunchKernelGGL(square_init_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void launch_square_step(const SquareStepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("square_step: image count out of range");
  if (!a.logp || !a.y || !a.x0 || !a.x_best || !a.x_cand || !a.state)
    throw std::runtime_error("square_step: null argument");
  if (misaligned(15, a.x0, a.x_best, a.x_cand))
    throw std::runtime_error("square_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.state)) throw std::runtime_error("square_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.logp, a.y)) throw std::runtime_error("square_step: logp and y must be 4-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("square_step: eps must be >= 0");
  if (a.side < 1 || a.side > IMG - 1) throw std::runtime_error("square_step: the side must be in [1, 27]");
  if ((uint64_t)a.id_base + (uint64_t)M > (1ull << 32))
    throw std::runtime_error("square_step: id_base + M must not exceed 2^32");
  hipLaunchKernelGGL(square_step_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_square() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&square_step_kernel));
}

}  // namespace mnist
