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

// ================================================= L2 =================================================
// The L2 branch of the authors' code on the same loop: the record, `first`, `last`, frozen, accept (strict <), done
// and the margin are square_step's, word for word.  The perturbation d = x - x0 lives on the L2 sphere of radius eps;
// a proposal takes the mass of a window W2 and puts it, with what the ball has left, into a window W1 under the
// pattern +-E_s, then rescales the whole perturbation to the sphere.  s is odd, 3 .. 27; E_s (the authors'
// meta_pseudo_gaussian_pert(s), unit norm, upper half positive, lower half negative) is made on the host in float64
// and read here from `table`, fp32 [s][s] row-major; its transpose is the index swap.
//
// DRAWS (kernels.h SQUARE_L2_PHILOX_DOMAIN, counter (q, domain, id_base + i, k), key = seed):
//   query q >= 1:  k = 0: row1 = (w0 * (29 - s)) >> 32, col1 = (w1 * (29 - s)) >> 32 (0 .. 28 - s), +E when w2 & 1
//                  else -E, transposed when w2 & 2;   k = 1: row2, col2 the same way from w0, w1
//   query 0:       k = 0: tile t = 5 tr + tc: +E_5 when bit t of w0 is set else -E_5, transposed when bit t of w1 is
//
// square_l2_init: the 25 tiles of side 5 at rows 1 + 5 tr, columns 1 + 5 tc; e = +-E_5[.] on a tile, 0 on the border;
//   g = eps / 5;  x_cand = C(x0 + e * g)                                   (every tile has unit norm: ||d|| = eps)
//
// square_l2_step, a live image that is not done, on a round that is not the last; x = x_best (the point just accepted
// or kept), W1 = rows row1 .. row1 + s - 1 x columns col1 .. col1 + s - 1, W2 likewise; every line one fp32 operation
// per element, rounded on its own (contraction off), in this order:
//   1  d = x - x0
//   2  q = d * d;  S1 = sum_{W1} q;  SU = sum_{W1 u W2} q;  SI = sum q      (a pixel outside a sum's set adds +0)
//   3  a = sqrt(S1);  b = 1e-10f + a;  n = (+-E[.]) + d / b  on W1;  SN = sum_{W1} n * n
//   4  h = eps * eps - SI;  h = h < 0 ? 0 : h;  u = h + SU;  f = sqrt(u) / sqrt(SN)
//      d' = n * f on W1,  0 on W2 \ W1,  d elsewhere;  SD = sum d' * d'
//   5  t = sqrt(SD);  x_cand = C(x0 + (d' / t) * eps)
//   SN == 0 or SD == 0:  x_cand = x_best (a select on the finished candidate, no division is looked at): with eps = 0
//   the start is x0, d = 0, f = 0, SD = 0 and every candidate is x0, bit for bit.
// A NaN pixel makes SI, hence u, f, t and every pixel of that image's candidate a NaN (h < 0 is false for a NaN);
// its margin is then a NaN and never accepted.  No other image reads it.
//
// SUMS: row_ops.h's fixed tree - a thread adds its four terms as (t0 + t1) + (t2 + t3), the xor butterfly over the
// wave, the four wave sums through LDS as (w0 + w1) + (w2 + w3) - each sum with LDS words of its own: S1, SU and SI
// behind one barrier (12 words), SN and SD behind one each.  No atomics; the same bits on any grid and stream.
//
// One workgroup per image, thread v < 196 owns the float4 v: x0, d and n / d' stay in registers through the three
// stages, each row is read once and x_cand written once.  The window tests are integer compares on the thread's row
// and its four columns; a thread reads its <= 4 pattern values by address (index 0 outside W1: always inside the
// table), through fully unrolled loops: no dynamically indexed register array.  A frozen workgroup returns before
// any LDS barrier; `done` and `last` are workgroup-uniform, so every wave reaches the same barriers.  Idle threads
// (v >= 196) carry d = 0 and belong to no window.
//
// RESOURCES (as above):
//   square_l2_step_kernel: VGPRs 45, SGPRs 50, LDS 80 B, scratch 0, occupancy 8 waves / SIMD
//   square_l2_init_kernel: VGPRs 17, SGPRs 22, LDS 0 B, scratch 0, occupancy 8 waves / SIMD
namespace {
// 5 x 5 tiles of side 5 on rows and columns 1 .. 25: a border of 1 before them (the authors' (28 - 25) / 2), 2 after
constexpr int L2_TILE = SQUARE_L2_INIT_SIDE, L2_TILES = IMG / L2_TILE;
static_assert(L2_TILES == 5 && 1 + L2_TILES * L2_TILE <= IMG && L2_TILES * L2_TILES <= 32, "one draw bit per tile");

// element e of a thread's float4, by a compile-time index
__device__ __forceinline__ float f4_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ float sum4(const float* t) {
#pragma clang fp contract(off)
  return (t[0] + t[1]) + (t[2] + t[3]);
}
}  // namespace

__global__ __launch_bounds__(ROW_THREADS) void square_l2_init_kernel(SquareL2InitArgs a) {
#pragma clang fp contract(off)
  RW_ENTRY();
  const int v = threadIdx.x;
  if (v >= ROW_VECS) return;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + v;
  const float4 c = reinterpret_cast<const float4*>(a.x0)[at];
  const u32x4 w = philox4x32(0u, SQUARE_L2_PHILOX_DOMAIN, a.id_base + (uint32_t)i, 0u, (uint32_t)a.seed,
                             (uint32_t)(a.seed >> 32));
  const float g = a.eps / (float)L2_TILE;
  const int r = v / 7, cb = 4 * (v - 7 * r);
  const bool in_rows = r >= 1 && r <= L2_TILES * L2_TILE;
  const int tr = in_rows ? (r - 1) / L2_TILE : 0, rr = in_rows ? (r - 1) - L2_TILE * tr : 0;
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int col = cb + e;
    const bool in = in_rows && col >= 1 && col <= L2_TILES * L2_TILE;
    const int tc = in ? (col - 1) / L2_TILE : 0, cc = in ? (col - 1) - L2_TILE * tc : 0;
    const int t = L2_TILES * tr + tc;
    const bool plus = ((w[0] >> t) & 1u) != 0u, swap = ((w[1] >> t) & 1u) != 0u;
    const float p = a.table[swap ? cc * L2_TILE + rr : rr * L2_TILE + cc];     // (outside the tiles: entry 0, unused)
    const float pat = in ? (plus ? p : -p) : 0.0f;
    o[e] = clamp_nan_passes(f4_get(c, e) + pat * g, a.lo, a.hi);
  }
  reinterpret_cast<float4*>(a.x_cand)[at] = float4{o[0], o[1], o[2], o[3]};
}

__global__ __launch_bounds__(ROW_THREADS) void square_l2_step_kernel(SquareL2StepArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[5][ROW_WAVES];                     // S1, SU, SI, SN, SD: words of their own
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
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
    float4 out = best;
    if (!done) {
      const float4 c = reinterpret_cast<const float4*>(a.x0)[at];
      const uint32_t id = a.id_base + (uint32_t)i, k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
      const u32x4 wa = philox4x32(a.q, SQUARE_L2_PHILOX_DOMAIN, id, 0u, k0, k1);
      const u32x4 wb = philox4x32(a.q, SQUARE_L2_PHILOX_DOMAIN, id, 1u, k0, k1);
      const int s = a.side;
      const uint32_t span = (uint32_t)(IMG + 1 - s);
      const int row1 = (int)(((uint64_t)wa[0] * span) >> 32), col1 = (int)(((uint64_t)wa[1] * span) >> 32);
      const int row2 = (int)(((uint64_t)wb[0] * span) >> 32), col2 = (int)(((uint64_t)wb[1] * span) >> 32);
      const bool plus = (wa[2] & 1u) != 0u, swap = (wa[2] & 2u) != 0u;
      const int r = tid / 7, cb = 4 * (tid - 7 * r);
      const bool rows1 = own && r >= row1 && r < row1 + s, rows2 = own && r >= row2 && r < row2 + s;
      const int rr = r - row1;
      // 1, 2
      float d[4], t1[4], tu[4], ti[4];
      bool in1[4], in2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = cb + e;
        d[e] = own ? f4_get(best, e) - f4_get(c, e) : 0.0f;
        in1[e] = rows1 && col >= col1 && col < col1 + s;
        in2[e] = rows2 && col >= col2 && col < col2 + s;
        const float q = d[e] * d[e];
        t1[e] = in1[e] ? q : 0.0f;
        tu[e] = (in1[e] || in2[e]) ? q : 0.0f;
        ti[e] = q;
      }
      const float w1 = wave_sum(sum4(t1)), wu = wave_sum(sum4(tu)), wi = wave_sum(sum4(ti));
      if (lane == 0) {
        part[0][wave] = w1;
        part[1][wave] = wu;
        part[2][wave] = wi;
      }
      lds_barrier();
      const float S1 = row_waves_sum(part[0]), SU = row_waves_sum(part[1]), SI = row_waves_sum(part[2]);
      // 3
      const float b = 1e-10f + sqrtf(S1);
      float n[4], tn[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cc = cb + e - col1;
        const float p = a.table[in1[e] ? (swap ? cc * s + rr : rr * s + cc) : 0];
        n[e] = (plus ? p : -p) + d[e] / b;
        tn[e] = in1[e] ? n[e] * n[e] : 0.0f;
      }
      const float SN = row_block_sum(sum4(tn), part[3], wave, lane);
      // 4
      float h = a.eps * a.eps - SI;
      h = h < 0.0f ? 0.0f : h;
      const float f = sqrtf(h + SU) / sqrtf(SN);
      float td[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        n[e] = in1[e] ? n[e] * f : in2[e] ? 0.0f : d[e];     // d'
        td[e] = n[e] * n[e];
      }
      const float SD = row_block_sum(sum4(td), part[4], wave, lane);
      // 5
      const float t = sqrtf(SD);
      if (!(SN == 0.0f || SD == 0.0f)) {
        out.x = clamp_nan_passes(c.x + (n[0] / t) * a.eps, a.lo, a.hi);
        out.y = clamp_nan_passes(c.y + (n[1] / t) * a.eps, a.lo, a.hi);
        out.z = clamp_nan_passes(c.z + (n[2] / t) * a.eps, a.lo, a.hi);
        out.w = clamp_nan_passes(c.w + (n[3] / t) * a.eps, a.lo, a.hi);
      }
    }
    if (own) reinterpret_cast<float4*>(a.x_cand)[at] = out;
  }
  if (tid == 0)
    reinterpret_cast<int4*>(a.state)[i] = int4{__float_as_int(margin_best), used, done ? 1 : 0, spare};
}

void launch_square_l2_init(const SquareL2InitArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("square_l2_init: image count out of range");
  if (!a.x0 || !a.x_cand || !a.table) throw std::runtime_error("square_l2_init: null argument");
  if (misaligned(15, a.x0, a.x_cand))
    throw std::runtime_error("square_l2_init: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(3, a.table)) throw std::runtime_error("square_l2_init: the pattern table must be 4-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("square_l2_init: eps must be >= 0");
  if ((uint64_t)a.id_base + (uint64_t)M > (1ull << 32))
    throw std::runtime_error("square_l2_init: id_base + M must not exceed 2^32");
  hipLaunchKernelGGL(square_l2_init_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void launch_square_l2_step(const SquareL2StepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("square_l2_step: image count out of range");
  if (!a.logp || !a.y || !a.x0 || !a.x_best || !a.x_cand || !a.state || !a.table)
    throw std::runtime_error("square_l2_step: null argument");
  if (misaligned(15, a.x0, a.x_best, a.x_cand))
    throw std::runtime_error("square_l2_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.state)) throw std::runtime_error("square_l2_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.logp, a.y, a.table))
    throw std::runtime_error("square_l2_step: logp, y and the pattern table must be 4-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("square_l2_step: eps must be >= 0");
  if (a.side < SQUARE_L2_MIN_SIDE || a.side > SQUARE_L2_MAX_SIDE || a.side % 2 == 0)
    throw std::runtime_error("square_l2_step: the side must be odd and in [3, 27]");
  if ((uint64_t)a.id_base + (uint64_t)M > (1ull << 32))
    throw std::runtime_error("square_l2_step: id_base + M must not exceed 2^32");
  hipLaunchKernelGGL(square_l2_step_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_square_l2() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&square_l2_step_kernel));
}

}  // namespace mnist
