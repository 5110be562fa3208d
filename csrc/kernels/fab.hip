// The Fast Adaptive Boundary attack (Croce & Hein, ICML 2020): one untargeted FAB iteration per image on the
// normalised image, fp32, in the L-inf or the L2 norm.
//
// Image i of a chunk of M owns the ten rows 10 i + c of the row buffer and of the gradient buffer, as in deepfool.hip:
// dx[10 i + c] = g_c = d NLL_c / d x, loss_rows[10 i + c] = -log p_c.  One workgroup of 256 threads per image; thread
// t < 196 owns the float4 t of each row.  With y = y[i], f_k = loss_y - loss_k, w_k = g_y - g_k and q the dual
// exponent (1 for L-inf, 2 for L2), and |.| the norm of the launch:
//
//   1. status[i] != FAB_RUNNING: the workgroup stores nothing (frozen).  y outside [0, 10): FAB_STUCK.
//   2. crossed (some loss_k < loss_y, or == with k < y): the backward step.  u = |x - x0|; u < norm_best[i]:
//      x_best[i] = x, norm_best[i] = u.  u == 0 (the clean point is outside its class): status[i] = FAB_DONE.
//      Otherwise, unless `last`: x = clamp(x0 + beta (x - x0)) into x[i] and the ten rows, iters[i] += 1.  (The
//      clamp binds only when the rounding of x0 + (x - x0) leaves the box by an ulp.)
//   3. not crossed and `last`: nothing is stored.
//   4. l = the first smallest (|f_k| + DF_SLACK) / |w_k|_q in ascending k under a strict <; a class with
//      |w_k|_q < PGD_L2_TINY or a NaN ratio is skipped.  No class left: if some ratio was a NaN (a NaN in g_y makes
//      every one a NaN) x[i], the ten rows and proj become NaN and iters[i] += 1 - the NaN is seen, not swallowed;
//      otherwise status[i] = FAB_STUCK and nothing else is stored.
//   5. w = w_l, r1 = f_l, r2 = f_l + sum w (x0 - x);  d1 = P(x, r1), d2 = P(x0, r2);  n1 = |d1|, n2 = |d2|;
//      alpha = min(n1 / (n1 + n2), alpha_max), 0 when n1 + n2 is not positive;
//      x = clamp((1 - alpha) (x + eta d1) + alpha (x0 + eta d2), lo, hi) into x[i] and the ten rows (a NaN passes
//      the clamp), iters[i] += 1; proj[i] = {d1, d2} when given.
//
// P(v, r): the delta of smallest norm with r + w . delta = 0 and lo <= v + delta <= hi.  Per element a = |w|, the
// direction d = -sgn(r) sgn(w), room = (d > 0 ? hi - v : v - lo) floored at 0, c = 1 (L-inf) or a (L2);
// delta = d min(tau c, room) with tau the smallest root of g(tau) = sum a min(tau c, room) = |r|.  Elements with
// a = 0 (or a NaN a) take no part: delta = 0.  g is piecewise linear with the breakpoints tau_e = room / c; on the
// sorted breakpoints g(tau_k) = R_k + tau_k S_k, R_k the sum of a room over the positions before k, S_k the sum of a c
// over the positions from k on.  k = the first position with g(tau_k) >= |r|, tau = (|r| - R_k) / S_k; no such
// position (the hyperplane misses the box): tau = +inf, every element goes to its bound.
//
// HOW THE WORK IS SPLIT.  Both projections run side by side and share every barrier.
//   sort   1024 slots a projection (784 breakpoints, the rest +inf) as 64-bit keys (bits of tau_e << 32 | e): the keys
//          are distinct, so the order is total and the hundreds of equal breakpoints of a flat background cannot
//          reorder the sums.  Thread t keeps the slots 4 t .. 4 t + 3 in registers through the whole bitonic network:
//          the strides 1 and 2 are compare-exchanges between its own registers, the strides 4 .. 128 reach a lane
//          of the same wave (cross-lane moves, no barrier), and only the three stages of stride 256 / 512 go
//          through LDS, two buffers in turn, one barrier each.
//   gather a room and a c were stored by element in LDS before the sort; each thread reads its four sorted slots'.
//   scan   R (forward) and S (backward) in a fixed order: four serial per thread, the wave by cross-lane moves
//          (Hillis-Steele over shfl_up / shfl_down), the four wave totals through LDS added in wave order.
//   pick   each thread's first slot with g >= |r| as (position << 32 | bits of its tau): the minimum over the wave by
//          cross-lane moves, over the four waves through LDS.  Positions are distinct: one tau wins, always the same.
// No atomics; every operation is rounded on its own (contraction off); nothing depends on the grid, the stream or
// the launch count: the same operands give the same bits.  Every early exit is taken by the whole workgroup (status,
// y, loss_rows and LDS sums decide, which every thread reads alike).  norm_best[i] is read by every thread and
// written by thread 0: a full barrier stands between.  The grid is exactly M workgroups: nothing past M is touched.
// Every LDS index is a slot number 4 t + s or a key's low ten bits: below 1024 whatever the operands hold.
//
// RESOURCES (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   fab_step_kernel<FAB_LINF>: VGPRs 94, SGPRs 78, LDS 45376 B, scratch 0, occupancy 3 waves / SIMD (LDS bound)
//   fab_step_kernel<FAB_L2>:   VGPRs 96, SGPRs 78, LDS 45376 B, scratch 0, occupancy 3
// As in deepfool_step, g_y, the chosen row and its loss are read by address and every index into registers is a
// counter of an unrolled loop: no scratch.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
constexpr int FAB_SLOTS = 1024, FAB_PER = 4;             // sorted slots a projection, slots a thread
static_assert(ROW_THREADS * FAB_PER == FAB_SLOTS && IMG * IMG <= FAB_SLOTS, "four slots per thread hold a row");
constexpr int FAB_OTHERS = DF_CLASSES - 1;
constexpr uint32_t FAB_INF_BITS = 0x7f800000u;

__device__ __forceinline__ float fab_abs_sum4(const float4& v) {
#pragma clang fp contract(off)
  return (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
}
__device__ __forceinline__ float fab_abs_max4(const float4& v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ float4 fab_sub4(const float4& a, const float4& b) {
#pragma clang fp contract(off)
  return float4{a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
}
__device__ __forceinline__ float fab_back(float c, float x, float beta, float lo, float hi) {
#pragma clang fp contract(off)
  const float t = x - c;
  const float s = beta * t;
  return clamp_nan_passes(c + s, lo, hi);
}
__device__ __forceinline__ float fab_mix(float x, float c, float d1, float d2, float eta, float al, float om, float lo,
                                         float hi) {
#pragma clang fp contract(off)
  const float t1 = eta * d1;
  const float p1 = x + t1;
  const float t2 = eta * d2;
  const float p2 = c + t2;
  const float m1 = om * p1;
  const float m2 = al * p2;
  return clamp_nan_passes(m1 + m2, lo, hi);
}
__device__ __forceinline__ float fab_sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// the norm of the launch over the workgroup: the fixed tree of row_block_sum (L2) or the maximum (L-inf, exact in
// any order); `part`: this reduction's own ROW_WAVES words, after a barrier of the caller's
template <int NORM>
__device__ __forceinline__ float fab_wave_norm(const float4& d) {
  if constexpr (NORM == FAB_L2) return wave_sum(row_sq4(d));
  else return wave_max(fab_abs_max4(d));
}
template <int NORM>
__device__ __forceinline__ float fab_waves_norm(const float* part) {
  if constexpr (NORM == FAB_L2) return sqrtf(row_waves_sum(part));
  else return fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

__device__ __forceinline__ void fab_cmpx(uint64_t& a, uint64_t& b, bool asc) {   // a before b when ascending
  const uint64_t mn = a < b ? a : b, mx = a < b ? b : a;
  a = asc ? mn : mx;
  b = asc ? mx : mn;
}
}  // namespace

template <int NORM>
__global__ __launch_bounds__(ROW_THREADS) void fab_step_kernel(FabStepArgs a) {
#pragma clang fp contract(off)
  __shared__ uint64_t ex[2][2][FAB_SLOTS];                // the sort's LDS stages: [buffer][projection][slot]
  __shared__ float ar[2][FAB_SLOTS];                      // a room by element, per projection
  __shared__ float ac[FAB_SLOTS];                         // a c by element (the same w in both projections)
  __shared__ float part[FAB_OTHERS + 3][ROW_WAVES];       // the nine class norms, r2's sum, n1, n2
  __shared__ float scan[4][ROW_WAVES];                    // wave totals: R of P1, R of P2, S of P1, S of P2
  __shared__ uint64_t hit[2][ROW_WAVES];                  // the waves' first crossing slot, per projection
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  RW_ENTRY();
  if (a.status[i] != FAB_RUNNING) return;                 // 1. frozen
  const int y = a.y[i];
  if (y < 0 || y >= DF_CLASSES) {
    if (tid == 0) a.status[i] = FAB_STUCK;
    return;
  }
  const float* lrow = a.loss_rows + i * DF_CLASSES;
  const float ly = lrow[y];
  float loss[DF_CLASSES];
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) loss[k] = lrow[k];
  bool crossed = false;
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) crossed = crossed || (k != y && (loss[k] < ly || (loss[k] == ly && k < y)));

  const int64_t at = i * ROW_VECS + (own ? tid : 0);      // (idle threads: a valid address, zeros in the registers)
  const float4 zero4{0.0f, 0.0f, 0.0f, 0.0f};
  float4 x = reinterpret_cast<const float4*>(a.x)[at];
  float4 c = reinterpret_cast<const float4*>(a.x0)[at];
  if (!own) x = c = zero4;
  float4* row = reinterpret_cast<float4*>(a.rows) + i * (DF_CLASSES * ROW_VECS) + tid;

  if (crossed) {                                          // 2. the backward step
    const float nb = a.norm_best[i];
    __syncthreads();                                      // every wave holds norm_best before thread 0 stores it
    const float m = fab_wave_norm<NORM>(fab_sub4(x, c));
    if (lane == 0) part[0][wave] = m;
    lds_barrier();
    const float u = fab_waves_norm<NORM>(part[0]);
    if (u < nb) {
      if (own) reinterpret_cast<float4*>(a.x_best)[at] = x;
      if (tid == 0) a.norm_best[i] = u;
    }
    if (u == 0.0f) {
      if (tid == 0) a.status[i] = FAB_DONE;
      return;
    }
    if (a.last) return;
    const float4 o{fab_back(c.x, x.x, a.beta, a.lo, a.hi), fab_back(c.y, x.y, a.beta, a.lo, a.hi),
                   fab_back(c.z, x.z, a.beta, a.lo, a.hi), fab_back(c.w, x.w, a.beta, a.lo, a.hi)};
    if (own) {
      reinterpret_cast<float4*>(a.x)[at] = o;
#pragma unroll
      for (int k = 0; k < DF_CLASSES; ++k) row[k * ROW_VECS] = o;
    }
    if (tid == 0) a.iters[i] = a.iters[i] + 1;
    return;
  }
  if (a.last) return;                                     // 3.

  // 4. the nearest linearised boundary in the dual norm
  const float4* grow = reinterpret_cast<const float4*>(a.dx) + i * (DF_CLASSES * ROW_VECS) + (own ? tid : 0);
  const float4 gy = grow[y * ROW_VECS];
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) {
    if (k == y) continue;
    const float4 wk = fab_sub4(gy, grow[k * ROW_VECS]);
    const float s = wave_sum(own ? (NORM == FAB_L2 ? row_sq4(wk) : fab_abs_sum4(wk)) : 0.0f);
    if (lane == 0) part[k - (k > y ? 1 : 0)][wave] = s;
  }
  lds_barrier();
  int l = -1, l_nan = -1;
  float best = 0.0f;
#pragma unroll
  for (int k = 0; k < DF_CLASSES; ++k) {
    if (k == y) continue;
    const float sum = row_waves_sum(part[k - (k > y ? 1 : 0)]);
    const float n = NORM == FAB_L2 ? sqrtf(sum) : sum;
    const float ratio = (fabsf(ly - loss[k]) + DF_SLACK) / n;
    if (ratio != ratio) {
      if (l_nan < 0) l_nan = k;
    } else if (!(n < PGD_L2_TINY) && (l < 0 || ratio < best)) {
      l = k; best = ratio;
    }
  }
  float4* pj = a.proj ? reinterpret_cast<float4*>(a.proj) + i * (2 * ROW_VECS) + tid : nullptr;
  if (l < 0) {
    if (l_nan < 0) {
      if (tid == 0) a.status[i] = FAB_STUCK;
      return;
    }
    const float qn = __builtin_nanf("");
    const float4 o{qn, qn, qn, qn};
    if (own) {
      reinterpret_cast<float4*>(a.x)[at] = o;
#pragma unroll
      for (int k = 0; k < DF_CLASSES; ++k) row[k * ROW_VECS] = o;
      if (pj) { pj[0] = o; pj[ROW_VECS] = o; }
    }
    if (tid == 0) a.iters[i] = a.iters[i] + 1;
    return;
  }

  // 5. the two hyperplane projections
  float4 w4 = fab_sub4(gy, grow[l * ROW_VECS]);            // (the chosen row again: a cache hit, not a register array)
  if (!own) w4 = zero4;
  const float r1 = ly - lrow[l];
  {
    const float4 t = fab_sub4(c, x);
    const float s = wave_sum((w4.x * t.x + w4.y * t.y) + (w4.z * t.z + w4.w * t.w));
    if (lane == 0) part[FAB_OTHERS][wave] = s;
  }
  lds_barrier();
  const float r2 = r1 + row_waves_sum(part[FAB_OTHERS]);
  const float rr[2] = {r1, r2};
  const float ra[2] = {fabsf(r1), fabsf(r2)};
  const float wv[FAB_PER] = {w4.x, w4.y, w4.z, w4.w};
  const float vv[2][FAB_PER] = {{x.x, x.y, x.z, x.w}, {c.x, c.y, c.z, c.w}};
  float dir[2][FAB_PER], room[2][FAB_PER], cc[FAB_PER];
  bool act[FAB_PER];
  uint64_t key[2][FAB_PER];
#pragma unroll
  for (int s = 0; s < FAB_PER; ++s) {
    const float aw = fabsf(wv[s]);
    act[s] = aw > 0.0f;
    cc[s] = NORM == FAB_L2 ? aw : 1.0f;
    ac[FAB_PER * tid + s] = act[s] ? aw * cc[s] : 0.0f;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float d = -(fab_sgn(rr[p]) * fab_sgn(wv[s]));
      float rm = d > 0.0f ? a.hi - vv[p][s] : vv[p][s] - a.lo;
      rm = rm < 0.0f ? 0.0f : rm;
      dir[p][s] = d;
      room[p][s] = rm;
      ar[p][FAB_PER * tid + s] = act[s] ? aw * rm : 0.0f;
      const uint32_t tb = act[s] ? (__float_as_uint(rm / cc[s]) & 0x7fffffffu) : FAB_INF_BITS;
      key[p][s] = ((uint64_t)tb << 32) | (uint32_t)(FAB_PER * tid + s);
    }
  }

  // the bitonic network over the 1024 slots: slot n = 4 tid + s
  int buf = 0;
#pragma unroll
  for (int k = 2; k <= FAB_SLOTS; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < FAB_PER) {                                  // both slots in this thread's registers
#pragma unroll
        for (int s = 0; s < FAB_PER; ++s) {
          if (s & j) continue;
          const bool asc = ((FAB_PER * tid + s) & k) == 0;
#pragma unroll
          for (int p = 0; p < 2; ++p) fab_cmpx(key[p][s], key[p][s | j], asc);
        }
      } else {                                            // the partner slot is slot s of thread tid ^ (j / 4)
        const int pt = j / FAB_PER;
        const bool keep_min = ((tid & pt) == 0) == (((FAB_PER * tid) & k) == 0);
        uint64_t other[2][FAB_PER];
        if (pt < 64) {                                    // a lane of this wave
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int s = 0; s < FAB_PER; ++s) other[p][s] = __shfl_xor(key[p][s], pt, 64);
        } else {                                          // another wave: through LDS
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int s = 0; s < FAB_PER; ++s) ex[buf][p][FAB_PER * tid + s] = key[p][s];
          lds_barrier();
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int s = 0; s < FAB_PER; ++s) other[p][s] = ex[buf][p][FAB_PER * (tid ^ pt) + s];
          buf ^= 1;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < FAB_PER; ++s) {
            const bool less = key[p][s] < other[p][s];
            key[p][s] = (less == keep_min) ? key[p][s] : other[p][s];
          }
      }
    }
  }

  // gather in sorted order, scan: R before each slot, S from each slot on
  float tau_s[2][FAB_PER], Rk[2][FAB_PER], Sk[2][FAB_PER], rex[2], sex[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float gr[FAB_PER], gs[FAB_PER];
#pragma unroll
    for (int s = 0; s < FAB_PER; ++s) {
      const int e = (int)((uint32_t)key[p][s] & (FAB_SLOTS - 1));
      gr[s] = ar[p][e];
      gs[s] = ac[e];
      tau_s[p][s] = __uint_as_float((uint32_t)(key[p][s] >> 32));
    }
    Rk[p][0] = 0.0f;
    Rk[p][1] = gr[0];
    Rk[p][2] = gr[0] + gr[1];
    Rk[p][3] = Rk[p][2] + gr[2];
    float v = Rk[p][3] + gr[3];
    Sk[p][3] = gs[3];
    Sk[p][2] = gs[3] + gs[2];
    Sk[p][1] = Sk[p][2] + gs[1];
    Sk[p][0] = Sk[p][1] + gs[0];
    float u = Sk[p][0];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float tv = __shfl_up(v, o, 64), tu = __shfl_down(u, o, 64);
      if (lane >= o) v = v + tv;
      if (lane + o < 64) u = u + tu;
    }
    const float ev = __shfl_up(v, 1, 64), eu = __shfl_down(u, 1, 64);
    rex[p] = lane == 0 ? 0.0f : ev;
    sex[p] = lane == 63 ? 0.0f : eu;
    if (lane == 63) scan[p][wave] = v;
    if (lane == 0) scan[2 + p][wave] = u;
  }
  lds_barrier();
  uint64_t cand[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float* tr = scan[p];
    const float* ts = scan[2 + p];
    const float r01 = tr[0] + tr[1], s32 = ts[3] + ts[2];
    const float roff = wave == 0 ? 0.0f : wave == 1 ? tr[0] : wave == 2 ? r01 : r01 + tr[2];
    const float soff = wave == 3 ? 0.0f : wave == 2 ? ts[3] : wave == 1 ? s32 : s32 + ts[1];
    const float rb = roff + rex[p], sb = soff + sex[p];
    cand[p] = ((uint64_t)FAB_SLOTS << 32) | FAB_INF_BITS;   // no crossing: tau = +inf
#pragma unroll
    for (int s = FAB_PER - 1; s >= 0; --s) {              // descending: the first slot wins
      const float R = rb + Rk[p][s], S = sb + Sk[p][s];
      const float ts_ = tau_s[p][s] * S;
      const float g = R + ts_;
      if (g >= ra[p]) {
        const float num = ra[p] - R;
        cand[p] = ((uint64_t)(uint32_t)(FAB_PER * tid + s) << 32) | __float_as_uint(num / S);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint64_t t = __shfl_xor(cand[p], o, 64);
      cand[p] = t < cand[p] ? t : cand[p];
    }
    if (lane == 0) hit[p][wave] = cand[p];
  }
  lds_barrier();
  float dl[2][FAB_PER];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint64_t h01 = hit[p][0] < hit[p][1] ? hit[p][0] : hit[p][1];
    const uint64_t h23 = hit[p][2] < hit[p][3] ? hit[p][2] : hit[p][3];
    const float tau = __uint_as_float((uint32_t)(h01 < h23 ? h01 : h23));
#pragma unroll
    for (int s = 0; s < FAB_PER; ++s) {
      const float t = tau * cc[s];
      const float mn = t < room[p][s] ? t : room[p][s];
      dl[p][s] = act[s] ? dir[p][s] * mn : 0.0f;
    }
  }
  const float4 d1{dl[0][0], dl[0][1], dl[0][2], dl[0][3]}, d2{dl[1][0], dl[1][1], dl[1][2], dl[1][3]};
  {
    const float m1 = fab_wave_norm<NORM>(d1), m2 = fab_wave_norm<NORM>(d2);
    if (lane == 0) {
      part[FAB_OTHERS + 1][wave] = m1;
      part[FAB_OTHERS + 2][wave] = m2;
    }
  }
  lds_barrier();
  const float n1 = fab_waves_norm<NORM>(part[FAB_OTHERS + 1]), n2 = fab_waves_norm<NORM>(part[FAB_OTHERS + 2]);
  const float ns = n1 + n2;
  float al = ns > 0.0f ? n1 / ns : 0.0f;
  al = al < a.alpha_max ? al : a.alpha_max;
  const float om = 1.0f - al;
  const float4 o{fab_mix(x.x, c.x, d1.x, d2.x, a.eta, al, om, a.lo, a.hi),
                 fab_mix(x.y, c.y, d1.y, d2.y, a.eta, al, om, a.lo, a.hi),
                 fab_mix(x.z, c.z, d1.z, d2.z, a.eta, al, om, a.lo, a.hi),
                 fab_mix(x.w, c.w, d1.w, d2.w, a.eta, al, om, a.lo, a.hi)};
  if (own) {
    reinterpret_cast<float4*>(a.x)[at] = o;
#pragma unroll
    for (int k = 0; k < DF_CLASSES; ++k) row[k * ROW_VECS] = o;
    if (pj) { pj[0] = d1; pj[ROW_VECS] = d2; }
  }
  if (tid == 0) a.iters[i] = a.iters[i] + 1;
}

void launch_fab_step(const FabStepArgs& a, int M, int norm, hipStream_t s) {
  if (M < 1 || M > DF_MAX_M) throw std::runtime_error("fab_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.y || !a.x0 || !a.x || !a.x_best || !a.norm_best || !a.rows || !a.status || !a.iters)
    throw std::runtime_error("fab_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.x, a.x_best, a.rows, a.proj))
    throw std::runtime_error("fab_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(3, a.loss_rows, a.y, a.norm_best, a.status, a.iters))
    throw std::runtime_error("fab_step: the per-image vectors must be 4-byte aligned");
  if (norm != FAB_LINF && norm != FAB_L2) throw std::runtime_error("fab_step: unknown norm");
  if (!(a.eta >= 1.0f)) throw std::runtime_error("fab_step: eta must be >= 1");
  if (!(a.beta > 0.0f && a.beta <= 1.0f)) throw std::runtime_error("fab_step: beta must be in (0, 1]");
  if (!(a.alpha_max >= 0.0f && a.alpha_max <= 1.0f)) throw std::runtime_error("fab_step: alpha_max must be in [0, 1]");
  if (norm == FAB_L2)
    hipLaunchKernelGGL(fab_step_kernel<FAB_L2>, dim3(M), dim3(ROW_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(fab_step_kernel<FAB_LINF>, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_fab() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fab_step_kernel<FAB_LINF>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fab_step_kernel<FAB_L2>));
}

}  // namespace mnist
