// L1 Auto-PGD (Croce & Hein, ICML 2021: "Mind the box: l1-APGD for sparse adversarial attacks on image classifiers")
// on the normalised image, fp32 [M][784]: the whole per-image update of one iteration in one launch - the best point,
// the checkpoint rule driven by the sparsity of the best point, the sparse steepest-ascent step on the top-k
// coordinates of the gradient and the exact Euclidean projection onto the INTERSECTION of the L1 ball around x0 and
// the pixel box.  (Projecting onto the ball and clamping afterwards wastes the budget on the ~70 % of MNIST pixels
// that sit at `lo` and have no room downwards.)
//
// One workgroup of ROW_THREADS per image, thread t < 196 owns the float4 t of each of the image's rows.  After the
// gradient chain at the iterate x: dx (input_grad's plain output), loss_rows (head_train / head_margin).  With
// L = sign * loss_rows[i], g = sign * dx[i], n = 784:
//
//   first:   eta = eps; loss_best = L; x_best = x; g_best = dx; k_sel = 157 (= n - floor(0.8 n)); sp_old = n;
//            iters = 0; restarted = 0; (src, gs) = (x, g)                 -- reads no state, writes all of it
//   else:    if L > loss_best: loss_best = L; x_best = x; g_best = dx      (a NaN loss never becomes the best)
//            last: store the records and stop (x and every other field keep their values)
//            (src, gs) = (x, g); restarted = 0
//            window > 0 (a checkpoint):
//                sp    = #{ e : x_best[e] != x0[e] }    (the best point as it is now: this launch's x if it improved)
//                red   = 100 sp < 95 sp_old             (integers)
//                k_sel = clamp((2 sp + 2) / 3, 1, n)    (integer division: ceil(2 sp / 3))
//                red:  eta = eps; (src, gs) = (x_best, sign * g_best); restarted = 1
//                else: eta = max(eta / 1.5, eps / 10)
//                sp_old = sp
//   step:    thr  = the k_sel-th largest |gs[e]| of the row (a value: ties cannot change it)
//            sel  = { e : |gs[e]| >= thr and gs[e] != 0 };  m = |sel|     (ties at thr are all taken)
//            t[e] = src[e] + (eta / max(m, 1)) * sgn(gs[e]) on sel, src[e] elsewhere
//   project: z = t - x0; s = sgn(z); a = |z|; cap = max(s > 0 ? hi - x0 : x0 - lo, 0); w = min(a, cap)
//            eps == 0:          d = s * 0, lam = 0                        (x = x0 exactly)
//            sum w <= eps:      d = s * w, lam = 0
//            otherwise:         d = s * min(max(a - lam, 0), cap), lam the root of
//                               phi(lam) = sum min(max(a - lam, 0), cap) = eps
//            x = clamp_nan_passes(x0 + d, lo, hi); iters += 1             (the clamp binds only by a rounding ulp)
//
// THE ROOT.  With b = max(a - cap, 0), phi(lam) = sum_{a_e > lam} (a_e - lam) - sum_{b_e > lam} (b_e - lam): piecewise
// linear and decreasing with the 1568 breakpoints {a_e} u {b_e}.  On the ascending breakpoints tau_k, with S_k the sum
// over the positions >= k of +a_e / -b_e and N_k the same sum of +-1, phi(tau_k) = S_k - tau_k N_k.  k = the first
// position with N_k > 0 and phi(tau_k) <= eps; lam = (S_k - eps) / N_k.  (N_k = 0 is a flat piece of phi: it cannot
// hold the first crossing but through rounding, and is passed over.)
//
// HOW THE WORK IS SPLIT.  One bitonic network (l1_sort), written once, templated on the key type and the slots a
// thread keeps: every thread holds its slots in registers through the whole network; strides below the slots a thread
// are compare-exchanges between its own registers, strides inside a wave are cross-lane moves (no barrier), and only
// the three stages whose partner sits in another wave go through LDS, two buffers in turn, one barrier each.
//   select   1024 int32 keys, four a thread: the bits of |gs| (non-negative floats order as integers), -1 in the
//            240 padding slots, below every real key.  thr is the key at position 1024 - k_sel; its owner finds it
//            with a compare of slot numbers in an unrolled loop (no indexed register array) and publishes it through
//            one LDS word.  The selection compares keys, so a NaN |gs| (above every number) is always selected and
//            shows in x.  The network was chosen over a radix / ballot select because it is the code the projection
//            needs anyway (one network to get right).  By the stage counts and key widths - 55 stages on four 32-bit
//            keys a thread against 66 on eight 64-bit keys - it should cost about a fifth of the projection's sort:
//            an estimate, the two sorts were not timed apart and no select-only variant was measured.
//   project  2048 uint64 keys, eight a thread: bits(tau) << 32 | slot id, a-breakpoints ids 0..783, b-breakpoints
//            1024..1807, the rest +inf.  The keys are distinct, so the order is total and the hundreds of equal
//            breakpoints of a flat background cannot reorder a sum.  The sort runs only when sum w > eps, a branch
//            every thread takes alike (the sum is read from LDS).
//   scan     a key carries its own breakpoint value in its high word and its kind in its id, so the sorted terms
//            +a / -b are read off the registers - nothing is gathered from LDS and no LDS index is ever derived
//            from a key.  S is a backward scan in a fixed order: eight serial per thread, Hillis-Steele over
//            shfl_down across the wave, the four wave totals through LDS added in wave order; N the same in integers.
//            S, phi and the quotient are float64 (a few dozen operations a thread): S_k cancels +a against -b of the
//            pixels far past the box and then eps against S_k, and a float32 S_k, a few ulps of 30 .. 100 off, left
//            lam off by up to 1.2e-6 on the iterates of a real attack, 16 times what four times the float32
//            reference's own error allows (its cumulative sum on the CPU is a float64 one).  lam is rounded once.
//   pick     each thread's first slot that crosses as (position << 32 | bits of its lam): the minimum over the wave
//            by cross-lane moves, over the four waves through LDS.  Positions are distinct: one lam wins.
// sp, m and N are integer counts, exact in any order.  No atomics; every float operation is rounded on its own
// (contraction off, no packed fp32); nothing depends on the grid, the stream or the launch count: the same operands
// give the same bits.  Every early exit is taken by the whole workgroup (launch flags, records and LDS sums decide).
//
// STATE: two 16-byte records an image (kernels.h); every thread loads them, thread 0 stores them, a __syncthreads
// stands between.  Row elements are read and written by their owner only and read before they are written.  The
// grid is exactly M workgroups: nothing past M is touched.
//
// NaN: a NaN loss never becomes the best (L > loss_best is false; the first launch stores the loss it is given).  A
// NaN gradient element is selected (its key is above every number), makes t, a, sum w and every S_k that covers it
// NaN, no position crosses, lam = NaN and the image's whole x is NaN - that image's only.  Under eps == 0 no sum is
// taken: lam = 0, x = x0, and the NaN shows in the element it entered by (d = s * 0 with s = NaN) and in no other.
// A record from elsewhere (k_sel outside [1, 784] on a launch that is no checkpoint) selects with the clamped slot and
// is stored as it came; no memory index is derived from it.
//
// RESOURCES (the build's flags: hipcc -O3 --offload-arch=gfx950 -munsafe-fp-atomics -fno-slp-vectorize
// -Xclang -target-feature -Xclang -packed-fp32-ops, with -Rpass-analysis=kernel-resource-usage):
//   apgd_l1_step_kernel: VGPRs 79, SGPRs 106 (28 kept in VGPR lanes), LDS 32904 B, scratch 0, occupancy 4 waves /
//   SIMD (LDS bound: four workgroups a CU).  The two 16 KB sort buffers are the whole of the LDS: the sorted terms
//   come out of the keys, so there is no 8 KB value array to gather from.
// x_best and g_best are re-read by address, every index into a register array is a counter of an unrolled loop.
#include "../runtime/host_logic.h"
#include "row_ops.h"

namespace mnist {

namespace {
constexpr int L1_N = IMG * IMG;                            // 784
constexpr int L1_SEL_PER = 4, L1_SEL_SLOTS = ROW_THREADS * L1_SEL_PER;        // 1024 int32 keys
constexpr int L1_PRJ_PER = 8, L1_PRJ_SLOTS = ROW_THREADS * L1_PRJ_PER;        // 2048 uint64 keys
static_assert(L1_N <= L1_SEL_SLOTS && L1_SEL_SLOTS + L1_N <= L1_PRJ_SLOTS, "a ids below 1024, b ids from 1024 on");
constexpr uint32_t L1_INF_BITS = 0x7f800000u, L1_NAN_BITS = 0x7fc00000u, L1_ABS = 0x7fffffffu;

__device__ __forceinline__ float l1_sgn(float s) { return s > 0.0f ? 1.0f : s < 0.0f ? -1.0f : s == s ? 0.0f : s; }

template <class K>
__device__ __forceinline__ void l1_cmpx(K& a, K& b, bool asc) {   // a before b when ascending
  const K mn = a < b ? a : b, mx = a < b ? b : a;
  a = asc ? mn : mx;
  b = asc ? mx : mn;
}

// ascending bitonic sort of ROW_THREADS * PER keys, slot n = PER * tid + s in key[s]; `ex`: 2 * ROW_THREADS * PER
// keys of LDS that no wave still reads (a barrier of the caller's stands before)
template <class K, int PER>
__device__ __forceinline__ void l1_sort(K (&key)[PER], K* ex, int tid) {
  constexpr int SLOTS = ROW_THREADS * PER;
  int buf = 0;
#pragma unroll
  for (int k = 2; k <= SLOTS; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < PER) {                                       // both slots in this thread's registers
#pragma unroll
        for (int s = 0; s < PER; ++s) {
          if (s & j) continue;
          l1_cmpx(key[s], key[s | j], ((PER * tid + s) & k) == 0);
        }
      } else {                                             // the partner slot is slot s of thread tid ^ (j / PER)
        const int pt = j / PER;
        const bool keep_min = ((tid & pt) == 0) == (((PER * tid) & k) == 0);
        K other[PER];
        if (pt < 64) {                                     // a lane of this wave
#pragma unroll
          for (int s = 0; s < PER; ++s) other[s] = __shfl_xor(key[s], pt, 64);
        } else {                                           // another wave: through LDS
          K* e = ex + buf * SLOTS;
#pragma unroll
          for (int s = 0; s < PER; ++s) e[PER * tid + s] = key[s];
          lds_barrier();
#pragma unroll
          for (int s = 0; s < PER; ++s) other[s] = e[PER * (tid ^ pt) + s];
          buf ^= 1;
        }
#pragma unroll
        for (int s = 0; s < PER; ++s) {
          const bool less = key[s] < other[s];
          key[s] = (less == keep_min) ? key[s] : other[s];
        }
      }
    }
  }
}

// an integer count over the workgroup (exact in any order); `part`: this count's own ROW_WAVES words
__device__ __forceinline__ int l1_block_count(int v, int* part, int wave, int lane) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) part[wave] = v;
  lds_barrier();
  return (part[0] + part[1]) + (part[2] + part[3]);
}
}  // namespace

__global__ __launch_bounds__(ROW_THREADS) void apgd_l1_step_kernel(ApgdL1StepArgs a) {
#pragma clang fp contract(off)
  __shared__ uint64_t ex[2 * L1_PRJ_SLOTS];                // the sorts' LDS stages (the select uses a quarter)
  __shared__ int cnt[2][ROW_WAVES];                        // sp, m
  __shared__ float part[ROW_WAVES];                        // sum w
  __shared__ double scan_s[ROW_WAVES];                     // wave totals of S
  __shared__ int scan_n[ROW_WAVES];                        // ... of N
  __shared__ uint64_t hit[ROW_WAVES];                      // the waves' first crossing slot
  __shared__ int thr_w;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool own = tid < ROW_VECS;
  const int64_t i = blockIdx.x;
  const int64_t at = i * ROW_VECS + (own ? tid : 0);       // (idle threads: a valid address, zeros in the registers)
  RW_ENTRY();
  const float L = a.sign * a.loss_rows[i];
  const float4 zero4{0.0f, 0.0f, 0.0f, 0.0f};
  float4 dx = reinterpret_cast<const float4*>(a.dx)[at];
  float4 x = reinterpret_cast<const float4*>(a.x)[at];
  float4 c = reinterpret_cast<const float4*>(a.x0)[at];
  if (!own) dx = x = c = zero4;

  float eta, loss_best, lam, thr;
  int k_sel, sp_old, iters, restarted = 0;
  bool improved;
  if (a.first) {
    eta = a.eps;
    loss_best = L;
    lam = thr = 0.0f;
    k_sel = L1_N - (L1_N * 4) / 5;                         // 157
    sp_old = L1_N; iters = 0;
    improved = true;                                       // x_best = x, g_best = dx
  } else {
    const float4 f = reinterpret_cast<const float4*>(a.fstate)[i];
    const int4 n = reinterpret_cast<const int4*>(a.istate)[i];
    // every wave holds the old records before thread 0 stores: it matters on the `last` exit, where the store follows
    // at once; on every other path LDS barriers stand before the store as well
    __syncthreads();
    eta = f.x; loss_best = f.y; lam = f.z; thr = f.w;
    k_sel = n.x; sp_old = n.y; iters = n.z; restarted = n.w;
    improved = L > loss_best;
    if (improved) loss_best = L;
  }
  if (improved && own) {
    reinterpret_cast<float4*>(a.x_best)[at] = x;
    reinterpret_cast<float4*>(a.g_best)[at] = dx;
  }
  if (a.last && !a.first) {
    if (tid == 0) {
      reinterpret_cast<float4*>(a.fstate)[i] = float4{eta, loss_best, lam, thr};
      reinterpret_cast<int4*>(a.istate)[i] = int4{k_sel, sp_old, iters, restarted};
    }
    return;
  }

  float4 src = x, gb = dx;
  if (!a.first) {
    restarted = 0;
    if (a.window > 0) {                                    // a checkpoint
      float4 xb = x;
      if (!improved && own) xb = reinterpret_cast<const float4*>(a.x_best)[at];
      const int d = (xb.x != c.x) + (xb.y != c.y) + (xb.z != c.z) + (xb.w != c.w);
      const int sp = l1_block_count(d, cnt[0], wave, lane);
      const bool red = 100 * sp < 95 * sp_old;
      k_sel = (2 * sp + 2) / 3;
      k_sel = k_sel < 1 ? 1 : k_sel > L1_N ? L1_N : k_sel;
      if (red) {
        eta = a.eps;
        restarted = 1;
        if (!improved) {                                   // (workgroup-uniform: the best point of an earlier launch)
          src = xb;
          gb = reinterpret_cast<const float4*>(a.g_best)[at];
          if (!own) gb = zero4;
        }
      } else {
        const float shrunk = eta / 1.5f, floor_ = a.eps / 10.0f;
        eta = shrunk > floor_ ? shrunk : floor_;
      }
      sp_old = sp;
    }
  }

  // the sparse step: the k_sel-th largest |gs| by the sort network
  const float gv[L1_SEL_PER] = {a.sign * gb.x, a.sign * gb.y, a.sign * gb.z, a.sign * gb.w};
  const float sv[L1_SEL_PER] = {src.x, src.y, src.z, src.w};
  const float cv[L1_SEL_PER] = {c.x, c.y, c.z, c.w};
  int ak[L1_SEL_PER], key[L1_SEL_PER];
#pragma unroll
  for (int s = 0; s < L1_SEL_PER; ++s) {
    ak[s] = (int)(__float_as_uint(gv[s]) & L1_ABS);
    key[s] = own ? ak[s] : -1;
  }
  l1_sort<int, L1_SEL_PER>(key, reinterpret_cast<int*>(ex), tid);
  {
    const int ks = k_sel < 1 ? 1 : k_sel > L1_N ? L1_N : k_sel;     // (a record from elsewhere: still a slot)
    const int p = L1_SEL_SLOTS - ks;
#pragma unroll
    for (int s = 0; s < L1_SEL_PER; ++s)
      if (L1_SEL_PER * tid + s == p) thr_w = key[s];
  }
  lds_barrier();
  const int thr_k = thr_w;
  thr = __uint_as_float((uint32_t)thr_k);
  bool sel[L1_SEL_PER];
  int msel = 0;
#pragma unroll
  for (int s = 0; s < L1_SEL_PER; ++s) {
    sel[s] = own && ak[s] >= thr_k && ak[s] != 0;
    msel += sel[s] ? 1 : 0;
  }
  const int m = l1_block_count(msel, cnt[1], wave, lane);
  const float step = eta / (float)(m < 1 ? 1 : m);

  // the projection onto the L1 ball and the box
  float sg[L1_SEL_PER], av[L1_SEL_PER], cap[L1_SEL_PER], w[L1_SEL_PER], dl[L1_SEL_PER];
#pragma unroll
  for (int s = 0; s < L1_SEL_PER; ++s) {
    const float mv = step * l1_sgn(gv[s]);
    const float t = sel[s] ? sv[s] + mv : sv[s];
    const float z = t - cv[s];
    sg[s] = l1_sgn(z);
    av[s] = fabsf(z);
    const float room = sg[s] > 0.0f ? a.hi - cv[s] : cv[s] - a.lo;
    cap[s] = room < 0.0f ? 0.0f : room;
    w[s] = cap[s] < av[s] ? cap[s] : av[s];                // (a NaN a stays a NaN)
  }
  const float sum_w = row_block_sum((w[0] + w[1]) + (w[2] + w[3]), part, wave, lane);
  if (a.eps == 0.0f) {
    lam = 0.0f;
#pragma unroll
    for (int s = 0; s < L1_SEL_PER; ++s) dl[s] = sg[s] * 0.0f;
  } else if (sum_w <= a.eps) {                             // inside the ball already
    lam = 0.0f;
#pragma unroll
    for (int s = 0; s < L1_SEL_PER; ++s) dl[s] = sg[s] * w[s];
  } else {
    uint64_t q[L1_PRJ_PER];
#pragma unroll
    for (int s = 0; s < L1_SEL_PER; ++s) {
      float b = av[s] - cap[s];
      b = b < 0.0f ? 0.0f : b;
      const uint32_t ta = own ? (__float_as_uint(av[s]) & L1_ABS) : L1_INF_BITS;
      const uint32_t tb = own ? (__float_as_uint(b) & L1_ABS) : L1_INF_BITS;
      q[s] = ((uint64_t)ta << 32) | (uint32_t)(L1_SEL_PER * tid + s);
      q[L1_SEL_PER + s] = ((uint64_t)tb << 32) | (uint32_t)(L1_SEL_SLOTS + L1_SEL_PER * tid + s);
    }
    l1_sort<uint64_t, L1_PRJ_PER>(q, ex, tid);
    float tau[L1_PRJ_PER];
    double Sk[L1_PRJ_PER];                                 // S in float64: a sum of floats, exact to its last bits
    int Nk[L1_PRJ_PER];
    bool real[L1_PRJ_PER];
    double us = 0.0;
    int un = 0;
#pragma unroll
    for (int s = L1_PRJ_PER - 1; s >= 0; --s) {            // the thread's own eight, backwards
      const uint32_t id = (uint32_t)q[s] & (L1_PRJ_SLOTS - 1);
      const bool isb = (id & L1_SEL_SLOTS) != 0;
      real[s] = (id & (L1_SEL_SLOTS - 1)) < L1_N;
      tau[s] = __uint_as_float((uint32_t)(q[s] >> 32));
      const double v = real[s] ? (double)(isb ? -tau[s] : tau[s]) : 0.0;
      const int n1 = real[s] ? (isb ? -1 : 1) : 0;
      us = s == L1_PRJ_PER - 1 ? v : us + v;
      un = un + n1;
      Sk[s] = us;
      Nk[s] = un;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                     // the suffix over the wave
      const double ts = __shfl_down(us, o, 64);
      const int tn = __shfl_down(un, o, 64);
      if (lane + o < 64) { us = us + ts; un = un + tn; }
    }
    const double es = __shfl_down(us, 1, 64);
    const int en = __shfl_down(un, 1, 64);
    const double sex = lane == 63 ? 0.0 : es;
    const int nex = lane == 63 ? 0 : en;
    if (lane == 0) { scan_s[wave] = us; scan_n[wave] = un; }
    lds_barrier();
    const double s32 = scan_s[3] + scan_s[2];
    const int n32 = scan_n[3] + scan_n[2];
    const double soff = wave == 3 ? 0.0 : wave == 2 ? scan_s[3] : wave == 1 ? s32 : s32 + scan_s[1];
    const int noff = wave == 3 ? 0 : wave == 2 ? scan_n[3] : wave == 1 ? n32 : n32 + scan_n[1];
    const double sb = soff + sex;
    const int nb = noff + nex;
    uint64_t cand = ((uint64_t)L1_PRJ_SLOTS << 32) | L1_NAN_BITS;    // no crossing (a NaN in the row): lam = NaN
#pragma unroll
    for (int s = L1_PRJ_PER - 1; s >= 0; --s) {            // descending: the first slot wins
      const double S = sb + Sk[s];
      const int N = nb + Nk[s];
      const double nf = (double)N;
      const double tn = (double)tau[s] * nf;
      const double phi = S - tn;
      if (real[s] && N > 0 && phi <= (double)a.eps) {
        const double num = S - (double)a.eps;              // lam is rounded to float32 once, here
        cand = ((uint64_t)(uint32_t)(L1_PRJ_PER * tid + s) << 32) | __float_as_uint((float)(num / nf));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint64_t t = __shfl_xor(cand, o, 64);
      cand = t < cand ? t : cand;
    }
    if (lane == 0) hit[wave] = cand;
    lds_barrier();
    const uint64_t h01 = hit[0] < hit[1] ? hit[0] : hit[1];
    const uint64_t h23 = hit[2] < hit[3] ? hit[2] : hit[3];
    lam = __uint_as_float((uint32_t)(h01 < h23 ? h01 : h23));
#pragma unroll
    for (int s = 0; s < L1_SEL_PER; ++s) {
      float t = av[s] - lam;
      t = t < 0.0f ? 0.0f : t;                             // (a NaN stays a NaN through both)
      t = cap[s] < t ? cap[s] : t;
      dl[s] = sg[s] * t;
    }
  }
  const float4 o{clamp_nan_passes(cv[0] + dl[0], a.lo, a.hi), clamp_nan_passes(cv[1] + dl[1], a.lo, a.hi),
                 clamp_nan_passes(cv[2] + dl[2], a.lo, a.hi), clamp_nan_passes(cv[3] + dl[3], a.lo, a.hi)};
  if (own) reinterpret_cast<float4*>(a.x)[at] = o;
  if (tid == 0) {
    reinterpret_cast<float4*>(a.fstate)[i] = float4{eta, loss_best, lam, thr};
    reinterpret_cast<int4*>(a.istate)[i] = int4{k_sel, sp_old, iters + 1, restarted};
  }
}

void launch_apgd_l1_step(const ApgdL1StepArgs& a, int M, hipStream_t s) {
  if (M < 1 || M > INPUT_GRAD_MAX_B) throw std::runtime_error("apgd_l1_step: image count out of range");
  if (!a.dx || !a.loss_rows || !a.x0 || !a.x || !a.x_best || !a.g_best || !a.fstate || !a.istate)
    throw std::runtime_error("apgd_l1_step: null argument");
  if (misaligned(15, a.dx, a.x0, a.x, a.x_best, a.g_best))
    throw std::runtime_error("apgd_l1_step: the fp32 row arrays must be 16-byte aligned");
  if (misaligned(15, a.fstate, a.istate))
    throw std::runtime_error("apgd_l1_step: the per-image records must be 16-byte aligned");
  if (misaligned(3, a.loss_rows)) throw std::runtime_error("apgd_l1_step: loss_rows must be 4-byte aligned");
  if (!(a.eps >= 0.0f)) throw std::runtime_error("apgd_l1_step: eps must be >= 0");
  if (a.sign != 1.0f && a.sign != -1.0f) throw std::runtime_error("apgd_l1_step: sign must be +1 or -1");
  if (a.window < 0) throw std::runtime_error("apgd_l1_step: window must be >= 0");
  if (a.first && a.last) throw std::runtime_error("apgd_l1_step: a launch is the first or the last, not both");
  hipLaunchKernelGGL(apgd_l1_step_kernel, dim3(M), dim3(ROW_THREADS), 0, s, a);
}

void preload_apgd_l1() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&apgd_l1_step_kernel));
}

}  // namespace mnist
