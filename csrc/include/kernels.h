// Host-visible launch interface of the hand-written gfx950 kernels.  Every launcher only
// enqueues on the given stream (no allocation, no sync) so the sequences are graph-capturable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mnist_common.h"

namespace mnist {

// write-through (sc1) stores for batches up to this size (device_utils.h store16)
constexpr int WT_MAX_B = 1024;

// ---------------- forward ----------------
struct TrunkFwdArgs {
  const uint8_t* data_u8;     // [N][784] raw dataset, HBM resident
  const int32_t* idx;         // epoch index vector; row b of step s = idx[s*idx_step_stride + b]
  int64_t idx_step_stride;    // = batch size for the training stream, 0 for a fixed batch
  const StepState* state;     // step counter + dropout RNG (may be null in eval)
  const float* w1c;           // conv1.weight fp32 [32][9]
  const float* b1c;           // conv1.bias   fp32 [32]
  const uint16_t* w2f;        // conv2 weight bf16 [64][9][32]
  const float* b2c;           // conv2.bias   fp32 [64]
  uint16_t* a1_out;           // bf16 [B][26][26][32]  (train only)
  uint16_t* p_out;            // bf16 [B][9216]
  uint8_t* pmask_out;         // u8   [B][9216]        (train only)
  const float* xin;           // optional fp32 [B][784] already-normalised input (module API);
                              // when set, data_u8/idx are ignored
  const int* wait_a;          // optional (schedule 3): completion held until *wait_a >= *wait_b
  const int* wait_b;
  int* wait_err;
};
void launch_trunk_fwd(const TrunkFwdArgs& a, int B, bool train, hipStream_t s);
constexpr int TRUNK_IMG_MAX_B = 256;      // B <= this: one workgroup per image (every image has a CU)
int trunk_strips_per_wg(int B);           // 3 (whole image per workgroup) or 1 (one strip)

// fc1 split-K partial GEMM: z1part[s][b][o] = sum_{i in chunk s} p[b][i] * w1[o][i]
constexpr int FC1_KSPLIT = 32;            // small batches: 16-row tiles, fragments straight from HBM/L2
constexpr int FC1_KSPLIT_BIG = 4;         // B >= FC1_BIG_MIN_B: 64x128 LDS-staged tiles, K/4 each
constexpr int FC1_BIG_MIN_B = 512;
__host__ __device__ inline int fc1_ksplit(int B) { return B >= FC1_BIG_MIN_B ? FC1_KSPLIT_BIG : FC1_KSPLIT; }
void launch_fc1_fwd(const uint16_t* p, const uint16_t* w1, float* z1part, int B, hipStream_t s);

// Head: reduce fc1 partials + bias -> ReLU -> dropout(0.5) -> fc2 -> log_softmax (+ NLL + backward)
struct HeadArgs {
  const float* z1part;        // [fc1_ksplit(B)][B][128]
  const float* b_fc1;         // [128]
  const float* w_fc2;         // [10][128] fp32
  const float* b_fc2;         // [10]
  const int32_t* labels;      // train: dataset labels [N] gathered through idx; eval: same
  const int32_t* idx;
  int64_t idx_step_stride;
  const StepState* state;
  float inv_batch;            // 1/B (nll mean)
  // outputs (train)
  float* loss_rows;           // [B] per-row NLL
  uint16_t* dz1;              // bf16 [Bp][128] grad wrt fc1 pre-activation (rows >= B zeroed)
  uint16_t* h_bf;             // bf16 [Bp][128] fc1 activations after ReLU+dropout (rows >= B zeroed)
  uint16_t* dl_bf;            // bf16 [Bp][16]  d loss / d logits (cols >= 10, rows >= B zeroed)
  // outputs (eval)
  float* logp_out;            // optional [B][10]
  int32_t* correct_out;       // [B] 1 if argmax == label
  const float* dlogp;         // module API backward: upstream grad wrt log-probs [B][10] (replaces NLL)
};
void launch_head_train(const HeadArgs& a, int B, int Bp, hipStream_t s);
void launch_head_eval(const HeadArgs& a, int B, hipStream_t s);
// module API forward: log-probs with (train) or without (eval) dropout-2
void launch_head_fwd(const HeadArgs& a, int B, bool train, hipStream_t s);

// Margin head (fc_head.hip): head_train's forward in inference semantics (no StepState, no dropout; z1, h and the
// logits z carry head_train's bits with dropout off) with a margin loss L on the logits in place of the NLL, and
// head_train's outputs under head_train's padding contract, so any fc_bwd role may follow.  Per row, with y =
// labels[b], s = scale, and the selections made with explicit > in ascending class order (the first of equals
// wins): pi1 the first maximum of z, pi2 / pi3 / pi4 the first maximum over the classes not yet taken, o the first
// maximum over j != y.  Every operation below is rounded on its own; dl starts at 0 and the terms are added in the
// order written:
//   MARGIN_CW:     L = z[o] - z[y];                              dl[o] += s; dl[y] -= s
//   MARGIN_DLR:    d = (z[pi1] - z[pi3]) + 1e-12f;  L = (z[o] - z[y]) / d;  dl[o] += s/d; dl[y] -= s/d;
//                  q = (s L) / d;  dl[pi1] -= q; dl[pi3] += q
//   MARGIN_DLR_T:  t = targets[b] (t != y is the caller's promise);  d = (z[pi1] - 0.5f (z[pi3] + z[pi4])) + 1e-12f;
//                  L = (z[y] - z[t]) / d;  dl[y] += s/d; dl[t] -= s/d;
//                  q = (s L) / d;  dl[pi1] -= q; dl[pi3] += 0.5f q; dl[pi4] += 0.5f q
// CW and DLR are ascended to leave y (with y a target class, descended to reach it); DLR_T is descended: it is the
// negative of the APGD-T objective of Croce & Hein (2020).
enum MarginKind : int { MARGIN_CW = 0, MARGIN_DLR = 1, MARGIN_DLR_T = 2 };
struct HeadMarginArgs {
  const float* z1part;        // [fc1_ksplit(B)][B][128]
  const float* b_fc1;         // [128]
  const float* w_fc2;         // [10][128] fp32
  const float* b_fc2;         // [10]
  const int32_t* labels;      // [B] one label per batch row
  const int32_t* targets;     // [B] MARGIN_DLR_T only (else unread, may be null)
  float scale;                // s: dl = s dL/dz
  float* loss_rows;           // [B] per-row L
  uint16_t* dz1;              // bf16 [Bp][128] (z1 > 0) ? sum_c dl[c] w2[c] : 0 (rows [B, Bp) zeroed)
  uint16_t* h_bf;             // bf16 [Bp][128] relu(z1) (rows [B, Bp) zeroed)
  uint16_t* dl_bf;            // bf16 [Bp][16]  (cols >= 10, rows [B, Bp) zeroed)
};
// Refuses, without launching: an unknown kind, a null pointer (targets: with MARGIN_DLR_T), B <= 0, a Bp that is
// not a multiple of 32 or is below B.  Grid: Bp one-wave workgroups, one row each.
void launch_head_margin(const HeadMarginArgs& a, int B, int Bp, int kind, hipStream_t s);

// ---------------- inference (infer_fwd.hip) ----------------
// One launch: B images -> log-probs, argmax (+ per-row NLL / hit with labels).  Grid = (INFER_BANDS,
// groups): workgroup (band, g) runs the conv trunk for pooled row `band` of the images
// [g * ipw, min(B, (g + 1) * ipw)), multiplies its [ipw x 768] feature tile (LDS only) by the band's
// 768 columns of the fc1 weight and writes z1part[band][b][128]; the workgroup of a group that draws
// the last ticket sums the 12 partials in band order and runs the head.  Nobody waits for anybody.
constexpr int INFER_BANDS = HP;           // 12 pooled rows = 12 split-K slices of 768 features
constexpr int INFER_MAX_IPW = 16;         // images per workgroup: the M of one MFMA tile
constexpr int INFER_FILL_GROUPS = 21;     // groups that fill the device: 21 x 12 bands = 252 workgroups
constexpr int INFER_MAX_B = 1 << 18;      // 32-bit byte offsets into the partials
// images per workgroup: 1 while B groups of one image still leave CUs idle, then growing so the grid
// stays at about one workgroup per CU and the band's w1 slice is re-read once per group
__host__ __device__ inline int infer_images_per_wg(int B) {
  const int ipw = (B + INFER_FILL_GROUPS - 1) / INFER_FILL_GROUPS;
  return ipw < 1 ? 1 : ipw > INFER_MAX_IPW ? INFER_MAX_IPW : ipw;
}
struct InferArgs {
  const uint8_t* data_u8;     // [N][784] raw rows (row b, or row idx[b]), or null with xin
  const int32_t* idx;         // optional [B] row index into data_u8 (and labels)
  const float* xin;           // fp32 [B][784] already-normalised input; when set, data_u8 / idx are ignored
  const int32_t* labels;      // optional: label of data row (idx given) or of batch row b
  const float* w1c;           // conv1.weight fp32 [32][9]
  const float* b1c;           // conv1.bias   fp32 [32]
  const uint16_t* w2f;        // conv2 weight bf16 [64][9][32]
  const float* b2c;           // conv2.bias   fp32 [64]
  const uint16_t* w1;         // fc1 weight bf16 [128][9216]
  const float* b_fc1;         // [128]
  const float* w_fc2;         // [10][128] fp32
  const float* b_fc2;         // [10]
  float* z1part;              // workspace [INFER_BANDS][B][128] fp32: written, never accumulated
  int* tickets;               // [groups] arrival counters: zero before and after every launch
  float* logp;                // [B][10]
  int32_t* pred;              // [B] argmax
  float* loss_rows;           // optional [B] per-row NLL (needs labels)
  int32_t* correct;           // optional [B] argmax == label (needs labels)
};
void launch_infer_fwd(const InferArgs& a, int B, hipStream_t s);

// ---------------- backward ----------------
// Compact gradient wrt the conv2 output (the max-pool backward input): one record per (image,
// pooled position) = 64 bf16 pooled gradients (already dropout-scaled, ReLU-masked) followed by the
// 64 argmax codes (2x2 window position, 0..3) as bit planes: per 8-channel chunk c8 two bytes at
// DYC_ROUTE + 2 c8, bit i of the first = bit 0 of channel 8 c8 + i's code, of the second = bit 1
// (16 B of codes instead of 64: 144-B records, 25 % fewer record bytes written by fc_bwd and read by
// the conv backward).  Dense dy[y][x][c] = (code == 2(y&1)+(x&1)) ? g : 0.
constexpr int DYC_REC = 144, DYC_ROUTE = 128;
constexpr int64_t DYC_BYTES_PER_IMAGE = (int64_t)NPOOL * DYC_REC;   // 20736

struct FcBwdArgs {
  const uint16_t* dz1;        // bf16 [Bp][128]
  const uint16_t* p;          // bf16 [Bp][9216] (rows >= B are masked)
  const uint8_t* pmask;       // [B][9216]
  const uint16_t* w1t;        // bf16 [9216][128] (read by role B)
  const uint16_t* h_bf;       // bf16 [Bp][128]
  const uint16_t* dl_bf;      // bf16 [Bp][16]
  const float* loss_rows;     // [B]
  const StepState* state;
  float* grad;                // flat fp32 grad buffer (writes fc1.w, fc1.b, fc2.w, fc2.b)
  uint8_t* dyc;               // compact grad wrt conv2 output: [B][144] records (see DYC_REC)
  float* loss_log;            // [steps] mean loss per step (indexed by state->step)
  float grad_scale;           // extra gradient scale applied in the epilogue.  The engine passes 1.0: its
                              // DDP averaging lives in the head (inv_batch = 1/(B*world)); only a caller
                              // that leaves inv_batch at 1/B would pass 1/world_size here
  float inv_batch;
  float* part;                // B > FC_BWD_SPLIT_ROWS: [fc_bwd_splits(B)][FCB_PART_STRIDE] partial fc grads
  int* signal_ctr;            // optional: the launch's first workgroup adds 1 at its start (schedule-3 hand-off)
};
// Large batches split the batch (= K of the fc weight gradients) over fc_bwd_splits(B) groups of
// workgroups writing fp32 partials that fc_grad_reduce sums in fixed order; B <= 1024 writes the
// gradients directly.  Role B processes FCB_MR(B) 16-row tiles per workgroup (w1 slice kept in VGPRs).
constexpr int FC_BWD_SPLIT_ROWS = 1024;
__host__ __device__ inline int fc_bwd_splits(int B) { return (B + FC_BWD_SPLIT_ROWS - 1) / FC_BWD_SPLIT_ROWS; }
__host__ __device__ inline int fcb_mr(int B) { return B >= 2048 ? 8 : B >= 128 ? 2 : 1; }   // role-B row tiles per workgroup (B = 200: 2 measured 73.1-73.2 vs 74.1-74.6 us/step)
// partial layout per split: fc1.w [128][9216], fc1.b [128], fc2.w [10][128], fc2.b [10], loss sum, pad
constexpr int64_t FCB_PART_W1 = 0, FCB_PART_B1 = 128 * 9216, FCB_PART_W2 = FCB_PART_B1 + 128,
                  FCB_PART_B2 = FCB_PART_W2 + 1280, FCB_PART_LOSS = FCB_PART_B2 + 10,
                  FCB_PART_STRIDE = (FCB_PART_LOSS + 1 + 63) / 64 * 64;
// reduce = false (B > 1024): the split partials are left for launch_fc_grad_reduce, which the
// engine runs on the comm stream ahead of the fc all-reduce / update (off the compute chain)
// fc_bwd workgroup roles (fc_head.hip): C = fc2 weight / bias gradient + loss, A = fc1 weight / bias
// gradient, B = gradient into the conv trunk (compact dy records)
constexpr int FCB_ROLE_C = 1, FCB_ROLE_A = 2, FCB_ROLE_B = 4, FCB_ROLES_ALL = 7;
void launch_fc_bwd(const FcBwdArgs& a, int B, int Bp, hipStream_t s, bool reduce = true, int roles = FCB_ROLES_ALL);
struct AdadeltaArgs;
// roles C + A with the fc Adadelta step fused (one split; single-GPU OVERLAP chain)
void launch_fc_wgrad_update(const FcBwdArgs& a, const AdadeltaArgs& u, int B, int Bp, hipStream_t s);
// role A (fc1 weight gradient split partials) alone, for B > 1024 with reduce = false / with_a = false
void launch_fc_bwd_dw1(const FcBwdArgs& a, int B, int Bp, hipStream_t s);
void launch_fc_grad_reduce(const FcBwdArgs& a, int B, hipStream_t s);   // no-op for B <= 1024
void launch_fc_bwd_role(const FcBwdArgs& a, int B, int Bp, int role, hipStream_t s);   // profiling aid

struct ConvBwdArgs {
  const uint8_t* dyc;         // compact un-pooled gradient (written by fc_bwd role B)
  const uint16_t* a1;         // bf16 [B][26][26][32]
  const uint16_t* w2d;        // bf16 [9][32][64]
  const float* w1c;           // conv1 fp32 [32][9]
  const float* b1c;           // [32]
  const uint8_t* data_u8;
  const int32_t* idx;
  int64_t idx_step_stride;
  const StepState* state;
  float* c1part;              // [4*B][320] conv1 wgrad(288)+bias(32) partials (dgrad kernel)
  float* w2part;              // [G][18432 + 64] conv2 wgrad + bias partials
  float* grad;                // flat fp32 grad buffer (conv params written by the reduce kernel)
  float grad_scale;           // as FcBwdArgs::grad_scale: 1.0 from the engine (averaging in the head)
  int wgrad_groups;           // G
  const float* xin;           // optional fp32 [B][784] input (module API), replaces data_u8/idx
  int* signal_ctr;            // optional: conv2_wgrad / conv2_dgrad add 1 at kernel start (schedule-3 hand-offs)
  // optional [C1_PRE_SLABS][320]: when set, launch_conv_dgrad pre-reduces the 4B conv1
  // partials into C1_PRE_SLABS fixed-order group sums and the conv reduce reads those (large B:
  // 20 reduce workgroups walking 4B slabs is a dependent-load chain, 81 us at B = 8192)
  float* c1red;
  int c1_rows;                // conv1 partial rows the dgrad launch writes: conv_dgrad_c1_rows(B)
  int dgrad_full_grid;        // 1: persistent dgrad on 2 x CUs workgroups; 0: the equal-count grid
};
// 4B: 4 strips of 7 rows per image, items of the persistent dgrad (2 workgroups per CU)
int conv_dgrad_c1_rows(int B);
// test / tuning hooks (host globals, read at enqueue): persistent dgrad grid (0 = 2 x CUs) and the
// wgrad form (-1 = by batch, 0 = lean lockstep halves, 1 = staggered halves)
void set_dgrad_grid(int n);
void set_wgrad_form(int f);
constexpr int C1_PRE_SLABS = 256;
constexpr int C1_PRE_MIN_SLABS = 1024;    // engine: pre-reduce when c1_rows exceeds this
int conv_wgrad_groups(int B);
void launch_conv_bwd(const ConvBwdArgs& a, int B, hipStream_t s);      // dgrad(+conv1 wgrad) and wgrad
void launch_conv_dgrad(const ConvBwdArgs& a, int B, hipStream_t s);    // conv2 dgrad + conv1 wgrad partials
void launch_conv_wgrad(const ConvBwdArgs& a, int B, hipStream_t s);    // conv2 wgrad + bias partials
void launch_conv_grad_reduce(const ConvBwdArgs& a, int B, hipStream_t s);
// reduce blocks [lo, hi) only (RED_W2_PARTS conv2 blocks, then the conv1 ones: see RED_ALL_PARTS)
void launch_conv_grad_reduce_parts(const ConvBwdArgs& a, int B, int lo, int hi, hipStream_t s);

// ---------------- input gradient (input_grad.hip; module API and Predictor only) ----------------
// dx = d loss / d (normalised input) from what the conv backward reads: the compact dy records, the
// stored conv1 activations and the two conv weights.  Items = (image, strip of IG_ROWS dx rows);
// every element of dx [B][784] is written exactly once by a plain store (no pre-zeroing).
constexpr int IG_ROWS = 7, IG_STRIPS = IMG / IG_ROWS;     // 4 strips of 7 dx rows
static_assert(IG_ROWS * IG_STRIPS == IMG, "the strips tile the image");
struct InputGradArgs {
  const uint8_t* dyc;         // compact un-pooled gradient [B][144] records (see DYC_REC)
  const uint16_t* a1;         // bf16 [B][26][26][32]
  const uint16_t* w2d;        // bf16 [9][32][64]
  const float* w1c;           // conv1.weight fp32 [32][9]
  float* dx;                  // fp32 [B][784]
};
// Persistent grid: at most two workgroups per CU (LDS), each walking items g, g + grid, ...; the
// item count is spread evenly over the fewest workgroups that keep the round count.
struct InputGradPlan {
  int items, rounds, grid;
};
inline InputGradPlan input_grad_plan(int B, int cus) {
  InputGradPlan p{};
  if (B < 1 || cus < 1) return p;
  p.items = IG_STRIPS * B;
  const int cap = 2 * cus;
  p.rounds = (p.items + cap - 1) / cap;
  p.grid = (p.items + p.rounds - 1) / p.rounds;
  return p;
}
constexpr int INPUT_GRAD_MAX_B = 1 << 20;   // 32-bit item index
// grid: 0 = the plan; a positive value only shrinks the planned grid (the tests' any-grid proof; no caller in
// the package passes it); negative: std::invalid_argument
void launch_input_grad(const InputGradArgs& a, int B, hipStream_t s, int grid = 0);
// The same kernel body with a projected-step epilogue (L-inf FGSM / PGD on the normalised image): the
// thread that owns dx element e = s writes, instead of s,
//   t = x[e] + alpha * sgn(s);  t = min(max(t, x0[e] - eps), x0[e] + eps);  x_next[e] = min(max(t, lo), hi)
// with sgn = torch.sign for finite s and NaN for a NaN s (which reaches x_next).  x_next may alias x;
// g.dx is optional here (null: the gradient is not stored).  Same plan, same bits on any grid.
struct InputGradStepArgs {
  InputGradArgs g;            // as launch_input_grad; g.dx may be null
  const float* x;             // fp32 [B][784] current iterate
  const float* x0;            // fp32 [B][784] centre of the eps ball (the clean image)
  float* x_next;              // fp32 [B][784]
  float alpha, eps, lo, hi;   // step size, radius, valid range: all in normalised units
};
void launch_input_grad_step(const InputGradStepArgs& a, int B, hipStream_t s, int grid = 0);

// L2 projected-gradient step (attack_step.hip; L2 PGD on the normalised image), one workgroup per image:
//   n = sqrt(sum dx^2);  t = x + (alpha / max(n, TINY)) * dx;  d = t - x0;  m = sqrt(sum d^2)
//   x_next = min(max(x0 + d * min(1, eps / max(m, TINY)), lo), hi)
// all fp32, both sums a fixed tree (the same bits on any stream and launch).  alpha < 0 descends (targeted);
// a zero dx leaves t = x; a NaN in an image's dx makes that image's x_next NaN and no other's.  x_next may
// alias x.  dx is what launch_input_grad wrote.  The arrays are 16-byte aligned (rows are 3136 B).
constexpr float PGD_L2_TINY = 1e-12f;       // floor of both norms (ops/functional.py PGD_L2_TINY)
struct PgdL2StepArgs {
  const float* dx;            // fp32 [B][784] gradient wrt the normalised image
  const float* x;             // fp32 [B][784] current iterate
  const float* x0;            // fp32 [B][784] centre of the eps ball (the clean image), inside [lo, hi]
  float* x_next;              // fp32 [B][784]
  float alpha, eps, lo, hi;   // step length, radius (both L2), valid range: all in normalised units
};
void launch_pgd_l2_step(const PgdL2StepArgs& a, int B, hipStream_t s);   // B in [1, INPUT_GRAD_MAX_B], eps >= 0

// ---------------- adversarial training (adv_train.hip) ----------------
// adv_init, the first launch of an adversarial training step: per batch row b of the step (row r = step *
// idx_step_stride + b; image and label idx[r] of the set, or r itself without an index vector: the
// pre-gathered epoch rows - as trunk_fwd / head_train resolve them)
//   x0[b] = the normalised image (bitwise trunk_fwd's in-register value);  labels_out[b] = its label
//   x[b]  = x0[b], or with random_start  min(max(x0 + (2u - 1) * eps, lo), hi),  u = (w >> 8) * 2^-24, one
//           Philox-4x32-10 word w per element keyed by (state->seed; state->step, element) in a counter
//           domain no dropout stream uses (layout: adv_train.hip)
// Rows past B are not written.  x0 / x 16-byte aligned, data_u8 4-byte aligned.
constexpr uint32_t ADV_PHILOX_DOMAIN = 0x41445631u;   // Philox counter word 1 of adv_init ("ADV1"; dropout: 0)
constexpr int ADV_INIT_MAX_B = 1 << 20;               // 32-bit Philox counter word 0 = b * 196 + float4
struct AdvInitArgs {
  const uint8_t* data_u8;     // [N][784] raw rows
  const int32_t* idx;         // optional index vector
  int64_t idx_step_stride;
  const int32_t* labels;      // label of data row
  const StepState* state;     // step (row offset, Philox counter) and seed (Philox key)
  float* x0;                  // fp32 [B][784]
  float* x;                   // fp32 [B][784]
  int32_t* labels_out;        // [B]
  float eps, lo, hi;          // random start: radius and valid range, normalised units
  int random_start;
};
void launch_adv_init(const AdvInitArgs& a, int B, hipStream_t s);

// ---------------- randomized smoothing (smooth.hip) ----------------
// smooth_noise: out[i * n + s] = x0_i + sigma * z for image i < M, sample s < n (fp32 rows of 784, no clamp), z
// one Box-Muller normal per element from Philox-4x32-10 words keyed by seed with counter (sample_base + s,
// SMOOTH_PHILOX_DOMAIN, id_base + i, float4 index): a domain neither dropout stream nor adv_init uses (layout:
// smooth.hip).  x0_i: exactly one of x_u8 (normalised in-register, bitwise trunk_fwd's value) and x_f32.
// Rows past M * n are not written.  out / x_f32 16-byte aligned, x_u8 4-byte aligned.
// Step form: x[b] = x0[b] + sigma * z for the B rows of a step, counter (low 32 bits of rng_base + 2 step,
// DOMAIN, b, float4 index), key state->seed; x may be x0 (in place).
// smooth_vote: counts[i][c] (+)= the number of rows s < n of logp[i * n + s][10] whose first maximum is class
// c; a row holding a NaN votes for nothing.  Rows of counts past M are not written.
constexpr uint32_t SMOOTH_PHILOX_DOMAIN = 0x534D5431u;   // Philox counter word 1 of smooth_noise ("SMT1")
static_assert(SMOOTH_PHILOX_DOMAIN != 0u && SMOOTH_PHILOX_DOMAIN != ADV_PHILOX_DOMAIN, "a counter domain of its own");
constexpr int64_t SMOOTH_MAX_ROWS = 1 << 23;             // one workgroup of 256 threads per row in a 32-bit grid
struct SmoothNoiseArgs {
  const uint8_t* x_u8;        // [M][784] raw rows, or null
  const float* x_f32;         // [M][784] normalised rows, or null
  float* out;                 // fp32 [M * n][784]
  const StepState* state;     // step form only
  float sigma;                // normalised units, >= 0
  uint64_t seed;              // Philox key
  uint32_t sample_base, id_base;
  int n;                      // samples per image
};
void launch_smooth_noise(const SmoothNoiseArgs& a, int M, hipStream_t s);
void launch_smooth_noise_step(const StepState* state, const float* x0, float* x, float sigma, int B, hipStream_t s);
struct SmoothVoteArgs {
  const float* logp;          // fp32 [M * n][10]
  int32_t* counts;            // [M][10]
  int n;
  int accumulate;
};
void launch_smooth_vote(const SmoothVoteArgs& a, int M, hipStream_t s);

// ---------------- attribution: integrated gradients, SmoothGrad (attr.hip) ----------------
// attr_path: out[i * ns + s] = b_i + alpha * (x_i - b_i) for image i < M, sample s < ns (fp32 rows of 784), alpha =
// (float(sample_base + s) + 0.5f) / float(n_total): the midpoints of n_total equal steps from the baseline b_i to
// the image x_i.  x_i: exactly one of x_u8 (normalised in-register, bitwise trunk_fwd's value) and x_f32; b_i: the
// fp32 rows `base`, or the scalar base_value when base is null.  Each operation rounded on its own.  Rows past
// M * ns are not written.  out / x_f32 / base 16-byte aligned, x_u8 4-byte aligned.
// attr_reduce: acc[i] (+)= sum over s < ns of dx[i * ns + s], per element in ascending s in fp32, from the stored
// acc (accumulate) or from 0: the same bits under any chunking of an image's samples over accumulating launches.
// finish (after the last add): ATTR_FINISH_SCALE stores out = acc * scale, ATTR_FINISH_PATH out = (acc * scale) *
// (x_i - b_i) with x_i, b_i as above; ATTR_FINISH_NONE stores the running sum to acc.  out may alias acc.  Rows of
// acc / out past M are not written.  No atomics.
constexpr int ATTR_MAX_STEPS = 1 << 24;                  // n_total: every sample index is an exact float
enum AttrFinish { ATTR_FINISH_NONE = 0, ATTR_FINISH_SCALE = 1, ATTR_FINISH_PATH = 2 };
struct AttrPathArgs {
  const uint8_t* x_u8;        // [M][784] raw rows, or null
  const float* x_f32;         // [M][784] normalised rows, or null
  const float* base;          // fp32 [M][784] baseline rows, or null: base_value everywhere
  float base_value;           // normalised units
  float* out;                 // fp32 [M * ns][784]
  int sample_base, n_total;   // this launch holds the samples [sample_base, sample_base + ns) of n_total
  int ns;                     // samples per image in this launch
};
void launch_attr_path(const AttrPathArgs& a, int M, hipStream_t s);
struct AttrReduceArgs {
  const float* dx;            // fp32 [M * ns][784] gradient rows
  float* acc;                 // fp32 [M][784] running sums
  float* out;                 // fp32 [M][784] (finish); may be acc
  const uint8_t* x_u8;        // ATTR_FINISH_PATH: the image and the baseline, as AttrPathArgs
  const float* x_f32;
  const float* base;
  float base_value;
  float scale;                // -1 / n as a float
  int ns;
  int accumulate;
  int finish;                 // AttrFinish
};
void launch_attr_reduce(const AttrReduceArgs& a, int M, hipStream_t s);

// ---------------- minimum-norm adversarial examples: L2 DeepFool (deepfool.hip) ----------------
// Image i < M of a chunk owns the DF_CLASSES rows 10 i + c of the fp32 row buffer `rows` (the xin of trunk_fwd, row
// c labelled c) and of the gradient buffer dx (input_grad's plain output): g_c = d NLL_c / d x, and head_train's
// loss_rows[10 i + c] = -log p_c.  One workgroup per image, fp32, fixed-tree sums, no atomics.
// deepfool_init: the ten rows and x[i] = the normalised image x0_i (exactly one of x_u8, normalised in-register,
// bitwise trunk_fwd's value, and x_f32), r_tot[i] = 0, status[i] = iters[i] = 0, norm[i] = 0; x0_out (required with
// x_u8, optional with x_f32) receives x0_i: the x0 of the step.
// deepfool_step, per image with y = y[i] the class being left (f_k = loss_y - loss_k, w_k = g_y - g_k, k != y):
//   status != 0                                  -> nothing is stored (frozen)
//   some loss_k < loss_y, or == with k < y       -> status = DF_CROSSED, nothing else stored (head_eval's argmax)
//   l = the first smallest (|f_k| + DF_SLACK) / sqrt(sum w_k^2) in ascending k, skipping sqrt(..) < PGD_L2_TINY and
//       NaN ratios; none left: the first k with a NaN ratio (its NaN then fills the image), else status = DF_STUCK
//       and nothing else stored (a y outside [0, 10) is stuck too)
//   r_tot += ((|f_l| + DF_SLACK) / sum w_l^2) * w_l;  x_next = min(max(x0 + (1 + overshoot) * r_tot, lo), hi) (a NaN
//   passes) -> x[i] and the ten rows;  norm[i] = sqrt(sum (x_next - x0)^2);  iters[i] += 1
// Rows and entries past M are not written.  The fp32 arrays are 16-byte aligned, x_u8 4-byte aligned.
constexpr int DF_CLASSES = 10;
constexpr float DF_SLACK = 1e-4f;                        // added to |f_k| (the constant of the authors' code)
constexpr int DF_MAX_M = (int)(SMOOTH_MAX_ROWS / DF_CLASSES);   // the rows of a chunk stay within SMOOTH_MAX_ROWS
enum DfStatus { DF_RUNNING = 0, DF_CROSSED = 1, DF_STUCK = 2 };
struct DeepfoolInitArgs {
  const uint8_t* x_u8;        // [M][784] raw rows, or null
  const float* x_f32;         // [M][784] normalised rows, or null
  float* rows;                // fp32 [10 M][784]
  float* x;                   // fp32 [M][784] the iterate
  float* x0_out;              // fp32 [M][784] the normalised image (required with x_u8)
  float* r_tot;               // fp32 [M][784] the accumulated perturbation
  int32_t* status;            // [M] DfStatus
  int32_t* iters;             // [M] updates made
  float* norm;                // [M] |x - x0|
};
void launch_deepfool_init(const DeepfoolInitArgs& a, int M, hipStream_t s);   // M in [1, DF_MAX_M]
struct DeepfoolStepArgs {
  const float* dx;            // fp32 [10 M][784] gradient rows
  const float* loss_rows;     // [10 M] -log p_c of row 10 i + c
  const int32_t* y;           // [M] the class being left
  const float* x0;            // fp32 [M][784] the clean normalised image
  float* r_tot;               // fp32 [M][784]
  float* x;                   // fp32 [M][784]
  float* rows;                // fp32 [10 M][784]
  int32_t* status;            // [M]
  int32_t* iters;             // [M]
  float* norm;                // [M]
  float overshoot, lo, hi;    // overshoot >= 0; valid range in normalised units
};
void launch_deepfool_step(const DeepfoolStepArgs& a, int M, hipStream_t s);   // M in [1, DF_MAX_M], overshoot >= 0

// ---------------- Auto-PGD (apgd.hip; Croce & Hein 2020) ----------------
// One iteration's per-image update in one launch, one workgroup per image, fp32, no atomics: dx / loss_rows are the
// gradient chain's outputs at the iterate x (input_grad's plain form, head_train's -log p_label).  With L = sign *
// loss_rows[i] and g = sign * dx[i]: the counters and the best point are brought up to date (n_up += L > loss_prev;
// L > loss_best: x_best = x, g_best = dx), a launch that closes a checkpoint window of k iterations halves eta and
// restarts from (x_best, g_best) when 4 n_up <= 3 k or (reduced == 0 and loss_check >= loss_best), and the momentum
// step z = Proj(src + step(eta, gs)); x = Proj(src + a (z - src) + (1 - a) (src - x_old)); x_old = src is made
// (a = 0.75; first launch: a = 1, no x_old term).  The exact form, the NaN rules and the one deliberate difference
// from the authors' code (the first comparison is against the start point's loss) are in apgd.hip.
// PER-IMAGE SCALARS, two 16-byte records an image (both arrays 16-byte aligned):
//   fstate[i] = {eta, loss_best, loss_prev, loss_check}   (fp32; the losses carry `sign`)
//   istate[i] = {n_up, reduced, iters, restarted}         (int32; restarted: 1 when the last update started from
//                                                          x_best, 0 when from x)
// first: reads no record and no x_old / x_best / g_best, writes all of them.  last: only loss_prev, n_up and the best
// point (loss_best, x_best, g_best) are brought up to date; x, x_old and the rest keep their values; window is
// ignored.  Rows and records past M are untouched.
struct ApgdStepArgs {
  const float* dx;            // fp32 [M][784] d NLL / d x at the iterate
  const float* loss_rows;     // [M] -log p_label at the iterate
  const float* x0;            // fp32 [M][784] the clean normalised image, inside [lo, hi]
  float* x;                   // fp32 [M][784] the iterate (the xin of the next chain run)
  float* x_old;               // fp32 [M][784] the point the last update started from
  float* x_best;              // fp32 [M][784] the point of the highest sign * loss so far
  float* g_best;              // fp32 [M][784] its dx row, stored raw (without sign)
  float* fstate;              // [M][4]
  int32_t* istate;            // [M][4]
  float sign;                 // +1 untargeted (ascent), -1 targeted (the labels' NLL is descended)
  float eps, lo, hi;          // radius (of the norm), valid range: normalised units
  int first, last;            // flags: launch 0 / the launch after the last update
  int window;                 // k > 0: this launch closes a checkpoint window of k iterations; else 0
};
// M in [1, INPUT_GRAD_MAX_B], eps >= 0, sign +-1, window >= 0, not first and last at once; l2: the L2 form
void launch_apgd_step(const ApgdStepArgs& a, int M, bool l2, hipStream_t s);

// ---------------- Square Attack (square.hip; Andriushchenko, Croce, Flammarion, Hein 2020), L-inf ----------------
// A score-based black-box attack: one query is one eval forward of the candidate x_cand, then square_step reads the
// candidate's margin from head_eval's logp row (untargeted lp[y] - max_{j != y} lp[j]; targeted the negative; < 0:
// broken), accepts it as the best point when it is strictly lower, freezes an image that is broken, and writes the
// next candidate: the best point with a square of side s set to clamp(x0 + eps) or clamp(x0 - eps), its place and
// sign drawn from Philox-4x32-10 words keyed by seed with counter (q, SQUARE_PHILOX_DOMAIN, id_base + i, k): a
// domain no dropout stream, adv_init or smooth_noise uses.  square_init writes the candidate of query 0, vertical
// stripes of +-eps.  The exact form and the NaN rules are in square.hip.
// PER-IMAGE RECORD, 16 bytes (the array 16-byte aligned): {margin_best fp32, queries_used int32, done int32, spare}.
// first: reads no record and no x_best, writes both.  A record with done != 0 on entry: nothing of the image is
// stored.  last: x_cand is not written.  Rows and records past M are untouched.
constexpr uint32_t SQUARE_PHILOX_DOMAIN = 0x53515231u;   // Philox counter word 1 of square_init / square_step ("SQR1")
static_assert(SQUARE_PHILOX_DOMAIN != 0u && SQUARE_PHILOX_DOMAIN != ADV_PHILOX_DOMAIN &&
                  SQUARE_PHILOX_DOMAIN != SMOOTH_PHILOX_DOMAIN, "a counter domain of its own");
struct SquareInitArgs {
  const float* x0;            // fp32 [M][784] the clean normalised image, inside [lo, hi]
  float* x_cand;              // fp32 [M][784] the candidate of query 0
  float eps, lo, hi;          // radius, valid range: normalised units
  uint64_t seed;              // Philox key
  uint32_t id_base;           // image i draws under the id id_base + i
};
void launch_square_init(const SquareInitArgs& a, int M, hipStream_t s);   // M in [1, INPUT_GRAD_MAX_B], eps >= 0
struct SquareStepArgs {
  const float* logp;          // fp32 [M][10] log-probabilities of x_cand (head_eval)
  const int32_t* y;           // [M] the label (targeted: the class to reach)
  const float* x0;            // fp32 [M][784] the clean normalised image
  float* x_best;              // fp32 [M][784] the point of the lowest margin so far
  float* x_cand;              // fp32 [M][784] the candidate (the xin of the next eval forward)
  void* state;                // [M] 16-byte records
  float eps, lo, hi;
  uint64_t seed;
  uint32_t q;                 // the query index of the proposal this launch writes (round j: j + 1)
  uint32_t id_base;
  int side;                   // of that proposal's square, in [1, 27]
  int first, last, targeted;  // flags
};
// M in [1, INPUT_GRAD_MAX_B], eps >= 0, side in [1, 27], id_base + M <= 2^32
void launch_square_step(const SquareStepArgs& a, int M, hipStream_t s);

// ---------------- optimizer ----------------
struct AdadeltaArgs {
  float* param;               // flat fp32
  const float* grad;
  float* square_avg;
  float* acc_delta;
  const float* lr;            // device scalar (StepLR writes it once per epoch)
  float rho, eps, weight_decay;
  uint16_t* w2f;              // bf16 shadows refreshed in the same pass
  uint16_t* w2d;
  uint16_t* w1;
  uint16_t* w1t;
  StepState* state_inc;       // if non-null, block 0 advances state->step (end-of-step marker)
  // optional completion hold (adadelta_reduce_kernel): the launch completes only once
  // *hold_a >= *hold_b (read when its last workgroup gets there); timeout -> *hold_err = 1
  const int* hold_a;
  const int* hold_b;
  int* hold_err;
  int wt;                     // write-through parameter / state / shadow stores (engine: B <= WT_MAX_B)
  int hold_delta;             // hold until *hold_a >= *hold_b + hold_delta (adadelta_kernel; the
                              // reduce kernel holds with delta 0)
  int* signal_start;          // optional: the first workgroup adds 1 at kernel start (the previous
                              // kernel on the stream has completed: a hand-off without a launch)
};
enum AdadeltaRegion { ADA_ALL = 0, ADA_FC = 1, ADA_CONV = 2 };
// grid > 0 (ADA_FC only): that many workgroups walk the 577 fc tiles grid-stride (ADA_FC_LEAN_GRID:
// the single-GPU overlapped update, which runs beside wgrad / dgrad with slack to spare)
constexpr int ADA_FC_LEAN_GRID = 144;
void launch_adadelta(const AdadeltaArgs& a, int region, hipStream_t s, int grid = 0);
// conv gradient slab reduce + the whole Adadelta update in one launch (serial single-GPU step tail)
void launch_adadelta_reduce(const AdadeltaArgs& a, const ConvBwdArgs& c, int B, hipStream_t s);
// conv-only form restricted to reduce parts [lo, hi) (conv_grad_reduce.h partition)
void launch_adadelta_reduce_parts(const AdadeltaArgs& a, const ConvBwdArgs& c, int B, int lo, int hi, hipStream_t s);
// the conv1 parts [RED_W2_PARTS, RED_ALL_PARTS) of that launch, bitwise equal, on 80 one-wave workgroups
// (one float4 column each, the slice tree on cross-lane moves)
void launch_adadelta_c1(const AdadeltaArgs& a, const ConvBwdArgs& c, int B, hipStream_t s);
// Refresh bf16 shadows from fp32 params without an update (after load_state_dict / broadcast).
void launch_refresh_shadows(const AdadeltaArgs& a, hipStream_t s);

// misc
void launch_set_step(StepState* st, int step, hipStream_t s);
void launch_set_state(StepState* st, const StepState& v, hipStream_t s);
// epoch pre-gather: dst rows [start, start+n) = src rows idx[start..start+n) (+ labels)
// synthetic data generator v3 (csrc/kernels/datagen.hip): render n images [n, 784] from a host plan
// (n x 96-B synth::Sample records, csrc/data/synth_render.h) and the zero-bordered templates
void launch_synth_render(const void* plan, const float* templates, int64_t n, uint8_t* out, hipStream_t s);
void launch_gather_rows(const uint8_t* src_u8, const int32_t* src_labels, const int32_t* idx, int64_t start,
                        int64_t n, uint8_t* dst_u8, int32_t* dst_labels, hipStream_t s);
// device-counter stream hand-offs (engine DDP schedule 3)
void launch_stream_signal(int* ctr, hipStream_t s);
// byte fill of [p, p + bytes) on `s` (hipMemset's job without the runtime's blit kernels)
void launch_fill(void* p, int64_t bytes, int value, hipStream_t s);
void launch_stream_wait(const int* a, const int* b, int delta, int* err, hipStream_t s, double timeout_s = 60.0);
// signal then wait in one launch (*sig += 1; wait *a >= *b + delta)
void launch_stream_signal_wait(int* sig, const int* a, const int* b, int delta, int* err, hipStream_t s,
                               double timeout_s = 60.0);
// dst[i] = src[i] * s (DDP bucket copy-in with the 1/world_size pre-division)
void launch_scale_copy(float* dst, const float* src, int64_t n, float s, hipStream_t stream);

// code-object preload, one per kernel translation unit (hipFuncGetAttributes on one of its kernels)
void preload_trunk();
void preload_fc_head();
void preload_conv_bwd();
void preload_adadelta();
void preload_comm();
void preload_xgmi();
void preload_f32();
void preload_input_grad();
void preload_input_grad_step();
void preload_attack_step();
void preload_adv_train();
void preload_smooth();
void preload_attr();
void preload_deepfool();
void preload_apgd();
void preload_square();
void preload_all_kernels();   // every one of the above, in this order (bindings.cpp: the one list)

// ---------------- fp32 step (--dtype fp32; f32_net.hip): f32-input MFMA GEMMs + VALU kernels
struct F32Step {
  // batch source: pre-gathered rows (idx = null, row = step * idx_step_stride + b) or dataset rows
  // through the index vector; eval: the test split, idx = test_idx + first row, stride 0
  const uint8_t* data_u8;
  const int32_t* idx;
  int64_t idx_step_stride;
  const int32_t* labels;
  const StepState* state;     // null in eval (step 0, no dropout)
  const float* param;         // flat fp32 parameters
  float* grad;                // flat fp32 gradient (every parameter written each step)
  float* loss_log;            // [steps] mean loss per step (train)
  float inv_batch;            // 1 / (B * world): DDP averaging folded into the loss gradient
  // workspace (fp32 unless noted)
  float* w2fwd;               // [9][32][64] conv2 weight, forward B operand
  float* w2bwd;               // [9][64][32] conv2 weight, input-gradient B operand
  float* w1p;                 // [128][144][64] fc1 weight with its input index position-major
                              // (pooled position, channel): the fc1 input-gradient B operand
  float* a1;                  // [B][26][26][32] ReLU(conv1)
  float* dx1;                 // [B][26][26][32] the conv1 pre-activation gradient (its own buffer, so
                              // the conv2 weight gradient - which reads a1 - can run beside it)
  float* y2;                  // [B][24][24][64] conv2 pre-activation; then its gradient
  float* p;                   // [B][9216] pooled + dropout, torch flatten order
  uint8_t* pm;                // [B][9216] argmax (bits 0-1), dropout keep (2), pooled > 0 (3)
  float* z1part;              // [f32_fc1_splits(B)][B][128]
  float* h;                   // [B][128] fc1 activations after ReLU + dropout
  float* dz1;                 // [B][128] gradient wrt the fc1 pre-activation
  float* dl;                  // [B][16] gradient wrt the logits
  float* loss_rows;           // [B] per-row NLL (train and eval)
  int32_t* correct;           // eval: [B] argmax == label
  float* c2part;              // [f32_conv2w_splits(B)][64][289] conv2 weight + bias partials
  float* c1part;              // [F32_C1W_BLOCKS][32][10] conv1 weight + bias partials
};
constexpr int F32_MAX_SPLITS = 128;
constexpr int F32_C1W_BLOCKS = 1024;         // conv1 weight-gradient workgroups (= partial slabs)
int f32_fc1_splits(int B);
int f32_conv2w_splits(int B);
int f32_conv1w_splits(int B);
// prep + conv1 + conv2 + pool (+dropout) + fc1 + head (train: loss + logit / dz1 gradients; eval:
// per-row NLL + hits).  `stages` (tests): only the kernels whose bit is set are launched, in that order
enum F32Stage : int {
  F32_STAGE_PREP = 1, F32_STAGE_CONV1 = 2, F32_STAGE_CONV2 = 4, F32_STAGE_POOL = 8, F32_STAGE_FC1 = 16,
  F32_STAGE_HEAD = 32, F32_STAGE_ALL = 63
};
void launch_f32_forward(const F32Step& a, int B, bool train, hipStream_t s, int stages = F32_STAGE_ALL);
// fc2 / fc1-bias grads + loss log, fc1 weight grad, fc1 input grad (+ unpool), conv2 weight grad,
// conv2 input grad (+ conv1 ReLU), conv1 weight grad, split-K reduce: every gradient of the step
void launch_f32_backward(const F32Step& a, int B, hipStream_t s);
void launch_f32_backward_fc(const F32Step& a, int B, hipStream_t s);     // = the first half of it:
void launch_f32_fc_small(const F32Step& a, int B, hipStream_t s);   // fc2 weight / bias, fc1 bias, loss log
void launch_f32_fc1w(const F32Step& a, int B, hipStream_t s);       // fc1 weight (reads dz1 + p)
void launch_f32_backward_conv(const F32Step& a, int B, hipStream_t s);   // = the second half
// ... which is, in order: fc1 input gradient (dy2), conv2 weight gradient (reads dy2 + a1), conv2
// input gradient + conv1 weight gradient (dy2 -> dx1), split-K reduce (both partial sets).  The
// OVERLAP schedule runs the weight gradient on the comm stream beside the input-gradient part.
void launch_f32_fc1x(const F32Step& a, int B, hipStream_t s);
void launch_f32_conv2w(const F32Step& a, int B, hipStream_t s);
void launch_f32_conv2x_conv1w(const F32Step& a, int B, hipStream_t s);
void launch_f32_conv_reduce(const F32Step& a, int B, hipStream_t s);

// direct xGMI all-reduce (reduce-scatter + all-gather over IPC-mapped peer buckets; xgmi_allreduce.hip)
constexpr int XGMI_MAX_RANKS = 8;          // one node
constexpr int XGMI_MAX_WG = 512;           // flag slots per (stage, rank)
constexpr int XGMI_FLAG_INTS = 2 * XGMI_MAX_RANKS * XGMI_MAX_WG;   // [stage][src rank][wg]
struct XgmiArgs {
  const float* in[XGMI_MAX_RANKS];   // every rank's input bucket (peer mappings; own = local)
  float* out[XGMI_MAX_RANKS];        // every rank's output bucket
  int* flags[XGMI_MAX_RANKS];        // every rank's flag block of this channel
  float* stage[XGMI_MAX_RANKS];      // one-shot: every rank's staging block of this channel (2 slots)
  int64_t slot_floats;               // one-shot: floats per staging slot
  int* ctr;                          // local per-WG call counters [XGMI_MAX_WG]
  int* err;                          // local error flag (timeout)
  int world, rank;
  int64_t nvec;                      // bucket length in float4s
  const uint64_t* timeout_ticks;     // device: stage-wait timeout, s_memrealtime ticks (100 MHz)
  // optional fused Adadelta (conv bucket): with fuse_ada, phase 2 applies the update to every element
  // it gathers (flat index ada_base + bucket index; grad = the reduced values), refreshes the conv2
  // bf16 shadows and advances ada.state_inc->step - the bucket's separate update launch disappears
  int fuse_ada;
  int64_t ada_base;
  AdadeltaArgs ada;
  int max_wg;                        // residency cap on the launch grid (XgmiGrids; every rank the same)
  int release;                       // system-scope release fence before each stage flag store
  int acquire;                       // system-scope acquire after each matched stage poll (opt-in)
};
// Every xGMI kernel's workgroup b spins until workgroup b of every peer arrives, so the workgroups
// that can be spinning at the same moment - on one GPU: the fc-bucket kernel on the comm stream and
// the conv-bucket kernel on the compute stream, times the ranks that share the GPU - must all be
// resident at once.  The kernels loop over their index sets (any grid >= a small minimum works) and
// the grids are sized from the occupancy API: co_ranks * sum(grid_k / (occupancy_k * CUs)) <= budget
// for each pair that runs concurrently.  Kernel ids in the error code (XgmiComm::error):
enum XgmiKernelId { XGMI_K_TWOSHOT = 1, XGMI_K_ONESHOT = 2, XGMI_K_FC_FUSED = 3, XGMI_K_CONV_FUSED = 4 };
struct XgmiGrids {
  int fc_fused, conv_fused;          // fused schedule: fc (comm stream) || conv (compute stream)
  int twoshot, oneshot;              // separate launches: two-shot fc || one-shot conv (caps)
  int cap_fc_fused, cap_conv_fused, cap_twoshot, cap_oneshot;   // resident WGs per GPU (occupancy x CUs)
  double load_fused, load_separate;  // co_ranks * sum(grid / cap) of each concurrent pair
};
// Throws std::runtime_error when even the minimum grids cannot be co-resident (caller falls back).
XgmiGrids xgmi_plan_grids(int world, int co_ranks, int64_t oneshot_max_floats, double budget);
constexpr int XGMI_CONV_VB_MAX = 8;        // conv fused: virtual reduce blocks per workgroup (grid >= 39)
int xgmi_workgroups(int64_t nvec, int world, bool fuse_ada);
void launch_xgmi_allreduce(const XgmiArgs& a, hipStream_t s);
// small buckets: one-shot variant - copy-in to a staging slot (alternating by call parity), ONE
// stage hand-off, every rank sums all ranks' slots itself (same rank order -> same bits as above)
void launch_xgmi_allreduce_oneshot(const XgmiArgs& a, hipStream_t s);
// the engine's fc bucket [0, OFF_CONV1_W) with the fc Adadelta step + w1/w1t shadows fused (two-shot,
// 64x32 fc1.weight tiles as the unit of work; needs a.ada and a.nvec == OFF_CONV1_W / 4)
int xgmi_fc_fused_workgroups(int world);
void launch_xgmi_fc_fused(const XgmiArgs& a, hipStream_t s);
// the engine's conv bucket [OFF_CONV1_W, PARAM_TOTAL): conv gradient slab reduce (conv_grad_reduce's
// partition and order) + one-shot all-reduce through the staging slots + Adadelta + conv2 shadows,
// one launch (needs a.ada; a.nvec == (PARAM_TOTAL - OFF_CONV1_W) / 4; c.grad is not written)
// `part` selects reduce blocks [lo, hi) of conv_grad_reduce's partition (RED_W2_WGS = 289 conv2
// blocks, then 20 conv1 blocks); the conv bucket split runs conv2 right after conv2_wgrad on the comm
// stream and conv1 after conv2_dgrad, whose launch holds its completion until *wait_a >= *wait_b.
constexpr int RED_W2_PARTS = 289, RED_ALL_PARTS = 309;   // = conv_grad_reduce.h RED_W2_WGS / RED_WGS
struct XgmiConvPart {
  int lo = 0, hi = RED_ALL_PARTS;
  const int* wait_a = nullptr;
  const int* wait_b = nullptr;
  int* wait_err = nullptr;
};
void launch_xgmi_conv_reduce_fused(const XgmiArgs& a, const ConvBwdArgs& c, int B, hipStream_t s,
                                   const XgmiConvPart& part = XgmiConvPart{});

}  // namespace mnist
