// Pure host-side logic of the runtime, kept free of HIP calls so it can be unit-tested on the CPU
// under AddressSanitizer / UndefinedBehaviorSanitizer (csrc/tests/host_logic_test.cpp,
// tools/sanitize_host.sh):
//   * the engine's workspace carve (offsets of every activation buffer for a batch capacity);
//   * the xGMI IPC export record: encode / decode / validation against this communicator;
//   * the residency planner's grid fitting;
//   * the DDP gradient scaling constants the engine hands its kernels;
//   * the pointer checks the row kernels' launchers share (alignment, the uint8-or-fp32 image source).
#pragma once
#include <stdint.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../include/kernels.h"

namespace mnist {

// ---------------------------------------------------------------------------- DDP gradient scaling
// The engine folds DDP's 1/world averaging into the head's loss-gradient scale: every rank's head
// scales by 1/(B * world) and the all-reduce SUMS, so each row's bf16 gradient operands are bitwise
// those of the world-1 run on the world*B batch.  The GEMM / slab-reduce epilogues then get 1.0
// (FcBwdArgs::grad_scale, ConvBwdArgs::grad_scale) - a caller that also divided there would
// average twice.
inline float ddp_head_inv_batch(int batch, int world) {
  if (batch < 1 || world < 1) throw std::runtime_error("ddp scale: bad batch / world");
  return 1.0f / (float)(batch * world);
}
constexpr float kDdpEpilogueScale = 1.0f;

// ---------------------------------------------------------------------------- step plan
enum Schedule : int { SERIAL = 0, OVERLAP = 1, RCCL = 2, XGMI = 3 };   // values exported to Python

// The engine's device counters (ints in the workspace's sync block).  The hand-off counters only
// ever grow, in matched pairs inside a completed chunk; Engine::reset_counters zeroes them.
enum Counter : int {
  WGRAD_STARTS = 0,    // conv2 wgrad launches started: that step's fc gradients are final
  FC_UPDATES = 1,      // fc updates done
  HANDOFF_ERR = 2,     // a hand-off wait timed out (Engine::errors)
  CONV2_UPDATES = 3,   // conv2 updates published
  DGRAD_STARTS = 4,    // conv2 dgrad launches started: that step's wgrad is done
  FCBWD_STARTS = 5,    // fc_bwd launches started: that step's head_train is done
  HANDOFF_COUNTERS = 6,
  PROBE_SCRATCH = 8,   // probe_stream_pair: a, b, zero, error
  FAULT_HOLD = 12,     // fault_hold: released, zero, the hold's own timeout flag, spare
};

struct StepSwitches {   // the engine's set_* switches; trace = inside the profile window
  bool two_buckets = true, rccl_handoff = false, fc_dw1_side = true, w1t_pingpong = true;
  bool xgmi_fuse_update = true, trace = false;
};

// Every schedule decision of one training step; Engine::enqueue_step only reads it.
struct StepPlan {
  bool side = false;                 // OVERLAP / XGMI: part of the step runs on the comm stream
  bool chain = false;                // ... with the hand-offs riding on its update kernels (untraced, fused)
  bool xgmi_separate = false;        // XGMI with separate all-reduce / update launches (fuse off)
  bool fc_reduce_side = false;       // B > 1024: the fc split partials are summed on the comm stream
  bool dw1_side = false;             // ... and fc_bwd role A runs there ahead of that sum
  bool fcw_side = false, w1t_pp = false;   // chain, B <= 1024: roles C + A there / writing the other w1t copy
  bool c2r = false;                  // RCCL: conv2's slab reduce on the comm stream under dgrad
  int roles = FCB_ROLES_ALL;         // fc_bwd roles left in the compute stream's launch
  bool fc_bwd_reduces = true;        // that launch also sums the split partials
  bool count_fc_bwd_start = false;   // it counts FCBWD_STARTS (wherever wgrad counts WGRAD_STARTS)
  Counter release = WGRAD_STARTS;    // what releases the comm chain's first launch of a step
  int dgrad_full_grid = 0, wt = 0;   // wt: write-through stores at small batches (store16)
  bool f32_chained = false;          // fp32: the two-stream chained step (else one stream, in order)
};

inline StepPlan plan_step(Schedule sched, int B, bool fp32, const StepSwitches& sw) {
  StepPlan p;
  const bool xg = sched == XGMI, rccl2 = sched == RCCL && sw.two_buckets;
  p.side = sched == OVERLAP || xg;
  if (fp32) {   // (the fp32 step reads nothing else)
    p.f32_chained = p.side || (rccl2 && sw.rccl_handoff && !sw.trace);
    return p;
  }
  // not in the traced profiling window, whose phase syncs would deadlock a hold
  p.chain = p.side && !sw.trace && (!xg || sw.xgmi_fuse_update);
  p.xgmi_separate = xg && !sw.xgmi_fuse_update;
  p.fc_reduce_side = fc_bwd_splits(B) > 1 && (p.side || rccl2);
  p.dw1_side = p.fc_reduce_side && sw.fc_dw1_side;
  p.fcw_side = p.chain && fc_bwd_splits(B) == 1 && sw.fc_dw1_side;
  p.w1t_pp = p.fcw_side && sw.w1t_pingpong;
  p.c2r = rccl2 && sw.rccl_handoff && !sw.trace;
  p.roles = p.fcw_side ? FCB_ROLE_B : p.dw1_side ? (FCB_ROLE_C | FCB_ROLE_B) : FCB_ROLES_ALL;
  p.fc_bwd_reduces = !p.fc_reduce_side;
  p.count_fc_bwd_start = p.side || rccl2;
  p.release = p.fcw_side ? FCBWD_STARTS : WGRAD_STARTS;
  p.dgrad_full_grid = sched == OVERLAP || sched == SERIAL ? 0 : 1;
  p.wt = B <= WT_MAX_B;
  return p;
}

// ---------------------------------------------------------------------------- inference plan
// Launch geometry and buffer sizes of the single-launch inference forward (infer_fwd.hip) at batch
// B: grid = (bands, groups), workgroup (band, g) serving images [g * images_per_wg, ...).  The
// workspace holds z1part[bands][B][128] fp32, sized for B + 15 rows (>= groups * images_per_wg, and
// growing with B: a buffer made for max_B serves every B <= max_B); one ticket per group.
struct InferPlan {
  int images_per_wg, groups, bands, grid_x, grid_y;
  int64_t workspace_bytes;
  int ticket_count;
};

inline InferPlan infer_plan(int B) {
  if (B < 1 || B > INFER_MAX_B) throw std::runtime_error("infer_plan: batch size out of range");
  InferPlan p{};
  p.images_per_wg = infer_images_per_wg(B);
  p.groups = (B + p.images_per_wg - 1) / p.images_per_wg;
  p.bands = INFER_BANDS;
  p.grid_x = p.bands;
  p.grid_y = p.groups;
  p.workspace_bytes = 4LL * INFER_BANDS * NH * ((int64_t)B + INFER_MAX_IPW - 1);
  p.ticket_count = p.groups;
  return p;
}

// ---------------------------------------------------------------------------- engine workspace
struct WorkspaceLayout {
  int64_t a1, p, pmask, z1part, loss_rows, dz1, h_bf, dl_bf, dyc, c1part, w2part, fcpart, sync, w2d_alt, c1red,
      w1t_alt;
  int64_t total;   // bytes
};

inline int64_t ws_align256(int64_t x) { return (x + 255) & ~int64_t(255); }

// wgrad_groups = conv_wgrad_groups(max_batch), fc_splits = fc_bwd_splits(max_batch) (both monotonic in B)
inline WorkspaceLayout compute_workspace_layout(int max_batch, int max_test_batch, int wgrad_groups, int fc_splits) {
  if (max_batch < 1 || max_test_batch < 0 || wgrad_groups < 1 || fc_splits < 1)
    throw std::runtime_error("workspace layout: bad sizes");
  auto round_up = [](int64_t x, int64_t m) { return (x + m - 1) / m * m; };
  // forward activations (p, fc1 partials) serve the training and the eval batch; backward-only
  // buffers only the training batch
  const int64_t Ma = max_batch > max_test_batch ? max_batch : max_test_batch;
  const int64_t M = max_batch;
  const int64_t Mp = round_up(M, 64), Map = round_up(Ma, 64);
  WorkspaceLayout L{};
  int64_t off = 0;
  auto carve = [&](int64_t bytes) { int64_t o = off; off += ws_align256(bytes); return o; };
  L.a1 = carve(M * H1 * H1 * C1 * 2);
  L.p = carve(Map * NFLAT * 2);
  L.pmask = carve(M * NFLAT);
  L.z1part = carve((int64_t)FC1_KSPLIT * Ma * NH * 4);
  L.loss_rows = carve(M * 4);
  L.dz1 = carve(Mp * NH * 2);
  L.h_bf = carve(Mp * NH * 2);
  L.dl_bf = carve(Mp * 16 * 2);
  L.dyc = carve(M * DYC_BYTES_PER_IMAGE);   // compact dy records
  L.c1part = carve(4 * M * 320 * 4);
  L.w2part = carve((int64_t)wgrad_groups * (18432 + 64) * 4);
  L.fcpart = carve(fc_splits > 1 ? (int64_t)fc_splits * FCB_PART_STRIDE * 4 : 256);   // large-batch partials
  L.sync = carve(256);                                                                // hand-off counters
  L.w2d_alt = carve((int64_t)9 * C1 * C2 * 2);                                         // alternate w2d
  L.c1red = carve((int64_t)C1_PRE_SLABS * 320 * 4);                                    // conv1 group sums
  L.w1t_alt = carve((int64_t)NFLAT * NH * 2);                                          // alternate w1t
  L.total = off;
  return L;
}

// ---------------------------------------------------------------------------- xGMI export block
// Everything a peer reads or writes lives in ONE exported allocation per rank, so a peer maps it
// with one hipIpcOpenMemHandle (W-1 per rank instead of 4(W-1): the IPC import is the dominant
// per-peer setup cost inside the reference's timer).  Regions 4 KiB aligned:
//   in [numel f32] | out [numel f32] | flags [channels][XGMI_FLAG_INTS] | stage [channels][2][oneshot_max] (+4) | sig [4][4 int32]
struct XgmiBlockLayout {
  int64_t in_off, out_off, flags_off, stage_off, sig_off, bytes;
};
constexpr int64_t kXgmiSigBytes = 16;
inline XgmiBlockLayout xgmi_block_layout(int64_t numel, int channels, int64_t oneshot_max) {
  if (numel < 4 || channels < 1 || oneshot_max < 0) throw std::runtime_error("xgmi block layout: bad sizes");
  auto al = [](int64_t x) { return (x + 4095) & ~int64_t(4095); };
  XgmiBlockLayout L{};
  L.in_off = 0;
  L.out_off = al(L.in_off + 4 * numel);
  L.flags_off = al(L.out_off + 4 * numel);
  L.stage_off = al(L.flags_off + 4LL * XGMI_FLAG_INTS * channels);
  L.sig_off = al(L.stage_off + 4LL * (2 * oneshot_max + 4) * channels);
  L.bytes = al(L.sig_off + 4 * kXgmiSigBytes);
  return L;
}

// ---------------------------------------------------------------------------- xGMI export record
// What one rank publishes (through the c10d store) about its block; peers map it with IPC.
struct XgmiRecord {
  hipIpcMemHandle_t blk_h;
  int64_t blk_off;                                  // the block's offset inside the IPC allocation
  XgmiBlockLayout layout;
  int64_t numel, oneshot_max;
  int32_t world, rank, channels, pid, device;
  int32_t grid_fc, grid_conv, grid_two, grid_one;   // residency-planned grids (must agree across ranks)
  char host[64];                                    // IPC mappings only exist between the GPUs of one node
};

inline std::vector<uint8_t> encode_record(const XgmiRecord& r) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(&r);
  return std::vector<uint8_t>(b, b + sizeof(r));
}

// Decode peer q's record and check it against this communicator; throws with the reason.
inline XgmiRecord decode_record(const std::vector<uint8_t>& bytes, int q, int world, int64_t numel, int channels,
                                int64_t oneshot_max, const XgmiGrids& grids, const char* my_host) {
  if (bytes.size() != sizeof(XgmiRecord)) throw std::runtime_error("xgmi: bad record size");
  XgmiRecord r;
  memcpy(&r, bytes.data(), sizeof(r));
  if (r.rank != q || r.world != world || r.numel != numel || r.channels != channels || r.oneshot_max != oneshot_max)
    throw std::runtime_error("xgmi: peer record does not match this communicator");
  const XgmiBlockLayout L = xgmi_block_layout(numel, channels, oneshot_max);
  if (r.blk_off < 0 || r.blk_off % 256 || memcmp(&r.layout, &L, sizeof(L)) != 0)
    throw std::runtime_error("xgmi: peer record has a different buffer layout");
  if (r.grid_fc != grids.fc_fused || r.grid_conv != grids.conv_fused || r.grid_two != grids.twoshot ||
      r.grid_one != grids.oneshot)
    throw std::runtime_error("xgmi: ranks planned different kernel grids (mixed GPUs or co_ranks?)");
  if (memchr(r.host, 0, sizeof(r.host)) == nullptr) throw std::runtime_error("xgmi: peer host name not terminated");
  if (strncmp(my_host, r.host, sizeof(r.host)) != 0)
    throw std::runtime_error("xgmi: ranks span more than one node (peer on " + std::string(r.host) + ")");
  return r;
}

// ---------------------------------------------------------------------------- launcher argument checks
// Does any of the pointers have a bit under `mask` set (mask 15: 16-byte alignment, 3: 4-byte)?  A null
// pointer counts as aligned: whether it may be null is the caller's own check.
template <class... Ps>
inline bool misaligned(uintptr_t mask, const Ps*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & mask) != 0;
}

// The image source of a row kernel is uint8 rows (read four pixels at a time) or normalised fp32 rows (read as
// float4), never both.  `who` is the launcher's name as its messages begin.  The two halves are separate because
// some launchers check their sizes in between, and which error a doubly wrong call gets is part of the interface.
inline void check_one_row_source(const char* who, const uint8_t* x_u8, const float* x_f32) {
  if ((x_u8 != nullptr) == (x_f32 != nullptr))
    throw std::runtime_error(std::string(who) + ": null argument (exactly one of the uint8 and the fp32 rows)");
}
inline void check_row_source_aligned(const char* who, const uint8_t* x_u8, const float* x_f32) {
  if (x_u8 ? misaligned(3, x_u8) : misaligned(15, x_f32))
    throw std::runtime_error(std::string(who) + ": the source rows must be 16-byte aligned (uint8 rows: 4-byte)");
}
inline void check_row_source(const char* who, const uint8_t* x_u8, const float* x_f32) {
  check_one_row_source(who, x_u8, x_f32);
  check_row_source_aligned(who, x_u8, x_f32);
}
// ... with the optional fp32 baseline rows of the attribution kernels
inline void check_row_source(const char* who, const uint8_t* x_u8, const float* x_f32, const float* base) {
  check_row_source(who, x_u8, x_f32);
  if (misaligned(15, base)) throw std::runtime_error(std::string(who) + ": the baseline rows must be 16-byte aligned");
}

// ---------------------------------------------------------------------------- residency planner
// Shrink grids a (minimum amin, capacity ca) and b so that co * (a/ca + b/cb) <= budget; returns
// the resulting load (may stay above budget when the minimums do not fit).
inline double fit_grid_pair(int* a, int amin, int ca, int* b, int bmin, int cb, int co, double budget) {
  if (ca < 1 || cb < 1 || co < 1 || budget <= 0.0) throw std::runtime_error("fit_grid_pair: bad arguments");
  auto load = [&] { return co * ((double)*a / ca + (double)*b / cb); };
  if (load() > budget) {
    const double s = budget / load();
    const int na = (int)(*a * s), nb = (int)(*b * s);
    *a = na > amin ? na : amin;
    *b = nb > bmin ? nb : bmin;
  }
  return load();
}

}  // namespace mnist
