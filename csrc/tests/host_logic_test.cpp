// Host-logic unit test, built and run under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
// (tools/sanitize_host.sh; tests/test_host_sanitizers.py).  Covers the parts of the native runtime
// that parse peer data or carve memory by hand (csrc/runtime/host_logic.h):
//   * the engine workspace layout for every batch capacity 1..9000 (+ eval capacities): buffers are
//     256-B aligned, disjoint, inside the allocation, and large enough for their contents;
//   * the xGMI record decoder: round trip, and rejection of truncated / oversized / mismatched /
//     unterminated records, plus random byte soup (must throw, never read out of bounds);
//   * the residency planner's grid fitting;
//   * the engine's step plan (plan_step) for every schedule, batch class and switch, and the values
//     of the named device counters;
//   * the row kernels' pointer checks (misaligned, check_row_source) and their exact messages.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <utility>

#include "../runtime/host_logic.h"

using namespace mnist;

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static int wgrad_groups(int B) {   // conv_bwd.hip's conv_wgrad_groups (monotonic, <= 256)
  const int g = (24 * B + 7) / 8;   // rows = H2 * B, WG_CH = 8 rows per chunk
  return g < 256 ? g : 256;
}

static void test_workspace() {
  const int caps[] = {0, 1, 1000, 10000};
  for (int B = 1; B <= 9000; B += (B < 300 ? 1 : 97)) {
    for (int T : caps) {
      const WorkspaceLayout L = compute_workspace_layout(B, T, wgrad_groups(B), fc_bwd_splits(B));
      const int64_t Ma = std::max<int64_t>(B, T);
      std::vector<std::pair<int64_t, int64_t>> bufs = {
          {L.a1, (int64_t)B * H1 * H1 * C1 * 2}, {L.p, ((Ma + 63) / 64 * 64) * NFLAT * 2},
          {L.pmask, (int64_t)B * NFLAT},          {L.z1part, (int64_t)FC1_KSPLIT * Ma * NH * 4},
          {L.loss_rows, (int64_t)B * 4},          {L.dz1, ((B + 63) / 64 * 64) * NH * 2},
          {L.h_bf, ((B + 63) / 64 * 64) * NH * 2}, {L.dl_bf, ((B + 63) / 64 * 64) * 16 * 2},
          {L.dyc, (int64_t)B * DYC_BYTES_PER_IMAGE}, {L.c1part, 4LL * B * 320 * 4},
          {L.w2part, (int64_t)wgrad_groups(B) * (18432 + 64) * 4},
          {L.fcpart, fc_bwd_splits(B) > 1 ? (int64_t)fc_bwd_splits(B) * FCB_PART_STRIDE * 4 : 4},
          {L.sync, 64},                           {L.w2d_alt, 9LL * C1 * C2 * 2},
          {L.c1red, (int64_t)C1_PRE_SLABS * 320 * 4}, {L.w1t_alt, (int64_t)NFLAT * NH * 2}};
      std::sort(bufs.begin(), bufs.end());
      int64_t end = 0;
      for (auto& b : bufs) {
        CHECK(b.first % 256 == 0);
        CHECK(b.first >= end);                    // disjoint
        end = b.first + b.second;
      }
      CHECK(end <= L.total);
    }
  }
  bool threw = false;
  try {
    compute_workspace_layout(0, 0, 1, 1);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
}

static XgmiGrids grids() {
  XgmiGrids g{};
  g.fc_fused = 73; g.conv_fused = 309; g.twoshot = 145; g.oneshot = 19;
  return g;
}

static XgmiRecord make_record(int q) {
  XgmiRecord r;
  memset(&r, 0, sizeof(r));
  r.blk_off = 0; r.layout = xgmi_block_layout(1200000, 2, 32768); r.numel = 1200000; r.oneshot_max = 32768;
  r.world = 8; r.rank = q; r.channels = 2; r.pid = 1234; r.device = q;
  const XgmiGrids g = grids();
  r.grid_fc = g.fc_fused; r.grid_conv = g.conv_fused; r.grid_two = g.twoshot; r.grid_one = g.oneshot;
  snprintf(r.host, sizeof(r.host), "node-a");
  return r;
}

static bool rejects(const std::vector<uint8_t>& bytes, int q) {
  try {
    decode_record(bytes, q, 8, 1200000, 2, 32768, grids(), "node-a");
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

static void test_records() {
  for (int q = 0; q < 8; ++q) {
    const std::vector<uint8_t> enc = encode_record(make_record(q));
    const XgmiRecord back = decode_record(enc, q, 8, 1200000, 2, 32768, grids(), "node-a");
    CHECK(back.rank == q && back.layout.out_off >= back.layout.in_off + 4800000 && back.device == q);
    CHECK(back.layout.bytes % 4096 == 0 && back.layout.sig_off + 64 <= back.layout.bytes);
    CHECK(rejects(enc, (q + 1) % 8));                                   // wrong rank slot
    std::vector<uint8_t> shorter(enc.begin(), enc.end() - 1), longer = enc;
    longer.push_back(0);
    CHECK(rejects(shorter, q));
    CHECK(rejects(longer, q));
    CHECK(rejects({}, q));
    XgmiRecord r = make_record(q);
    r.numel = 4; CHECK(rejects(encode_record(r), q));
    r = make_record(q); r.grid_conv = 87; CHECK(rejects(encode_record(r), q));
    r = make_record(q); r.blk_off = -256; CHECK(rejects(encode_record(r), q));
    r = make_record(q); r.blk_off = 6; CHECK(rejects(encode_record(r), q));
    r = make_record(q); r.layout.out_off += 4096; CHECK(rejects(encode_record(r), q));
    r = make_record(q); r.layout.bytes -= 4096; CHECK(rejects(encode_record(r), q));
    r = make_record(q); snprintf(r.host, sizeof(r.host), "node-b"); CHECK(rejects(encode_record(r), q));
    r = make_record(q); memset(r.host, 'x', sizeof(r.host)); CHECK(rejects(encode_record(r), q));   // no NUL
  }
  std::mt19937_64 rng(7);
  for (int it = 0; it < 20000; ++it) {                                  // byte soup: reject, never crash
    std::vector<uint8_t> junk(rng() % (2 * sizeof(XgmiRecord) + 1));
    for (auto& b : junk) b = (uint8_t)rng();
    if (junk.size() == sizeof(XgmiRecord) && it % 2 == 0) {            // plausible header, garbage rest
      XgmiRecord r = make_record(3);
      memcpy(junk.data(), &r, offsetof(XgmiRecord, blk_off));
    }
    (void)rejects(junk, 3);
  }
}

static void test_ddp_scale() {
  // world W: head 1/(B*W), epilogues 1.0 - the W-rank SUM of per-rank gradients is the mean-NLL
  // gradient of the W*B batch; the same constant as the world-1 run on W*B rows (bitwise)
  CHECK(ddp_head_inv_batch(200, 8) == 1.0f / 1600.0f);
  CHECK(ddp_head_inv_batch(1600, 1) == ddp_head_inv_batch(200, 8));
  CHECK(ddp_head_inv_batch(200, 1) == 1.0f / 200.0f);
  CHECK(kDdpEpilogueScale == 1.0f);
  bool threw = false;
  try {
    ddp_head_inv_batch(0, 8);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
}

// infer_plan: every image in exactly one group, buffers that cover the grid and grow with B
static void test_infer_plan() {
  int64_t last = 0;
  for (int B = 1; B <= 10000; B = B < 700 ? B + 1 : B + 997) {
    const InferPlan p = infer_plan(B);
    CHECK(p.images_per_wg >= 1 && p.images_per_wg <= INFER_MAX_IPW && p.bands == INFER_BANDS);
    CHECK((int64_t)p.groups * p.images_per_wg >= B && (int64_t)(p.groups - 1) * p.images_per_wg < B);
    CHECK(p.grid_x == p.bands && p.grid_y == p.groups && p.grid_y <= 65535 && p.ticket_count >= p.groups);
    CHECK(p.workspace_bytes >= 4LL * p.bands * p.groups * p.images_per_wg * NH && p.workspace_bytes >= last);
    last = p.workspace_bytes;
  }
  CHECK(infer_plan(INFER_MAX_B).grid_y <= 65535);
  CHECK(4LL * INFER_BANDS * INFER_MAX_B * NH < (1LL << 31));   // 32-bit byte offsets into the partials
  for (int bad : {0, -1, INFER_MAX_B + 1}) {
    bool threw = false;
    try {
      infer_plan(bad);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
  }
}

// plan_step: every schedule decision of the engine's step, against literal expectations
static void test_plan_step() {
  const int CB = FCB_ROLE_C | FCB_ROLE_B, ALL = FCB_ROLES_ALL, Bo = FCB_ROLE_B;
  const int small[] = {200, 1024}, large[] = {1025, 8192}, any[] = {200, 1024, 1025, 8192};
  const StepSwitches def;
  auto nothing_on_comm = [](const StepPlan& p) {
    return !p.fc_reduce_side && !p.dw1_side && !p.fcw_side && !p.chain && !p.c2r && !p.w1t_pp;
  };
  StepSwitches one_bucket, one_bucket_handoff, handoff, no_dw1, no_pp, traced, no_fuse, handoff_traced;
  one_bucket.two_buckets = one_bucket_handoff.two_buckets = false;
  one_bucket_handoff.rccl_handoff = true;
  handoff.rccl_handoff = true;
  no_dw1.fc_dw1_side = false;
  no_pp.w1t_pingpong = false;
  traced.trace = true;
  no_fuse.xgmi_fuse_update = false;
  handoff_traced.rccl_handoff = handoff_traced.trace = true;
  for (int B : any) {
    StepPlan p = plan_step(SERIAL, B, false, def);
    CHECK(p.roles == ALL && p.fc_bwd_reduces && nothing_on_comm(p) && !p.count_fc_bwd_start && p.dgrad_full_grid == 0);
    CHECK(!p.side && !p.xgmi_separate);
    for (const StepSwitches& sw : {one_bucket, one_bucket_handoff}) {
      p = plan_step(RCCL, B, false, sw);
      CHECK(nothing_on_comm(p) && p.roles == ALL && p.fc_bwd_reduces && !p.count_fc_bwd_start && !p.side);
    }
    CHECK(!plan_step(RCCL, B, false, def).c2r && !plan_step(RCCL, B, false, handoff_traced).c2r);
    CHECK(plan_step(RCCL, B, false, handoff).c2r);
    CHECK(plan_step(OVERLAP, B, false, def).wt == (B == 200 || B == 1024 ? 1 : 0));
  }
  for (Schedule s : {OVERLAP, XGMI}) {   // XGMI with the fused kernels plans as OVERLAP, on the full dgrad grid
    const int full = s == XGMI ? 1 : 0;
    for (int B : small) {
      StepPlan p = plan_step(s, B, false, def);
      CHECK(p.side && p.fcw_side && p.roles == Bo && p.w1t_pp && p.chain && p.release == FCBWD_STARTS);
      CHECK(!p.fc_reduce_side && !p.dw1_side && p.fc_bwd_reduces && p.count_fc_bwd_start && !p.c2r && !p.xgmi_separate);
      CHECK(p.dgrad_full_grid == full);
      p = plan_step(s, B, false, no_dw1);
      CHECK(p.roles == ALL && !p.fcw_side && p.chain && !p.w1t_pp && p.release == WGRAD_STARTS);
      p = plan_step(s, B, false, no_pp);
      CHECK(p.fcw_side && !p.w1t_pp && p.roles == Bo);
      p = plan_step(s, B, false, traced);
      CHECK(!p.fcw_side && !p.chain && p.roles == ALL && !p.w1t_pp);
    }
    for (int B : large) {
      StepPlan p = plan_step(s, B, false, def);
      CHECK(p.fc_reduce_side && p.dw1_side && p.roles == CB && !p.fc_bwd_reduces && !p.fcw_side && !p.w1t_pp);
      CHECK(p.chain && p.release == WGRAD_STARTS && p.dgrad_full_grid == full && p.wt == 0);
      p = plan_step(s, B, false, no_dw1);
      CHECK(p.fc_reduce_side && !p.dw1_side && p.roles == ALL && !p.fc_bwd_reduces);
      p = plan_step(s, B, false, traced);
      CHECK(p.dw1_side && !p.chain && p.roles == CB);
    }
  }
  StepPlan p = plan_step(XGMI, 200, false, no_fuse);
  CHECK(!p.fcw_side && !p.chain && p.roles == ALL && p.xgmi_separate && p.side && p.dgrad_full_grid == 1);
  p = plan_step(XGMI, 1025, false, no_fuse);
  CHECK(p.dw1_side && p.roles == CB && !p.chain && p.xgmi_separate);
  for (int B : small) {
    p = plan_step(RCCL, B, false, handoff);
    CHECK(p.roles == ALL && p.c2r && p.count_fc_bwd_start && p.dgrad_full_grid == 1 && p.fc_bwd_reduces && !p.side);
    CHECK(!p.chain && !p.fcw_side && !p.fc_reduce_side && p.release == WGRAD_STARTS);
  }
  for (int B : large) {
    p = plan_step(RCCL, B, false, handoff);
    CHECK(p.fc_reduce_side && p.dw1_side && p.roles == CB && p.c2r && !p.fc_bwd_reduces && p.count_fc_bwd_start);
  }
  for (int B : any) {   // fp32: which schedules run the chained two-stream step
    CHECK(plan_step(OVERLAP, B, true, def).f32_chained && plan_step(XGMI, B, true, def).f32_chained);
    CHECK(plan_step(OVERLAP, B, true, traced).f32_chained && plan_step(XGMI, B, true, no_fuse).f32_chained);
    CHECK(plan_step(RCCL, B, true, handoff).f32_chained);
    CHECK(!plan_step(RCCL, B, true, def).f32_chained && !plan_step(RCCL, B, true, handoff_traced).f32_chained);
    CHECK(!plan_step(RCCL, B, true, one_bucket_handoff).f32_chained && !plan_step(SERIAL, B, true, def).f32_chained);
    CHECK(!plan_step(OVERLAP, B, false, def).f32_chained);
  }
  // the counter block: the values the kernels' arguments were built from before the counters had names
  CHECK(WGRAD_STARTS == 0 && FC_UPDATES == 1 && HANDOFF_ERR == 2 && CONV2_UPDATES == 3 && DGRAD_STARTS == 4);
  CHECK(FCBWD_STARTS == 5 && HANDOFF_COUNTERS == 6 && PROBE_SCRATCH == 8 && FAULT_HOLD == 12);
  CHECK((FAULT_HOLD + 4) * (int)sizeof(int) <= 256);   // inside the workspace's sync block (carve(256))
  CHECK(SERIAL == 0 && OVERLAP == 1 && RCCL == 2 && XGMI == 3);
}

static void test_fit() {
  int a = 145, b = 309;
  double l = fit_grid_pair(&a, 8, 1024, &b, 39, 1024, 1, 0.5);
  CHECK(a == 145 && b == 309 && l < 0.5);                               // one rank per GPU: untouched
  a = 145; b = 309;
  l = fit_grid_pair(&a, 8, 1024, &b, 39, 1024, 4, 0.5);
  CHECK(l <= 0.5 + 1e-9 && a >= 8 && b >= 39 && a < 145 && b < 309);  // four ranks: shrunk to fit
  a = 512; b = 512;
  l = fit_grid_pair(&a, 400, 100, &b, 400, 100, 8, 0.5);
  CHECK(a == 400 && b == 400 && l > 1.0);                               // minimums cannot fit: reported
  bool threw = false;
  try {
    fit_grid_pair(&a, 1, 0, &b, 1, 1, 1, 0.5);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
}

// the message a check throws, "" when it passes
template <class F>
static std::string thrown(F f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

// the row kernels' pointer checks: the predicate, and the launchers' messages word for word
static void test_row_checks() {
  alignas(16) static unsigned char mem[64];
  const uint8_t* u0 = mem;
  const float* f0 = reinterpret_cast<const float*>(mem);
  const float* f4 = reinterpret_cast<const float*>(mem + 4);   // 4-byte aligned only
  const float* fnull = nullptr;
  CHECK(!misaligned(15, fnull) && !misaligned(3, fnull) && !misaligned(15));   // null counts as aligned
  CHECK(!misaligned(3, f4) && misaligned(15, f4) && !misaligned(15, f0) && misaligned(3, u0 + 1));
  CHECK(misaligned(15, f0, fnull, f4) && misaligned(15, f4, f0) && !misaligned(15, f0, fnull, u0 + 16));   // the OR
  CHECK(misaligned(3, f0, u0 + 2, f4) && !misaligned(3, f0, u0, f4));

  const std::string one = "smooth_noise: null argument (exactly one of the uint8 and the fp32 rows)";
  const std::string src = "smooth_noise: the source rows must be 16-byte aligned (uint8 rows: 4-byte)";
  CHECK(thrown([&] { check_row_source("smooth_noise", nullptr, nullptr); }) == one);
  CHECK(thrown([&] { check_row_source("smooth_noise", u0, f0); }) == one);
  CHECK(thrown([&] { check_row_source("smooth_noise", u0 + 1, nullptr); }) == src);
  CHECK(thrown([&] { check_row_source("smooth_noise", u0 + 2, nullptr); }) == src);
  CHECK(thrown([&] { check_row_source("smooth_noise", nullptr, f4); }) == src);
  CHECK(thrown([&] { check_row_source("smooth_noise", u0 + 4, nullptr); }) == "");   // uint8 rows: 4 bytes suffice
  CHECK(thrown([&] { check_row_source("smooth_noise", nullptr, f0); }) == "");
  CHECK(thrown([&] { check_one_row_source("deepfool_init", u0, f0); }) ==
        "deepfool_init: null argument (exactly one of the uint8 and the fp32 rows)");
  CHECK(thrown([&] { check_one_row_source("deepfool_init", u0 + 1, nullptr); }) == "");   // alignment is the other half
  CHECK(thrown([&] { check_row_source_aligned("smooth_noise", nullptr, f4); }) == src);

  CHECK(thrown([&] { check_row_source("attr_path", nullptr, nullptr, f0); }) ==
        "attr_path: null argument (exactly one of the uint8 and the fp32 rows)");
  CHECK(thrown([&] { check_row_source("attr_reduce", u0 + 1, nullptr, f4); }) ==   // the source is checked first
        "attr_reduce: the source rows must be 16-byte aligned (uint8 rows: 4-byte)");
  CHECK(thrown([&] { check_row_source("attr_path", u0, nullptr, f4); }) == "attr_path: the baseline rows must be 16-byte aligned");
  CHECK(thrown([&] { check_row_source("attr_reduce", nullptr, f0, f4); }) ==
        "attr_reduce: the baseline rows must be 16-byte aligned");
  CHECK(thrown([&] { check_row_source("attr_path", u0 + 4, nullptr, nullptr); }) == "");   // no baseline rows: a scalar
  CHECK(thrown([&] { check_row_source("attr_path", nullptr, f0, f0 + 4); }) == "");
}

int main() {
  test_row_checks();
  test_workspace();
  test_records();
  test_fit();
  test_ddp_scale();
  test_infer_plan();
  test_plan_step();
  if (failures) {
    fprintf(stderr, "HOST_LOGIC_TEST FAILED (%d)\n", failures);
    return 1;
  }
  printf("HOST_LOGIC_TEST PASS\n");
  return 0;
}
