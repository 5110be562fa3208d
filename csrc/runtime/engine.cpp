#include "engine.h"

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace mnist {

#define HIP_OK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_));           \
  } while (0)

namespace {
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
}  // namespace

Engine::Engine(const EngineBuffers& buf, int max_batch, int max_test_batch, hipStream_t compute,
               hipStream_t comm, int world_size, float rho, float eps, float weight_decay, bool fp32)
    : buf_(buf), max_batch_(max_batch), max_test_batch_(max_test_batch), compute_(compute),
      comm_stream_(comm), world_(world_size), rho_(rho), eps_(eps), wd_(weight_decay), f32_(fp32) {
  if (max_batch < 1 || max_test_batch < 0) throw std::runtime_error("bad batch sizes");
  HIP_OK(hipEventCreateWithFlags(&ev_fc_, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
  for (SideLauncher& l : side_) HIP_OK(hipEventCreateWithFlags(&l.join, hipEventDisableTiming));
  alloc_workspace();
  if (f32_) alloc_workspace_f32();
}

Engine::~Engine() {
  for (SideLauncher& l : side_) {
    if (l.thread.joinable()) {
      {
        std::lock_guard<std::mutex> lk(l.mu);
        l.stop = true;
      }
      l.cv.notify_all();
      l.thread.join();
    }
    if (l.join) hipEventDestroy(l.join);
  }
  for (auto g : side_graphs_)
    if (g) hipGraphExecDestroy(g);
  for (auto g : graphs_) hipGraphExecDestroy(g);
  for (auto g : graph_defs_) hipGraphDestroy(g);
  for (hipEvent_t e : {ev_fc_, ev_done_, ev_fork_})
    if (e) hipEventDestroy(e);
  if (ws_) hipFree(ws_);
  if (ws32_) hipFree(ws32_);
  if (adv_ws_) hipFree(adv_ws_);
}

void Engine::alloc_workspace() {
  const WorkspaceLayout L =
      compute_workspace_layout(max_batch_, max_test_batch_, conv_wgrad_groups(max_batch_), fc_bwd_splits(max_batch_));
  ws_bytes_ = L.total;
  HIP_OK(hipMalloc(&ws_, ws_bytes_));
  launch_fill(ws_, ws_bytes_, 0, nullptr);   // padding rows of p etc. must be finite
  HIP_OK(hipStreamSynchronize(nullptr));
  char* base = static_cast<char*>(ws_);
  a1_ = reinterpret_cast<uint16_t*>(base + L.a1);
  p_ = reinterpret_cast<uint16_t*>(base + L.p);
  pmask_ = reinterpret_cast<uint8_t*>(base + L.pmask);
  z1part_ = reinterpret_cast<float*>(base + L.z1part);
  loss_rows_ = reinterpret_cast<float*>(base + L.loss_rows);
  dz1_ = reinterpret_cast<uint16_t*>(base + L.dz1);
  h_bf_ = reinterpret_cast<uint16_t*>(base + L.h_bf);
  dl_bf_ = reinterpret_cast<uint16_t*>(base + L.dl_bf);
  dyc_ = reinterpret_cast<uint8_t*>(base + L.dyc);
  c1part_ = reinterpret_cast<float*>(base + L.c1part);
  w2part_ = reinterpret_cast<float*>(base + L.w2part);
  fcpart_ = reinterpret_cast<float*>(base + L.fcpart);
  sync_ = reinterpret_cast<int*>(base + L.sync);
  w2d_alt_ = reinterpret_cast<uint16_t*>(base + L.w2d_alt);
  c1red_ = reinterpret_cast<float*>(base + L.c1red);
  w1t_alt_ = reinterpret_cast<uint16_t*>(base + L.w1t_alt);
}

void Engine::alloc_workspace_f32() {
  const int64_t M = max_batch_, Ma = max_batch_ > max_test_batch_ ? max_batch_ : max_test_batch_;
  // fc1 split-K partials: 36 splits up to 1024 rows, 9 beyond (f32_fc1_splits), for any batch <= Ma
  const int64_t z1rows = std::max<int64_t>(36 * std::min<int64_t>(Ma, 1024), 9 * Ma);
  int64_t off = 0;
  auto carve = [&](int64_t bytes) { int64_t o = off; off += ws_align256(bytes); return o; };
  const int64_t o_w2f = carve(9 * C1 * C2 * 4), o_w2b = carve(9 * C1 * C2 * 4), o_w1p = carve((int64_t)NH * NFLAT * 4);
  const int64_t o_a1 = carve(Ma * H1 * H1 * C1 * 4), o_y2 = carve(Ma * H2 * H2 * C2 * 4);
  const int64_t o_p = carve(Ma * NFLAT * 4), o_pm = carve(Ma * NFLAT), o_z1 = carve(z1rows * NH * 4);
  const int64_t o_h = carve(M * NH * 4), o_dz1 = carve(M * NH * 4), o_dl = carve(M * 16 * 4);
  const int64_t o_loss = carve(M * 4);
  const int64_t o_c2 = carve((int64_t)F32_MAX_SPLITS * C2 * (9 * C1 + 1) * 4);
  const int64_t o_c1 = carve((int64_t)F32_C1W_BLOCKS * C1 * 10 * 4);
  const int64_t o_dx1 = carve(M * H1 * H1 * C1 * 4);
  HIP_OK(hipMalloc(&ws32_, off));
  launch_fill(ws32_, off, 0, nullptr);
  HIP_OK(hipStreamSynchronize(nullptr));
  ws_bytes_ += off;
  char* b = static_cast<char*>(ws32_);
  F32Step& w = f32ws_;
  w.w2fwd = reinterpret_cast<float*>(b + o_w2f);
  w.w2bwd = reinterpret_cast<float*>(b + o_w2b);
  w.w1p = reinterpret_cast<float*>(b + o_w1p);
  w.a1 = reinterpret_cast<float*>(b + o_a1);
  w.dx1 = reinterpret_cast<float*>(b + o_dx1);
  w.y2 = reinterpret_cast<float*>(b + o_y2);
  w.p = reinterpret_cast<float*>(b + o_p);
  w.pm = reinterpret_cast<uint8_t*>(b + o_pm);
  w.z1part = reinterpret_cast<float*>(b + o_z1);
  w.h = reinterpret_cast<float*>(b + o_h);
  w.dz1 = reinterpret_cast<float*>(b + o_dz1);
  w.dl = reinterpret_cast<float*>(b + o_dl);
  w.loss_rows = reinterpret_cast<float*>(b + o_loss);
  w.c2part = reinterpret_cast<float*>(b + o_c2);
  w.c1part = reinterpret_cast<float*>(b + o_c1);
}

// pre-gathered epoch rows when available (one load level less on every step's critical path)
Engine::StepInput Engine::train_input() const {
  if (buf_.epoch_u8) return {buf_.epoch_u8, nullptr, idx_stride_, buf_.epoch_labels};
  return {buf_.train_u8, buf_.train_idx, idx_stride_, buf_.train_labels};
}

F32Step Engine::f32_args(const StepInput& in, StepState* state, float inv_batch) const {
  F32Step a = f32ws_;
  a.param = buf_.param;
  a.grad = buf_.grad;
  a.loss_log = buf_.loss_log;
  a.data_u8 = in.data;
  a.idx = in.idx;
  a.idx_step_stride = in.stride;
  a.labels = in.labels;
  a.state = state;
  a.inv_batch = inv_batch;
  return a;
}

AdadeltaArgs Engine::adadelta_args() const {
  return AdadeltaArgs{buf_.param, buf_.grad, buf_.square_avg, buf_.acc_delta, buf_.lr, rho_, eps_, wd_,
                      buf_.w2f, buf_.w2d, buf_.w1, buf_.w1t, nullptr};
}

// the update holds its completion until counter a >= counter b + delta
AdadeltaArgs Engine::held(AdadeltaArgs u, Counter a, Counter b, int delta) const {
  u.hold_a = ctr(a);
  u.hold_b = ctr(b);
  u.hold_delta = delta;
  u.hold_err = ctr(HANDOFF_ERR);
  return u;
}

static ConvBwdArgs with_signal(ConvBwdArgs c, int* ctr) { c.signal_ctr = ctr; return c; }   // adds 1 at its start

static void check_batch(int batch, int cap, const char* what) {
  if (batch < 1 || batch > cap) throw std::runtime_error(std::string(what) + " exceeds engine capacity");
}

void Engine::attach_comm(std::shared_ptr<RcclComm> comm) {
  if (comm && comm->world_size() != world_) throw std::runtime_error("comm world size mismatch");
  comm_ = std::move(comm);
}

void Engine::attach_xgmi(std::shared_ptr<XgmiComm> x) {
  if (x && x->world_size() != world_) throw std::runtime_error("xgmi world size mismatch");
  if (x && x->world_size() > 1 && !x->connected()) throw std::runtime_error("xgmi communicator not connected");
  if (x && x->numel() != PARAM_TOTAL) throw std::runtime_error("xgmi communicator must cover the flat gradient");
  if (x && x->channels() <= XGMI_CH_CONV2) throw std::runtime_error("xgmi communicator needs 3 channels");
  if (!x && sched_ == XGMI) {           // no schedule until set_schedule (enqueue refuses SERIAL at world > 1)
    sync_streams();
    sched_ = SERIAL;
  }
  if (!grad_own_) grad_own_ = buf_.grad;
  // the gradient producers write straight into the communicator's (IPC-exported) input buffer
  buf_.grad = x ? x->in() : grad_own_;
  xgmi_ = std::move(x);
}

void Engine::set_schedule(int s) {
  if (s == SERIAL || s == OVERLAP) {
    if (world_ != 1 || comm_ || xgmi_)
      throw std::runtime_error("engine: the single-GPU schedules need world size 1 and no transport attached");
  } else if (s == RCCL) {
    if (!comm_) throw std::runtime_error("engine: the RCCL schedule needs an RCCL communicator");
    if (xgmi_) throw std::runtime_error("engine: detach the xgmi communicator before selecting RCCL");
  } else if (s == XGMI) {
    if (!xgmi_) throw std::runtime_error("engine: the XGMI schedule needs an xgmi communicator");
  } else {
    throw std::runtime_error("engine: unknown schedule " + std::to_string(s));
  }
  if (adv_.steps > 0) check_adversarial_scope(s);
  if (noise_) check_adversarial_scope(s, "Gaussian-noise training");
  sched_ = s;
  reset_counters();
}

// Adversarial steps run on the compute stream alone.  The side-stream schedules update the bf16 shadows
// (w1, w1t, w2d) under the previous step's backward, ordered against the next step's readers by hand-off
// holds that know nothing of the attack's launches; the fp32 step has no xin form.
void Engine::check_adversarial_scope(int sched, const char* what) const {
  const std::string w = std::string("engine: ") + what;
  if (f32_) throw std::runtime_error(w + " is limited to the bf16 step (fp32 is not supported)");
  if (world_ != 1 || comm_ || xgmi_)
    throw std::runtime_error(w + " is limited to world size 1 (no RCCL / XGMI transport)");
  if (sched != SERIAL) {
    static const char* names[] = {"SERIAL", "OVERLAP", "RCCL", "XGMI"};
    throw std::runtime_error(w + " is limited to the SERIAL schedule (not " +
                             (sched >= 0 && sched < 4 ? names[sched] : "?") + ")");
  }
}

void Engine::alloc_adversarial_workspace() {
  if (adv_ws_) return;
  const int64_t rows = ws_align256((int64_t)max_batch_ * IMG * IMG * sizeof(float));
  const int64_t labs = ws_align256((int64_t)round_up(max_batch_, 32) * sizeof(int32_t));
  const int64_t total = 2 * rows + labs + ws_align256(sizeof(StepState));
  HIP_OK(hipMalloc(&adv_ws_, total));
  launch_fill(adv_ws_, total, 0, nullptr);
  HIP_OK(hipStreamSynchronize(nullptr));
  char* b = static_cast<char*>(adv_ws_);
  adv_x0_ = reinterpret_cast<float*>(b);
  adv_x_ = reinterpret_cast<float*>(b + rows);
  adv_labels_ = reinterpret_cast<int32_t*>(b + 2 * rows);
  adv_state_ = reinterpret_cast<StepState*>(b + 2 * rows + labs);
  adv_bytes_ = total;
  // inference semantics from the start (begin_epoch rewrites it with the epoch's seed)
  launch_set_state(adv_state_, StepState{0, STEP_FLAG_NO_DROPOUT, 0, 0}, compute_);
}

void Engine::set_noise(float sigma, bool on) {
  if (!on) {                 // off: the plain step, nothing of it is launched (the buffers stay)
    noise_ = false;
    noise_sigma_ = 0.0f;
    return;
  }
  if (!(sigma >= 0.0f)) throw std::runtime_error("engine: Gaussian-noise training needs sigma >= 0");
  if (adv_.steps > 0)
    throw std::runtime_error("engine: Gaussian-noise training and adversarial training are mutually exclusive");
  check_adversarial_scope(sched_, "Gaussian-noise training");
  alloc_adversarial_workspace();
  noise_ = true;
  noise_sigma_ = sigma;
}

void Engine::set_adversarial(float eps, float step_size, int steps, bool random_start, float lo, float hi) {
  if (steps < 0) throw std::runtime_error("engine: adversarial steps must be >= 0");
  if (steps == 0) {          // off: the plain step, nothing of the attack is launched (the buffers stay)
    adv_ = {};
    return;
  }
  if (!(eps >= 0.0f) || !(step_size >= 0.0f) || !(lo <= hi))
    throw std::runtime_error("engine: adversarial training needs eps >= 0, step_size >= 0 and lo <= hi");
  if (noise_)
    throw std::runtime_error("engine: adversarial training and Gaussian-noise training are mutually exclusive");
  check_adversarial_scope(sched_);
  alloc_adversarial_workspace();
  adv_ = AdvConfig{eps, step_size, lo, hi, steps, random_start};
}

void Engine::reset_counters() {
  // the hand-off counters only move in matched pairs inside a completed chunk; after a schedule
  // change or an aborted chunk they restart from zero, and so does the hand-off error flag
  // HANDOFF_ERR (callers read it with check_errors before they get here)
  sync_streams();
  launch_fill(ctr(0), HANDOFF_COUNTERS * sizeof(int), 0, compute_);
  HIP_OK(hipStreamSynchronize(compute_));
  reset_host_state();
}

void Engine::begin_epoch(uint64_t seed, uint64_t rng_base, int step0, int flags) {
  // 24 bytes as kernel arguments, ordered on the compute stream (never inside a captured graph):
  // no host sync, so the next epoch is enqueued while the previous one still runs
  launch_set_state(buf_.state, StepState{step0, flags, seed, rng_base}, compute_);
  // the attack's state next to it: inference semantics (no dropout), whatever the training flags
  if (adv_.steps > 0)
    launch_set_state(adv_state_, StepState{step0, flags | STEP_FLAG_NO_DROPOUT, seed, rng_base}, compute_);
}

void Engine::phase_begin(const char* name) {
  if (sw_.trace) roctx_push(name);
}

void Engine::phase_end() {
  if (!sw_.trace) return;
  HIP_OK(hipStreamSynchronize(compute_));
  HIP_OK(hipStreamSynchronize(comm_stream_));
  roctx_pop();
}

void Engine::profile_steps(int n, int batch, int stride) {
  check_batch(batch, max_batch_, "batch");
  idx_stride_ = stride;
  sw_.trace = true;
  try {
    for (int i = 0; i < n; ++i) {
      roctx_push("train_step");
      enqueue_step(batch, i == n - 1);
      HIP_OK(hipStreamSynchronize(compute_));
      roctx_pop();
    }
  } catch (...) {
    sw_.trace = false;
    throw;
  }
  sw_.trace = false;
  HIP_OK(hipGetLastError());
}

struct Engine::StepArgs {
  int B, Bp;
  bool last;
  StepPlan plan;
  FcBwdArgs fb;
  AdadeltaArgs ad, adc;   // adc: the step's last update, which advances the device step counter
  ConvBwdArgs cb;
};

// once per chunk: order the comm stream after the chunk start
void Engine::fork_comm_once() {
  if (cur_.side_forked) return;
  HIP_OK(hipEventRecord(ev_fc_, compute_));
  HIP_OK(hipStreamWaitEvent(comm_stream_, ev_fc_, 0));
  cur_.side_forked = true;
}

// chunk end: one real join edge, the comm stream into compute (split capture: an event at replay)
void Engine::end_chunk() {
  if (pass_.main && !pass_.replay_join) {
    HIP_OK(hipEventRecord(ev_done_, comm_stream_));
    HIP_OK(hipStreamWaitEvent(compute_, ev_done_, 0));
  }
  cur_.side_pending = cur_.side_forked = false;
}

// The attack of an adversarial step (set_adversarial): adv_init, then per iteration the launch sequence of
// ops/attack.py fused_adversarial on the engine's own activation buffers, under the attack's StepState.
// BUFFERS: the attack overwrites a1_, p_, pmask_, z1part_, loss_rows_, dz1_, h_bf_, dl_bf_ and dyc_ with the
// same kernels at the same B that the training step runs right after it, and each of those writes all it
// owns whatever it finds there: trunk_fwd every a1 / p / pmask element of rows < B, fc1_fwd every z1part
// slice, head_train rows < B of loss_rows / dz1 / h_bf / dl_bf and zeros in their padding rows [B, Bp),
// fc_bwd role B every byte of every record of rows < B (rows >= B of p are masked, not read).  So every
// buffer the training step reads is written by the training step's own launches; the attack never
// touches grad, the partials (fcpart_, w2part_, c1part_), loss_log or the training state.
void Engine::enqueue_attack(const TrunkFwdArgs& tf, const HeadArgs& ha, const StepInput& in, int B, int Bp) {
  launch_adv_init(AdvInitArgs{in.data, in.idx, in.stride, in.labels, buf_.state, adv_x0_, adv_x_, adv_labels_,
                              adv_.eps, adv_.lo, adv_.hi, adv_.random_start ? 1 : 0},
                  B, compute_);
  TrunkFwdArgs t = tf;
  t.xin = adv_x_;
  t.state = adv_state_;
  t.wait_a = t.wait_b = nullptr;
  t.wait_err = nullptr;
  HeadArgs h = ha;
  h.labels = adv_labels_; h.idx = nullptr; h.idx_step_stride = 0;
  h.state = adv_state_; h.inv_batch = 1.0f;                 // the summed NLL, as Predictor.adversarial
  const FcBwdArgs fb{dz1_, p_, pmask_, buf_.w1t, h_bf_, dl_bf_, loss_rows_, adv_state_, nullptr, dyc_,
                     nullptr, 1.0f, 1.0f, fcpart_};
  const InputGradStepArgs ig{{dyc_, a1_, buf_.w2d, t.w1c, nullptr}, adv_x_, adv_x0_, adv_x_,
                             adv_.alpha, adv_.eps, adv_.lo, adv_.hi};
  for (int k = 0; k < adv_.steps; ++k) {
    launch_trunk_fwd(t, B, true, compute_);
    launch_fc1_fwd(p_, buf_.w1, z1part_, B, compute_);
    launch_head_train(h, B, Bp, compute_);
    launch_fc_bwd_role(fb, B, Bp, 2, compute_);             // role B alone: the dy records
    launch_input_grad_step(ig, B, compute_);                // x <- the projected step, in place
  }
}

void Engine::enqueue_step(int batch, bool last) {
  if (adv_.steps > 0) check_adversarial_scope(sched_);
  if (noise_) check_adversarial_scope(sched_, "Gaussian-noise training");
  // the head scales by 1/(B*world): without a transport every rank would train alone on a gradient
  // world times too small
  if (world_ > 1 && sched_ != RCCL && sched_ != XGMI)
    throw std::runtime_error("engine: world size > 1 needs the RCCL or XGMI schedule");
  const StepPlan plan = plan_step((Schedule)sched_, batch, f32_, sw_);
  if (f32_) return enqueue_step_f32(batch, last, plan);
  const int B = batch, Bp = round_up(B, 32);
  float* P = buf_.param;
  // DDP averaging: each rank's head scales the loss gradient by 1/(world*B) and the all-reduce sums,
  // so every row's bf16 gradient operands (dz1, dl) are bitwise those of the world-1 run on the
  // world*B batch (scaling by 1/B and then by 1/world rounds the fp32 constant differently and flips
  // bf16 ties: a systematic ~7e-6 gradient offset, tools/ddp_equivalence.py)
  const float gscale = kDdpEpilogueScale;
  const bool M = pass_.main;   // split capture (capture_train_split): only the pass's own stream is fed
  const StepInput in = train_input();

  // ---- the kernel arguments, shared by every schedule
  TrunkFwdArgs tf{in.data, in.idx, in.stride, buf_.state, P + OFF_CONV1_W, P + OFF_CONV1_B,
                  buf_.w2f, P + OFF_CONV2_B, a1_, p_, pmask_, nullptr};
  // the previous step's fc update (comm stream) must be done before fc1_fwd reads w1: trunk_fwd
  // holds its completion for it (device counters, no extra launch)
  if (cur_.side_pending) {
    tf.wait_a = ctr(FC_UPDATES);
    tf.wait_b = ctr(WGRAD_STARTS);
    tf.wait_err = ctr(HANDOFF_ERR);
  }
  cur_.side_pending = false;
  HeadArgs ha{};
  ha.z1part = z1part_; ha.b_fc1 = P + OFF_FC1_B; ha.w_fc2 = P + OFF_FC2_W; ha.b_fc2 = P + OFF_FC2_B;
  ha.labels = in.labels; ha.idx = in.idx; ha.idx_step_stride = in.stride;
  ha.state = buf_.state; ha.inv_batch = ddp_head_inv_batch(B, world_);
  ha.loss_rows = loss_rows_; ha.dz1 = dz1_; ha.h_bf = h_bf_; ha.dl_bf = dl_bf_;
  // fc_bwd's roles (plan_step).  B > 1024: the fc split partials are summed on the comm stream, ahead
  // of the fc update / all-reduce that consumes them, instead of on the compute chain (SERIAL /
  // one-bucket RCCL: here), and the fc1 weight gradient itself (role A: 145 workgroups per 1024-row
  // split streaming p from HBM) leaves the compute chain for the comm stream, ahead of that reduce,
  // where it runs beside conv2_wgrad / conv2_dgrad.  The next step cannot overwrite p / dz1 before it
  // is done: the comm stream's later launches (fc update, conv2 update) gate the next trunk_fwd /
  // fc1_fwd.
  // OVERLAP / XGMI chain, B <= 1024: both fc weight gradients (roles C + A, 146 workgroups) leave the
  // compute launch for the comm stream, released by fc_bwd's start (FCBWD_STARTS: head_train done)
  // instead of by wgrad's start, so the fc update (or fc all-reduce + update) that follows them
  // starts ~wgrad's length earlier and the comm chain - conv2's reduce + update at its end gates the
  // next trunk_fwd - finishes earlier.  The compute chain keeps role B (dy records) only ...
  StepArgs a{B, Bp, last, plan,
             FcBwdArgs{dz1_, p_, pmask_, buf_.w1t, h_bf_, dl_bf_, loss_rows_, buf_.state, buf_.grad, dyc_,
                       buf_.loss_log, gscale, 1.0f / (float)B, fcpart_},
             adadelta_args(), {},
             ConvBwdArgs{dyc_, a1_, buf_.w2d, P + OFF_CONV1_W, P + OFF_CONV1_B, in.data, in.idx, in.stride,
                         buf_.state, c1part_, w2part_, buf_.grad, gscale, conv_wgrad_groups(B), nullptr}};
  if (plan.count_fc_bwd_start) a.fb.signal_ctr = ctr(FCBWD_STARTS);   // in lockstep with FC_UPDATES
  // ... so that fc update runs beside role B, which reads w1t: role B reads this step's copy while the
  // update writes the other (ping-pong like w2d in tail_chain; every element is rewritten each step)
  // (w1t_pingpong off: test hook only - the update overwrites the copy role B reads, the race the
  // ping-pong exists for; docs/DEBUGGING.md "race-window widening")
  uint16_t* const w1t_cur = cur_.w1t_in_alt ? w1t_alt_ : buf_.w1t;
  a.fb.w1t = w1t_cur;
  a.ad.w1t = plan.w1t_pp ? (cur_.w1t_in_alt ? buf_.w1t : w1t_alt_) : w1t_cur;
  if (plan.w1t_pp) cur_.w1t_in_alt = !cur_.w1t_in_alt;
  a.ad.wt = plan.wt;
  a.adc = a.ad;
  a.adc.state_inc = buf_.state;
  a.cb.c1_rows = conv_dgrad_c1_rows(B);
  if (a.cb.c1_rows > C1_PRE_MIN_SLABS) a.cb.c1red = c1red_;   // large batch: conv1 partials pre-reduced
  a.cb.dgrad_full_grid = plan.dgrad_full_grid;

  // ---- adversarial step (SERIAL only): the attack, then today's step on the attacked batch
  if (adv_.steps > 0) {
    phase_begin("attack");
    enqueue_attack(tf, ha, in, B, Bp);
    phase_end();
    tf.xin = a.cb.xin = adv_x_;
    ha.labels = adv_labels_; ha.idx = nullptr; ha.idx_step_stride = 0;
  }

  // ---- Gaussian-noise step (SERIAL only): the batch normalised and gathered, the noise in place, today's step
  if (noise_) {
    phase_begin("noise");
    launch_adv_init(AdvInitArgs{in.data, in.idx, in.stride, in.labels, buf_.state, adv_x0_, adv_x_, adv_labels_,
                                0.0f, 0.0f, 0.0f, 0},
                    B, compute_);
    launch_smooth_noise_step(buf_.state, adv_x0_, adv_x_, noise_sigma_, B, compute_);
    phase_end();
    tf.xin = a.cb.xin = adv_x_;
    ha.labels = adv_labels_; ha.idx = nullptr; ha.idx_step_stride = 0;
  }

  // ---- forward and fc_bwd, then the schedule's tail
  if (plan.side) fork_comm_once();
  phase_begin("fwd");
  if (M) launch_trunk_fwd(tf, B, true, compute_);
  if (M) launch_fc1_fwd(p_, buf_.w1, z1part_, B, compute_);
  if (M) launch_head_train(ha, B, Bp, compute_);
  phase_next("bwd_fc");
  if (M) launch_fc_bwd(a.fb, B, Bp, compute_, plan.fc_bwd_reduces, plan.roles);
  phase_end();
  if (sched_ == SERIAL) return tail_serial(a);
  if (sched_ == RCCL) return tail_rccl(a);
  tail_chain(a);
}

void Engine::tail_serial(StepArgs& a) {
  phase_begin("bwd_conv_wgrad");
  launch_conv_wgrad(a.cb, a.B, compute_);
  phase_next("bwd_conv_dgrad");
  launch_conv_dgrad(a.cb, a.B, compute_);
  phase_next("grad_reduce+update");          // conv slab reduce + the whole Adadelta update
  launch_adadelta_reduce(a.adc, a.cb, a.B, compute_);
  phase_end();
}

void Engine::tail_rccl(StepArgs& a) {
  const int B = a.B;
  const StepPlan& plan = a.plan;
  const ConvBwdArgs& cb = a.cb;
  if (!sw_.two_buckets) {                       // one bucket: one all-reduce after the whole backward
    launch_conv_wgrad(cb, B, compute_);
    launch_conv_dgrad(cb, B, compute_);
    launch_conv_grad_reduce(cb, B, compute_);
    comm_->allreduce_sum(buf_.grad, PARAM_TOTAL, 0, compute_);
    launch_adadelta(a.adc, ADA_ALL, compute_);
    return;
  }
  // the fc bucket (98.4 % of the bytes) forks onto the comm stream as soon as fc_bwd is done and
  // overlaps the conv backward; the conv bucket follows on compute after the join, so the one
  // communicator sees fc, conv in the same order on every rank and never two collectives at once.
  // The join waits for the fc all-reduce (and conv2's slab reduce, below) only: the fc update runs
  // after them on the comm stream (144 workgroups, beside the conv tail) and is ordered before the
  // next step's fc1_fwd by trunk_fwd's completion hold on device counters (WGRAD_STARTS, FC_UPDATES),
  // as in OVERLAP - at world > 1 the update is not on the path to the conv all-reduce.
  // (capture order matters: the graph executor keeps a fork's first-captured child on the
  // launching queue, so conv2 wgrad is enqueued before the comm branch)
  HIP_OK(hipEventRecord(ev_fc_, compute_));
  phase_begin("bwd_conv_wgrad");                // wgrad's start: this step's fc grads are final
  launch_conv_wgrad(with_signal(cb, ctr(WGRAD_STARTS)), B, compute_);
  phase_next("allreduce_fc+update");
  HIP_OK(hipStreamWaitEvent(comm_stream_, ev_fc_, 0));
  if (plan.dw1_side) launch_fc_bwd_dw1(a.fb, B, a.Bp, comm_stream_);
  if (plan.fc_reduce_side) launch_fc_grad_reduce(a.fb, B, comm_stream_);
  comm_->allreduce_sum(buf_.grad + OFF_FC1_W, OFF_CONV1_W - OFF_FC1_W, 0, comm_stream_);
  // hand-offs (distinct queues; plan.c2r): conv2's slab reduce (289 of the conv bucket's 309 reduce
  // workgroups) follows the fc all-reduce on the comm stream, released by dgrad's start (wgrad,
  // which writes the slabs, is done) and running under dgrad; the join waits for it, so the step
  // tail keeps only conv1's 20 reduce workgroups before the conv all-reduce.  The fc update comes
  // after it (world 1, 600 steps: 82.5-82.6 -> 75.3 us/step; the update before it, so that the
  // join also waits for the update: 86.7; profiles/r5/ddp_world1/rccl_conv2_reduce_side.txt)
  if (plan.c2r) {
    launch_stream_wait(ctr(DGRAD_STARTS), ctr(CONV2_UPDATES), 1, ctr(HANDOFF_ERR), comm_stream_);
    launch_conv_grad_reduce_parts(cb, B, 0, RED_W2_PARTS, comm_stream_);
    launch_stream_signal(ctr(CONV2_UPDATES), comm_stream_);
  }
  if (sw_.rccl_handoff) {
    HIP_OK(hipEventRecord(ev_done_, comm_stream_));
    launch_adadelta(a.ad, ADA_FC, comm_stream_, ADA_FC_LEAN_GRID);
    launch_stream_signal(ctr(FC_UPDATES), comm_stream_);   // fc update of this step done
    cur_.side_pending = true;
  } else {                                      // streams share a hardware queue: no counter holds
    launch_adadelta(a.ad, ADA_FC, comm_stream_);
    HIP_OK(hipEventRecord(ev_done_, comm_stream_));
  }
  phase_next("bwd_conv_dgrad");
  // c2r: dgrad's start releases conv2's reduce on the comm stream
  launch_conv_dgrad(plan.c2r ? with_signal(cb, ctr(DGRAD_STARTS)) : cb, B, compute_);
  phase_next("allreduce_conv+update");
  if (plan.c2r)
    launch_conv_grad_reduce_parts(cb, B, RED_W2_PARTS, RED_ALL_PARTS, compute_);
  else
    launch_conv_grad_reduce(cb, B, compute_);
  HIP_OK(hipStreamWaitEvent(compute_, ev_done_, 0));
  comm_->allreduce_sum(buf_.grad + OFF_CONV1_W, PARAM_TOTAL - OFF_CONV1_W, 0, compute_);
  launch_adadelta(a.adc, ADA_CONV, compute_);
  phase_end();
  if (a.last && sw_.rccl_handoff) end_chunk();   // the comm stream joins (fc update done)
}

// OVERLAP / XGMI: device-counter hand-offs between the compute and comm streams
void Engine::tail_chain(StepArgs& a) {
  const int B = a.B, Bp = a.Bp;
  const StepPlan& plan = a.plan;
  const bool M = pass_.main, S = pass_.side, xg = sched_ == XGMI, chain = plan.chain;
  AdadeltaArgs &ad = a.ad, &adc = a.adc;
  ConvBwdArgs& cb = a.cb;
  int* const err = ctr(HANDOFF_ERR);
  if (xg) ad.grad = adc.grad = xgmi_->out();    // the update reads the all-reduced gradients
  phase_begin("bwd_conv_wgrad");                // wgrad's start: fc grads of this step are final
  if (M) launch_conv_wgrad(with_signal(cb, ctr(WGRAD_STARTS)), B, compute_);
  // OVERLAP chain (plan.chain): the comm chain's hand-offs ride on its update kernels - the fc update
  // holds its completion until dgrad has started, conv2's reduce + update signals "fc update done"
  // (FC_UPDATES) at its start, and its own "conv2 update done" (CONV2_UPDATES) is signalled by the
  // next step's first comm launch, which then waits for that step's wgrad: one small launch per step
  // instead of two waits and two signals
  // XGMI (fused kernels) runs the same chain: the fc all-reduce + update holds its completion, the
  // conv2 reduce + all-reduce + update signals FC_UPDATES at its start (world-1 timeline: two hand-off
  // launches a step fewer, conv2's part no longer queued behind them)
  phase_next("allreduce_fc+update");
  if (S) {
    int* const rel = ctr(plan.release);         // fc_bwd's start / wgrad's start
    if (chain && cur_.sig3_pending)
      launch_stream_signal_wait(ctr(CONV2_UPDATES), rel, ctr(FC_UPDATES), 1, err, comm_stream_);
    else
      launch_stream_wait(rel, ctr(FC_UPDATES), 1, err, comm_stream_);
    cur_.sig3_pending = false;
    FcBwdArgs fw = a.fb;
    fw.signal_ctr = nullptr;
    if (plan.fcw_side && xg) launch_fc_bwd(fw, B, Bp, comm_stream_, true, FCB_ROLE_C | FCB_ROLE_A);
    if (plan.dw1_side) launch_fc_bwd_dw1(a.fb, B, Bp, comm_stream_);
    if (plan.fc_reduce_side) launch_fc_grad_reduce(a.fb, B, comm_stream_);
    // chain: the fc update completes once this step's dgrad has started
    const AdadeltaArgs af = chain ? held(ad, DGRAD_STARTS, CONV2_UPDATES, 1) : ad;
    if (plan.xgmi_separate) {
      xgmi_->allreduce(XGMI_CH_FC, OFF_FC1_W, OFF_CONV1_W - OFF_FC1_W, comm_stream_);
      launch_adadelta(ad, ADA_FC, comm_stream_);
    } else if (xg) {                            // fc bucket all-reduce with the fc Adadelta step fused
      xgmi_->allreduce_fc_fused(XGMI_CH_FC, comm_stream_, af);
    } else if (plan.fcw_side) {                 // the update is fused into the side weight gradients'
      launch_fc_wgrad_update(fw, af, B, Bp, comm_stream_);   // 146 workgroups (one launch)
    } else {
      // 144 workgroups instead of 577: the update has ~15 us of slack before the next step's trunk
      // ends, and fewer co-resident waves leave wgrad / dgrad more of the CUs (600 steps, two boxes:
      // 65.9 -> 65.2, 65.0-65.7 -> 64.4-64.9 us/step; 96 / 64 workgroups: 67.6 / 74-75)
      launch_adadelta(af, ADA_FC, comm_stream_, ADA_FC_LEAN_GRID);
    }
    if (!chain) launch_stream_signal(ctr(FC_UPDATES), comm_stream_);   // fc update of this step done
  }
  phase_end();
  cur_.side_pending = true;
  if (plan.xgmi_separate) {
    // separate launches (reference for the fused kernels' bits): the conv bucket after dgrad
    phase_begin("bwd_conv_dgrad");
    if (M) launch_conv_dgrad(cb, B, compute_);
    phase_next("allreduce_conv+update");
    if (M) {
      launch_conv_grad_reduce(cb, B, compute_);
      xgmi_->allreduce(XGMI_CH_CONV, OFF_CONV1_W, PARAM_TOTAL - OFF_CONV1_W, compute_);
      launch_adadelta(adc, ADA_CONV, compute_);
    }
    phase_end();
    if (a.last) end_chunk();
    return;
  }
  // conv2's slab reduce (+ exchange) + update on the comm stream after the fc update, released by
  // dgrad's start (= wgrad done, DGRAD_STARTS) and running under conv2_dgrad, which reads this step's
  // w2d while the update writes the other copy (ping-pong, host-tracked and static within a
  // captured chunk; a chunk that ends on the alternate copy copies it back); CONV2_UPDATES = conv2
  // updates published.  Only conv1's part (20 reduce workgroups) stays on the compute stream, and
  // that launch holds its completion until CONV2_UPDATES catches up, so the next trunk_fwd reads the
  // new conv2 weights.
  AdadeltaArgs u2 = adc;
  u2.state_inc = nullptr;
  u2.w2d = cur_.w2d_in_alt ? buf_.w2d : w2d_alt_;
  cb.w2d = cur_.w2d_in_alt ? w2d_alt_ : buf_.w2d;
  if (S) {
    if (!chain) launch_stream_wait(ctr(DGRAD_STARTS), ctr(CONV2_UPDATES), 1, err, comm_stream_);
    if (chain) u2.signal_start = ctr(FC_UPDATES);   // the fc update (previous launch) is done
    if (xg)
      xgmi_->conv_reduce_fused(XGMI_CH_CONV2, cb, B, comm_stream_, u2, XgmiConvPart{0, RED_W2_PARTS});
    else
      launch_adadelta_reduce_parts(u2, cb, B, 0, RED_W2_PARTS, comm_stream_);
    if (chain && !a.last)
      cur_.sig3_pending = true;                 // signalled by the next step's first comm launch
    else
      launch_stream_signal(ctr(CONV2_UPDATES), comm_stream_);
  }
  phase_begin("bwd_conv_dgrad");
  if (M) launch_conv_dgrad(with_signal(cb, ctr(DGRAD_STARTS)), B, compute_);
  phase_next("allreduce_conv1+update");
  if (M && xg) {
    const XgmiConvPart p1{RED_W2_PARTS, RED_ALL_PARTS, ctr(CONV2_UPDATES), ctr(DGRAD_STARTS), err};
    xgmi_->conv_reduce_fused(XGMI_CH_CONV, cb, B, compute_, adc, p1);
  } else if (M) {
    const AdadeltaArgs u1 = held(adc, CONV2_UPDATES, DGRAD_STARTS, 0);
    if (c1_lanes_)
      launch_adadelta_c1(u1, cb, B, compute_);
    else
      launch_adadelta_reduce_parts(u1, cb, B, RED_W2_PARTS, RED_ALL_PARTS, compute_);
  }
  phase_end();
  cur_.w2d_in_alt = !cur_.w2d_in_alt;
  if (!a.last) return;
  // chunk end: a shadow in its alternate copy goes home (after the conv1 part: the fc update is published)
  const size_t w1t_bytes = (size_t)NFLAT * NH * sizeof(uint16_t), w2d_bytes = (size_t)9 * C1 * C2 * sizeof(uint16_t);
  if (M && cur_.w1t_in_alt) HIP_OK(hipMemcpyAsync(buf_.w1t, w1t_alt_, w1t_bytes, hipMemcpyDeviceToDevice, compute_));
  if (M && cur_.w2d_in_alt) HIP_OK(hipMemcpyAsync(buf_.w2d, w2d_alt_, w2d_bytes, hipMemcpyDeviceToDevice, compute_));
  cur_.w1t_in_alt = cur_.w2d_in_alt = false;
  end_chunk();
}

// fp32 step: forward, every gradient, (RCCL: one all-reduce of the whole flat gradient on the
// compute stream), the whole Adadelta update (which advances the device step counter) - SERIAL / RCCL.
// Chained (plan.f32_chained) - OVERLAP (single GPU): the fc update (98 % of the parameters) runs on the
// comm stream beside the conv backward once the fc gradients are final; the next step's first kernel
// waits for it.  The conv2 weight gradient (reads dy2 + a1) runs there too, beside the conv2 input
// gradient + conv1 weight gradient.  The counters mean, in this step: WGRAD_STARTS = fc gradients
// final, DGRAD_STARTS = fc1 input gradients (dy2) done, CONV2_UPDATES = conv2 weight gradients done.
//   C: (wait FC_UPDATES >= WGRAD_STARTS) forward, fc2 / fc1-bias grads, +WGRAD_STARTS, fc1 input grad,
//      +DGRAD_STARTS, conv2 input grad + conv1 weight grad, wait CONV2_UPDATES >= DGRAD_STARTS,
//      conv reduce, conv update (+step)
//   M: wait WGRAD_STARTS >= FC_UPDATES+1, fc1 weight grad, fc update, +FC_UPDATES,
//      wait DGRAD_STARTS >= CONV2_UPDATES+1, conv2 weight grad, +CONV2_UPDATES
// XGMI (world > 1) runs the same two chains with each update replaced by its bucket's all-reduce with
// the Adadelta step fused: the fc bucket (two-shot) on the comm stream beside the conv backward, the
// conv bucket (one-shot) at the step tail (different channels, so the two never share flags).
// RCCL with hand-offs: the same chains in one graph, the fc bucket's all-reduce ahead of the fc
// update on the comm stream, the conv bucket's after compute's wait for CONV2_UPDATES (which follows
// the fc all-reduce on the comm stream: the communicator never has two collectives in flight, fc first)
void Engine::enqueue_step_f32(int batch, bool last, const StepPlan& plan) {
  F32Step a = f32_args(train_input(), buf_.state, ddp_head_inv_batch(batch, world_));
  AdadeltaArgs ad = adadelta_args();
  if (!plan.f32_chained) {
    phase_begin("fwd");
    launch_f32_forward(a, batch, true, compute_);
    phase_next("bwd");
    launch_f32_backward(a, batch, compute_);
    phase_next("allreduce+update");
    ad.state_inc = buf_.state;
    if (sched_ == RCCL) comm_->allreduce_sum(buf_.grad, PARAM_TOTAL, 0, compute_);
    launch_adadelta(ad, ADA_ALL, compute_);
    phase_end();
    return;
  }
  const bool xg = sched_ == XGMI, rc = sched_ == RCCL, M = pass_.main, S = pass_.side;
  int* const err = ctr(HANDOFF_ERR);
  fork_comm_once();
  if (M) {
    if (cur_.side_pending) launch_stream_wait(ctr(FC_UPDATES), ctr(WGRAD_STARTS), 0, err, compute_);
    launch_f32_forward(a, batch, true, compute_);
    launch_f32_fc_small(a, batch, compute_);
    launch_stream_signal(ctr(WGRAD_STARTS), compute_);
    launch_f32_fc1x(a, batch, compute_);
    launch_stream_signal(ctr(DGRAD_STARTS), compute_);
    launch_f32_conv2x_conv1w(a, batch, compute_);
    launch_stream_wait(ctr(CONV2_UPDATES), ctr(DGRAD_STARTS), 0, err, compute_);
    launch_f32_conv_reduce(a, batch, compute_);
  }
  // one bucket's all-reduce + update (XGMI: one launch)
  auto bucket = [&](int ch, int lo, int hi, int region, hipStream_t s, AdadeltaArgs u) {
    if (xg) {
      u.grad = xgmi_->out();
      return xgmi_->allreduce(ch, lo, hi - lo, s, &u);
    }
    if (rc) comm_->allreduce_sum(buf_.grad + lo, hi - lo, 0, s);
    launch_adadelta(u, region, s);
  };
  // the conv bucket's tail (compute stream).  RCCL runs one communicator's collectives in ISSUE order,
  // even across streams, so with RCCL the conv all-reduce is enqueued after the comm chain's fc
  // all-reduce: compute reaches it only after CONV2_UPDATES >= DGRAD_STARTS, which the comm chain
  // signals after the fc all-reduce - issued the other way round, the fc all-reduce would queue behind
  // a conv all-reduce that waits for it (a cycle broken only by the 60 s hand-off timeout)
  AdadeltaArgs adc = ad;
  adc.state_inc = buf_.state;
  if (M && !rc) bucket(XGMI_CH_CONV, OFF_CONV1_W, PARAM_TOTAL, ADA_CONV, compute_, adc);
  if (S) {
    launch_stream_wait(ctr(WGRAD_STARTS), ctr(FC_UPDATES), 1, err, comm_stream_);
    launch_f32_fc1w(a, batch, comm_stream_);
    bucket(XGMI_CH_FC, OFF_FC1_W, OFF_CONV1_W, ADA_FC, comm_stream_, ad);
    launch_stream_signal(ctr(FC_UPDATES), comm_stream_);
    launch_stream_wait(ctr(DGRAD_STARTS), ctr(CONV2_UPDATES), 1, err, comm_stream_);
    launch_f32_conv2w(a, batch, comm_stream_);
    launch_stream_signal(ctr(CONV2_UPDATES), comm_stream_);
  }
  if (M && rc) bucket(XGMI_CH_CONV, OFF_CONV1_W, PARAM_TOTAL, ADA_CONV, compute_, adc);
  cur_.side_pending = true;
  if (last) end_chunk();
}

void Engine::train_steps(int n, int batch, int stride) {
  check_batch(batch, max_batch_, "batch");
  idx_stride_ = stride;
  for (int i = 0; i < n; ++i) enqueue_step(batch, i == n - 1);
  HIP_OK(hipGetLastError());
}

// Captures what `enqueue` issues on stream s; a throw ends the capture and resets the host state.
template <class F>
hipGraph_t Engine::capture_on(hipStream_t s, F&& enqueue) {
  hipGraph_t g = nullptr;
  HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
  try {
    enqueue();
  } catch (...) {
    reset_host_state();
    (void)hipStreamEndCapture(s, &g);
    if (g) (void)hipGraphDestroy(g);
    throw;
  }
  HIP_OK(hipStreamEndCapture(s, &g));
  return g;
}

// Instantiates a captured chunk (split capture: its side chain too) and files it under a new graph id.
int Engine::add_graphs(hipGraph_t side, hipGraph_t main) {
  // (no hipGraphUpload: on this ROCm 7 runtime it segfaults right after instantiate - measured on
  // the box; first-replay costs are taken by an untimed warm replay instead, FusedTrainer.warm_graphs)
  for (hipGraph_t g : {side, main})
    if (g) graph_defs_.push_back(g);
  hipGraphExec_t xs = nullptr, xm = nullptr;
  if (side) HIP_OK(hipGraphInstantiate(&xs, side, nullptr, nullptr, 0));
  HIP_OK(hipGraphInstantiate(&xm, main, nullptr, nullptr, 0));
  graphs_.push_back(xm);
  side_graphs_.push_back(xs);
  graph_main_defs_.push_back(main);
  return (int)graphs_.size() - 1;
}

int Engine::graph_nodes(int id) const {
  if (id < 0 || id >= (int)graph_main_defs_.size()) throw std::runtime_error("engine: unknown graph id");
  size_t n = 0;
  HIP_OK(hipGraphGetNodes(graph_main_defs_[id], nullptr, &n));
  return (int)n;
}

int Engine::capture_train(int n, int batch, int stride) {
  check_batch(batch, max_batch_, "batch");
  idx_stride_ = stride;
  if (side_schedule()) return capture_train_split(n, batch);
  // SERIAL / RCCL: one graph, steps in order (RCCL: the communicator's collectives are captured in
  // the order every rank issues them - fc, conv, fc, ... - so RCCL's own ordering of one
  // communicator's kernels across streams can never chain a collective behind a later step's)
  return add_graphs(nullptr, capture_on(compute_, [&] {
    for (int i = 0; i < n; ++i) enqueue_step(batch, i == n - 1);
  }));
}

// OVERLAP / XGMI chunks as TWO graphs: the side chain (comm stream: per step counter waits, the fc
// update or all-reduce, the conv2 part, counter signals) and the compute chain, captured in two
// passes over the same steps (both start from the same chunk cursor - the shadow ping-pongs, the
// pending hand-off - and must end in the same one) and launched concurrently from two host threads
// (replay()).  One multi-stream graph submitted its side branch only after the whole compute branch
// (~3.6 us of host time per node), so after every host sync the second step's trunk_fwd sat ~0.45 ms
// (20-step chunk) on the device counter the side chain had not yet reached the queue to signal: the
// driver's 20-step bench window read 93-97 us/step against 73.5 steady state.  The fork (chunk start
// -> comm stream) and the join (comm stream -> compute) become two events at replay.
int Engine::capture_train_split(int n, int batch) {
  ChunkCursor start = cur_, end[2];
  start.side_forked = true;                    // forks / joins are events at replay, not captured edges
  const EnqueuePass passes[2] = {{false, true, true}, {true, false, true}};   // comm chain, compute chain
  hipGraph_t g[2] = {nullptr, nullptr};
  try {
    for (int k = 0; k < 2; ++k) {
      cur_ = start;
      pass_ = passes[k];
      g[k] = capture_on(k ? compute_ : comm_stream_, [&] {
        for (int i = 0; i < n; ++i) enqueue_step(batch, i == n - 1);
      });
      end[k] = cur_;
    }
    pass_ = {};
    if (!(end[0] == end[1])) throw std::runtime_error("engine: the two capture passes ended in different states");
  } catch (...) {
    reset_host_state();
    for (hipGraph_t x : g)
      if (x) (void)hipGraphDestroy(x);
    throw;
  }
  return add_graphs(g[0], g[1]);
}

// --- side-graph launcher thread: hipGraphLaunch(side, comm stream) + the join event, concurrently
// with the compute graph's launch on the calling thread (measured 20-step window, single GPU: 75.8
// vs 78.9 us/step launching both from the calling thread)
void Engine::side_worker(int k) {
  SideLauncher& l = side_[k];
  std::unique_lock<std::mutex> lk(l.mu);
  for (;;) {
    l.cv.wait(lk, [&l] { return l.stop || l.job != nullptr; });
    if (l.stop) return;
    hipGraphExec_t job = l.job;
    hipStream_t s = l.stream;
    lk.unlock();
    hipError_t e = hipGraphLaunch(job, s);
    if (e == hipSuccess) e = hipEventRecord(l.join, s);
    lk.lock();
    l.err = e;
    l.job = nullptr;
    l.done = true;
    l.cv.notify_all();
  }
}

void Engine::side_start(int k, hipGraphExec_t g, hipStream_t s) {
  SideLauncher& l = side_[k];
  {
    std::lock_guard<std::mutex> lk(l.mu);
    if (!l.thread.joinable()) l.thread = std::thread(&Engine::side_worker, this, k);
    l.job = g;
    l.stream = s;
    l.done = false;
  }
  l.cv.notify_all();
}

hipError_t Engine::side_wait(int k) {
  SideLauncher& l = side_[k];
  std::unique_lock<std::mutex> lk(l.mu);
  l.cv.wait(lk, [&l] { return l.done; });
  return l.err;
}

void Engine::gather_rows(int64_t start, int64_t n) {
  if (!buf_.epoch_u8 || !buf_.epoch_labels) throw std::runtime_error("gather_rows: no epoch buffers");
  launch_gather_rows(buf_.train_u8, buf_.train_labels, buf_.train_idx, start, n, buf_.epoch_u8, buf_.epoch_labels,
                     compute_);
  HIP_OK(hipGetLastError());
}

void Engine::replay(int id) {
  if (id < 0 || id >= (int)graphs_.size()) throw std::runtime_error("bad graph id");
  hipGraphExec_t side = side_graphs_[id];
  if (!side) {
    HIP_OK(hipGraphLaunch(graphs_[id], compute_));
    return;
  }
  HIP_OK(hipEventRecord(ev_fork_, compute_));          // side chain ordered after earlier compute work
  HIP_OK(hipStreamWaitEvent(comm_stream_, ev_fork_, 0));
  side_start(0, side, comm_stream_);
  const hipError_t em = hipGraphLaunch(graphs_[id], compute_);
  const hipError_t es = side_wait(0);
  HIP_OK(em);
  HIP_OK(es);
  HIP_OK(hipStreamWaitEvent(compute_, side_[0].join, 0));   // chunk end: compute joins the side chain
}

void Engine::enqueue_eval(int n_total, int batch) {
  const float* P = buf_.param;
  for (int s = 0; s < n_total; s += batch) {
    const int B = (n_total - s) < batch ? (n_total - s) : batch;
    if (f32_) {
      F32Step a = f32_args({buf_.test_u8, buf_.test_idx + s, 0, buf_.test_labels}, nullptr, 0.0f);
      a.loss_rows = buf_.test_loss_rows + s;
      a.correct = buf_.test_correct + s;
      launch_f32_forward(a, B, false, compute_);
      continue;
    }
    TrunkFwdArgs tf{buf_.test_u8, buf_.test_idx + s, 0, nullptr, P + OFF_CONV1_W, P + OFF_CONV1_B,
                    buf_.w2f, P + OFF_CONV2_B, nullptr, p_, nullptr, nullptr};
    launch_trunk_fwd(tf, B, false, compute_);
    launch_fc1_fwd(p_, buf_.w1, z1part_, B, compute_);
    HeadArgs ha{};
    ha.z1part = z1part_; ha.b_fc1 = P + OFF_FC1_B; ha.w_fc2 = P + OFF_FC2_W; ha.b_fc2 = P + OFF_FC2_B;
    ha.labels = buf_.test_labels; ha.idx = buf_.test_idx + s; ha.idx_step_stride = 0;
    ha.loss_rows = buf_.test_loss_rows + s; ha.correct_out = buf_.test_correct + s;
    launch_head_eval(ha, B, compute_);
  }
}

void Engine::eval(int n_total, int batch) {
  check_batch(batch, max_test_batch_, "test batch");
  enqueue_eval(n_total, batch);
  HIP_OK(hipGetLastError());
}

int Engine::capture_eval(int n_total, int batch) {
  check_batch(batch, max_test_batch_, "test batch");
  return add_graphs(nullptr, capture_on(compute_, [&] { enqueue_eval(n_total, batch); }));
}

void Engine::refresh_shadows() {
  launch_refresh_shadows(adadelta_args(), compute_);
  HIP_OK(hipGetLastError());
}

void Engine::broadcast_params(int root) {
  if (!comm_) throw std::runtime_error("no communicator attached");
  comm_->broadcast(buf_.param, PARAM_TOTAL, 0, root, compute_);
  refresh_shadows();
}

bool Engine::probe_stream_pair(hipStream_t x, hipStream_t y, double timeout_s) {
  int *const a = ctr(PROBE_SCRATCH), *const b = a + 1, *const zero = a + 2, *const perr = a + 3;
  launch_fill(a, 4 * sizeof(int), 0, x);
  HIP_OK(hipStreamSynchronize(x));
  launch_stream_wait(a, zero, 1, perr, x, timeout_s);   // x waits ...
  launch_stream_signal(a, y);                            // ... for y
  launch_stream_wait(b, zero, 1, perr, y, timeout_s);   // y waits ...
  launch_stream_signal(b, x);                            // ... for x
  HIP_OK(hipStreamSynchronize(x));
  HIP_OK(hipStreamSynchronize(y));
  int err = 0;
  HIP_OK(hipMemcpy(&err, perr, sizeof(int), hipMemcpyDeviceToHost));
  return err == 0;
}

bool Engine::probe_stream_handoff(double timeout_s) { return probe_stream_pair(compute_, comm_stream_, timeout_s); }

// fault injection (tests): the compute stream spins until fault_release (FAULT_HOLD block: released,
// zero, the hold's own timeout flag - never the engine's error flag HANDOFF_ERR)
void Engine::fault_hold(double timeout_s) {
  int* const h = ctr(FAULT_HOLD);
  launch_fill(h, 4 * sizeof(int), 0, compute_);
  launch_stream_wait(h, h + 1, 1, h + 2, compute_, timeout_s);
  HIP_OK(hipGetLastError());
}

void Engine::fault_release(hipStream_t s) {
  launch_stream_signal(ctr(FAULT_HOLD), s);
  HIP_OK(hipGetLastError());
}

std::pair<int, int> Engine::errors() const {
  int err = 0;
  HIP_OK(hipMemcpy(&err, ctr(HANDOFF_ERR), sizeof(int), hipMemcpyDeviceToHost));
  return {err, xgmi_ ? xgmi_->error() : 0};
}

std::string Engine::describe_xgmi_error(int code) {
  static const char* names[] = {"?", "two-shot all-reduce", "one-shot all-reduce", "fused fc all-reduce+Adadelta",
                                "fused conv reduce+all-reduce+Adadelta"};
  const int kid = (code >> 24) & 0xff;
  return std::string(names[kid >= 1 && kid <= 4 ? kid : 0]) + " kernel, stage " + std::to_string((code >> 16) & 0xf) +
         ", waiting for peer rank " + std::to_string((code >> 12) & 0xf) + ", workgroup " + std::to_string(code & 0xfff);
}

void Engine::check_errors() const {
  const auto e = errors();
  if (e.first) throw std::runtime_error("engine: a stream hand-off timed out (results invalid)");
  if (e.second)
    throw std::runtime_error("engine: an xGMI all-reduce stage timed out (results invalid): " +
                             describe_xgmi_error(e.second));
}

void Engine::sync_streams() {
  HIP_OK(hipStreamSynchronize(compute_));
  HIP_OK(hipStreamSynchronize(comm_stream_));
}

void Engine::synchronize() {
  sync_streams();
  check_errors();
}

}  // namespace mnist
