// Python bindings (pybind11) for the native MI355X runtime.  Tensors cross the boundary as raw
// device pointers (tensor.data_ptr()) and HIP streams as integer handles
// (torch.cuda.Stream.cuda_stream): the runtime never includes libtorch headers, so it is immune
// to torch C++ ABI details and compiles in seconds.
#include <pybind11/pybind11.h>
#include <chrono>
#include <vector>
#include <pybind11/stl.h>

#include <stdexcept>

#include "include/kernels.h"
#include "runtime/bucket_reducer.h"
#include "runtime/engine.h"
#include "runtime/rccl_comm.h"

namespace py = pybind11;

#ifdef MNIST_TIMELINE
namespace mnist {
void tl_dump_trunk(std::vector<uint64_t>&);
void tl_dump_fc_head(std::vector<uint64_t>&);
void tl_dump_conv_bwd(std::vector<uint64_t>&);
void tl_dump_adadelta(std::vector<uint64_t>&);
void tl_dump_comm(std::vector<uint64_t>&);
void tl_dump_xgmi(std::vector<uint64_t>&);
}  // namespace mnist
#endif
using namespace mnist;

void mnist::preload_all_kernels() {
  preload_trunk();
  preload_fc_head();
  preload_conv_bwd();
  preload_adadelta();
  preload_comm();
  preload_xgmi();
  preload_f32();
  preload_input_grad();
  preload_input_grad_step();
  preload_attack_step();
  preload_adv_train();
  preload_smooth();
  preload_attr();
  preload_deepfool();
  preload_apgd();
  preload_square();
}

namespace {
template <typename T>
T* P(uintptr_t x) { return reinterpret_cast<T*>(x); }
hipStream_t S(uintptr_t x) { return reinterpret_cast<hipStream_t>(x); }

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("kernel launch failed: ") + hipGetErrorString(e));
}

// ---- minimal DLPack (v0.8 ABI) export of a device fp32 vector; the capsule keeps `owner` alive
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
};
struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(DLManagedTensor*);
};
constexpr int32_t kDLROCM = 10;
constexpr uint8_t kDLFloat = 2;

struct DLCtx {
  std::shared_ptr<void> owner;
  int64_t shape[1];
  DLManagedTensor mt;
};

void dl_deleter(DLManagedTensor* mt) { delete static_cast<DLCtx*>(mt->manager_ctx); }

py::capsule dlpack_f32(float* data, int64_t n, int device, std::shared_ptr<void> owner) {
  auto* ctx = new DLCtx{std::move(owner), {n}, {}};
  ctx->mt.dl_tensor = DLTensor{data, DLDevice{kDLROCM, device}, 1, DLDataType{kDLFloat, 32, 1}, ctx->shape, nullptr, 0};
  ctx->mt.manager_ctx = ctx;
  ctx->mt.deleter = dl_deleter;
  return py::capsule(&ctx->mt, "dltensor", [](PyObject* cap) {
    // an unconsumed capsule still owns the tensor (a consumer renames it to "used_dltensor")
    if (PyCapsule_IsValid(cap, "dltensor")) {
      auto* mt = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor"));
      if (mt && mt->deleter) mt->deleter(mt);
    }
  });
}

// the device pointer under key k, null where the key is absent
uintptr_t dict_ptr(const py::dict& d, const char* k) { return d.contains(k) ? d[k].cast<uintptr_t>() : 0; }

EngineBuffers buffers_from_dict(const py::dict& d) {
  EngineBuffers b;
  b.param = P<float>(dict_ptr(d, "param"));
  b.grad = P<float>(dict_ptr(d, "grad"));
  b.square_avg = P<float>(dict_ptr(d, "square_avg"));
  b.acc_delta = P<float>(dict_ptr(d, "acc_delta"));
  b.lr = P<float>(dict_ptr(d, "lr"));
  b.w2f = P<uint16_t>(dict_ptr(d, "w2f"));
  b.w2d = P<uint16_t>(dict_ptr(d, "w2d"));
  b.w1 = P<uint16_t>(dict_ptr(d, "w1"));
  b.w1t = P<uint16_t>(dict_ptr(d, "w1t"));
  b.state = P<StepState>(dict_ptr(d, "state"));
  b.loss_log = P<float>(dict_ptr(d, "loss_log"));
  b.train_u8 = P<const uint8_t>(dict_ptr(d, "train_u8"));
  b.train_labels = P<const int32_t>(dict_ptr(d, "train_labels"));
  b.train_idx = P<const int32_t>(dict_ptr(d, "train_idx"));
  b.epoch_u8 = P<uint8_t>(dict_ptr(d, "epoch_u8"));
  b.epoch_labels = P<int32_t>(dict_ptr(d, "epoch_labels"));
  b.test_u8 = P<const uint8_t>(dict_ptr(d, "test_u8"));
  b.test_labels = P<const int32_t>(dict_ptr(d, "test_labels"));
  b.test_idx = P<const int32_t>(dict_ptr(d, "test_idx"));
  b.test_loss_rows = P<float>(dict_ptr(d, "test_loss_rows"));
  b.test_correct = P<int32_t>(dict_ptr(d, "test_correct"));
  if (!b.param || !b.grad || !b.square_avg || !b.acc_delta || !b.lr || !b.w2f || !b.w2d || !b.w1 ||
      !b.w1t || !b.state)
    throw std::runtime_error("engine buffers: missing model/optimizer pointer");
  return b;
}

// AdadeltaArgs of a stand-alone launch from ModelState.buffers() + the optimizer scalars.  The hold
// pointers and signal_start stay null: the completion holds wait on another stream's counters and
// belong to the engine.
AdadeltaArgs ada_from_dict(const py::dict& d) {
  AdadeltaArgs a{};
  a.param = P<float>(dict_ptr(d, "param"));
  a.grad = P<const float>(dict_ptr(d, "grad"));
  a.square_avg = P<float>(dict_ptr(d, "square_avg"));
  a.acc_delta = P<float>(dict_ptr(d, "acc_delta"));
  a.lr = P<const float>(dict_ptr(d, "lr"));
  a.rho = d["rho"].cast<float>();
  a.eps = d["eps"].cast<float>();
  a.weight_decay = d["weight_decay"].cast<float>();
  a.w2f = P<uint16_t>(dict_ptr(d, "w2f"));
  a.w2d = P<uint16_t>(dict_ptr(d, "w2d"));
  a.w1 = P<uint16_t>(dict_ptr(d, "w1"));
  a.w1t = P<uint16_t>(dict_ptr(d, "w1t"));
  a.state_inc = P<StepState>(dict_ptr(d, "state_inc"));
  a.wt = d.contains("wt") && d["wt"].cast<bool>() ? 1 : 0;
  if (!a.param || !a.grad || !a.square_avg || !a.acc_delta || !a.lr || !a.w2f || !a.w2d || !a.w1 || !a.w1t)
    throw std::runtime_error("adadelta arguments: missing model/optimizer pointer");
  return a;
}

// ConvBwdArgs of a stand-alone conv backward launch (the conv_bwd binding and XgmiComm.conv_reduce_fused)
ConvBwdArgs conv_args(uintptr_t dyc, uintptr_t a1, uintptr_t w2d, uintptr_t w1c, uintptr_t b1c, uintptr_t data_u8,
                      uintptr_t idx, int64_t idx_stride, uintptr_t state, uintptr_t c1part, uintptr_t w2part,
                      uintptr_t grad, float grad_scale, int B, uintptr_t xin, uintptr_t c1red) {
  ConvBwdArgs a{P<const uint8_t>(dyc), P<const uint16_t>(a1), P<const uint16_t>(w2d),
                P<const float>(w1c), P<const float>(b1c), P<const uint8_t>(data_u8), P<const int32_t>(idx),
                idx_stride, P<const StepState>(state), P<float>(c1part), P<float>(w2part), P<float>(grad),
                grad_scale, conv_wgrad_groups(B), P<const float>(xin)};
  a.c1_rows = conv_dgrad_c1_rows(B);
  a.c1red = P<float>(c1red);
  return a;
}

// F32Step of a stand-alone fp32 launch from caller-owned device pointers (null where a key is absent)
F32Step f32_from_dict(const py::dict& d, int64_t idx_step_stride, float inv_batch) {
  F32Step a{};
  a.data_u8 = P<const uint8_t>(dict_ptr(d, "data_u8"));
  a.idx = P<const int32_t>(dict_ptr(d, "idx"));
  a.idx_step_stride = idx_step_stride;
  a.labels = P<const int32_t>(dict_ptr(d, "labels"));
  a.state = P<const StepState>(dict_ptr(d, "state"));
  a.param = P<const float>(dict_ptr(d, "param"));
  a.grad = P<float>(dict_ptr(d, "grad"));
  a.loss_log = P<float>(dict_ptr(d, "loss_log"));
  a.inv_batch = inv_batch;
  a.w2fwd = P<float>(dict_ptr(d, "w2fwd"));
  a.w2bwd = P<float>(dict_ptr(d, "w2bwd"));
  a.w1p = P<float>(dict_ptr(d, "w1p"));
  a.a1 = P<float>(dict_ptr(d, "a1"));
  a.dx1 = P<float>(dict_ptr(d, "dx1"));
  a.y2 = P<float>(dict_ptr(d, "y2"));
  a.p = P<float>(dict_ptr(d, "p"));
  a.pm = P<uint8_t>(dict_ptr(d, "pm"));
  a.z1part = P<float>(dict_ptr(d, "z1part"));
  a.h = P<float>(dict_ptr(d, "h"));
  a.dz1 = P<float>(dict_ptr(d, "dz1"));
  a.dl = P<float>(dict_ptr(d, "dl"));
  a.loss_rows = P<float>(dict_ptr(d, "loss_rows"));
  a.correct = P<int32_t>(dict_ptr(d, "correct"));
  a.c2part = P<float>(dict_ptr(d, "c2part"));
  a.c1part = P<float>(dict_ptr(d, "c1part"));
  return a;
}
}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "MI355X (gfx950) native kernels + runtime for the MNIST DDP framework";

  m.attr("PARAM_TOTAL") = PARAM_TOTAL;
  m.attr("FC1_KSPLIT") = FC1_KSPLIT;
  m.attr("DYC_REC") = DYC_REC;
  py::dict offs;
  offs["fc1.weight"] = OFF_FC1_W; offs["fc1.bias"] = OFF_FC1_B;
  offs["fc2.weight"] = OFF_FC2_W; offs["fc2.bias"] = OFF_FC2_B;
  offs["conv1.weight"] = OFF_CONV1_W; offs["conv1.bias"] = OFF_CONV1_B;
  offs["conv2.weight"] = OFF_CONV2_W; offs["conv2.bias"] = OFF_CONV2_B;
  m.attr("PARAM_OFFSETS") = offs;
  m.attr("BUCKET_SPLIT") = OFF_CONV1_W;
  m.def("conv_wgrad_groups", &conv_wgrad_groups);
  m.def("set_dgrad_grid", &set_dgrad_grid, "persistent dgrad grid override (0 = 2 x CUs; tests)");
  m.def("set_wgrad_form", &set_wgrad_form, "wgrad form override (-1 = by batch, 0 lean, 1 staggered; tests)");
  m.attr("SCHED_SERIAL") = (int)Engine::SERIAL;
  m.attr("SCHED_OVERLAP") = (int)Engine::OVERLAP;
  m.attr("SCHED_RCCL") = (int)Engine::RCCL;
  m.attr("SCHED_XGMI") = (int)Engine::XGMI;

  // ---------------- per-kernel entry points ----------------
  m.def("trunk_fwd", [](uintptr_t data_u8, uintptr_t idx, int64_t idx_stride, uintptr_t state, uintptr_t w1c,
                        uintptr_t b1c, uintptr_t w2f, uintptr_t b2c, uintptr_t a1_out, uintptr_t p_out,
                        uintptr_t pmask_out, int B, bool train, uintptr_t stream, uintptr_t xin) {
    TrunkFwdArgs a{P<const uint8_t>(data_u8), P<const int32_t>(idx), idx_stride, P<const StepState>(state),
                   P<const float>(w1c), P<const float>(b1c), P<const uint16_t>(w2f), P<const float>(b2c),
                   P<uint16_t>(a1_out), P<uint16_t>(p_out), P<uint8_t>(pmask_out), P<const float>(xin)};
    launch_trunk_fwd(a, B, train, S(stream));
    check_launch();
  }, py::arg("data_u8"), py::arg("idx"), py::arg("idx_stride"), py::arg("state"), py::arg("w1c"), py::arg("b1c"),
     py::arg("w2f"), py::arg("b2c"), py::arg("a1_out"), py::arg("p_out"), py::arg("pmask_out"), py::arg("B"),
     py::arg("train"), py::arg("stream"), py::arg("xin") = 0);
  m.def("fc1_fwd", [](uintptr_t p, uintptr_t w1, uintptr_t z1part, int B, uintptr_t stream) {
    launch_fc1_fwd(P<const uint16_t>(p), P<const uint16_t>(w1), P<float>(z1part), B, S(stream));
    check_launch();
  });
  m.def("head_train", [](uintptr_t z1part, uintptr_t b_fc1, uintptr_t w_fc2, uintptr_t b_fc2, uintptr_t labels,
                         uintptr_t idx, int64_t idx_stride, uintptr_t state, float inv_batch, uintptr_t loss_rows,
                         uintptr_t dz1, uintptr_t h_bf, uintptr_t dl_bf, int B, int Bp, uintptr_t stream,
                         uintptr_t dlogp) {
    HeadArgs a{};
    a.z1part = P<const float>(z1part); a.b_fc1 = P<const float>(b_fc1); a.w_fc2 = P<const float>(w_fc2);
    a.b_fc2 = P<const float>(b_fc2); a.labels = P<const int32_t>(labels); a.idx = P<const int32_t>(idx);
    a.idx_step_stride = idx_stride; a.state = P<const StepState>(state); a.inv_batch = inv_batch;
    a.loss_rows = P<float>(loss_rows); a.dz1 = P<uint16_t>(dz1); a.h_bf = P<uint16_t>(h_bf);
    a.dl_bf = P<uint16_t>(dl_bf); a.dlogp = P<const float>(dlogp);
    launch_head_train(a, B, Bp, S(stream));
    check_launch();
  }, py::arg("z1part"), py::arg("b_fc1"), py::arg("w_fc2"), py::arg("b_fc2"), py::arg("labels"), py::arg("idx"),
     py::arg("idx_stride"), py::arg("state"), py::arg("inv_batch"), py::arg("loss_rows"), py::arg("dz1"),
     py::arg("h_bf"), py::arg("dl_bf"), py::arg("B"), py::arg("Bp"), py::arg("stream"), py::arg("dlogp") = 0);
  m.attr("MARGIN_CW") = (int)MARGIN_CW;
  m.attr("MARGIN_DLR") = (int)MARGIN_DLR;
  m.attr("MARGIN_DLR_T") = (int)MARGIN_DLR_T;
  m.def("head_margin", [](uintptr_t z1part, uintptr_t b_fc1, uintptr_t w_fc2, uintptr_t b_fc2, uintptr_t labels,
                          uintptr_t targets, int kind, float scale, uintptr_t loss_rows, uintptr_t dz1,
                          uintptr_t h_bf, uintptr_t dl_bf, int B, int Bp, uintptr_t stream) {
    HeadMarginArgs a{};
    a.z1part = P<const float>(z1part); a.b_fc1 = P<const float>(b_fc1); a.w_fc2 = P<const float>(w_fc2);
    a.b_fc2 = P<const float>(b_fc2); a.labels = P<const int32_t>(labels); a.targets = P<const int32_t>(targets);
    a.scale = scale; a.loss_rows = P<float>(loss_rows); a.dz1 = P<uint16_t>(dz1); a.h_bf = P<uint16_t>(h_bf);
    a.dl_bf = P<uint16_t>(dl_bf);
    launch_head_margin(a, B, Bp, kind, S(stream));
    check_launch();
  }, py::arg("z1part"), py::arg("b_fc1"), py::arg("w_fc2"), py::arg("b_fc2"), py::arg("labels"), py::arg("targets"),
     py::arg("kind"), py::arg("scale"), py::arg("loss_rows"), py::arg("dz1"), py::arg("h_bf"), py::arg("dl_bf"),
     py::arg("B"), py::arg("Bp"), py::arg("stream"));
  m.def("head_fwd", [](uintptr_t z1part, uintptr_t b_fc1, uintptr_t w_fc2, uintptr_t b_fc2, uintptr_t state,
                       uintptr_t logp, int B, bool train, uintptr_t stream) {
    HeadArgs a{};
    a.z1part = P<const float>(z1part); a.b_fc1 = P<const float>(b_fc1); a.w_fc2 = P<const float>(w_fc2);
    a.b_fc2 = P<const float>(b_fc2); a.state = P<const StepState>(state); a.logp_out = P<float>(logp);
    launch_head_fwd(a, B, train, S(stream));
    check_launch();
  });
  m.def("head_eval", [](uintptr_t z1part, uintptr_t b_fc1, uintptr_t w_fc2, uintptr_t b_fc2, uintptr_t labels,
                        uintptr_t idx, uintptr_t loss_rows, uintptr_t correct, uintptr_t logp, int B,
                        uintptr_t stream) {
    HeadArgs a{};
    a.z1part = P<const float>(z1part); a.b_fc1 = P<const float>(b_fc1); a.w_fc2 = P<const float>(w_fc2);
    a.b_fc2 = P<const float>(b_fc2); a.labels = P<const int32_t>(labels); a.idx = P<const int32_t>(idx);
    a.loss_rows = P<float>(loss_rows); a.correct_out = P<int32_t>(correct); a.logp_out = P<float>(logp);
    launch_head_eval(a, B, S(stream));
    check_launch();
  });
  m.def("fc_bwd", [](uintptr_t dz1, uintptr_t p, uintptr_t pmask, uintptr_t w1t, uintptr_t h_bf, uintptr_t dl_bf,
                     uintptr_t loss_rows, uintptr_t state, uintptr_t grad, uintptr_t dyc, uintptr_t loss_log,
                     float grad_scale, float inv_batch, int B, int Bp, uintptr_t stream, int role,
                     uintptr_t part, py::object ada) {
    FcBwdArgs a{P<const uint16_t>(dz1), P<const uint16_t>(p), P<const uint8_t>(pmask), P<const uint16_t>(w1t),
                P<const uint16_t>(h_bf), P<const uint16_t>(dl_bf), P<const float>(loss_rows),
                P<const StepState>(state), P<float>(grad), P<uint8_t>(dyc), P<float>(loss_log), grad_scale,
                inv_batch, P<float>(part)};
    if (!ada.is_none()) {                        // roles C + A with the fc Adadelta step in the epilogue
      if (role >= 0) throw std::runtime_error("fc_bwd: the fused update takes no role");
      launch_fc_wgrad_update(a, ada_from_dict(ada.cast<py::dict>()), B, Bp, S(stream));
    } else if (role < 0) launch_fc_bwd(a, B, Bp, S(stream));
    else if (role == 3) launch_fc_bwd_dw1(a, B, Bp, S(stream));                  // role A alone, lean kernel
    else if (role == 4) launch_fc_bwd(a, B, Bp, S(stream), false, FCB_ROLE_C | FCB_ROLE_B);   // B > 1024
    else if (role == 5) launch_fc_bwd(a, B, Bp, S(stream), false, FCB_ROLE_C | FCB_ROLE_A);   // weight grads
    else if (role == 6) launch_fc_bwd(a, B, Bp, S(stream), false, FCB_ROLE_B);
    else if (role == 7) launch_fc_grad_reduce(a, B, S(stream));                  // B > 1024: the partials' sum alone
    else launch_fc_bwd_role(a, B, Bp, role, S(stream));
    check_launch();
  }, py::arg("dz1"), py::arg("p"), py::arg("pmask"), py::arg("w1t"), py::arg("h_bf"), py::arg("dl_bf"),
     py::arg("loss_rows"), py::arg("state"), py::arg("grad"), py::arg("dyc"), py::arg("loss_log"),
     py::arg("grad_scale"), py::arg("inv_batch"), py::arg("B"), py::arg("Bp"), py::arg("stream"),
     py::arg("role") = -1, py::arg("part") = 0, py::arg("ada") = py::none());
  m.def("fc_bwd_splits", &fc_bwd_splits);
  m.attr("FCB_PART_STRIDE") = FCB_PART_STRIDE;
  m.def("conv_bwd", [](uintptr_t dyc, uintptr_t a1, uintptr_t w2d, uintptr_t w1c, uintptr_t b1c,
                       uintptr_t data_u8, uintptr_t idx, int64_t idx_stride, uintptr_t state, uintptr_t c1part,
                       uintptr_t w2part, uintptr_t grad, float grad_scale, int B, uintptr_t stream,
                       uintptr_t xin, int stages, uintptr_t c1red, int update, int upd_lo, int upd_hi,
                       py::object ada) {
    const ConvBwdArgs a = conv_args(dyc, a1, w2d, w1c, b1c, data_u8, idx, idx_stride, state, c1part, w2part, grad,
                                    grad_scale, B, xin, c1red);
    // stages: 1 = dgrad (+ the conv1 pre-reduce with c1red), 2 = wgrad, 4 = reduce (reads c1red when given)
    if (stages <= 0 || stages > 7) throw std::runtime_error("conv_bwd: bad stage mask");
    if (stages & 1) launch_conv_dgrad(a, B, S(stream));
    if (stages & 2) launch_conv_wgrad(a, B, S(stream));
    // update (with the reduce stage): 0 = conv_grad_reduce, else the reduce fused with the Adadelta step:
    // 1 = the whole single launch, 2 = reduce parts [upd_lo, upd_hi) of the conv bucket, 3 = adadelta_c1
    if (update < 0 || update > 3 || (update && (!(stages & 4) || ada.is_none())))
      throw std::runtime_error("conv_bwd: bad update form");
    if ((stages & 4) && update == 0) {
      launch_conv_grad_reduce(a, B, S(stream));
    } else if (stages & 4) {
      const AdadeltaArgs u = ada_from_dict(ada.cast<py::dict>());
      if (update == 1) launch_adadelta_reduce(u, a, B, S(stream));
      else if (update == 2) launch_adadelta_reduce_parts(u, a, B, upd_lo, upd_hi, S(stream));
      else launch_adadelta_c1(u, a, B, S(stream));
    }
    check_launch();
  }, py::arg("dy"), py::arg("a1"), py::arg("w2d"), py::arg("w1c"), py::arg("b1c"), py::arg("data_u8"), py::arg("idx"),
     py::arg("idx_stride"), py::arg("state"), py::arg("c1part"), py::arg("w2part"), py::arg("grad"),
     py::arg("grad_scale"), py::arg("B"), py::arg("stream"), py::arg("xin") = 0, py::arg("stages") = 7,
     py::arg("c1red") = 0, py::arg("update") = 0, py::arg("upd_lo") = 0, py::arg("upd_hi") = 0,
     py::arg("ada") = py::none());
  m.attr("C1_PRE_SLABS") = C1_PRE_SLABS;
  m.attr("RED_W2_PARTS") = RED_W2_PARTS;
  m.attr("RED_ALL_PARTS") = RED_ALL_PARTS;
  m.attr("ADA_FC_LEAN_GRID") = ADA_FC_LEAN_GRID;
  m.attr("WT_MAX_B") = WT_MAX_B;
  m.def("adadelta", [](uintptr_t param, uintptr_t grad, uintptr_t sq, uintptr_t acc, uintptr_t lr, float rho,
                       float eps, float wd, uintptr_t w2f, uintptr_t w2d, uintptr_t w1, uintptr_t w1t,
                       uintptr_t state_inc, int region, bool update, uintptr_t stream, int grid, bool wt) {
    AdadeltaArgs a{P<float>(param), P<const float>(grad), P<float>(sq), P<float>(acc), P<const float>(lr), rho,
                   eps, wd, P<uint16_t>(w2f), P<uint16_t>(w2d), P<uint16_t>(w1), P<uint16_t>(w1t),
                   P<StepState>(state_inc)};
    a.wt = wt ? 1 : 0;
    if (grid < 0) throw std::runtime_error("adadelta: negative grid");
    if (update) launch_adadelta(a, region, S(stream), grid);   // grid > 0: the fc region's grid-stride form
    else launch_refresh_shadows(a, S(stream));
    check_launch();
  }, py::arg("param"), py::arg("grad"), py::arg("square_avg"), py::arg("acc_delta"), py::arg("lr"), py::arg("rho"),
     py::arg("eps"), py::arg("weight_decay"), py::arg("w2f"), py::arg("w2d"), py::arg("w1"), py::arg("w1t"),
     py::arg("state_inc"), py::arg("region"), py::arg("update"), py::arg("stream"), py::arg("grid") = 0,
     py::arg("wt") = false);

  // ---------------- fp32 step, one launcher at a time (tests) ----------------
  m.attr("F32_MAX_SPLITS") = F32_MAX_SPLITS;
  m.attr("F32_C1W_BLOCKS") = F32_C1W_BLOCKS;
  m.attr("F32_STAGE_ALL") = (int)F32_STAGE_ALL;
  m.def("f32_fc1_splits", &f32_fc1_splits);
  m.def("f32_conv2w_splits", &f32_conv2w_splits);
  m.def("f32_conv1w_splits", &f32_conv1w_splits);
  m.def("f32_forward", [](py::dict ptrs, int64_t idx_stride, float inv_batch, int B, bool train, int stages,
                          uintptr_t stream) {
    launch_f32_forward(f32_from_dict(ptrs, idx_stride, inv_batch), B, train, S(stream), stages);
    check_launch();
  }, py::arg("ptrs"), py::arg("idx_stride"), py::arg("inv_batch"), py::arg("B"), py::arg("train"), py::arg("stages"),
     py::arg("stream"),
     "launch_f32_forward on caller-owned buffers; stages: bit 0 prep, 1 conv1, 2 conv2, 3 pool, 4 fc1, 5 head");
  m.def("f32_backward", [](py::dict ptrs, int64_t idx_stride, float inv_batch, int B, int stage, uintptr_t stream) {
    const F32Step a = f32_from_dict(ptrs, idx_stride, inv_batch);
    if (B < 1) throw std::runtime_error("f32_backward: empty batch");
    switch (stage) {
      case 0: launch_f32_fc_small(a, B, S(stream)); break;
      case 1: launch_f32_fc1w(a, B, S(stream)); break;
      case 2: launch_f32_fc1x(a, B, S(stream)); break;
      case 3: launch_f32_conv2w(a, B, S(stream)); break;
      case 4: launch_f32_conv2x_conv1w(a, B, S(stream)); break;
      case 5: launch_f32_conv_reduce(a, B, S(stream)); break;
      default: throw std::runtime_error("f32_backward: bad stage");
    }
    check_launch();
  }, py::arg("ptrs"), py::arg("idx_stride"), py::arg("inv_batch"), py::arg("B"), py::arg("stage"), py::arg("stream"),
     "one backward launcher: 0 fc_small, 1 fc1w, 2 fc1x, 3 conv2w, 4 conv2x + conv1w, 5 conv_reduce");

  // ---------------- single-launch inference forward ----------------
  m.attr("INFER_BANDS") = INFER_BANDS;
  m.def("infer_plan", [](int B) {
    const InferPlan p = infer_plan(B);
    py::dict d;
    d["images_per_wg"] = p.images_per_wg; d["groups"] = p.groups; d["bands"] = p.bands;
    d["grid"] = py::make_tuple(p.grid_x, p.grid_y);            // (bands, groups)
    d["workspace_bytes"] = p.workspace_bytes; d["ticket_count"] = p.ticket_count;
    return d;
  }, py::arg("B"), "launch geometry and buffer sizes of infer_fwd at batch B (pure; no GPU needed)");
  m.def("infer_fwd", [](uintptr_t data_u8, uintptr_t idx, uintptr_t xin, uintptr_t labels, uintptr_t w1c,
                        uintptr_t b1c, uintptr_t w2f, uintptr_t b2c, uintptr_t w1, uintptr_t b_fc1,
                        uintptr_t w_fc2, uintptr_t b_fc2, uintptr_t z1part, uintptr_t tickets, uintptr_t logp,
                        uintptr_t pred, uintptr_t loss_rows, uintptr_t correct, int B, uintptr_t stream) {
    InferArgs a{P<const uint8_t>(data_u8), P<const int32_t>(idx), P<const float>(xin), P<const int32_t>(labels),
                P<const float>(w1c), P<const float>(b1c), P<const uint16_t>(w2f), P<const float>(b2c),
                P<const uint16_t>(w1), P<const float>(b_fc1), P<const float>(w_fc2), P<const float>(b_fc2),
                P<float>(z1part), P<int>(tickets), P<float>(logp), P<int32_t>(pred), P<float>(loss_rows),
                P<int32_t>(correct)};
    launch_infer_fwd(a, B, S(stream));
    check_launch();
  }, py::arg("data_u8"), py::arg("idx"), py::arg("xin"), py::arg("labels"), py::arg("w1c"), py::arg("b1c"),
     py::arg("w2f"), py::arg("b2c"), py::arg("w1"), py::arg("b_fc1"), py::arg("w_fc2"), py::arg("b_fc2"),
     py::arg("z1part"), py::arg("tickets"), py::arg("logp"), py::arg("pred"), py::arg("loss_rows"),
     py::arg("correct"), py::arg("B"), py::arg("stream"));

  // ---------------- input gradient (module API / Predictor) ----------------
  m.def("input_grad_plan", [](int B, int cus) {
    const InputGradPlan p = input_grad_plan(B, cus);
    if (p.grid < 1) throw std::runtime_error("input_grad_plan: B and cus must be positive");
    py::dict d;
    d["items"] = p.items; d["rounds"] = p.rounds; d["grid"] = p.grid;
    return d;
  }, py::arg("B"), py::arg("cus") = 256, "items, rounds and grid of input_grad at batch B (pure; no GPU needed)");
  m.def("input_grad", [](uintptr_t dyc, uintptr_t a1, uintptr_t w2d, uintptr_t w1c, uintptr_t dx, int B,
                         uintptr_t stream, int grid) {
    InputGradArgs a{P<const uint8_t>(dyc), P<const uint16_t>(a1), P<const uint16_t>(w2d), P<const float>(w1c),
                    P<float>(dx)};
    if (grid < 0) throw py::value_error("input_grad: grid must not be negative");
    launch_input_grad(a, B, S(stream), grid);
    check_launch();
  }, py::arg("dyc"), py::arg("a1"), py::arg("w2d"), py::arg("w1c"), py::arg("dx"), py::arg("B"), py::arg("stream"),
     py::arg("grid") = 0);
  m.def("input_grad_step", [](uintptr_t dyc, uintptr_t a1, uintptr_t w2d, uintptr_t w1c, uintptr_t x, uintptr_t x0,
                              uintptr_t x_next, float alpha, float eps, float lo, float hi, int B,
                              uintptr_t stream, uintptr_t dx, int grid) {
    InputGradStepArgs a{{P<const uint8_t>(dyc), P<const uint16_t>(a1), P<const uint16_t>(w2d), P<const float>(w1c),
                         P<float>(dx)},
                        P<const float>(x), P<const float>(x0), P<float>(x_next), alpha, eps, lo, hi};
    if (grid < 0) throw py::value_error("input_grad_step: grid must not be negative");
    launch_input_grad_step(a, B, S(stream), grid);
    check_launch();
  }, py::arg("dyc"), py::arg("a1"), py::arg("w2d"), py::arg("w1c"), py::arg("x"), py::arg("x0"), py::arg("x_next"),
     py::arg("alpha"), py::arg("eps"), py::arg("lo"), py::arg("hi"), py::arg("B"), py::arg("stream"),
     py::arg("dx") = 0, py::arg("grid") = 0,
     "input_grad with the projected-step epilogue: x_next = clamp(clamp(x + alpha sgn(dx), x0 -+ eps), lo, hi)");
  m.attr("PGD_L2_TINY") = PGD_L2_TINY;
  m.def("pgd_l2_step", [](uintptr_t dx, uintptr_t x, uintptr_t x0, uintptr_t x_next, float alpha, float eps,
                          float lo, float hi, int B, uintptr_t stream) {
    PgdL2StepArgs a{P<const float>(dx), P<const float>(x), P<const float>(x0), P<float>(x_next), alpha, eps, lo, hi};
    launch_pgd_l2_step(a, B, S(stream));
    check_launch();
  }, py::arg("dx"), py::arg("x"), py::arg("x0"), py::arg("x_next"), py::arg("alpha"), py::arg("eps"),
     py::arg("lo"), py::arg("hi"), py::arg("B"), py::arg("stream"),
     "L2 projected-gradient step per image: t = x + alpha dx / |dx|; x_next = clamp(x0 + proj_eps(t - x0), lo, hi)");

  // ---------------- adversarial training ----------------
  m.attr("ADV_PHILOX_DOMAIN") = ADV_PHILOX_DOMAIN;
  m.def("adv_init", [](uintptr_t data_u8, uintptr_t idx, int64_t idx_stride, uintptr_t labels, uintptr_t state,
                       uintptr_t x0, uintptr_t x, uintptr_t labels_out, float eps, float lo, float hi,
                       bool random_start, int B, uintptr_t stream) {
    AdvInitArgs a{P<const uint8_t>(data_u8), P<const int32_t>(idx), idx_stride, P<const int32_t>(labels),
                  P<const StepState>(state), P<float>(x0), P<float>(x), P<int32_t>(labels_out), eps, lo, hi,
                  random_start ? 1 : 0};
    launch_adv_init(a, B, S(stream));
    check_launch();
  }, py::arg("data_u8"), py::arg("idx"), py::arg("idx_stride"), py::arg("labels"), py::arg("state"), py::arg("x0"),
     py::arg("x"), py::arg("labels_out"), py::arg("eps"), py::arg("lo"), py::arg("hi"), py::arg("random_start"),
     py::arg("B"), py::arg("stream"),
     "first launch of an adversarial training step: x0 = the step's batch normalised, x = x0 or its random "
     "start clamp(x0 + (2u - 1) eps, lo, hi), labels_out = the batch's labels");

  // ---------------- randomized smoothing ----------------
  m.attr("SMOOTH_PHILOX_DOMAIN") = SMOOTH_PHILOX_DOMAIN;
  m.def("smooth_noise", [](uintptr_t x_u8, uintptr_t x_f32, uintptr_t out, float sigma, uint64_t seed,
                           int64_t sample_base, int64_t id_base, int M, int n, uintptr_t stream) {
    if (sample_base < 0 || id_base < 0 || sample_base > 0xFFFFFFFFll || id_base > 0xFFFFFFFFll)
      throw std::runtime_error("smooth_noise: sample_base and id_base must fit 32 bits");
    SmoothNoiseArgs a{P<const uint8_t>(x_u8), P<const float>(x_f32), P<float>(out), nullptr, sigma, seed,
                      (uint32_t)sample_base, (uint32_t)id_base, n};
    launch_smooth_noise(a, M, S(stream));
    check_launch();
  }, py::arg("x_u8"), py::arg("x_f32"), py::arg("out"), py::arg("sigma"), py::arg("seed"), py::arg("sample_base"),
     py::arg("id_base"), py::arg("M"), py::arg("n"), py::arg("stream"),
     "out[i * n + s] = x0_i + sigma * z: n Gaussian-noised fp32 copies of each of M images (Philox + Box-Muller)");
  m.def("smooth_noise_step", [](uintptr_t state, uintptr_t x0, uintptr_t x, float sigma, int B, uintptr_t stream) {
    launch_smooth_noise_step(P<const StepState>(state), P<const float>(x0), P<float>(x), sigma, B, S(stream));
    check_launch();
  }, py::arg("state"), py::arg("x0"), py::arg("x"), py::arg("sigma"), py::arg("B"), py::arg("stream"),
     "step form of smooth_noise: x[b] = x0[b] + sigma * z, counters from the StepState");
  m.def("smooth_vote", [](uintptr_t logp, uintptr_t counts, int M, int n, bool accumulate, uintptr_t stream) {
    launch_smooth_vote(SmoothVoteArgs{P<const float>(logp), P<int32_t>(counts), n, accumulate ? 1 : 0}, M, S(stream));
    check_launch();
  }, py::arg("logp"), py::arg("counts"), py::arg("M"), py::arg("n"), py::arg("accumulate"), py::arg("stream"),
     "counts[i][argmax logp[i * n + s]] (+)= 1 over the n rows of each of M images; NaN rows vote for nothing");

  // ---------------- attribution ----------------
  m.attr("ATTR_MAX_STEPS") = ATTR_MAX_STEPS;
  m.attr("ATTR_FINISH_NONE") = (int)ATTR_FINISH_NONE;
  m.attr("ATTR_FINISH_SCALE") = (int)ATTR_FINISH_SCALE;
  m.attr("ATTR_FINISH_PATH") = (int)ATTR_FINISH_PATH;
  m.def("attr_path", [](uintptr_t x_u8, uintptr_t x_f32, uintptr_t base, float base_value, uintptr_t out,
                        int sample_base, int n_total, int M, int ns, uintptr_t stream) {
    AttrPathArgs a{P<const uint8_t>(x_u8), P<const float>(x_f32), P<const float>(base), base_value, P<float>(out),
                   sample_base, n_total, ns};
    launch_attr_path(a, M, S(stream));
    check_launch();
  }, py::arg("x_u8"), py::arg("x_f32"), py::arg("base"), py::arg("base_value"), py::arg("out"),
     py::arg("sample_base"), py::arg("n_total"), py::arg("M"), py::arg("ns"), py::arg("stream"),
     "out[i * ns + s] = b_i + alpha (x_i - b_i), alpha = (sample_base + s + 1/2) / n_total: the integration path's rows");
  m.def("attr_reduce", [](uintptr_t dx, uintptr_t acc, uintptr_t out, uintptr_t x_u8, uintptr_t x_f32, uintptr_t base,
                          float base_value, float scale, int M, int ns, bool accumulate, int finish,
                          uintptr_t stream) {
    AttrReduceArgs a{P<const float>(dx), P<float>(acc), P<float>(out), P<const uint8_t>(x_u8), P<const float>(x_f32),
                     P<const float>(base), base_value, scale, ns, accumulate ? 1 : 0, finish};
    launch_attr_reduce(a, M, S(stream));
    check_launch();
  }, py::arg("dx"), py::arg("acc"), py::arg("out"), py::arg("x_u8"), py::arg("x_f32"), py::arg("base"),
     py::arg("base_value"), py::arg("scale"), py::arg("M"), py::arg("ns"), py::arg("accumulate"), py::arg("finish"),
     py::arg("stream"),
     "acc[i] (+)= the sum of dx[i * ns + s] in ascending s; finish: out = acc * scale [* (x_i - b_i)]");

  // ---------------- minimum-norm adversarial examples (DeepFool) ----------------
  m.attr("DF_CLASSES") = DF_CLASSES;
  m.attr("DF_SLACK") = DF_SLACK;
  m.attr("DF_MAX_M") = DF_MAX_M;
  m.attr("DF_RUNNING") = (int)DF_RUNNING;
  m.attr("DF_CROSSED") = (int)DF_CROSSED;
  m.attr("DF_STUCK") = (int)DF_STUCK;
  m.def("deepfool_init", [](uintptr_t x_u8, uintptr_t x_f32, uintptr_t rows, uintptr_t x, uintptr_t x0_out,
                            uintptr_t r_tot, uintptr_t status, uintptr_t iters, uintptr_t norm, int M,
                            uintptr_t stream) {
    DeepfoolInitArgs a{P<const uint8_t>(x_u8), P<const float>(x_f32), P<float>(rows), P<float>(x), P<float>(x0_out),
                       P<float>(r_tot), P<int32_t>(status), P<int32_t>(iters), P<float>(norm)};
    launch_deepfool_init(a, M, S(stream));
    check_launch();
  }, py::arg("x_u8"), py::arg("x_f32"), py::arg("rows"), py::arg("x"), py::arg("x0_out"), py::arg("r_tot"),
     py::arg("status"), py::arg("iters"), py::arg("norm"), py::arg("M"), py::arg("stream"),
     "rows[10 i + c] = x[i] = x0_i for c < 10, r_tot = 0, status = iters = 0, norm = 0: the start of a DeepFool run");
  m.def("deepfool_step", [](uintptr_t dx, uintptr_t loss_rows, uintptr_t y, uintptr_t x0, uintptr_t r_tot, uintptr_t x,
                            uintptr_t rows, uintptr_t status, uintptr_t iters, uintptr_t norm, float overshoot,
                            float lo, float hi, int M, uintptr_t stream) {
    DeepfoolStepArgs a{P<const float>(dx), P<const float>(loss_rows), P<const int32_t>(y), P<const float>(x0),
                       P<float>(r_tot), P<float>(x), P<float>(rows), P<int32_t>(status), P<int32_t>(iters),
                       P<float>(norm), overshoot, lo, hi};
    launch_deepfool_step(a, M, S(stream));
    check_launch();
  }, py::arg("dx"), py::arg("loss_rows"), py::arg("y"), py::arg("x0"), py::arg("r_tot"), py::arg("x"), py::arg("rows"),
     py::arg("status"), py::arg("iters"), py::arg("norm"), py::arg("overshoot"), py::arg("lo"), py::arg("hi"),
     py::arg("M"), py::arg("stream"),
     "one L2 DeepFool step per image from its ten gradient rows and losses: r_tot += the step to the nearest "
     "linearised boundary, x = rows = clamp(x0 + (1 + overshoot) r_tot, lo, hi); crossed / stuck images freeze");

  // ---------------- Auto-PGD ----------------
  m.def("apgd_step", [](uintptr_t dx, uintptr_t loss_rows, uintptr_t x0, uintptr_t x, uintptr_t x_old, uintptr_t x_best,
                        uintptr_t g_best, uintptr_t fstate, uintptr_t istate, float sign, float eps, float lo, float hi,
                        bool l2, bool first, bool last, int window, int M, uintptr_t stream) {
    ApgdStepArgs a{P<const float>(dx), P<const float>(loss_rows), P<const float>(x0), P<float>(x), P<float>(x_old),
                   P<float>(x_best), P<float>(g_best), P<float>(fstate), P<int32_t>(istate), sign, eps, lo, hi,
                   first ? 1 : 0, last ? 1 : 0, window};
    launch_apgd_step(a, M, l2, S(stream));
    check_launch();
  }, py::arg("dx"), py::arg("loss_rows"), py::arg("x0"), py::arg("x"), py::arg("x_old"), py::arg("x_best"),
     py::arg("g_best"), py::arg("fstate"), py::arg("istate"), py::arg("sign"), py::arg("eps"), py::arg("lo"),
     py::arg("hi"), py::arg("l2"), py::arg("first"), py::arg("last"), py::arg("window"), py::arg("M"),
     py::arg("stream"),
     "one Auto-PGD iteration per image: counters and best point, checkpoint (halve eta, restart from the best), "
     "momentum step; fstate [M][4] = eta, loss_best, loss_prev, loss_check; istate [M][4] = n_up, reduced, iters, "
     "restarted");

  // ---------------- Square Attack ----------------
  m.attr("SQUARE_PHILOX_DOMAIN") = SQUARE_PHILOX_DOMAIN;
  m.def("square_init", [](uintptr_t x0, uintptr_t x_cand, float eps, float lo, float hi, uint64_t seed,
                          int64_t id_base, int M, uintptr_t stream) {
    if (id_base < 0 || id_base > 0xFFFFFFFFll) throw std::runtime_error("square_init: id_base must fit 32 bits");
    SquareInitArgs a{P<const float>(x0), P<float>(x_cand), eps, lo, hi, seed, (uint32_t)id_base};
    launch_square_init(a, M, S(stream));
    check_launch();
  }, py::arg("x0"), py::arg("x_cand"), py::arg("eps"), py::arg("lo"), py::arg("hi"), py::arg("seed"),
     py::arg("id_base"), py::arg("M"), py::arg("stream"),
     "x_cand = clamp(x0 +- eps, lo, hi) in vertical stripes drawn from Philox: the candidate of query 0 of a Square "
     "Attack");
  m.def("square_step", [](uintptr_t logp, uintptr_t y, uintptr_t x0, uintptr_t x_best, uintptr_t x_cand,
                          uintptr_t state, float eps, float lo, float hi, uint64_t seed, int64_t q, int64_t id_base,
                          int side, bool first, bool last, bool targeted, int M, uintptr_t stream) {
    if (q < 0 || q > 0xFFFFFFFFll || id_base < 0 || id_base > 0xFFFFFFFFll)
      throw std::runtime_error("square_step: q and id_base must fit 32 bits");
    SquareStepArgs a{P<const float>(logp), P<const int32_t>(y), P<const float>(x0), P<float>(x_best), P<float>(x_cand),
                     P<void>(state), eps, lo, hi, seed, (uint32_t)q, (uint32_t)id_base, side, first ? 1 : 0,
                     last ? 1 : 0, targeted ? 1 : 0};
    launch_square_step(a, M, S(stream));
    check_launch();
  }, py::arg("logp"), py::arg("y"), py::arg("x0"), py::arg("x_best"), py::arg("x_cand"), py::arg("state"),
     py::arg("eps"), py::arg("lo"), py::arg("hi"), py::arg("seed"), py::arg("q"), py::arg("id_base"), py::arg("side"),
     py::arg("first"), py::arg("last"), py::arg("targeted"), py::arg("M"), py::arg("stream"),
     "one Square Attack query per image: accept the candidate when its margin is strictly lower, freeze a broken "
     "image, write the next candidate (a square of +-eps at a Philox-drawn place); state [M] records of 16 bytes = "
     "margin_best, queries_used, done, spare");

  // ---------------- communicator ----------------
  py::class_<RcclComm, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def(py::init([](py::bytes uid, int world, int rank, int device, double init_timeout_s, bool wait) {
             std::string s = uid;
             std::shared_ptr<RcclComm> c;
             {
               // the init waits for its bootstrap: let other Python threads run meanwhile
               // (distributed.PendingRcclComm overlaps it with data / model / trainer setup)
               py::gil_scoped_release nogil;
               c = std::make_shared<RcclComm>(std::vector<uint8_t>(s.begin(), s.end()), world, rank, device,
                                              init_timeout_s, wait);
             }
             return c;
           }),
           py::arg("unique_id"), py::arg("world_size"), py::arg("rank"), py::arg("device"),
           py::arg("init_timeout_s") = 600.0, py::arg("wait") = true)
      .def("abort", [](RcclComm& c) {
        py::gil_scoped_release nogil;
        c.abort();
      })
      .def_property_readonly("aborted", &RcclComm::aborted)
      .def_property_readonly("nonblocking", &RcclComm::nonblocking)
      .def("async_error", &RcclComm::async_error)
      .def("init_status", &RcclComm::init_status, py::call_guard<py::gil_scoped_release>())
      .def_static("error_string", &RcclComm::error_string)
      .def_static("available", &RcclComm::available)
      .def_static("version", &RcclComm::version)
      .def_static("unique_id", []() {
        auto v = RcclComm::unique_id();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
      })
      .def("allreduce_sum", [](RcclComm& c, uintptr_t buf, int64_t count, int dtype, uintptr_t stream) {
        c.allreduce_sum(P<void>(buf), count, dtype, S(stream));
      })
      .def("broadcast", [](RcclComm& c, uintptr_t buf, int64_t count, int dtype, int root, uintptr_t stream) {
        c.broadcast(P<void>(buf), count, dtype, root, S(stream));
      })
      .def_property_readonly("world_size", &RcclComm::world_size)
      .def_property_readonly("rank", &RcclComm::rank);

  py::class_<XgmiComm, std::shared_ptr<XgmiComm>>(m, "XgmiComm", py::dynamic_attr())
      .def(py::init([](int world, int rank, int device, int64_t numel, int channels, int64_t oneshot_max,
                       int co_ranks, double budget) {
             // device allocation + memsets + a device sync: other Python threads run meanwhile
             // (distributed.PendingXgmiComm overlaps the setup with the main thread's)
             py::gil_scoped_release nogil;
             return std::make_shared<XgmiComm>(world, rank, device, numel, channels, oneshot_max, co_ranks,
                                               budget);
           }),
           py::arg("world_size"), py::arg("rank"), py::arg("device"), py::arg("numel"), py::arg("channels") = 2,
           py::arg("oneshot_max") = 32768, py::arg("co_ranks") = 1, py::arg("budget") = 0.5)
      // the communicator's own buffers as DLPack capsules (torch.utils.dlpack.from_dlpack): zero-copy
      // fp32 [numel] views that keep the communicator alive
      .def("dlpack", [](std::shared_ptr<XgmiComm> c, const std::string& which) {
        // "flags" / "stage" (tests): this rank's flag blocks [channels][2][8][512] (int32 bits behind a
        // float view) and staging slots [channels][2][oneshot_max]
        if (which == "flags")
          return dlpack_f32(reinterpret_cast<float*>(c->flags()), (int64_t)c->channels() * XGMI_FLAG_INTS, c->device(), c);
        if (which == "stage") return dlpack_f32(c->stage(), (int64_t)c->channels() * 2 * c->oneshot_max(), c->device(), c);
        if (which != "in" && which != "out") throw std::runtime_error("dlpack: which must be 'in', 'out', 'flags' or 'stage'");
        return dlpack_f32(which == "in" ? c->in() : c->out(), c->numel(), c->device(), c);
      })
      .def_property_readonly("ordering", &XgmiComm::ordering)
      .def_property_readonly("grids", [](const XgmiComm& c) {
        const XgmiGrids& g = c.grids();
        py::dict d;
        d["fc_fused"] = g.fc_fused; d["conv_fused"] = g.conv_fused; d["twoshot"] = g.twoshot; d["oneshot"] = g.oneshot;
        d["cap_fc_fused"] = g.cap_fc_fused; d["cap_conv_fused"] = g.cap_conv_fused;
        d["cap_twoshot"] = g.cap_twoshot; d["cap_oneshot"] = g.cap_oneshot;
        d["load_fused"] = g.load_fused; d["load_separate"] = g.load_separate;
        return d;
      })
      .def("record", [](const XgmiComm& c) {
        auto v = c.record();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
      })
      .def("connect", [](XgmiComm& c, std::vector<py::bytes> recs) {
        std::vector<std::vector<uint8_t>> v;
        for (auto& r : recs) {
          std::string s = r;
          v.emplace_back(s.begin(), s.end());
        }
        py::gil_scoped_release nogil;   // one IPC import per peer
        c.connect(v);
      })
      // ada (a dict as the adadelta / conv_bwd bindings take; hold pointers, signal_start and the conv
      // part's wait_* stay null: the engine's) fuses the Adadelta step; max_wg > 0 shrinks the planned grid
      .def("allreduce", [](XgmiComm& c, int channel, int64_t offset, int64_t count, uintptr_t stream, py::object ada,
                           int max_wg) {
        if (ada.is_none()) {
          c.allreduce(channel, offset, count, S(stream), nullptr, max_wg);
        } else {
          const AdadeltaArgs u = ada_from_dict(ada.cast<py::dict>());
          c.allreduce(channel, offset, count, S(stream), &u, max_wg);
        }
        check_launch();
      }, py::arg("channel"), py::arg("offset"), py::arg("count"), py::arg("stream"), py::arg("ada") = py::none(),
         py::arg("max_wg") = 0)
      .def("allreduce_fc_fused", [](XgmiComm& c, int channel, uintptr_t stream, py::dict ada, int max_wg) {
        c.allreduce_fc_fused(channel, S(stream), ada_from_dict(ada), max_wg);
        check_launch();
      }, py::arg("channel"), py::arg("stream"), py::arg("ada"), py::arg("max_wg") = 0)
      .def("conv_reduce_fused", [](XgmiComm& c, int channel, uintptr_t dyc, uintptr_t a1, uintptr_t w2d, uintptr_t w1c,
                                   uintptr_t b1c, uintptr_t data_u8, uintptr_t idx, int64_t idx_stride,
                                   uintptr_t state, uintptr_t c1part, uintptr_t w2part, uintptr_t grad,
                                   float grad_scale, int B, uintptr_t stream, py::dict ada, uintptr_t xin,
                                   uintptr_t c1red, int lo, int hi, int max_wg) {
        if (lo < 0 || hi > RED_ALL_PARTS || lo >= hi) throw std::runtime_error("conv_reduce_fused: bad reduce parts");
        XgmiConvPart part;
        part.lo = lo;
        part.hi = hi;
        c.conv_reduce_fused(channel, conv_args(dyc, a1, w2d, w1c, b1c, data_u8, idx, idx_stride, state, c1part,
                                               w2part, grad, grad_scale, B, xin, c1red),
                            B, S(stream), ada_from_dict(ada), part, max_wg);
        check_launch();
      }, py::arg("channel"), py::arg("dy"), py::arg("a1"), py::arg("w2d"), py::arg("w1c"), py::arg("b1c"),
         py::arg("data_u8"), py::arg("idx"), py::arg("idx_stride"), py::arg("state"), py::arg("c1part"),
         py::arg("w2part"), py::arg("grad"), py::arg("grad_scale"), py::arg("B"), py::arg("stream"), py::arg("ada"),
         py::arg("xin") = 0, py::arg("c1red") = 0, py::arg("lo") = 0, py::arg("hi") = RED_ALL_PARTS,
         py::arg("max_wg") = 0)
      .def("error", &XgmiComm::error)
      .def("set_timeout_seconds", &XgmiComm::set_timeout_seconds)
      .def("set_fences", &XgmiComm::set_fences)
      .def_property_readonly("fences", &XgmiComm::fences)
      .def("close_peers", &XgmiComm::close_peers, py::call_guard<py::gil_scoped_release>())
      .def("mark_recyclable", &XgmiComm::mark_recyclable)
      // rank `root`'s parameters to every rank through the IPC-mapped output buffers (DDP construction
      // broadcast without RCCL): root stages `count` floats of `buf` into its output buffer, then -
      // after the caller's barrier - every other rank copies them out of root's; the caller barriers
      // again before the buffers are reused
      .def("stage_out", [](XgmiComm& c, uintptr_t buf, int64_t count, uintptr_t stream) {
        c.stage_out(P<const float>(buf), count, S(stream));
      })
      .def("read_peer_out", [](XgmiComm& c, int peer, uintptr_t buf, int64_t count, uintptr_t stream) {
        c.read_peer_out(peer, P<float>(buf), count, S(stream));
      })
      .def_property_readonly("connected", &XgmiComm::connected)
      .def_property_readonly("world_size", &XgmiComm::world_size)
      .def_property_readonly("rank", &XgmiComm::rank);

  // ---------------- DDP gradient reducer (module-level path) ----------------
  py::class_<BucketReducer>(m, "BucketReducer")
      .def(py::init([](std::vector<std::vector<int64_t>> numels, int world, std::shared_ptr<RcclComm> comm) {
             return new BucketReducer(numels, world, std::move(comm));
           }),
           py::arg("bucket_numels"), py::arg("world_size"), py::arg("comm") = nullptr)
      .def("prepare", &BucketReducer::prepare)
      .def("mark_ready", [](BucketReducer& r, int b, int slot, uintptr_t grad, uintptr_t out, uintptr_t stream) {
        r.mark_ready(b, slot, P<const float>(grad), P<float>(out), S(stream));
      })
      .def("finalize", [](BucketReducer& r, uintptr_t stream) { r.finalize(S(stream)); })
      .def_property_readonly("num_buckets", &BucketReducer::num_buckets)
      .def("bucket_numel", &BucketReducer::bucket_numel)
      .def("bucket_ptr", &BucketReducer::bucket_ptr)
      .def_property_readonly("launches", &BucketReducer::launches);

  // ---------------- engine ----------------
  py::class_<Engine>(m, "Engine")
      .def(py::init([](py::dict bufs, int max_batch, int max_test_batch, uintptr_t compute, uintptr_t comm,
                       int world, float rho, float eps, float wd, bool fp32) {
             return new Engine(buffers_from_dict(bufs), max_batch, max_test_batch, S(compute), S(comm), world, rho,
                               eps, wd, fp32);
           }),
           py::arg("buffers"), py::arg("max_batch"), py::arg("max_test_batch"), py::arg("compute_stream"),
           py::arg("comm_stream"), py::arg("world_size"), py::arg("rho"), py::arg("eps"), py::arg("weight_decay"),
           py::arg("fp32") = false)
      .def_property_readonly("fp32", &Engine::fp32)
      .def("attach_comm", &Engine::attach_comm)
      .def("attach_xgmi", &Engine::attach_xgmi)
      .def("set_xgmi_fuse_update", &Engine::set_xgmi_fuse_update)
      .def("set_bucket_split", &Engine::set_bucket_split)
      .def("set_rccl_handoff", &Engine::set_rccl_handoff)
      .def_property("fc_dw1_side", &Engine::fc_dw1_side, &Engine::set_fc_dw1_side)
      .def_property("w1t_pingpong", &Engine::w1t_pingpong, &Engine::set_w1t_pingpong)
      .def_property("c1_lanes", &Engine::c1_lanes, &Engine::set_c1_lanes)
      .def("fault_hold", &Engine::fault_hold)
      .def("fault_release", [](Engine& e, uintptr_t stream) { e.fault_release(S(stream)); })
      .def("set_schedule", &Engine::set_schedule, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("schedule", &Engine::schedule)
      .def("set_adversarial", &Engine::set_adversarial, py::arg("eps"), py::arg("step_size"), py::arg("steps"),
           py::arg("random_start"), py::arg("lo"), py::arg("hi"),
           "adversarial training step form (normalised units; steps = 0: off); SERIAL, bf16, world 1 only")
      .def_property_readonly("adversarial_steps", &Engine::adversarial_steps)
      .def_property_readonly("adversarial_bytes", &Engine::adversarial_bytes)
      .def("set_noise", &Engine::set_noise, py::arg("sigma"), py::arg("on") = true,
           "Gaussian-noise training step form (sigma in normalised units; on = false: off); SERIAL, bf16, world 1 only")
      .def_property_readonly("noise_on", &Engine::noise_on)
      .def_property_readonly("noise_sigma", &Engine::noise_sigma)
      .def("reset_counters", &Engine::reset_counters, py::call_guard<py::gil_scoped_release>())
      .def("probe_stream_handoff", &Engine::probe_stream_handoff, py::arg("timeout_s") = 2.0,
           py::call_guard<py::gil_scoped_release>())
      .def("begin_epoch", &Engine::begin_epoch, py::arg("seed"), py::arg("rng_base"), py::arg("step0") = 0, py::arg("flags") = 0)
      .def("train_steps", &Engine::train_steps, py::call_guard<py::gil_scoped_release>())
      .def("capture_train", &Engine::capture_train)
      .def("graph_nodes", &Engine::graph_nodes, py::arg("id"), "nodes of a captured chunk's compute-chain graph")
      .def("profile_steps", &Engine::profile_steps, py::call_guard<py::gil_scoped_release>())
      .def("gather_rows", &Engine::gather_rows, py::arg("start"), py::arg("n"))
      .def("replay", &Engine::replay, py::call_guard<py::gil_scoped_release>())
      .def("eval", &Engine::eval)
      .def("capture_eval", &Engine::capture_eval)
      .def("refresh_shadows", &Engine::refresh_shadows)
      .def("broadcast_params", &Engine::broadcast_params)
      .def("synchronize", &Engine::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("sync_streams", &Engine::sync_streams, py::call_guard<py::gil_scoped_release>())
      .def("errors", &Engine::errors)
      .def("check_errors", &Engine::check_errors)
      .def_static("describe_xgmi_error", &Engine::describe_xgmi_error)
      .def_property_readonly("workspace_bytes", &Engine::workspace_bytes);

#ifdef MNIST_TIMELINE
  m.attr("TIMELINE") = true;
  // every instrumented wave since the last dump as little-endian uint64 triples (kernel id, start,
  // end; s_memrealtime ticks of 10 ns); the rings are rewound
  m.def("timeline_dump", []() {
    std::vector<uint64_t> v;
    tl_dump_trunk(v);
    tl_dump_fc_head(v);
    tl_dump_conv_bwd(v);
    tl_dump_adadelta(v);
    tl_dump_comm(v);
    tl_dump_xgmi(v);
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(uint64_t));
  });
#else
  m.attr("TIMELINE") = false;
#endif
  m.def("hip_prewarm", [](int device) {
    // the HIP runtime + this process's context on `device` and every kernel TU's code object, with
    // the GIL released (the driver's prewarm thread: the main thread keeps building data and model)
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("hip_prewarm: hipSetDevice failed");
    (void)hipFree(nullptr);
    const auto t1 = clk::now();
    preload_all_kernels();
    const auto t2 = clk::now();
    // the runtime's own first-use costs the setup would otherwise pay on the main thread: the blit
    // kernels behind hipMemset and the staging path of pageable host copies (measured on the box:
    // 80 ms of first hipMemsets, 28 ms of first pageable H2D copies inside the reference timer)
    clk::time_point tm = t2, th = t2, td = t2;
    {
      constexpr size_t kBytes = 1 << 20;
      void* d = nullptr;
      std::vector<char> h(kBytes, 0);
      if (hipMalloc(&d, kBytes) == hipSuccess) {
        launch_fill(d, kBytes, 0, nullptr);         // (our fill kernel: no blit-kernel load)
        (void)hipDeviceSynchronize();
        tm = clk::now();
        (void)hipMemcpy(d, h.data(), kBytes, hipMemcpyHostToDevice);
        th = clk::now();
        (void)hipMemcpy(h.data(), d, 4096, hipMemcpyDeviceToHost);
        td = clk::now();
        (void)hipFree(d);
      }
    }
    const auto t3 = clk::now();
    auto sec = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    return std::make_tuple(sec(t0, t1), sec(t1, t2), sec(t2, t3), sec(t2, tm), sec(tm, th), sec(th, td));
  }, py::call_guard<py::gil_scoped_release>(), py::arg("device"));
  // physical identity of a device (PCI domain:bus:device.function + UUID) straight from the HIP
  // runtime: callable from any thread, no amdsmi (torch.cuda.get_device_properties counts devices
  // through amdsmi, and from a helper thread it refused a valid index on the box)
  m.def("device_identity", [](int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, device) != hipSuccess)
      throw std::runtime_error("device_identity: hipDeviceGetPCIBusId failed");
    hipUUID uuid;
    std::string u;
    if (hipDeviceGetUuid(&uuid, device) == hipSuccess) {
      static const char* hx = "0123456789abcdef";
      for (int i = 0; i < 16; ++i) {
        u += hx[((unsigned char)uuid.bytes[i]) >> 4];
        u += hx[((unsigned char)uuid.bytes[i]) & 15];
      }
    }
    return std::string(bus) + "|" + u;
  });
  // raw HIP streams for the engine: "dedicated" = hipExtStreamCreateWithCUMask over every CU (the
  // runtime gives a CU-masked stream a hardware queue of its own instead of sharing a pooled one),
  // else hipStreamCreateWithPriority(non-blocking, priority)
  m.def("create_stream", [](int device, bool dedicated, int priority) {
    if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("create_stream: hipSetDevice failed");
    hipStream_t st = nullptr;
    if (dedicated) {
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        throw std::runtime_error("create_stream: CU count");
      std::vector<uint32_t> mask((cus + 31) / 32, 0xffffffffu);
      if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
      if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess)
        throw std::runtime_error("hipExtStreamCreateWithCUMask failed");
    } else if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority) != hipSuccess) {
      throw std::runtime_error("hipStreamCreateWithPriority failed");
    }
    return reinterpret_cast<uintptr_t>(st);
  }, py::arg("device"), py::arg("dedicated") = true, py::arg("priority") = 0);
  m.def("destroy_stream", [](uintptr_t s) { (void)hipStreamDestroy(S(s)); });
  // do two streams hand off through device counters (x waits for y's signal, then y for x's)?  False
  // when they share a hardware queue: the first wait times out (timeout_s) before the signal queued
  // behind it runs.  Engine-independent form of Engine::probe_stream_handoff (make_streams).
  m.def("probe_streams", [](uintptr_t xs, uintptr_t ys, double timeout_s) {
    hipStream_t x = S(xs), y = S(ys);
    int* c = nullptr;
    if (hipMalloc(&c, 4 * sizeof(int)) != hipSuccess) throw std::runtime_error("probe_streams: hipMalloc failed");
    launch_fill(c, 4 * sizeof(int), 0, x);
    bool ok = hipStreamSynchronize(x) == hipSuccess;
    launch_stream_wait(c + 0, c + 2, 1, c + 3, x, timeout_s);
    launch_stream_signal(c + 0, y);
    launch_stream_wait(c + 1, c + 2, 1, c + 3, y, timeout_s);
    launch_stream_signal(c + 1, x);
    ok = ok && hipStreamSynchronize(x) == hipSuccess && hipStreamSynchronize(y) == hipSuccess;
    int err = 1;
    if (ok) ok = hipMemcpyAsync(&err, c + 3, sizeof(int), hipMemcpyDeviceToHost, x) == hipSuccess &&
                 hipStreamSynchronize(x) == hipSuccess;
    (void)hipFree(c);
    return ok && err == 0;
  }, py::call_guard<py::gil_scoped_release>(), py::arg("x"), py::arg("y"), py::arg("timeout_s") = 0.5);
  m.def("synth_render", [](uintptr_t plan, uintptr_t templates, int64_t n, uintptr_t out, uintptr_t stream) {
    launch_synth_render(P<const void>(plan), P<const float>(templates), n, P<uint8_t>(out), S(stream));
    check_launch();
  }, py::arg("plan"), py::arg("templates"), py::arg("n"), py::arg("out"), py::arg("stream"),
     "render n synthetic images [n, 784] on the device from a host-made plan (generator v3)");
  // the support kernels of comm_kernels.hip on caller-owned pointers (tests)
  m.def("scale_copy", [](uintptr_t dst, uintptr_t src, int64_t n, float s, uintptr_t stream) {
    launch_scale_copy(P<float>(dst), P<const float>(src), n, s, S(stream));
    check_launch();
  }, py::arg("dst"), py::arg("src"), py::arg("n"), py::arg("s"), py::arg("stream"));
  m.def("fill", [](uintptr_t ptr, int64_t nbytes, int value, uintptr_t stream) {
    launch_fill(P<void>(ptr), nbytes, value, S(stream));
    check_launch();
  }, py::arg("ptr"), py::arg("nbytes"), py::arg("value"), py::arg("stream"));
  m.def("gather_rows", [](uintptr_t src_u8, uintptr_t src_labels, uintptr_t idx, int64_t start, int64_t n,
                          uintptr_t dst_u8, uintptr_t dst_labels, uintptr_t stream) {
    launch_gather_rows(P<const uint8_t>(src_u8), P<const int32_t>(src_labels), P<const int32_t>(idx), start, n,
                       P<uint8_t>(dst_u8), P<int32_t>(dst_labels), S(stream));
    check_launch();
  }, py::arg("src_u8"), py::arg("src_labels"), py::arg("idx"), py::arg("start"), py::arg("n"), py::arg("dst_u8"),
     py::arg("dst_labels"), py::arg("stream"));
  m.def("memset_sync", [](uintptr_t ptr, int value, int64_t nbytes) {
    // setup-time buffer initialisation without a torch fill kernel (whose code object would load on
    // first launch inside the reference timer); synchronous
    if (nbytes > 0) {
      launch_fill(reinterpret_cast<void*>(ptr), nbytes, value, nullptr);
      if (hipStreamSynchronize(nullptr) != hipSuccess) throw std::runtime_error("memset_sync: fill failed");
    }
  }, py::call_guard<py::gil_scoped_release>());
  m.def("preload_code_objects", &preload_all_kernels, py::call_guard<py::gil_scoped_release>(),
        "load every kernel translation unit's code object on the current device");
  m.def("roctx_push", [](const std::string& s) { roctx_push(s.c_str()); });
  m.def("roctx_pop", []() { roctx_pop(); });
}
