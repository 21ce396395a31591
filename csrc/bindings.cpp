// The torchbooster_amd native module (_C): the ops are bound per domain in the bind_*.cpp files
// (helpers in bind_common.h); here are the module itself, the bounds-checked debug build's
// readout, the stop-event / priority-stream hooks and the one-shot all-reduce.
#include "bind_common.h"
#include "runtime.h"

using namespace tbbind;

void register_norm(pybind11::module& m);
void register_loss(pybind11::module& m);
void register_optim(pybind11::module& m);
void register_conv(pybind11::module& m);
void register_conv_small(pybind11::module& m);
void register_gemm(pybind11::module& m);
void register_attn(pybind11::module& m);
void register_data(pybind11::module& m);
void register_runtime(pybind11::module& m);

// ---- bounds-checked debug build: every kernel file registers a reader of its flag
static std::vector<unsigned (*)()>& bounds_readers() {
  static std::vector<unsigned (*)()> r;
  return r;
}
namespace tbamd {
void bounds_register_reader(unsigned (*reader)()) { bounds_readers().push_back(reader); }
}  // namespace tbamd

// OR of every kernel file's violation bits since the last call (0 in normal builds)
static int64_t bounds_check() {
  unsigned v = 0;
  for (auto* r : bounds_readers()) v |= r();
  return (int64_t)v;
}

static bool bounds_enabled() {
#ifdef TBAMD_BOUNDS
  return true;
#else
  return false;
#endif
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torchbooster_amd native library (gfx950 HIP kernels + C++ runtime)";
  m.def("bounds_check", &bounds_check, "OR of the bounds-violation bits since the last call (debug build)");
  m.def("bounds_enabled", &bounds_enabled);
  // x[i] through one guarded device read (normal build: unchecked; bounds build: -1 + flag when i >= numel)
  m.def("bounds_probe", [](const Tensor& x, int64_t i) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous(), "bounds_probe: f32 cuda tensor");
    Tensor out = at::empty({1}, x.options());
    // (the probe is only ever called with i inside the allocation's first page in tests)
    tbamd::bounds_probe(x.data_ptr<float>(), x.numel(), i, out.data_ptr<float>(), cur_stream());
    return out;
  });
  register_norm(m);
  register_loss(m);
  register_optim(m);
  register_conv(m);
  register_conv_small(m);
  register_gemm(m);
  register_attn(m);
  register_data(m);
  m.def("stop_event_arm", &tbamd::stop_event_arm);
  m.def("stop_event_disarm", &tbamd::stop_event_disarm);
  m.def("stream_wait_stop_event", [](int64_t stream, int64_t id) {
    tbamd::stream_wait_stop_event(reinterpret_cast<hipStream_t>(stream), id);
  });
  // a non-blocking stream at an explicit HIP priority (torch's pool only hands out priorities
  // <= 0; the backward side stream is created at the LOWEST priority so the caller's stream --
  // the input-gradient chain -- dispatches ahead of it without the caller changing streams).
  // Returns (stream handle, least priority, greatest priority); the stream lives for the process.
  m.def("stream_create_priority", [](int device, int priority) {
    int least = 0, greatest = 0, prev = 0;
    TORCH_CHECK(hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess, "hipSetDevice failed");
    TORCH_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess, "stream priority range");
    hipStream_t s = nullptr;
    const hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    (void)hipSetDevice(prev);
    TORCH_CHECK(e == hipSuccess, "hipStreamCreateWithPriority: ", hipGetErrorString(e));
    return py::make_tuple(reinterpret_cast<int64_t>(s), least, greatest);
  });
  register_runtime(m);
  // one-shot all-reduce over IPC-mapped peer buffers (csrc/oneshot.hip)
  py::class_<tbamd::OneShotComm>(m, "OneShotComm")
      .def(py::init<int, int, int64_t, int64_t, double>(), py::arg("rank"), py::arg("world"),
           py::arg("capacity_bytes") = (int64_t)2 << 20, py::arg("chunk_bytes") = (int64_t)64 << 10,
           py::arg("timeout_s") = 600.0)
      .def("handles", [](const tbamd::OneShotComm& c) { return py::bytes(c.handles()); })
      .def("open",
           [](tbamd::OneShotComm& c, std::vector<py::bytes> all) {
             std::vector<std::string> v;
             for (auto& b : all) v.emplace_back(std::string(b));
             c.open(v);
           })
      .def("allreduce",
           [](tbamd::OneShotComm& c, const Tensor& in, Tensor& out, double scale) {
             TORCH_CHECK(in.is_cuda() && out.is_cuda() && in.is_contiguous() && out.is_contiguous(),
                         "oneshot allreduce: contiguous device tensors");
             TORCH_CHECK(in.numel() == out.numel() && in.scalar_type() == out.scalar_type(),
                         "oneshot allreduce: in / out mismatch");
             const at::DeviceGuard guard(in.device());
             c.allreduce(in.data_ptr(), out.data_ptr(), in.numel(), dt_code(in), (float)scale, cur_stream());
           },
           py::arg("input"), py::arg("output"), py::arg("scale") = 1.0)
      .def("error", &tbamd::OneShotComm::error)
      .def_property_readonly("capacity", &tbamd::OneShotComm::capacity);
}
