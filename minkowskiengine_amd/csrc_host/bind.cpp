// pybind11 module of the native host layer: the names, argument order and argument meaning of the reference's
// `MinkowskiEngineBackend._C` (pybind/extern.hpp:515-838) for the hot path, plus torch::autograd functions so that a
// training step's backward pass runs without entering Python (the reference's autograd Functions are Python,
// MinkowskiConvolution.py:42-121; this is where its per-layer host time goes).
#include <torch/csrc/autograd/custom_function.h>

#include <set>
#include <sstream>

#include "host.hpp"

namespace py = pybind11;
using namespace meh;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

namespace {

int to_int(const py::object &o) { return py::cast<int>(py::int_(o)); }   // pybind enums, Python IntEnums, ints

KeyT keyt(const CoordinateMapKey *k) { return k->get(); }

// the `offset` argument of an operator: the [K, D] list of a RegionType.CUSTOM layer (an integer tensor of any dtype, on
// any device); the built-in regions do not read it
ivec region_offsets(const py::object &offset, int region_type, const ivec &kernel_size) {
  if (region_type != ME_REGION_CUSTOM || offset.is_none()) return ivec();
  return offsets_of(py::cast<Tensor>(offset), (int64_t)kernel_size.size());
}

CoordinateMapKey *new_key(const KeyT &k) { return new CoordinateMapKey(k.first, k.second); }

// ---- autograd: convolution ----------------------------------------------------------------------------------------------------
struct KmHolder : torch::CustomClassHolder {
  std::shared_ptr<KernelMap> km;
  explicit KmHolder(std::shared_ptr<KernelMap> k) : km(std::move(k)) {}
};

struct ConvFn : public torch::autograd::Function<ConvFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &in_feat_, const Tensor &kernel,
                        const std::shared_ptr<KernelMap> &km) {
    Tensor in_feat = in_feat_.contiguous();
    ctx->save_for_backward({in_feat, kernel});
    ctx->saved_data["km"] = c10::IValue::make_capsule(c10::make_intrusive<KmHolder>(km));
    return conv_forward_km(in_feat, kernel, *km);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grad_outputs) {
    auto saved = ctx->get_saved_variables();
    auto holder = c10::static_intrusive_pointer_cast<KmHolder>(ctx->saved_data["km"].toCapsule());
    Tensor gy = grad_outputs[0].contiguous();
    auto r = conv_backward_km(saved[0], gy, saved[1], *holder->km, ctx->needs_input_grad(0));
    return {r.first, r.second, Tensor()};
  }
};

Tensor conv_autograd(const Tensor &in_feat, const Tensor &kernel, const ivec &kernel_size, const ivec &kernel_stride,
                     const ivec &kernel_dilation, const py::object &region_type, bool expand_coordinates,
                     CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *manager, bool transpose,
                     const py::object &offset) {
  auto km = prepare_conv(in_feat, kernel, kernel_size, kernel_stride, kernel_dilation, to_int(region_type),
                         expand_coordinates, in_key, out_key, manager, transpose,
                         region_offsets(offset, to_int(region_type), kernel_size));
  return ConvFn::apply(in_feat, kernel, km);
}

// ---- autograd: training-mode batch norm (+ residual add + ReLU) -------------------------------------------------------------------
struct BnFn : public torch::autograd::Function<BnFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &x_, const c10::optional<Tensor> &skip_o,
                        const c10::optional<Tensor> &weight_o, const c10::optional<Tensor> &bias_o,
                        const c10::optional<Tensor> &rm_o, const c10::optional<Tensor> &rv_o, double momentum, double eps,
                        bool relu, const c10::optional<Tensor> &nbt_o) {
    const Tensor skip_ = skip_o.value_or(Tensor()), weight = weight_o.value_or(Tensor()), bias = bias_o.value_or(Tensor());
    const Tensor running_mean = rm_o.value_or(Tensor()), running_var = rv_o.value_or(Tensor());
    const Tensor num_batches_tracked = nbt_o.value_or(Tensor());
    Tensor x = x_.contiguous();
    Tensor skip = skip_.defined() ? skip_.contiguous() : Tensor();
    Tensor w32 = weight.defined() ? weight.to(at::kFloat) : Tensor();
    Tensor b32 = bias.defined() ? bias.to(at::kFloat) : Tensor();
    auto st = bn_stats(x, eps, momentum, running_mean, running_var, num_batches_tracked);
    Tensor y = bn_apply(x, st.first, st.second, w32, b32, relu, skip);
    const bool residual = skip.defined();
    ctx->save_for_backward({x, (residual && relu) ? y : Tensor(), st.first, st.second, w32, b32});
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["residual"] = residual;
    ctx->saved_data["wdtype"] = weight.defined() ? (int64_t)weight.scalar_type() : (int64_t)-1;
    ctx->saved_data["has_bias"] = bias.defined();
    return y;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grad_outputs) {
    auto s = ctx->get_saved_variables();
    const bool relu = ctx->saved_data["relu"].toBool(), residual = ctx->saved_data["residual"].toBool();
    auto r = bn_backward(s[0], grad_outputs[0], s[1], s[2], s[3], s[4], s[5], relu, residual,
                         residual && ctx->needs_input_grad(1));
    const int64_t wd = ctx->saved_data["wdtype"].toInt();
    Tensor gw = wd >= 0 ? std::get<2>(r).to((at::ScalarType)wd) : Tensor();
    Tensor gb = ctx->saved_data["has_bias"].toBool() ? std::get<3>(r).to((at::ScalarType)wd) : Tensor();
    return {std::get<0>(r), std::get<1>(r), gw, gb, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// window_size / shift of window attention: an int (all axes) or one int per spatial axis
ivec axes_arg(const py::object &o) {
  if (py::isinstance<py::int_>(o)) return ivec{py::cast<int32_t>(o)};
  return py::cast<ivec>(o);
}
// unit of rotary position embedding: None (empty: the tensor stride of the map), an int or one int per spatial axis
ivec unit_arg(const py::object &o) {
  if (o.is_none()) return ivec{};
  const ivec v = axes_arg(o);
  if (v.empty()) throw std::invalid_argument("unit must be None, an int or one int per spatial axis, got no value");
  return v;
}
Tensor opt_tensor(const py::object &o) { return o.is_none() ? Tensor() : py::cast<Tensor>(o); }
c10::optional<Tensor> opt_opt(const py::object &o) {
  return o.is_none() ? c10::optional<Tensor>() : c10::optional<Tensor>(py::cast<Tensor>(o));
}

Tensor batch_norm_train(const Tensor &x, const py::object &skip, const py::object &weight, const py::object &bias,
                        const py::object &running_mean, const py::object &running_var, double momentum, double eps,
                        bool relu, const py::object &num_batches_tracked) {
  return BnFn::apply(x, opt_opt(skip), opt_opt(weight), opt_opt(bias), opt_opt(running_mean), opt_opt(running_var),
                     momentum, eps, relu, opt_opt(num_batches_tracked));
}

py::object opt_out(const Tensor &t) { return t.defined() ? py::cast(t) : py::none(); }
// the activation of ConditionalGroupNorm{Forward,Backward}GPU: None -> 0 (identity), "silu" -> 1 (me_gnorm_cond_*'s act)
int gnorm_cond_act(const py::object &o) {
  if (o.is_none()) return 0;
  if (py::isinstance<py::str>(o) && py::cast<std::string>(o) == "silu") return 1;
  throw std::runtime_error("activation must be None or 'silu', not " + py::cast<std::string>(py::repr(o)));
}

// enums of pybind/extern.hpp:669-741
enum GPUMemoryAllocatorType { PYTORCH = 0, CUDA = 1 };
enum CUDAKernelMapMode { KM_MEMORY_EFFICIENT = 0, KM_SPEED_OPTIMIZED = 1 };
enum MinkowskiAlgorithm { DEFAULT = 0, MEMORY_EFFICIENT = 1, SPEED_OPTIMIZED = 2 };
enum CoordinateMapType { MAP_CPU = 0, MAP_CUDA = 1 };
enum RegionType { HYPER_CUBE = 0, HYPER_CROSS = 1, CUSTOM = 2 };
enum PoolingMode {
    LOCAL_SUM_POOLING = 0, LOCAL_AVG_POOLING, LOCAL_MAX_POOLING, GLOBAL_SUM_POOLING_DEFAULT, GLOBAL_AVG_POOLING_DEFAULT,
    GLOBAL_MAX_POOLING_DEFAULT, GLOBAL_SUM_POOLING_KERNEL, GLOBAL_AVG_POOLING_KERNEL, GLOBAL_MAX_POOLING_KERNEL,
    GLOBAL_SUM_POOLING_PYTORCH_INDEX, GLOBAL_AVG_POOLING_PYTORCH_INDEX, GLOBAL_MAX_POOLING_PYTORCH_INDEX
  };
enum BroadcastMode { ELEMENTWISE_ADDITON = 0, ELEMENTWISE_MULTIPLICATION = 1 };
enum ConvolutionMode { CONV_DEFAULT = 0, DIRECT_GEMM = 1, COPY_GEMM = 2 };

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native operator module (MinkowskiEngineBackend._C for the sparse-convolution hot path)";
  m.attr("_host") = "native";

  // ---- enums (pybind/extern.hpp:669-741) ----
  py::enum_<GPUMemoryAllocatorType>(m, "GPUMemoryAllocatorType").value("PYTORCH", PYTORCH).value("CUDA", CUDA);
  py::enum_<CUDAKernelMapMode>(m, "CUDAKernelMapMode")
      .value("MEMORY_EFFICIENT", KM_MEMORY_EFFICIENT)
      .value("SPEED_OPTIMIZED", KM_SPEED_OPTIMIZED);
  py::enum_<MinkowskiAlgorithm>(m, "MinkowskiAlgorithm")
      .value("DEFAULT", DEFAULT)
      .value("MEMORY_EFFICIENT", MEMORY_EFFICIENT)
      .value("SPEED_OPTIMIZED", SPEED_OPTIMIZED);
  py::enum_<CoordinateMapType>(m, "CoordinateMapType").value("CPU", MAP_CPU).value("CUDA", MAP_CUDA);
  py::enum_<RegionType>(m, "RegionType").value("HYPER_CUBE", HYPER_CUBE).value("HYPER_CROSS", HYPER_CROSS).value("CUSTOM", CUSTOM);
  py::enum_<PoolingMode>(m, "PoolingMode")
      .value("LOCAL_SUM_POOLING", LOCAL_SUM_POOLING)
      .value("LOCAL_AVG_POOLING", LOCAL_AVG_POOLING)
      .value("LOCAL_MAX_POOLING", LOCAL_MAX_POOLING)
      .value("GLOBAL_SUM_POOLING_DEFAULT", GLOBAL_SUM_POOLING_DEFAULT)
      .value("GLOBAL_AVG_POOLING_DEFAULT", GLOBAL_AVG_POOLING_DEFAULT)
      .value("GLOBAL_MAX_POOLING_DEFAULT", GLOBAL_MAX_POOLING_DEFAULT)
      .value("GLOBAL_SUM_POOLING_KERNEL", GLOBAL_SUM_POOLING_KERNEL)
      .value("GLOBAL_AVG_POOLING_KERNEL", GLOBAL_AVG_POOLING_KERNEL)
      .value("GLOBAL_MAX_POOLING_KERNEL", GLOBAL_MAX_POOLING_KERNEL)
      .value("GLOBAL_SUM_POOLING_PYTORCH_INDEX", GLOBAL_SUM_POOLING_PYTORCH_INDEX)
      .value("GLOBAL_AVG_POOLING_PYTORCH_INDEX", GLOBAL_AVG_POOLING_PYTORCH_INDEX)
      .value("GLOBAL_MAX_POOLING_PYTORCH_INDEX", GLOBAL_MAX_POOLING_PYTORCH_INDEX);
  py::enum_<BroadcastMode>(m, "BroadcastMode")
      .value("ELEMENTWISE_ADDITON", ELEMENTWISE_ADDITON)
      .value("ELEMENTWISE_MULTIPLICATION", ELEMENTWISE_MULTIPLICATION);
  py::enum_<ConvolutionMode>(m, "ConvolutionMode")
      .value("DEFAULT", CONV_DEFAULT)
      .value("DIRECT_GEMM", DIRECT_GEMM)
      .value("COPY_GEMM", COPY_GEMM);

  m.def("conv_bn_stats_hint", &conv_bn_stats_hint, py::arg("flag"));
  m.def("set_conv_bn_stats", &set_conv_bn_stats, py::arg("enabled"));
  m.def("invalidate_packed_weights", &invalidate_packed_weights);
  m.def("invalidate_packed_weights_for", &invalidate_packed_weights_for, py::arg("sorted_ptrs"));
  m.def("invalidate_packed_weights_in", &invalidate_packed_weights_in, py::arg("begins"), py::arg("ends"));
  m.def("set_grad_destination", [](const Tensor &param, const py::object &dest) { set_grad_destination(param, opt_tensor(dest)); });
  m.def("clear_grad_destinations", &clear_grad_destinations);
  m.def("debug_fail_next_plan_batch", &debug_fail_next_plan_batch);
  m.def("arm_grad_destinations", &arm_grad_destinations);
  m.def("arm_grad_destinations_for", &arm_grad_destinations_for);
  m.def("drop_grad_destinations", &drop_grad_destinations);
  m.def("set_policy", &Policy::set, "integer policies of the native host by name (tests, tuning scripts)");
  m.def("timing_enable", &timing_enable);
  m.def("timing_records", &timing_records, py::arg("clear") = true);
  m.def("is_cuda_available", [] { return true; });
  m.def("cuda_version", [] { return -1; });
  m.def("cudart_version", [] { return -1; });
  m.def("get_gpu_memory_info", [] {
    py::object mem = py::module_::import("torch").attr("cuda").attr("mem_get_info")();
    return mem;
  });

  // ---- CoordinateMapKey (pybind/extern.hpp:744-764) ----
  py::class_<CoordinateMapKey>(m, "CoordinateMapKey")
      .def(py::init<int>())
      .def(py::init<ivec, std::string>(), py::arg("tensor_stride"), py::arg("string_id") = "")
      .def("get_coordinate_size", [](const CoordinateMapKey &k) { return k.coordinate_size; })
      .def("is_key_set", [](const CoordinateMapKey &k) { return k.key_set; })
      .def("set_key", [](CoordinateMapKey &k, const ivec &ts, const std::string &sid) { k.set_key(ts, sid); })
      .def("set_key", [](CoordinateMapKey &k, const std::pair<ivec, std::string> &p) { k.set_key(p.first, p.second); })
      .def("get_key", [](const CoordinateMapKey &k) { return std::make_pair(k.get().first, k.get().second); })
      .def("get_tensor_stride", [](const CoordinateMapKey &k) { return k.get().first; })
      .def("__eq__", [](const CoordinateMapKey &a, const py::object &b) {
        if (!py::isinstance<CoordinateMapKey>(b)) return false;
        return a.equals(py::cast<const CoordinateMapKey &>(b));
      })
      .def("__hash__", [](const CoordinateMapKey &k) {
        const KeyT &kk = k.get();
        size_t h = std::hash<std::string>()(kk.second);
        for (int v : kk.first) h = h * 1000003u + (size_t)v;
        return (int64_t)(h & 0x7fffffffffffffffull);
      })
      .def("__repr__", &CoordinateMapKey::repr);

  // ---- CoordinateMapManager (pybind/extern.hpp:767-806) ----
  auto mgr = py::class_<CoordinateMapManager>(m, "CoordinateMapManagerGPU_c10");
  mgr.def(py::init([](const py::object &algorithm, int num_threads) {
            return new CoordinateMapManager(algorithm.is_none() ? 0 : to_int(algorithm), num_threads);
          }),
          py::arg("algorithm") = py::none(), py::arg("num_threads") = 0)
      .def("exists", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return k->key_set && s.exists(k->key); })
      .def("insert_and_map",
           [](CoordinateMapManager &s, const Tensor &coords, const ivec &ts, const std::string &sid) {
             auto r = [&] {
               py::gil_scoped_release nogil;   // (see prefetch)
               return s.insert_and_map(coords, ts, sid);
             }();
             return py::make_tuple(py::cast(new_key(std::get<0>(r)), py::return_value_policy::take_ownership),
                                   py::make_tuple(std::get<1>(r), std::get<2>(r)));
           },
           py::arg("coordinates"), py::arg("tensor_stride"), py::arg("string_id") = "")
      .def("stride",
           [](CoordinateMapManager &s, const CoordinateMapKey *k, const ivec &stride, const std::string &sid) {
             return new_key(s.stride(keyt(k), stride, sid));
           },
           py::arg("in_key"), py::arg("kernel_stride"), py::arg("string_id") = "", py::return_value_policy::take_ownership)
      .def("stride_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *a, const CoordinateMapKey *b) {
             auto r = s.stride_map(keyt(a), keyt(b));
             return py::make_tuple(r.first, r.second);
           })
      .def("origin", [](CoordinateMapManager &s) { return new_key(s.origin()); }, py::return_value_policy::take_ownership)
      .def("origin_map_size",
           [](CoordinateMapManager &s) { return s.get(s.maps.empty() ? s.origin_field(nullptr) : s.origin())->n; })
      // origin map of fields (pybind/extern.hpp:791, 801): the key origin() uses, built from a field when absent
      .def("origin_field",
           [](CoordinateMapManager &s, const py::object &field_key) {
             if (field_key.is_none()) return new_key(s.origin_field(nullptr));
             const KeyT k = keyt(field_key.cast<const CoordinateMapKey *>());
             return new_key(s.origin_field(&k));
           },
           py::arg("field_key") = py::none(), py::return_value_policy::take_ownership)
      .def("origin_field_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *k) {
             Tensor rows = s.origin_field_rows(keyt(k));
             py::dict d;
             d[py::int_(0)] = at::stack({at::arange(rows.numel(), rows.options()), rows});
             return d;
           })
      .def("_origin_field_rows",
           [](CoordinateMapManager &s, const CoordinateMapKey *k) { return s.origin_field_rows(keyt(k)); })
      .def("exists_field", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return k->key_set && s.exists_field(k->key); })
      .def("origin_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *k) {
             Tensor rows = s.origin_rows(keyt(k));
             py::dict d;
             d[py::int_(0)] = at::stack({at::arange(rows.numel(), rows.options()), rows});
             return d;
           })
      .def("_origin_rows", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return s.origin_rows(keyt(k)); })
      .def("_instance_rows",
           [](CoordinateMapManager &s, const CoordinateMapKey *k) {
             const auto &r = s.instance_rows(keyt(k));
             return py::make_tuple(r.first, r.second);
           })
      .def("_patch_rows",
           [](CoordinateMapManager &s, const CoordinateMapKey *k, int64_t patch_size, const std::string &order) {
             const auto &r = s.patch_rows(keyt(k), patch_size, serial_order_code(order));
             return py::make_tuple(r[0], r[1], r[2], r[3]);
           })
      .def("_window_rows",
           [](CoordinateMapManager &s, const CoordinateMapKey *k, const py::object &window_size, const py::object &shift) {
             const auto &r = s.window_rows(keyt(k), axes_arg(window_size), axes_arg(shift));
             return py::make_tuple(r[0], r[1], r[2], r[3]);
           },
           py::arg("key"), py::arg("window_size"), py::arg("shift") = py::int_(0))
      .def("_rope_table",
           [](CoordinateMapManager &s, const CoordinateMapKey *k, int64_t d, double base, const py::object &unit,
              bool f64) { return s.rope_table(keyt(k), d, base, unit_arg(unit), f64); },
           py::arg("key"), py::arg("d"), py::arg("base") = 10000.0, py::arg("unit") = py::none(), py::arg("f64") = false)
      .def("_context_rows",
           [](CoordinateMapManager &s, int64_t n_batch, int64_t tokens, const py::object &device,
              const py::object &lengths) {
             const c10::Device dev = py::cast<c10::Device>(py::module_::import("torch").attr("device")(device));
             const auto r = s.context_rows(n_batch, tokens, dev, opt_tensor(lengths));
             return py::make_tuple(r[0], r[1], r[2]);
           },
           py::arg("n_batch"), py::arg("tokens"), py::arg("device"), py::arg("lengths") = py::none())
      .def("get_coordinates", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return s.get(keyt(k))->coords; })
      // tensor fields (pybind/extern.hpp:780-805; field.cpp)
      .def("insert_field",
           [](CoordinateMapManager &s, const Tensor &coords, const ivec &ts, const std::string &sid) {
             return new_key(s.insert_field(coords, ts, sid));
           },
           py::arg("coordinates"), py::arg("tensor_stride"), py::arg("string_id") = "",
           py::return_value_policy::take_ownership)
      .def("get_coordinate_field", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return s.field(keyt(k)); })
      .def("field_to_sparse_insert_and_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *fk, const ivec &ts, const std::string &sid) {
             auto r = s.field_to_sparse_insert_and_map(keyt(fk), ts, sid);
             return py::make_tuple(py::cast(new_key(std::get<0>(r)), py::return_value_policy::take_ownership),
                                   py::make_tuple(std::get<1>(r), std::get<2>(r)));
           },
           py::arg("field_key"), py::arg("sparse_tensor_stride"), py::arg("string_id") = "")
      .def("field_to_sparse_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *fk, const CoordinateMapKey *sk) {
             auto r = s.field_to_sparse_map(keyt(fk), keyt(sk));
             return py::make_tuple(r.first, r.second);
           })
      .def("exists_field_to_sparse",
           [](CoordinateMapManager &s, const CoordinateMapKey *fk, const CoordinateMapKey *sk) {
             const std::pair<KeyT, KeyT> k{keyt(fk), keyt(sk)};
             return s.field_maps.count(k) != 0 || s.field_lookups.count(k) != 0;
           })
      .def("get_field_to_sparse_map",   // see backend.CoordinateMapManagerGPU_c10.get_field_to_sparse_map
           [](CoordinateMapManager &s, const CoordinateMapKey *fk, const CoordinateMapKey *sk) {
             const std::pair<KeyT, KeyT> k{keyt(fk), keyt(sk)};
             auto it = s.field_maps.find(k);
             if (it != s.field_maps.end()) return py::make_tuple(it->second.first, it->second.second);
             auto jt = s.field_lookups.find(k);
             check(jt != s.field_lookups.end(), "Field To Sparse Map doesn't exist");
             return py::make_tuple(jt->second.second, jt->second.first);
           })
      .def("field_to_sparse_keys",   // in key order
           [](CoordinateMapManager &s, const CoordinateMapKey *fk) {
             const KeyT f = keyt(fk);
             std::set<KeyT> keys;
             for (const auto &kv : s.field_maps)
               if (kv.first.first == f) keys.insert(kv.first.second);
             for (const auto &kv : s.field_lookups)
               if (kv.first.first == f) keys.insert(kv.first.second);
             py::list out;
             for (const KeyT &k : keys) out.append(py::cast(new_key(k), py::return_value_policy::take_ownership));
             return out;
           })
      .def("_interpolation_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *k, const Tensor &samples) {
             auto r = s.interpolation_map(keyt(k), samples);
             return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r));
           })
      .def("interpolation_map_weight",   // (samples, key): the reference's argument order
           [](CoordinateMapManager &s, const Tensor &samples, const CoordinateMapKey *k) {
             auto r = s.interpolation_map(keyt(k), samples);
             return std::vector<Tensor>{std::get<0>(r), std::get<1>(r), std::get<2>(r)};
           })
      .def("size", [](CoordinateMapManager &s, const CoordinateMapKey *k) { return s.get(keyt(k))->n; })
      .def("get_random_string_id",
           [](CoordinateMapManager &s, const ivec &ts, const std::string &sid) {
             KeyT k = s.random_string_id(ts, sid);
             return std::make_pair(k.first, k.second);
           })
      .def("get_coordinate_map_keys",
           [](CoordinateMapManager &s, const ivec &ts) {
             py::list out;
             for (const KeyT &k : s.map_order)
               if (k.first == ts) out.append(py::cast(new_key(k), py::return_value_policy::take_ownership));
             return out;
           })
      .def("union_map",
           [](CoordinateMapManager &s, const std::vector<CoordinateMapKey *> &in_keys, CoordinateMapKey *out_key) {
             std::vector<KeyT> ks;
             for (auto *k : in_keys) ks.push_back(keyt(k));
             return s.union_map(ks, out_key);
           })
      .def("union_arith_maps",
           [](CoordinateMapManager &s, const CoordinateMapKey *key_a, const CoordinateMapKey *key_b) {
             const auto &r = s.union_arith_maps(keyt(key_a), keyt(key_b));
             return py::make_tuple(py::cast(new_key(r.first), py::return_value_policy::take_ownership), r.second[0],
                                   r.second[1], r.second[2], r.second[3]);
           })
      .def("prune", [](CoordinateMapManager &s, const CoordinateMapKey *k, const Tensor &keep) {
             return new_key(s.prune(keyt(k), keep));
           }, py::return_value_policy::take_ownership)
      .def("kernel_map",
           [](CoordinateMapManager &s, const CoordinateMapKey *ik, const CoordinateMapKey *ok, const ivec &ks,
              const ivec &st, const ivec &dl, const py::object &region_type, const py::object &offset,
              bool is_transpose, bool is_pool) {
             const int rt = to_int(region_type);
             return s.kernel_map(keyt(ik), keyt(ok), ks, st, dl, rt, is_transpose, is_pool, region_offsets(offset, rt, ks))
                 ->to_dict();
           })
      .def("kernel_map_pairs",    // (not in the reference) number of pairs of a cached / built kernel map
           [](CoordinateMapManager &s, const CoordinateMapKey *ik, const CoordinateMapKey *ok, const ivec &ks,
              const ivec &st, const ivec &dl, const py::object &region_type, bool is_transpose, bool is_pool) {
             return s.kernel_map(keyt(ik), keyt(ok), ks, st, dl, to_int(region_type), is_transpose, is_pool)->n_pairs();
           })
      .def("_conv_cfg",           // (bench / tests) builds the tile plan of a launch side -> (tile_rows, batch_groups)
           [](CoordinateMapManager &s, const CoordinateMapKey *ik, const CoordinateMapKey *ok, const ivec &ks,
              const ivec &st, const ivec &dl, const py::object &region_type, bool is_transpose, const std::string &target,
              int c_src, int c_dst, bool bf16) {
             auto km = s.kernel_map(keyt(ik), keyt(ok), ks, st, dl, to_int(region_type), is_transpose, false);
             const ConvCfg &c = km->conv_cfg(target, target == "out" ? km->n_out : km->n_in, c_src, c_dst, bf16);
             return py::make_tuple(c.tile_rows, c.batch_groups);
           })
      .def("recipe", [](CoordinateMapManager &s) { return s.recipe_log->snapshot(); })
      // (no GIL while the maps and plans of a scene are built: a loader thread can prepare the next scene — on its own
      // stream — while the training thread launches the current step)
      .def("prefetch", [](CoordinateMapManager &s, const std::vector<std::string> &r) { return s.prefetch(r); },
           py::call_guard<py::gil_scoped_release>())
      .def("record_stream",
           [](CoordinateMapManager &s, const py::object &stream) {
             // (torch.cuda.Stream -> c10::Stream, then no Python object and no GIL: a loader thread hands a scene's
             // ~300 map tensors to the training stream without stalling the training thread)
             const c10::Stream st = c10::Stream::unpack3(stream.attr("stream_id").cast<int64_t>(),
                                                         (c10::DeviceIndex)stream.attr("device_index").cast<int64_t>(),
                                                         (c10::DeviceType)stream.attr("device_type").cast<int64_t>());
             py::gil_scoped_release nogil;
             for (const Tensor &t : s.device_tensors()) t.record_stream(st);
           })
      .def("print_coordinate_map",   // manager_type::to_string(key): pybind/extern.hpp:777-779
           [](CoordinateMapManager &s, const CoordinateMapKey *key) {
             const KeyT &k = keyt(key);
             auto m = s.get(k);
             std::ostringstream o;
             o << "[";
             for (size_t i = 0; i < k.first.size(); ++i) o << (i ? ", " : "") << k.first[i];
             o << "]" << (k.second.empty() ? "" : ":" + k.second) << " : CoordinateMapGPU:" << m->n << "x" << m->coords.size(1);
             return o.str();
           })
      .def("__repr__", &CoordinateMapManager::repr);
  m.attr("CoordinateMapManagerGPU_default") = m.attr("CoordinateMapManagerGPU_c10");

  // ---- operators with the reference's signatures (pybind/extern.hpp:53-392, 515-646) ----
  m.def("ConvolutionForwardGPU",
        [](const Tensor &in_feat, const Tensor &kernel, const ivec &ks, const ivec &st, const ivec &dl,
           const py::object &region_type, const py::object &offset, bool expand_coordinates,
           const py::object & /*convolution_mode*/, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
           CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          auto km = prepare_conv(in_feat, kernel, ks, st, dl, rt, expand_coordinates, in_key, out_key, mgr, false,
                                 region_offsets(offset, rt, ks));
          return conv_forward_km(in_feat, kernel, *km);
        });
  m.def("ConvolutionTransposeForwardGPU",
        [](const Tensor &in_feat, const Tensor &kernel, const ivec &ks, const ivec &st, const ivec &dl,
           const py::object &region_type, const py::object &offset, bool expand_coordinates,
           const py::object & /*convolution_mode*/, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
           CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          auto km = prepare_conv(in_feat, kernel, ks, st, dl, rt, expand_coordinates, in_key, out_key, mgr, true,
                                 region_offsets(offset, rt, ks));
          return conv_forward_km(in_feat, kernel, *km);
        });
  auto conv_bwd = [](bool transpose) {
    return [transpose](const Tensor &in_feat, Tensor grad_out, const Tensor &kernel, const ivec &ks, const ivec &st,
                       const ivec &dl, const py::object &region_type, const py::object &offset,
                       const py::object & /*convolution_mode*/, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
                       CoordinateMapManager *mgr, bool need_grad_in) {
      check(in_feat.size(1) == kernel.size(1), "Input feature size and kernel size mismatch");
      check(grad_out.size(1) == kernel.size(2), "Output feature size and kernel size mismatch");
      grad_out = grad_out.contiguous();
      const int rt = to_int(region_type);
      auto km = mgr->kernel_map(in_key->get(), out_key->get(), ks, st, dl, rt, transpose, false, region_offsets(offset, rt, ks));
      check(grad_out.size(0) == km->n_out, "Invalid grad_out size");
      auto r = conv_backward_km(in_feat.contiguous(), grad_out, kernel, *km, need_grad_in);
      return py::make_tuple(opt_out(r.first), r.second);
    };
  };
  m.def("ConvolutionBackwardGPU", conv_bwd(false), py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("kernel"),
        py::arg("kernel_size"), py::arg("kernel_stride"), py::arg("kernel_dilation"), py::arg("region_type"),
        py::arg("offset"), py::arg("convolution_mode"), py::arg("in_key"), py::arg("out_key"), py::arg("manager"),
        py::arg("need_grad_in") = true);
  m.def("ConvolutionTransposeBackwardGPU", conv_bwd(true), py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("kernel"),
        py::arg("kernel_size"), py::arg("kernel_stride"), py::arg("kernel_dilation"), py::arg("region_type"),
        py::arg("offset"), py::arg("convolution_mode"), py::arg("in_key"), py::arg("out_key"), py::arg("manager"),
        py::arg("need_grad_in") = true);

  m.def("LocalPoolingForwardGPU",
        [](const Tensor &in_feat, const ivec &ks, const ivec &st, const ivec &dl, const py::object &region_type,
           const py::object &offset, const py::object &pooling_mode, CoordinateMapKey *in_key,
           CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          auto r = local_pooling_forward(in_feat, ks, st, dl, rt, to_int(pooling_mode), in_key, out_key, mgr,
                                         region_offsets(offset, rt, ks));
          return py::make_tuple(r.first, r.second);
        });
  m.def("LocalPoolingBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, const Tensor &num_nonzero, const ivec &ks, const ivec &st,
           const ivec &dl, const py::object &region_type, const py::object &offset, const py::object &pooling_mode,
           CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          return local_pooling_backward(in_feat, grad_out, num_nonzero, ks, st, dl, rt, to_int(pooling_mode), in_key,
                                        out_key, mgr, region_offsets(offset, rt, ks));
        });
  m.def("LocalPoolingTransposeForwardGPU",
        [](const Tensor &in_feat, const ivec &ks, const ivec &st, const ivec &dl, const py::object &region_type,
           const py::object &offset, bool generate_new_coordinates, const py::object &pooling_mode,
           CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          auto r = local_pooling_transpose_forward(in_feat, ks, st, dl, rt, generate_new_coordinates, to_int(pooling_mode),
                                                   in_key, out_key, mgr, region_offsets(offset, rt, ks));
          return py::make_tuple(r.first, r.second);
        });
  m.def("LocalPoolingTransposeBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, const Tensor &num_nonzero, const ivec &ks, const ivec &st,
           const ivec &dl, const py::object &region_type, const py::object &offset, const py::object &pooling_mode,
           CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          const int rt = to_int(region_type);
          return local_pooling_transpose_backward(in_feat, grad_out, num_nonzero, ks, st, dl, rt, to_int(pooling_mode),
                                                  in_key, out_key, mgr, region_offsets(offset, rt, ks));
        });
  // channelwise convolution: no reference native operator (MinkowskiChannelwiseConvolution.py runs in Python); the
  // names follow the package's <Op>{Forward,Backward}GPU convention.  The GIL is released around the map and launches.
  m.def("ChannelwiseConvolutionForwardGPU",
        [](const Tensor &in_feat, const Tensor &kernel, const py::object &bias, const ivec &ks, const ivec &st,
           const ivec &dl, const py::object &region_type, const py::object &offset, CoordinateMapKey *in_key,
           CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          const Tensor b = opt_tensor(bias);
          const int rt = to_int(region_type);
          const ivec offs = region_offsets(offset, rt, ks);
          py::gil_scoped_release nogil;
          return channelwise_forward(in_feat, kernel, b, ks, st, dl, rt, in_key, out_key, mgr, offs);
        },
        py::arg("in_feat"), py::arg("kernel"), py::arg("bias"), py::arg("kernel_size"), py::arg("kernel_stride"),
        py::arg("kernel_dilation"), py::arg("region_type"), py::arg("offset"), py::arg("in_key"), py::arg("out_key"),
        py::arg("manager"));
  m.def("ChannelwiseConvolutionBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, const Tensor &kernel, const ivec &ks, const ivec &st,
           const ivec &dl, const py::object &region_type, const py::object &offset, CoordinateMapKey *in_key,
           CoordinateMapKey *out_key, CoordinateMapManager *mgr, bool need_grad_in, bool need_grad_bias) {
          const int rt = to_int(region_type);
          const ivec offs = region_offsets(offset, rt, ks);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = channelwise_backward(in_feat, grad_out, kernel, ks, st, dl, rt, in_key, out_key, mgr, need_grad_in,
                                     need_grad_bias, offs);
          }
          return py::make_tuple(opt_out(std::get<0>(r)), std::get<1>(r), opt_out(std::get<2>(r)));
        },
        py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("kernel"), py::arg("kernel_size"), py::arg("kernel_stride"),
        py::arg("kernel_dilation"), py::arg("region_type"), py::arg("offset"), py::arg("in_key"), py::arg("out_key"),
        py::arg("manager"), py::arg("need_grad_in") = true, py::arg("need_grad_bias") = true);
  // instance normalisation: no reference native operator either (its module chains global poolings and broadcasts in
  // Python, MinkowskiNormalization.py:194-399); one fused operator pair on csrc/instance_norm.hip
  m.def("InstanceNormForwardGPU",
        [](const Tensor &in_feat, const py::object &weight, const py::object &bias, double eps, CoordinateMapKey *in_key,
           CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          const Tensor w = opt_tensor(weight), b = opt_tensor(bias);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = instance_norm_forward(in_feat, w, b, eps, in_key, glob_key, mgr);
          }
          return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r));
        },
        py::arg("in_feat"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("in_key"), py::arg("glob_key"),
        py::arg("manager"));
  m.def("InstanceNormBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, const py::object &weight, const Tensor &mean, const Tensor &rstd,
           CoordinateMapKey *in_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr, bool need_grad_in,
           bool need_grad_weight, bool need_grad_bias) {
          const Tensor w = opt_tensor(weight);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = instance_norm_backward(in_feat, grad_out, w, mean, rstd, in_key, glob_key, mgr, need_grad_in,
                                       need_grad_weight, need_grad_bias);
          }
          return py::make_tuple(opt_out(std::get<0>(r)), opt_out(std::get<1>(r)), opt_out(std::get<2>(r)));
        },
        py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("weight"), py::arg("mean"), py::arg("rstd"),
        py::arg("in_key"), py::arg("glob_key"), py::arg("manager"), py::arg("need_grad_in") = true,
        py::arg("need_grad_weight") = true, py::arg("need_grad_bias") = true);
  // group normalisation: torch.nn.GroupNorm's arithmetic per instance of a sparse tensor (no reference operator); one
  // fused operator pair on csrc/group_norm.hip
  m.def("GroupNormForwardGPU",
        [](const Tensor &in_feat, int64_t num_groups, const py::object &weight, const py::object &bias, double eps,
           CoordinateMapKey *in_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          const Tensor w = opt_tensor(weight), b = opt_tensor(bias);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = group_norm_forward(in_feat, num_groups, w, b, eps, in_key, glob_key, mgr);
          }
          return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r));
        },
        py::arg("in_feat"), py::arg("num_groups"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("in_key"),
        py::arg("glob_key"), py::arg("manager"));
  m.def("GroupNormBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, int64_t num_groups, const py::object &weight, const Tensor &mean,
           const Tensor &rstd, CoordinateMapKey *in_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr,
           bool need_grad_in, bool need_grad_weight, bool need_grad_bias) {
          const Tensor w = opt_tensor(weight);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = group_norm_backward(in_feat, grad_out, num_groups, w, mean, rstd, in_key, glob_key, mgr, need_grad_in,
                                    need_grad_weight, need_grad_bias);
          }
          return py::make_tuple(opt_out(std::get<0>(r)), opt_out(std::get<1>(r)), opt_out(std::get<2>(r)));
        },
        py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("num_groups"), py::arg("weight"), py::arg("mean"),
        py::arg("rstd"), py::arg("in_key"), py::arg("glob_key"), py::arg("manager"), py::arg("need_grad_in") = true,
        py::arg("need_grad_weight") = true, py::arg("need_grad_bias") = true);
  // conditional group normalisation: group norm with a per-instance scale / shift and an optional fused SiLU
  // (activation: None or "silu"), on the k_gnc_* kernels of csrc/group_norm.hip
  m.def("ConditionalGroupNormForwardGPU",
        [](const Tensor &in_feat, int64_t num_groups, const py::object &weight, const py::object &bias,
           const py::object &scale, const py::object &shift, const py::object &activation, double eps,
           CoordinateMapKey *in_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          const Tensor w = opt_tensor(weight), b = opt_tensor(bias), sc = opt_tensor(scale), sh = opt_tensor(shift);
          const int act = gnorm_cond_act(activation);
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = cond_group_norm_forward(in_feat, num_groups, w, b, sc, sh, act, eps, in_key, glob_key, mgr);
          }
          return py::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r));
        },
        py::arg("in_feat"), py::arg("num_groups"), py::arg("weight"), py::arg("bias"), py::arg("scale"), py::arg("shift"),
        py::arg("activation"), py::arg("eps"), py::arg("in_key"), py::arg("glob_key"), py::arg("manager"));
  m.def("ConditionalGroupNormBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, int64_t num_groups, const py::object &weight,
           const py::object &bias, const py::object &scale, const py::object &shift, const py::object &activation,
           const Tensor &mean, const Tensor &rstd, CoordinateMapKey *in_key, CoordinateMapKey *glob_key,
           CoordinateMapManager *mgr, bool need_grad_in, bool need_grad_weight, bool need_grad_bias, bool need_grad_scale,
           bool need_grad_shift) {
          const Tensor w = opt_tensor(weight), b = opt_tensor(bias), sc = opt_tensor(scale), sh = opt_tensor(shift);
          const int act = gnorm_cond_act(activation);
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = cond_group_norm_backward(in_feat, grad_out, num_groups, w, b, sc, sh, act, mean, rstd, in_key, glob_key, mgr,
                                         need_grad_in, need_grad_weight, need_grad_bias, need_grad_scale, need_grad_shift);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]), opt_out(r[3]), opt_out(r[4]));
        },
        py::arg("in_feat"), py::arg("grad_out_feat"), py::arg("num_groups"), py::arg("weight"), py::arg("bias"),
        py::arg("scale"), py::arg("shift"), py::arg("activation"), py::arg("mean"), py::arg("rstd"), py::arg("in_key"),
        py::arg("glob_key"), py::arg("manager"), py::arg("need_grad_in") = true, py::arg("need_grad_weight") = true,
        py::arg("need_grad_bias") = true, py::arg("need_grad_scale") = true, py::arg("need_grad_shift") = true);
  // per-instance multi-head attention on the kernels of csrc/attention.hip (strided row views go in without copies)
  m.def("AttentionForwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, int64_t num_heads, double scale, CoordinateMapKey *q_key,
           CoordinateMapKey *kv_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = attention_forward(q, k, v, num_heads, scale, q_key, kv_key, glob_key, mgr);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("num_heads"), py::arg("scale"), py::arg("q_key"),
        py::arg("kv_key"), py::arg("glob_key"), py::arg("manager"));
  m.def("AttentionBackwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse, const Tensor &grad_out,
           int64_t num_heads, double scale, CoordinateMapKey *q_key, CoordinateMapKey *kv_key, CoordinateMapKey *glob_key,
           CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k, bool need_grad_v) {
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = attention_backward(q, k, v, out, lse, grad_out, num_heads, scale, q_key, kv_key, glob_key, mgr, need_grad_q,
                                   need_grad_k, need_grad_v);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("grad_out"),
        py::arg("num_heads"), py::arg("scale"), py::arg("q_key"), py::arg("kv_key"), py::arg("glob_key"),
        py::arg("manager"), py::arg("need_grad_q") = true, py::arg("need_grad_k") = true, py::arg("need_grad_v") = true);
  // cross-attention to a dense context: the attention kernels on the context row lists, dK / dV split over the queries
  m.def("CrossAttentionForwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const py::object &context_lengths, int64_t num_heads,
           double scale, CoordinateMapKey *q_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          const Tensor len = opt_tensor(context_lengths);
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = cross_attention_forward(q, k, v, len, num_heads, scale, q_key, glob_key, mgr);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("context_lengths"), py::arg("num_heads"), py::arg("scale"),
        py::arg("q_key"), py::arg("glob_key"), py::arg("manager"));
  m.def("CrossAttentionBackwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const py::object &context_lengths, const Tensor &out,
           const Tensor &lse, const Tensor &grad_out, int64_t num_heads, double scale, CoordinateMapKey *q_key,
           CoordinateMapKey *glob_key, CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k, bool need_grad_v,
           const py::object &kv_splits) {
          const Tensor len = opt_tensor(context_lengths);
          const int64_t splits = kv_splits.is_none() ? 0 : kv_splits.cast<int64_t>();
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = cross_attention_backward(q, k, v, len, out, lse, grad_out, num_heads, scale, q_key, glob_key, mgr,
                                         need_grad_q, need_grad_k, need_grad_v, splits);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("context_lengths"), py::arg("out"), py::arg("lse"),
        py::arg("grad_out"), py::arg("num_heads"), py::arg("scale"), py::arg("q_key"), py::arg("glob_key"),
        py::arg("manager"), py::arg("need_grad_q") = true, py::arg("need_grad_k") = true, py::arg("need_grad_v") = true,
        py::arg("kv_splits") = py::none());
  // local attention over a kernel map on the kernels of csrc/local_attention.hip (strided row views go in without copies)
  m.def("LocalAttentionForwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const py::object &rel_pos_bias, int64_t num_heads,
           double scale, const ivec &ks, const ivec &st, const ivec &dl, const py::object &region_type,
           const py::object &offset, CoordinateMapKey *q_key, CoordinateMapKey *kv_key, CoordinateMapManager *mgr) {
          const Tensor b = opt_tensor(rel_pos_bias);
          const int rt = to_int(region_type);
          const ivec offs = region_offsets(offset, rt, ks);
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = local_attention_forward(q, k, v, b, num_heads, scale, ks, st, dl, rt, q_key, kv_key, mgr, offs);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("rel_pos_bias"), py::arg("num_heads"), py::arg("scale"),
        py::arg("kernel_size"), py::arg("kernel_stride"), py::arg("kernel_dilation"), py::arg("region_type"),
        py::arg("offset"), py::arg("q_key"), py::arg("kv_key"), py::arg("manager"));
  m.def("LocalAttentionBackwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const py::object &rel_pos_bias, const Tensor &out,
           const Tensor &lse, const Tensor &grad_out, int64_t num_heads, double scale, const ivec &ks, const ivec &st,
           const ivec &dl, const py::object &region_type, const py::object &offset, CoordinateMapKey *q_key,
           CoordinateMapKey *kv_key, CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k, bool need_grad_v,
           bool need_grad_bias) {
          const Tensor b = opt_tensor(rel_pos_bias);
          const int rt = to_int(region_type);
          const ivec offs = region_offsets(offset, rt, ks);
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = local_attention_backward(q, k, v, b, out, lse, grad_out, num_heads, scale, ks, st, dl, rt, q_key, kv_key,
                                         mgr, offs, need_grad_q, need_grad_k, need_grad_v, need_grad_bias);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]), opt_out(r[3]));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("rel_pos_bias"), py::arg("out"), py::arg("lse"),
        py::arg("grad_out"), py::arg("num_heads"), py::arg("scale"), py::arg("kernel_size"), py::arg("kernel_stride"),
        py::arg("kernel_dilation"), py::arg("region_type"), py::arg("offset"), py::arg("q_key"), py::arg("kv_key"),
        py::arg("manager"), py::arg("need_grad_q") = true, py::arg("need_grad_k") = true, py::arg("need_grad_v") = true,
        py::arg("need_grad_bias") = true);
  // serialized patch attention: the attention kernels on the patch lists and block table of csrc/serial_attention.hip
  m.def("SerializedAttentionForwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, int64_t num_heads, double scale, int64_t patch_size,
           const std::string &order, CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = serialized_attention_forward(q, k, v, num_heads, scale, patch_size, order, in_key, mgr);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("num_heads"), py::arg("scale"), py::arg("patch_size"),
        py::arg("order"), py::arg("in_key"), py::arg("manager"));
  m.def("SerializedAttentionBackwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse, const Tensor &grad_out,
           int64_t num_heads, double scale, int64_t patch_size, const std::string &order, CoordinateMapKey *in_key,
           CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k, bool need_grad_v) {
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = serialized_attention_backward(q, k, v, out, lse, grad_out, num_heads, scale, patch_size, order, in_key, mgr,
                                              need_grad_q, need_grad_k, need_grad_v);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("grad_out"),
        py::arg("num_heads"), py::arg("scale"), py::arg("patch_size"), py::arg("order"), py::arg("in_key"),
        py::arg("manager"), py::arg("need_grad_q") = true, py::arg("need_grad_k") = true, py::arg("need_grad_v") = true);
  // shifted-window attention: the attention kernels on the window lists and block table of csrc/serial_attention.hip
  m.def("WindowAttentionForwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, int64_t num_heads, double scale, const py::object &window_size,
           const py::object &shift, CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
          const ivec ws = axes_arg(window_size), sh = axes_arg(shift);
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = window_attention_forward(q, k, v, num_heads, scale, ws, sh, in_key, mgr);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("num_heads"), py::arg("scale"), py::arg("window_size"),
        py::arg("shift"), py::arg("in_key"), py::arg("manager"));
  m.def("WindowAttentionBackwardGPU",
        [](const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &out, const Tensor &lse, const Tensor &grad_out,
           int64_t num_heads, double scale, const py::object &window_size, const py::object &shift,
           CoordinateMapKey *in_key, CoordinateMapManager *mgr, bool need_grad_q, bool need_grad_k, bool need_grad_v) {
          const ivec ws = axes_arg(window_size), sh = axes_arg(shift);
          std::vector<Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = window_attention_backward(q, k, v, out, lse, grad_out, num_heads, scale, ws, sh, in_key, mgr, need_grad_q,
                                          need_grad_k, need_grad_v);
          }
          return py::make_tuple(opt_out(r[0]), opt_out(r[1]), opt_out(r[2]));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("grad_out"),
        py::arg("num_heads"), py::arg("scale"), py::arg("window_size"), py::arg("shift"), py::arg("in_key"),
        py::arg("manager"), py::arg("need_grad_q") = true, py::arg("need_grad_k") = true, py::arg("need_grad_v") = true);
  // rotary position embedding from voxel coordinates: csrc/rope.hip on the manager's table
  m.def("RotaryEmbeddingForwardGPU",
        [](const Tensor &x, int64_t num_heads, double base, const py::object &unit, CoordinateMapKey *in_key,
           CoordinateMapManager *mgr) {
          const ivec u = unit_arg(unit);
          py::gil_scoped_release nogil;
          return rotary_embedding_forward(x, num_heads, base, u, in_key, mgr);
        },
        py::arg("x"), py::arg("num_heads"), py::arg("base"), py::arg("unit"), py::arg("in_key"), py::arg("manager"));
  m.def("RotaryEmbeddingBackwardGPU",
        [](const Tensor &grad_out, int64_t num_heads, double base, const py::object &unit, CoordinateMapKey *in_key,
           CoordinateMapManager *mgr) {
          const ivec u = unit_arg(unit);
          py::gil_scoped_release nogil;
          return rotary_embedding_backward(grad_out, num_heads, base, u, in_key, mgr);
        },
        py::arg("grad_out"), py::arg("num_heads"), py::arg("base"), py::arg("unit"), py::arg("in_key"),
        py::arg("manager"));
  // tensor fields (field.cpp): the reference's InterpolationForwardGPU / InterpolationBackwardGPU and coo_spmm_int32 /
  // coo_spmm_average_int32 (pybind/extern.hpp:497-506), plus the CSR building blocks the autograd functions cache
  m.def("CsrFromCooGPU",
        [](const Tensor &keys, int64_t n_rows, const py::object &cols, const py::object &vals) {
          auto r = csr_from_coo(keys, n_rows, opt_tensor(cols), opt_tensor(vals));
          return py::make_tuple(std::get<0>(r), std::get<1>(r), opt_out(std::get<2>(r)));
        },
        py::arg("keys"), py::arg("n_rows"), py::arg("cols") = py::none(), py::arg("vals") = py::none());
  m.def("CsrGatherGPU",
        [](const Tensor &x, const Tensor &rowptr, const Tensor &col, const py::object &w, const py::object &scale) {
          return csr_gather(x, rowptr, col, opt_tensor(w), opt_tensor(scale));
        },
        py::arg("x"), py::arg("rowptr"), py::arg("col"), py::arg("w") = py::none(), py::arg("scale") = py::none());
  m.def("InterpolationForwardGPU",
        [](const Tensor &in_feat, const Tensor &tfield, const CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
          return interpolation_forward(in_feat, tfield, keyt(in_key), mgr);
        });
  m.def("InterpolationBackwardGPU",
        [](const Tensor &grad_out, const Tensor &in_map, const Tensor &out_map, const Tensor &weights,
           const CoordinateMapKey *in_key, CoordinateMapManager *mgr) {
          return interpolation_backward(grad_out, in_map, out_map, weights, keyt(in_key), mgr);
        });
  m.def("coo_spmm_int32",
        [](const Tensor &rows, const Tensor &cols, const Tensor &vals, int64_t dim_i, int64_t dim_j, const Tensor &mat2,
           int64_t /*spmm_algorithm_id*/, bool /*is_sorted*/) { return coo_spmm(rows, cols, vals, dim_i, dim_j, mat2); },
        py::arg("rows"), py::arg("cols"), py::arg("vals"), py::arg("dim_i"), py::arg("dim_j"), py::arg("mat2"),
        py::arg("spmm_algorithm_id") = 1, py::arg("is_sorted") = false);
  m.def("coo_spmm_average_int32",
        [](const Tensor &rows, const Tensor &cols, int64_t dim_i, int64_t dim_j, const Tensor &mat2,
           int64_t /*spmm_algorithm_id*/) { return coo_spmm_average(rows, cols, dim_i, dim_j, mat2); },
        py::arg("rows"), py::arg("cols"), py::arg("dim_i"), py::arg("dim_j"), py::arg("mat2"),
        py::arg("spmm_algorithm_id") = 1);
  // direct max pooling (pybind/extern.hpp:654-656)
  m.def("direct_max_pool_fw",
        [](const Tensor &in_map, const Tensor &out_map, const Tensor &in_feat, int64_t out_nrows, bool is_sorted) {
          auto r = direct_max_pool_fw(in_map, out_map, in_feat, out_nrows, is_sorted);
          return py::make_tuple(r.first, r.second);
        },
        py::arg("in_map"), py::arg("out_map"), py::arg("in_feat"), py::arg("out_nrows"), py::arg("is_sorted") = false);
  m.def("direct_max_pool_bw", &direct_max_pool_bw, py::arg("grad_out_feat"), py::arg("max_index"), py::arg("in_nrows"));
  m.def("union_arith_fw", &union_arith_fw, py::arg("a_feat"), py::arg("b_feat"), py::arg("a_of_u"), py::arg("b_of_u"),
        py::arg("op"));
  m.def("union_arith_bw",
        [](const Tensor &grad_out, const Tensor &a_feat, const Tensor &b_feat, const Tensor &u_of_a, const Tensor &u_of_b,
           const Tensor &a_of_u, const Tensor &b_of_u, const std::string &op, bool need_grad_a, bool need_grad_b) {
          auto r = union_arith_bw(grad_out, a_feat, b_feat, u_of_a, u_of_b, a_of_u, b_of_u, op, need_grad_a, need_grad_b);
          return py::make_tuple(r.first.defined() ? py::cast(r.first) : py::none(),
                                r.second.defined() ? py::cast(r.second) : py::none());
        },
        py::arg("grad_out"), py::arg("a_feat"), py::arg("b_feat"), py::arg("u_of_a"), py::arg("u_of_b"), py::arg("a_of_u"),
        py::arg("b_of_u"), py::arg("op"), py::arg("need_grad_a") = true, py::arg("need_grad_b") = true);
  m.def("GlobalPoolingForwardGPU",
        [](const Tensor &in_feat, const py::object &pooling_mode, CoordinateMapKey *in_key, CoordinateMapKey *out_key,
           CoordinateMapManager *mgr) {
          auto r = global_pooling_forward(in_feat, to_int(pooling_mode), in_key, out_key, mgr);
          return py::make_tuple(r.first, r.second);
        });
  m.def("GlobalPoolingBackwardGPU",
        [](const Tensor &in_feat, const Tensor &grad_out, const Tensor &num_nonzero, const py::object &pooling_mode,
           CoordinateMapKey *in_key, CoordinateMapKey *out_key, CoordinateMapManager *mgr) {
          return global_pooling_backward(in_feat, grad_out, num_nonzero, to_int(pooling_mode), in_key, out_key, mgr);
        });
  m.def("BroadcastForwardGPU",
        [](const Tensor &in_feat, const Tensor &glob, const py::object &mode, CoordinateMapKey *in_key,
           CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          return broadcast_forward(in_feat, glob, to_int(mode), in_key, glob_key, mgr);
        });
  m.def("BroadcastBackwardGPU",
        [](const Tensor &in_feat, const Tensor &glob, const Tensor &grad_out, const py::object &mode,
           CoordinateMapKey *in_key, CoordinateMapKey *glob_key, CoordinateMapManager *mgr) {
          auto r = broadcast_backward(in_feat, glob, grad_out, to_int(mode), in_key, glob_key, mgr);
          return py::make_tuple(r.first, r.second);
        });
  // dense <-> sparse conversion (csrc/dense.hip): torch indexing in the reference's Python (MinkowskiSparseTensor.py:460-557,
  // MinkowskiOps.py:246-348), so these operator names are this package's own; the GIL is released around the launches
  m.attr("DENSE_AUTO") = 0;
  m.attr("DENSE_ROW_STATIONARY") = ME_DENSE_ROW_STATIONARY;
  m.attr("DENSE_CELL_STATIONARY") = ME_DENSE_CELL_STATIONARY;
  m.def("DensePolicy", &dense_policy, py::arg("n"), py::arg("n_cells"), py::arg("c"), py::arg("elem_bytes"),
        py::arg("to_box"));
  m.def("DenseCellIndexGPU",
        [](const Tensor &coordinates, const ivec &min_coordinate, const ivec &divisor, const std::vector<int64_t> &shape,
           bool want_grid) {
          std::tuple<Tensor, Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = dense_cell_index(coordinates, min_coordinate, divisor, shape, want_grid);
          }
          return py::make_tuple(std::get<0>(r), opt_out(std::get<1>(r)), std::get<2>(r));
        },
        py::arg("coordinates"), py::arg("min_coordinate"), py::arg("divisor"), py::arg("shape"),
        py::arg("want_grid") = true);
  m.def("DenseGridGPU",
        [](const Tensor &cell, int64_t n_cells) {
          py::gil_scoped_release nogil;
          return dense_grid(cell, n_cells);
        },
        py::arg("cell"), py::arg("n_cells"));
  m.def("DenseRowsToBoxGPU",
        [](const Tensor &rows, const py::object &cell, const py::object &grid, int64_t outer, int64_t inner,
           int64_t policy) {
          const Tensor c = opt_tensor(cell), g = opt_tensor(grid);
          py::gil_scoped_release nogil;
          return dense_rows_to_box(rows, c, g, outer, inner, policy);
        },
        py::arg("rows"), py::arg("cell"), py::arg("grid"), py::arg("outer"), py::arg("inner"), py::arg("policy") = 0);
  m.def("DenseBoxToRowsGPU",
        [](const Tensor &box, const py::object &cell, const py::object &grid, int64_t n, int64_t outer, int64_t inner,
           int64_t policy) {
          const Tensor c = opt_tensor(cell), g = opt_tensor(grid);
          py::gil_scoped_release nogil;
          return dense_box_to_rows(box, c, g, n, outer, inner, policy);
        },
        py::arg("box"), py::arg("cell"), py::arg("grid"), py::arg("n"), py::arg("outer"), py::arg("inner"),
        py::arg("policy") = 0);
  m.def("DenseOccupiedGPU",
        [](const Tensor &box, int64_t outer, int64_t inner, const std::vector<int64_t> &shape) {
          std::pair<Tensor, Tensor> r;
          {
            py::gil_scoped_release nogil;
            r = dense_occupied(box, outer, inner, shape);
          }
          return py::make_tuple(r.first, r.second);
        },
        py::arg("box"), py::arg("outer"), py::arg("inner"), py::arg("shape"));
  m.def("DenseCoordinatesGPU",
        [](const std::vector<int64_t> &shape, const py::object &device) {
          const c10::Device dev = py::cast<c10::Device>(py::module_::import("torch").attr("device")(device));
          py::gil_scoped_release nogil;
          return dense_coordinates(shape, dev);
        },
        py::arg("shape"), py::arg("device"));
  m.def("PruningForwardGPU", &pruning_forward);
  m.def("PruningBackwardGPU", &pruning_backward);

  // ---- batch norm over feature rows (not in the reference's module: its MinkowskiBatchNorm is torch's BatchNorm1d) ----
  m.def("bn_stats",
        [](const Tensor &x, double eps, double momentum, const py::object &rm, const py::object &rv, const py::object &nbt) {
          auto r = bn_stats(x, eps, momentum, opt_tensor(rm), opt_tensor(rv), opt_tensor(nbt));
          return py::make_tuple(r.first, r.second);
        },
        py::arg("x"), py::arg("eps"), py::arg("momentum"), py::arg("running_mean") = py::none(),
        py::arg("running_var") = py::none(), py::arg("num_batches_tracked") = py::none());
  m.def("bn_apply",
        [](const Tensor &x, const Tensor &mean, const Tensor &rstd, const py::object &gamma, const py::object &beta,
           bool relu) { return bn_apply(x, mean, rstd, opt_tensor(gamma), opt_tensor(beta), relu, Tensor()); },
        py::arg("x"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"), py::arg("beta"), py::arg("relu") = false);

  // ---- autograd entry points (the Python modules call these; backward never enters Python) ----
  m.def("conv_autograd", &conv_autograd, py::arg("in_feat"), py::arg("kernel"), py::arg("kernel_size"),
        py::arg("kernel_stride"), py::arg("kernel_dilation"), py::arg("region_type"), py::arg("expand_coordinates"),
        py::arg("in_key"), py::arg("out_key"), py::arg("manager"), py::arg("transpose"),
        py::arg("region_offsets") = py::none());
  m.def("batch_norm_train", &batch_norm_train, py::arg("x"), py::arg("skip"), py::arg("weight"), py::arg("bias"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"), py::arg("relu"),
        py::arg("num_batches_tracked"));
}
